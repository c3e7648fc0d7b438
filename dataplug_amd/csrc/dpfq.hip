// dpfq.hip — MI355X (gfx950, CDNA4) read lengths and cumulative bases of an uncompressed FASTQ + the C ABI of
// libdpfq.so (include/dpfq.h, which holds the definition of the index).
//
// fq_read_kernel: one lane per read.  The lane reads the starts of its four lines and of the line behind them as
// three aligned 16-byte loads, then the four bytes the definition looks at -- the first byte of lines 0 and 2, the
// byte before the terminator of lines 1 and 3 -- whose addresses all follow from the starts alone: the four byte
// loads do not depend on one another, so they are issued together and waited for once (vpos_parse_kernel walks a
// line's prefix dword after dword, each step behind the one before).  A workgroup adds its reads' bases to one uint64
// (wave shuffles, then LDS); a wave updates each result word with at most one atomic, and none where a look at the
// word shows that its own minimum or maximum would not change it.
// fq_scan_kernel: one workgroup turns the workgroups' sums into exclusive sums in place, looping over them.
// fq_sample_kernel: one lane per read; a workgroup scans its own len[] on top of its block sum and the lanes of every
// K-th read write (start of the read, bases before it) to their own slots.
// No workgroup ever waits on another: no look-back, no spin, no flag, no ticket -- only atomics on the result words,
// which are initialised on the stream; the kernel boundaries are the only ordering.  Loads are plain loads with
// compiler-placed waits; outputs are ordinary vector stores and atomics.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "../../include/dpfq.h"

namespace {

constexpr int kWave = 64;
constexpr int kBlock = 256;                        // reads per workgroup of the read and the sample kernel
constexpr int kScan = 1024;                        // lanes of the scan kernel's one workgroup

typedef unsigned long long u64;

__device__ __forceinline__ u64 wave_sum(u64 v) {
#pragma unroll
  for (int d = 1; d < kWave; d <<= 1) v += (u64)__shfl_xor((long long)v, d, kWave);
  return v;
}

// the inclusive sums over the lanes of a wave
__device__ __forceinline__ u64 wave_scan(u64 v, int lane) {
#pragma unroll
  for (int d = 1; d < kWave; d <<= 1) {
    const u64 t = (u64)__shfl_up((long long)v, d, kWave);
    if (lane >= d) v += t;
  }
  return v;
}

struct ReadArgs {
  const uint8_t* buf;
  uint64_t len;                // the buffer's bytes below the object's end
  uint64_t buf_base;           // object offset of buf[0]
  const ulonglong2* starts;    // the 16-byte word that holds entry 0 of d_starts
  uint64_t e0;                 // read 0's first line, in entries from that word: (d_starts is its upper half) + skip
  uint64_t n_entries;          // e0 + 4n: no 16-byte word that begins at or beyond this entry is read
  uint64_t n, last_end;
  uint32_t* len_out;
  uint8_t* flags;
  u64* block;
  u64* res;
};

__global__ void __launch_bounds__(kBlock) fq_read_kernel(ReadArgs A) {
  __shared__ u64 wsum[kBlock / kWave];
  const uint64_t r = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  const int lane = threadIdx.x & (kWave - 1);
  const bool in = r < A.n;                         // no lane leaves early: the reductions want the whole wave
  uint32_t ln = 0, fl = 0;
  if (in) {
    const uint64_t e = A.e0 + 4 * r;
    const uint64_t p = e >> 1;
    const ulonglong2 a = A.starts[p], b = A.starts[p + 1];
    ulonglong2 c = make_ulonglong2(0, 0);
    if (2 * (p + 2) < A.n_entries) c = A.starts[p + 2];
    const bool odd = e & 1;
    const uint64_t s0 = odd ? a.y : a.x, s1 = odd ? b.x : a.y, s2 = odd ? b.y : b.x, s3 = odd ? c.x : b.y;
    const uint64_t end3 = r + 1 < A.n ? (odd ? c.y : c.x) - 1 : A.last_end;
    // the lines' lengths up to their terminators (0 where the starts do not ascend)
    const uint64_t raw0 = s1 > s0 ? s1 - 1 - s0 : 0, raw1 = s2 > s1 ? s2 - 1 - s1 : 0;
    const uint64_t raw2 = s3 > s2 ? s3 - 1 - s2 : 0, raw3 = end3 > s3 ? end3 - s3 : 0;
    // the four bytes: addresses from the starts alone, clamped into the buffer, loaded together
    const uint64_t q0 = s0, q1 = s2 - 2, q2 = s2, q3 = end3 - 1;
    const bool k0 = raw0 >= 1 && q0 >= A.buf_base && q0 - A.buf_base < A.len;
    const bool k1 = raw1 >= 1 && q1 >= A.buf_base && q1 - A.buf_base < A.len;
    const bool k2 = raw2 >= 1 && q2 >= A.buf_base && q2 - A.buf_base < A.len;
    const bool k3 = raw3 >= 1 && q3 >= A.buf_base && q3 - A.buf_base < A.len;
    uint32_t b0 = 0, b1 = 0, b2 = 0, b3 = 0;
    if (A.len) {                                   // (uniform) index 0 is a byte of the buffer
      const uint8_t v0 = A.buf[k0 ? q0 - A.buf_base : 0], v1 = A.buf[k1 ? q1 - A.buf_base : 0];
      const uint8_t v2 = A.buf[k2 ? q2 - A.buf_base : 0], v3 = A.buf[k3 ? q3 - A.buf_base : 0];
      b0 = k0 ? v0 : 0u;
      b1 = k1 ? v1 : 0u;
      b2 = k2 ? v2 : 0u;
      b3 = k3 ? v3 : 0u;
    }
    const uint64_t c1 = raw1 - (b1 == '\r'), c3 = raw3 - (b3 == '\r');   // (b == '\r' only where raw >= 1)
    if (b0 != '@') fl = DFQ_BAD_HEADER;
    else if (b2 != '+') fl = DFQ_BAD_SEPARATOR;
    else if (c1 != c3 || (c1 >> 32)) fl = DFQ_LENGTH_MISMATCH;
    ln = (uint32_t)c1;
    A.len_out[r] = ln;
    A.flags[r] = (uint8_t)fl;
  }
  const u64 ws = wave_sum(in ? ln : 0u);
  uint32_t mx = in ? ln : 0u, mn = in ? ln : 0xFFFFFFFFu;
#pragma unroll
  for (int d = 1; d < kWave; d <<= 1) {
    const uint32_t ox = (uint32_t)__shfl_xor((int)mx, d, kWave), on = (uint32_t)__shfl_xor((int)mn, d, kWave);
    mx = ox > mx ? ox : mx;
    mn = on < mn ? on : mn;
  }
  const u64 bm = __ballot(in && fl != 0);
  if (lane == 0) {
    wsum[threadIdx.x / kWave] = ws;
    if (in) {                                      // lane 0 holds the wave's lowest read: the wave has reads
      // every wave of the launch meets at these two words, and atomics on one address take their turns in L2: a wave
      // looks first and leaves out the atomic that cannot change the word.  The maximum only grows and the minimum
      // only shrinks, so a stale look costs an atomic that was not needed, never one that was.
      if ((u64)mx > __atomic_load_n(A.res + DFQ_R_MAX_LEN, __ATOMIC_RELAXED)) atomicMax(A.res + DFQ_R_MAX_LEN, (u64)mx);
      if ((u64)mn < __atomic_load_n(A.res + DFQ_R_MIN_LEN, __ATOMIC_RELAXED)) atomicMin(A.res + DFQ_R_MIN_LEN, (u64)mn);
    }
    if (bm) {
      atomicAdd(A.res + DFQ_R_MALFORMED, (u64)__popcll(bm));
      atomicMin(A.res + DFQ_R_MIN_MALFORMED, (u64)(r + (uint64_t)__builtin_ctzll(bm)));
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    u64 t = 0;
#pragma unroll
    for (int w = 0; w < kBlock / kWave; ++w) t += wsum[w];
    A.block[blockIdx.x] = t;
  }
}

__global__ void __launch_bounds__(kScan) fq_scan_kernel(u64* block, uint64_t nb, u64* res) {
  __shared__ u64 wtot[kScan / kWave];
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  u64 carry = 0;
  for (uint64_t base = 0; base < nb; base += kScan) {     // (uniform) every lane takes every turn
    const uint64_t i = base + threadIdx.x;
    const u64 v = i < nb ? block[i] : 0;
    const u64 inc = wave_scan(v, lane);
    if (lane == kWave - 1) wtot[wave] = inc;
    __syncthreads();
    u64 pre = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < kScan / kWave; ++w) {
      const u64 t = wtot[w];
      pre += w < wave ? t : 0;
      tot += t;
    }
    if (i < nb) block[i] = carry + pre + inc - v;
    carry += tot;
    __syncthreads();
  }
  if (threadIdx.x == 0) res[DFQ_R_BASES] = carry;
}

struct SampleArgs {
  const u64* starts;             // entry 0 of read 0's first line (d_starts + skip)
  const uint32_t* len;
  const u64* block;
  uint64_t n, read0, slot0;      // slot0 = ceil(read0 / every)
  uint32_t mask, shift;          // every - 1, log2(every)
  ulonglong2* samples;
};

__global__ void __launch_bounds__(kBlock) fq_sample_kernel(SampleArgs A) {
  __shared__ u64 wtot[kBlock / kWave];
  const uint64_t r = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const bool in = r < A.n;
  const u64 v = in ? A.len[r] : 0;
  const u64 inc = wave_scan(v, lane);
  if (lane == kWave - 1) wtot[wave] = inc;
  __syncthreads();
  u64 pre = A.block[blockIdx.x];
#pragma unroll
  for (int w = 0; w < kBlock / kWave; ++w) pre += w < wave ? wtot[w] : 0;
  const uint64_t g = A.read0 + r;
  if (in && (g & A.mask) == 0) A.samples[(g >> A.shift) - A.slot0] = make_ulonglong2(A.starts[4 * r], pre + inc - v);
}

// ------------------------------------------------------------------------------------------ host side
thread_local std::string g_err;

int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}
#define HIPCHK(expr)                                                                       \
  do {                                                                                     \
    hipError_t _e = (expr);                                                                \
    if (_e != hipSuccess)                                                                  \
      return fail(DFQ_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));         \
  } while (0)

}  // namespace

struct dfq_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
};

extern "C" {

int dfq_abi_version(void) { return DFQ_ABI_VERSION; }

const char* dfq_last_error(void) { return g_err.c_str(); }

int dfq_ctx_create(int device, void* stream, dfq_ctx** out) {
  if (!out) return fail(DFQ_ERR_INVALID, "null out");
  *out = nullptr;
  int n = 0;
  HIPCHK(hipGetDeviceCount(&n));
  if (device < 0 || device >= n) return fail(DFQ_ERR_INVALID, "device " + std::to_string(device) + " out of range");
  HIPCHK(hipSetDevice(device));
  dfq_ctx* c = new dfq_ctx();
  c->device = device;
  c->stream = (hipStream_t)stream;
  *out = c;
  return DFQ_OK;
}

int dfq_ctx_destroy(dfq_ctx* c) {
  if (!c) return DFQ_OK;
  (void)hipSetDevice(c->device);
  (void)hipStreamSynchronize(c->stream);
  delete c;
  return DFQ_OK;
}

int dfq_reads_async(dfq_ctx* c, const uint8_t* d_buf, uint64_t buf_len, uint64_t buf_base, uint64_t size,
                    const uint64_t* d_starts, uint32_t skip, uint64_t n, uint64_t last_end, uint32_t* d_len,
                    uint8_t* d_flags, uint64_t* d_block, uint64_t* d_result) {
  if (!c) return fail(DFQ_ERR_INVALID, "null ctx");
  if (buf_len && !d_buf) return fail(DFQ_ERR_INVALID, "null buffer");
  if (buf_base + buf_len < buf_base) return fail(DFQ_ERR_INVALID, "the buffer wraps the offset space");
  if (skip > 3) return fail(DFQ_ERR_INVALID, "skip must be 0..3");
  if (n >= (1ull << 32)) return fail(DFQ_ERR_INVALID, "too many reads for one launch");
  if (!d_result) return fail(DFQ_ERR_INVALID, "null result");
  if (n && (!d_starts || !d_len || !d_flags || !d_block)) return fail(DFQ_ERR_INVALID, "null line or output array");
  if ((((uintptr_t)d_starts | (uintptr_t)d_block | (uintptr_t)d_result) & 7u) || ((uintptr_t)d_len & 3u))
    return fail(DFQ_ERR_INVALID, "misaligned line or output array");
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipMemsetAsync(d_result, 0, DFQ_R_MIN_MALFORMED * sizeof(uint64_t), c->stream));
  HIPCHK(hipMemsetAsync(d_result + DFQ_R_MIN_MALFORMED, 0xFF, (DFQ_R_WORDS - DFQ_R_MIN_MALFORMED) * sizeof(uint64_t),
                        c->stream));
  if (n == 0) return DFQ_OK;
  uint64_t len = buf_len;                          // the buffer's bytes below the object's end
  if (size <= buf_base) len = 0;
  else if (size - buf_base < len) len = size - buf_base;
  ReadArgs a;
  a.buf = d_buf;
  a.len = len;
  a.buf_base = buf_base;
  a.starts = (const ulonglong2*)((uintptr_t)d_starts & ~(uintptr_t)15);
  a.e0 = (uint64_t)(((uintptr_t)d_starts >> 3) & 1u) + skip;
  a.n_entries = a.e0 + 4 * n;
  a.n = n;
  a.last_end = last_end;
  a.len_out = d_len;
  a.flags = d_flags;
  a.block = (u64*)d_block;
  a.res = (u64*)d_result;
  hipLaunchKernelGGL(fq_read_kernel, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, c->stream, a);
  HIPCHK(hipGetLastError());
  return DFQ_OK;
}

int dfq_scan_async(dfq_ctx* c, uint64_t* d_block, uint64_t n_blocks, uint64_t* d_result) {
  if (!c) return fail(DFQ_ERR_INVALID, "null ctx");
  if (!d_result || (n_blocks && !d_block)) return fail(DFQ_ERR_INVALID, "null block or result array");
  if (((uintptr_t)d_block | (uintptr_t)d_result) & 7u) return fail(DFQ_ERR_INVALID, "misaligned block or result array");
  HIPCHK(hipSetDevice(c->device));
  hipLaunchKernelGGL(fq_scan_kernel, dim3(1), dim3(kScan), 0, c->stream, (u64*)d_block, n_blocks, (u64*)d_result);
  HIPCHK(hipGetLastError());
  return DFQ_OK;
}

int dfq_sample_async(dfq_ctx* c, const uint64_t* d_starts, uint32_t skip, const uint32_t* d_len,
                     const uint64_t* d_block, uint64_t n, uint64_t read0, uint32_t every, uint64_t* d_samples) {
  if (!c) return fail(DFQ_ERR_INVALID, "null ctx");
  if (every == 0 || (every & (every - 1))) return fail(DFQ_ERR_INVALID, "every must be a power of two");
  if (skip > 3) return fail(DFQ_ERR_INVALID, "skip must be 0..3");
  if (n >= (1ull << 32)) return fail(DFQ_ERR_INVALID, "too many reads for one launch");
  if (read0 + n < read0) return fail(DFQ_ERR_INVALID, "the read indices wrap");
  if (n && (!d_starts || !d_len || !d_block || !d_samples)) return fail(DFQ_ERR_INVALID, "null line or sample array");
  if ((((uintptr_t)d_starts | (uintptr_t)d_block) & 7u) || ((uintptr_t)d_len & 3u) || ((uintptr_t)d_samples & 15u))
    return fail(DFQ_ERR_INVALID, "misaligned line or sample array");
  HIPCHK(hipSetDevice(c->device));
  if (n == 0) return DFQ_OK;
  SampleArgs a;
  a.starts = (const u64*)d_starts + skip;
  a.len = d_len;
  a.block = (const u64*)d_block;
  a.n = n;
  a.read0 = read0;
  a.mask = every - 1u;
  a.shift = (uint32_t)__builtin_ctz(every);
  a.slot0 = (read0 + a.mask) >> a.shift;
  a.samples = (ulonglong2*)d_samples;
  hipLaunchKernelGGL(fq_sample_kernel, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, c->stream, a);
  HIPCHK(hipGetLastError());
  return DFQ_OK;
}

int dfq_geometry(dfq_ctx* c, int* reads_per_wg, int* scan_lanes) {
  if (!c) return fail(DFQ_ERR_INVALID, "null ctx");
  if (reads_per_wg) *reads_per_wg = kBlock;
  if (scan_lanes) *scan_lanes = kScan;
  return DFQ_OK;
}

}  // extern "C"
