// dpvpos.hip — MI355X (gfx950, CDNA4) CHROM / POS parse of the lines of a VCF body + the C ABI of libdpvpos.so
// (include/dpvpos.h, which holds the definition of the index).
//
// vpos_parse_kernel: one lane per line.  The lane reads its line's prefix as aligned dwords from the line's start and
// walks the bytes through a two-phase state (CHROM up to the first tab, POS digits up to the second), at most
// VPOS_PREFIX_MAX bytes and never beyond the buffer or the object's end; then it compares its CHROM byte by byte with
// the bytes at the previous line's start (that line's first field must end in a tab right behind them).  The previous
// line's bytes were just read by the neighbouring lane, so they come from L1 / L2.
// vpos_reduce_kernel: one lane per line over the parse outputs: the sampled POS at their own slots, the run starts
// and run ends compacted through one counter each (a wave takes its slots with one atomic: ballot, popcount of the
// lanes below, the leader's atomicAdd broadcast), the counts and lowest indices of malformed and unsorted lines.
// vpos_name_kernel: one wave per run start copies its CHROM bytes into a packed buffer (fai_name_kernel's copy step)
// and writes the line's start, so the uint64 starts themselves never leave the device.
// No workgroup ever waits on another: no look-back, no spin, no flag, no ticket -- only atomics on the result words,
// which are initialised on the stream at every launch; the kernel boundary between parse and reduce is the only
// ordering.  Loads are plain loads with compiler-placed waits; outputs are ordinary vector stores and atomics.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "../../include/dpvpos.h"

namespace {

constexpr int kWave = 64;
constexpr int kBlock = 256;                        // lines per workgroup of both kernels

struct ParseArgs {
  const uint8_t* base;         // 4-byte aligned; the coordinates below are relative to it
  uint64_t lo, hi;             // the buffer's bytes below the object's end: coordinates [lo, hi), lo in 0..3
  uint64_t buf_base;           // object offset of coordinate lo
  const unsigned long long* starts;
  uint64_t n;
  uint32_t* pos;
  uint16_t* clen;
  uint8_t* flags;
};

__global__ void __launch_bounds__(kBlock) vpos_parse_kernel(ParseArgs A) {
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= A.n) return;
  const uint64_t s = A.starts[i];
  uint32_t st = 0;                                 // 0 open, 1 well formed, 2 malformed
  uint32_t phase = 0, nd = 0, cl = 0;
  uint64_t val = 0;
  uint64_t c = 0;
  if (s < A.buf_base || s - A.buf_base >= A.hi - A.lo) {
    st = 2;                                        // the start lies outside the buffer (or at / past the object's end)
  } else {
    c = s - A.buf_base + A.lo;
    const uint64_t lim = c + VPOS_PREFIX_MAX < A.hi ? c + VPOS_PREFIX_MAX : A.hi;
    for (uint64_t a = c & ~3ull; st == 0 && a < lim; a += 4) {
      const uint32_t w = *reinterpret_cast<const uint32_t*>(A.base + a);   // holds a byte of [lo, hi)
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const uint64_t q = a + k;
        if (st != 0 || q < c || q >= lim) continue;
        const uint32_t b = (w >> (8 * k)) & 0xFFu;
        if (phase == 0) {
          if (b == '\t') {
            cl = (uint32_t)(q - c);
            if (cl == 0) st = 2;
            phase = 1;
          } else if (b == '\n') {
            st = 2;
          }
        } else if (b - '0' < 10u) {
          val = val * 10u + (b - '0');
          if (++nd > 10u) st = 2;
        } else if (b == '\t') {
          st = (nd >= 1u && val <= (uint64_t)VPOS_POS_MAX) ? 1u : 2u;
        } else {
          st = 2;
        }
      }
    }
    if (st == 0) st = 2;                           // the prefix ran out: 1024 bytes, the object's or the buffer's end
  }
  uint32_t same = 0;
  if (st == 1 && i > 0) {
    const uint64_t sp = A.starts[i - 1];
    if (sp >= A.buf_base && sp - A.buf_base < A.hi - A.lo) {
      const uint64_t cp = sp - A.buf_base + A.lo;
      if (cp + cl < A.hi && A.base[cp + cl] == '\t') {
        same = 1;
        for (uint32_t j = 0; j < cl; ++j) {
          if (A.base[cp + j] != A.base[c + j]) {
            same = 0;
            break;
          }
        }
      }
    }
  }
  A.pos[i] = st == 1 ? (uint32_t)val : 0u;
  A.clen[i] = st == 1 ? (uint16_t)cl : (uint16_t)0;
  A.flags[i] = (uint8_t)(st == 1 ? same : VPOS_MALFORMED);
}

struct ReduceArgs {
  const uint32_t* pos;
  const uint16_t* clen;
  const uint8_t* flags;
  uint64_t n, ordinal0, slot0;   // slot0 = ceil(ordinal0 / every)
  uint32_t mask, shift;          // every - 1, log2(every)
  uint32_t* samples;
  unsigned long long* runs;
  unsigned long long* run_ends;
  uint32_t* run_clen;
  uint64_t run_cap;
  unsigned long long* res;
};

// the slots of the wave's lanes with `want`: one atomicAdd by lane 0, each lane its rank among the lanes below it
__device__ __forceinline__ uint64_t wave_slots(bool want, unsigned long long* counter, int lane) {
  const unsigned long long b = __ballot(want);
  unsigned long long base = 0;
  if (lane == 0 && b) base = atomicAdd(counter, (unsigned long long)__popcll(b));
  base = (unsigned long long)__shfl((long long)base, 0, kWave);
  return base + (uint64_t)__popcll(b & ((1ull << lane) - 1ull));
}

__global__ void __launch_bounds__(kBlock) vpos_reduce_kernel(ReduceArgs A) {
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  const int lane = threadIdx.x & (kWave - 1);
  const bool in = i < A.n;                         // no lane leaves early: the ballots want the whole wave
  const uint32_t f = in ? A.flags[i] : VPOS_SAME;
  const uint32_t p = in ? A.pos[i] : 0u;
  const uint64_t ord = A.ordinal0 + i;
  if (in && (ord & A.mask) == 0) A.samples[(ord >> A.shift) - A.slot0] = p;
  const bool start = in && !(f & VPOS_SAME);
  const bool end = in && (i + 1 == A.n || !(A.flags[i + 1] & VPOS_SAME));
  const bool mal = in && (f & VPOS_MALFORMED);
  const bool uns = in && i > 0 && (f & VPOS_SAME) && p < A.pos[i - 1];
  const uint64_t ks = wave_slots(start, A.res + DVP_R_RUNS, lane);
  if (start && ks < A.run_cap) {
    A.runs[ks] = ((unsigned long long)i << 32) | p;
    A.run_clen[ks] = A.clen[i];
  }
  const uint64_t ke = wave_slots(end, A.res + DVP_R_RUN_ENDS, lane);
  if (end && ke < A.run_cap) A.run_ends[ke] = ((unsigned long long)i << 32) | p;
  const unsigned long long bm = __ballot(mal), bu = __ballot(uns);
  if (lane == 0) {
    const uint64_t i0 = i;                         // the wave's first line
    if (bm) {
      atomicAdd(A.res + DVP_R_MALFORMED, (unsigned long long)__popcll(bm));
      atomicMin(A.res + DVP_R_MIN_MALFORMED, (unsigned long long)(i0 + (uint64_t)__builtin_ctzll(bm)));
    }
    if (bu) {
      atomicAdd(A.res + DVP_R_UNSORTED, (unsigned long long)__popcll(bu));
      atomicMin(A.res + DVP_R_MIN_UNSORTED, (unsigned long long)(i0 + (uint64_t)__builtin_ctzll(bu)));
    }
  }
  if (in && i == 0) A.res[DVP_R_FIRST_POS] = p;
  if (in && i + 1 == A.n) A.res[DVP_R_LAST_POS] = p;
}

struct NameArgs {
  const uint8_t* buf;
  uint64_t buf_len, buf_base;
  const unsigned long long* starts;
  const uint16_t* clen;
  uint64_t n;
  const uint32_t* lines;
  const unsigned long long* off;
  uint64_t m;
  uint8_t* out;
  uint64_t out_cap;
  unsigned long long* line_start;
};

__global__ void __launch_bounds__(kBlock) vpos_name_kernel(NameArgs A) {
  const uint64_t j = (uint64_t)blockIdx.x * (kBlock / kWave) + (threadIdx.x / kWave);
  if (j >= A.m) return;
  const uint64_t line = A.lines[j];
  if (line >= A.n) return;
  const uint64_t s = A.starts[line], o = A.off[j];
  const uint32_t len = A.clen[line];
  if (threadIdx.x % kWave == 0) A.line_start[j] = s;
  if (s < A.buf_base) return;
  for (uint32_t k = threadIdx.x % kWave; k < len; k += kWave) {
    const uint64_t src = s - A.buf_base + k;
    if (src < A.buf_len && o + k < A.out_cap && o + k >= o) A.out[o + k] = A.buf[src];
  }
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
      return fail(DVP_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));         \
  } while (0)

}  // namespace

struct dvp_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
};

extern "C" {

int dvp_abi_version(void) { return DVP_ABI_VERSION; }

const char* dvp_last_error(void) { return g_err.c_str(); }

int dvp_ctx_create(int device, void* stream, dvp_ctx** out) {
  if (!out) return fail(DVP_ERR_INVALID, "null out");
  *out = nullptr;
  int n = 0;
  HIPCHK(hipGetDeviceCount(&n));
  if (device < 0 || device >= n) return fail(DVP_ERR_INVALID, "device " + std::to_string(device) + " out of range");
  HIPCHK(hipSetDevice(device));
  dvp_ctx* c = new dvp_ctx();
  c->device = device;
  c->stream = (hipStream_t)stream;
  *out = c;
  return DVP_OK;
}

int dvp_ctx_destroy(dvp_ctx* c) {
  if (!c) return DVP_OK;
  (void)hipSetDevice(c->device);
  (void)hipStreamSynchronize(c->stream);
  delete c;
  return DVP_OK;
}

int dvp_parse_async(dvp_ctx* c, const uint8_t* d_buf, uint64_t buf_len, uint64_t buf_base, uint64_t size,
                    const uint64_t* d_starts, uint64_t n, uint32_t* d_pos, uint16_t* d_clen, uint8_t* d_flags) {
  if (!c) return fail(DVP_ERR_INVALID, "null ctx");
  if (buf_len && !d_buf) return fail(DVP_ERR_INVALID, "null buffer");
  if (buf_base + buf_len < buf_base) return fail(DVP_ERR_INVALID, "the buffer wraps the offset space");
  if (n >= (1ull << 32)) return fail(DVP_ERR_INVALID, "too many lines for one launch");
  if (n && (!d_starts || !d_pos || !d_clen || !d_flags)) return fail(DVP_ERR_INVALID, "null line or output array");
  if (((uintptr_t)d_starts & 7u) || ((uintptr_t)d_pos & 3u) || ((uintptr_t)d_clen & 1u))
    return fail(DVP_ERR_INVALID, "misaligned line or output array");
  HIPCHK(hipSetDevice(c->device));
  if (n == 0) return DVP_OK;
  const uint64_t shift = (uint64_t)((uintptr_t)d_buf & 3u);
  uint64_t len = buf_len;                          // the buffer's bytes below the object's end
  if (size <= buf_base) len = 0;
  else if (size - buf_base < len) len = size - buf_base;
  ParseArgs a;
  a.base = (const uint8_t*)((uintptr_t)d_buf - (uintptr_t)shift);
  a.lo = shift;
  a.hi = shift + len;
  a.buf_base = buf_base;
  a.starts = (const unsigned long long*)d_starts;
  a.n = n;
  a.pos = d_pos;
  a.clen = d_clen;
  a.flags = d_flags;
  hipLaunchKernelGGL(vpos_parse_kernel, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, c->stream, a);
  HIPCHK(hipGetLastError());
  return DVP_OK;
}

int dvp_reduce_async(dvp_ctx* c, const uint32_t* d_pos, const uint16_t* d_clen, const uint8_t* d_flags, uint64_t n,
                     uint64_t ordinal0, uint32_t every, uint32_t* d_samples, uint64_t* d_runs, uint64_t* d_run_ends,
                     uint32_t* d_run_clen, uint64_t run_cap, uint64_t* d_result) {
  if (!c) return fail(DVP_ERR_INVALID, "null ctx");
  if (every == 0 || (every & (every - 1))) return fail(DVP_ERR_INVALID, "every must be a power of two");
  if (n >= (1ull << 32)) return fail(DVP_ERR_INVALID, "too many lines for one launch");
  if (ordinal0 + n < ordinal0) return fail(DVP_ERR_INVALID, "the ordinals wrap");
  if (!d_result) return fail(DVP_ERR_INVALID, "null result");
  if (n && (!d_pos || !d_clen || !d_flags || !d_samples)) return fail(DVP_ERR_INVALID, "null line or sample array");
  if (run_cap && (!d_runs || !d_run_ends || !d_run_clen)) return fail(DVP_ERR_INVALID, "null run array");
  if (((uintptr_t)d_result | (uintptr_t)d_runs | (uintptr_t)d_run_ends) & 7u)
    return fail(DVP_ERR_INVALID, "misaligned run or result array");
  if ((((uintptr_t)d_pos | (uintptr_t)d_samples | (uintptr_t)d_run_clen) & 3u) || ((uintptr_t)d_clen & 1u))
    return fail(DVP_ERR_INVALID, "misaligned line or sample array");
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipMemsetAsync(d_result, 0, DVP_R_MIN_MALFORMED * sizeof(uint64_t), c->stream));
  HIPCHK(hipMemsetAsync(d_result + DVP_R_MIN_MALFORMED, 0xFF, (DVP_R_WORDS - DVP_R_MIN_MALFORMED) * sizeof(uint64_t),
                        c->stream));
  if (n == 0) return DVP_OK;
  ReduceArgs a;
  a.pos = d_pos;
  a.clen = d_clen;
  a.flags = d_flags;
  a.n = n;
  a.ordinal0 = ordinal0;
  a.mask = every - 1u;
  a.shift = (uint32_t)__builtin_ctz(every);
  a.slot0 = (ordinal0 + a.mask) >> a.shift;
  a.samples = d_samples;
  a.runs = (unsigned long long*)d_runs;
  a.run_ends = (unsigned long long*)d_run_ends;
  a.run_clen = d_run_clen;
  a.run_cap = run_cap;
  a.res = (unsigned long long*)d_result;
  hipLaunchKernelGGL(vpos_reduce_kernel, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, c->stream, a);
  HIPCHK(hipGetLastError());
  return DVP_OK;
}

int dvp_names_async(dvp_ctx* c, const uint8_t* d_buf, uint64_t buf_len, uint64_t buf_base, const uint64_t* d_starts,
                    const uint16_t* d_clen, uint64_t n, const uint32_t* d_lines, const uint64_t* d_off, uint64_t m,
                    uint8_t* d_out, uint64_t out_cap, uint64_t* d_line_start) {
  if (!c) return fail(DVP_ERR_INVALID, "null ctx");
  if (buf_len && !d_buf) return fail(DVP_ERR_INVALID, "null buffer");
  if (buf_base + buf_len < buf_base) return fail(DVP_ERR_INVALID, "the buffer wraps the offset space");
  if (m >= (1ull << 32)) return fail(DVP_ERR_INVALID, "too many names for one launch");
  if (m && (!d_starts || !d_clen || !d_lines || !d_off || !d_line_start || (out_cap && !d_out)))
    return fail(DVP_ERR_INVALID, "null line or output array");
  if ((((uintptr_t)d_starts | (uintptr_t)d_off | (uintptr_t)d_line_start) & 7u) || ((uintptr_t)d_lines & 3u) || ((uintptr_t)d_clen & 1u))
    return fail(DVP_ERR_INVALID, "misaligned line or output array");
  HIPCHK(hipSetDevice(c->device));
  if (m == 0) return DVP_OK;
  NameArgs a;
  a.buf = d_buf;
  a.buf_len = buf_len;
  a.buf_base = buf_base;
  a.starts = (const unsigned long long*)d_starts;
  a.clen = d_clen;
  a.n = n;
  a.lines = d_lines;
  a.off = (const unsigned long long*)d_off;
  a.m = m;
  a.out = d_out;
  a.out_cap = out_cap;
  a.line_start = (unsigned long long*)d_line_start;
  const uint64_t per = kBlock / kWave;
  hipLaunchKernelGGL(vpos_name_kernel, dim3((unsigned)((m + per - 1) / per)), dim3(kBlock), 0, c->stream, a);
  HIPCHK(hipGetLastError());
  return DVP_OK;
}

int dvp_geometry(dvp_ctx* c, int* parse_lines, int* reduce_lines) {
  if (!c) return fail(DVP_ERR_INVALID, "null ctx");
  if (parse_lines) *parse_lines = kBlock;
  if (reduce_lines) *reduce_lines = kBlock;
  return DVP_OK;
}

}  // extern "C"
