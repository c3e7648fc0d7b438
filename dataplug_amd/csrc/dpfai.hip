// dpfai.hip — MI355X (gfx950, CDNA4) per-sequence line-break counts of a FASTA object + the C ABI of libdpfai.so
// (include/dpfai.h, which holds the definition of the index).
//
// fai_count_kernel is a segmented count over the bytes: n ascending, disjoint segments (the sequence bodies, clipped
// to the buffer) and per segment the '\n' and '\r' bytes and the first '\n' (pass 1), or the '\n' bytes that do not
// lie on the segment's line grid and the last of them (pass 2).  A one-wave workgroup of a persistent grid takes a
// run of consecutive 16 KiB ranges, 16 rows of one 16-byte chunk per lane, and
//   - finds the first segment that reaches into its range by a binary search (wave-uniform; after the wave's first
//     range a gallop from the range before's answer: one load where the segment is still the same);
//   - fast path, a range that lies inside one segment (genomes): masks, popcounts and one wave reduction, then one
//     atomic per output per range;
//   - general path: a lane whose chunk holds a byte of interest finds the chunk's segments (binary search from the
//     lane's cursor) and adds the masked popcounts into kSlots per-wave LDS counters indexed by
//     segment - first segment of the range; the touched slots are flushed with global atomics at the range's end.
//     Segments beyond kSlots in one range go straight to global atomics.
// No workgroup ever waits on another: no look-back, no spin, no flag -- only atomics on the output arrays, which are
// initialised on the stream at every launch.  Loads are plain uint4 loads with compiler-placed waits, issued only for
// 16-byte chunks that hold a byte of the buffer; outputs are ordinary vector atomics.
//
// fai_name_kernel (headers are a few % of the bytes; straightforward code): one launch writes each header's name
// length, a second one copies the names into one packed buffer at the caller's exclusive sums.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "../../include/dpfai.h"

namespace {

constexpr int kWave = 64;
constexpr int kRowBytes = kWave * 16;              // one 16-byte chunk per lane
constexpr int kRows = 16;                          // rows per range
constexpr int kHalf = kRows / 2;                   // rows per load batch (32 VGPRs of destinations)
constexpr int kRangeBytes = kRowBytes * kRows;     // 16 KiB
constexpr int kSlots = 256;                        // per-wave segment slots in LDS
constexpr int kMaxWavesPerCU = 16;
static_assert(kRangeBytes <= 0xFFFF, "range counts are packed in 16 bits");

constexpr uint32_t kSel12 = 0x0C0C0C0Cu;           // v_perm selector that yields 0x00
constexpr uint32_t kKeyNl = 0x0A0A0A0Au ^ kSel12;
constexpr uint32_t kKeyCr = 0x0D0D0D0Du ^ kSel12;
constexpr uint32_t kNone32 = 0xFFFFFFFFu;

struct CountArgs {
  const uint8_t* base;         // 16-byte aligned; the coordinates below are relative to it
  uint64_t lo, hi;             // the buffer's bytes: coordinates [lo, hi), lo in 0..15
  uint64_t obj0;               // object offset of coordinate 0 (mod 2^64: only coordinates >= lo are object bytes)
  uint64_t nranges;
  const unsigned long long* slo;   // segments as object offsets
  const unsigned long long* shi;
  const unsigned long long* sorg;
  const uint32_t* swid;        // pass 2
  uint64_t n;
  unsigned long long* o0;      // pass 1: nl      pass 2: off
  unsigned long long* o1;      //         cr              lastoff
  unsigned long long* o2;      //         first
};

// 0x00 in every byte of w that equals the key's pattern byte, 0xFF in every other byte (exact for all 256 values).
__device__ __forceinline__ uint32_t match4(uint32_t w, uint32_t key) {
  return __builtin_amdgcn_perm(0xFFFFFFFFu, 0xFFFFFFFFu, w ^ key);
}
// match4 bytes of a lane's 4 dwords -> 16-bit mask, bit i = byte i matched (four v_dot4_i32_i8 with weights 1, 2, 4,
// 8 over bytes that are 0 or -1, never a data byte: each subtracts the non-matching weights from 15)
__device__ __forceinline__ uint32_t mask16(const uint4& v, uint32_t key) {
  const int d0 = __builtin_amdgcn_sdot4((int)match4(v.x, key), 0x08040201, 0xFFFF, false);
  const int d1 = __builtin_amdgcn_sdot4((int)match4(v.y, key), 0x08040201, 0, false);
  const int d2 = __builtin_amdgcn_sdot4((int)match4(v.z, key), 0x08040201, 0, false);
  const int d3 = __builtin_amdgcn_sdot4((int)match4(v.w, key), 0x08040201, 0, false);
  const uint32_t lo = ((uint32_t)d1 << 4) + (uint32_t)d0;
  const uint32_t hi = ((uint32_t)d3 << 4) + (uint32_t)d2;
  return ((hi << 8) + lo) & 0xFFFFu;
}
// the bytes of the 16-byte chunk at coordinate x that lie in [lo, hi), as 16 bits (x < hi and x + 16 > lo)
__device__ __forceinline__ uint32_t valid16(uint64_t x, uint64_t lo, uint64_t hi) {
  const uint32_t a = lo > x ? (uint32_t)(lo - x) : 0u;              // < 16
  const uint32_t b = hi - x < 16u ? (uint32_t)(hi - x) : 16u;       // 1..16
  return (0xFFFFu >> (16u - b)) & (0xFFFFu << a);
}
__device__ __forceinline__ uint32_t wave_sum(uint32_t x) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) x += (uint32_t)__shfl_xor((int)x, d, kWave);
  return x;
}
__device__ __forceinline__ uint32_t wave_min(uint32_t x) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const uint32_t y = (uint32_t)__shfl_xor((int)x, d, kWave);
    x = y < x ? y : x;
  }
  return x;
}
__device__ __forceinline__ uint32_t wave_max(uint32_t x) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const uint32_t y = (uint32_t)__shfl_xor((int)x, d, kWave);
    x = y > x ? y : x;
  }
  return x;
}
// the wave's LDS atomics of before are done and visible to its LDS reads of after (the slots are the wave's own)
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}
// is the '\n' at object offset p off the line grid of a segment with origin b and line width w: (p - b + 1) % w != 0
__device__ __forceinline__ bool off_grid(uint64_t p, uint64_t b, uint32_t w) {
  if (w == 0u) return true;
  const uint64_t d = p - b + 1u;
  return (d >> 32) ? (d % w) != 0u : ((uint32_t)d % w) != 0u;
}

// PASS 1: nl, cr, first.  PASS 2: off, lastoff.
template <int PASS>
__global__ void __launch_bounds__(kWave) fai_count_kernel(CountArgs A) {
  // pass 1: '\n' count, '\r' count, lowest '\n' position in the range (kNone32: none)
  // pass 2: off-grid count, highest off-grid position in the range + 1 (0: none)
  __shared__ uint32_t s_a[kSlots], s_b[kSlots], s_c[kSlots];
  const int lane = threadIdx.x;
  for (int k = lane; k < kSlots; k += kWave) {
    s_a[k] = 0u;
    s_b[k] = 0u;
    s_c[k] = kNone32;
  }
  wave_sync();

  // a wave takes `per` consecutive ranges, so the segment search of a range starts at the range before's answer
  const uint64_t per = (A.nranges + gridDim.x - 1) / gridDim.x;
  const uint64_t rbeg = (uint64_t)blockIdx.x * per;
  const uint64_t rend = rbeg + per < A.nranges ? rbeg + per : A.nranges;
  uint64_t s0 = 0;
  for (uint64_t r = rbeg; r < rend; ++r) {
    const uint64_t x0 = r * kRangeBytes;
    const uint64_t xa = x0 > A.lo ? x0 : A.lo;                        // the range's bytes of the buffer: [xa, xb)
    const uint64_t xb = x0 + kRangeBytes < A.hi ? x0 + kRangeBytes : A.hi;
    // the first segment that reaches beyond xa (wave-uniform): a bisection for the wave's first range, then a
    // gallop from the range before's answer (every segment below s0 ends at or before xa)
    uint64_t e = A.n;
    if (r != rbeg) {
      uint64_t step = 1;
      e = s0;
      while (e < A.n && A.shi[e] - A.obj0 <= xa) {
        s0 = e + 1;
        e = s0 + step;
        step <<= 1;
      }
      if (e > A.n) e = A.n;
    }
    while (s0 < e) {
      const uint64_t m = s0 + ((e - s0) >> 1);
      if (A.shi[m] - A.obj0 > xa) e = m;
      else s0 = m + 1;
    }
    if (s0 >= A.n) break;                                             // every later range lies beyond the segments
    const uint64_t l0 = A.slo[s0] - A.obj0, h0 = A.shi[s0] - A.obj0;
    if (l0 >= xb) continue;                                           // no segment holds a byte of the range
    const uint64_t xl = x0 + (uint64_t)lane * 16u;

    if (l0 <= xa && h0 >= xb) {
      // ---- fast path: the range lies inside segment s0
      uint32_t cnt = 0;                            // pass 1: nl | cr << 16 (<= 256 each per lane); pass 2: off
      uint32_t pos = PASS == 1 ? kNone32 : 0u;
      uint64_t org = 0;
      uint32_t wid = 0;
      if (PASS == 2) {
        org = A.sorg[s0];
        wid = A.swid[s0];
      }
#pragma unroll
      for (int h = 0; h < kRows; h += kHalf) {
        uint4 v[kHalf];
        uint32_t ok[kHalf];
#pragma unroll
        for (int i = 0; i < kHalf; ++i) {
          const uint64_t x = xl + (uint64_t)(h + i) * kRowBytes;
          v[i] = make_uint4(0u, 0u, 0u, 0u);
          ok[i] = 0u;
          if (x < A.hi && x + 16u > A.lo) {        // the chunk holds a byte of the buffer: inside its pages
            v[i] = *reinterpret_cast<const uint4*>(A.base + x);
            ok[i] = valid16(x, A.lo, A.hi);
          }
        }
#pragma unroll
        for (int i = 0; i < kHalf; ++i) {
          const uint64_t x = xl + (uint64_t)(h + i) * kRowBytes;
          uint32_t nl = mask16(v[i], kKeyNl) & ok[i];
          if (PASS == 1) {
            const uint32_t cr = mask16(v[i], kKeyCr) & ok[i];
            cnt += (uint32_t)__popc(nl) | ((uint32_t)__popc(cr) << 16);
            if (nl) {
              const uint32_t p = (uint32_t)(x - x0) + (uint32_t)__builtin_ctz(nl);
              pos = p < pos ? p : pos;
            }
          } else {
            while (nl) {
              const uint32_t bit = (uint32_t)__builtin_ctz(nl);
              nl &= nl - 1u;
              if (off_grid(A.obj0 + x + bit, org, wid)) {
                ++cnt;
                const uint32_t p = (uint32_t)(x - x0) + bit + 1u;
                pos = p > pos ? p : pos;
              }
            }
          }
        }
      }
      cnt = wave_sum(cnt);                         // <= 16384 per half: no carry between the halves
      pos = PASS == 1 ? wave_min(pos) : wave_max(pos);
      if (lane == 0) {
        if (PASS == 1) {
          if (cnt & 0xFFFFu) atomicAdd(A.o0 + s0, (unsigned long long)(cnt & 0xFFFFu));
          if (cnt >> 16) atomicAdd(A.o1 + s0, (unsigned long long)(cnt >> 16));
          if (pos != kNone32) atomicMin(A.o2 + s0, (unsigned long long)(A.obj0 + x0 + pos));
        } else if (cnt) {
          atomicAdd(A.o0 + s0, (unsigned long long)cnt);
          atomicMax(A.o1 + s0, (unsigned long long)(A.obj0 + x0 + pos - 1u));
        }
      }
      continue;
    }

    // ---- general path: several segments, or gaps, in the range
    // the first segment that starts at or beyond xb: a gallop from s0, then a bisection
    uint64_t s1 = s0 + 1;
    e = s1;
    for (uint64_t step = 1; e < A.n && A.slo[e] - A.obj0 < xb; step <<= 1) {
      s1 = e + 1;
      e = s1 + step;
    }
    if (e > A.n) e = A.n;
    while (s1 < e) {
      const uint64_t m = s1 + ((e - s1) >> 1);
      if (A.slo[m] - A.obj0 >= xb) e = m;
      else s1 = m + 1;
    }
    uint64_t seg = s0;                             // the lane's cursor: its chunks ascend
#pragma unroll 1
    for (int h = 0; h < kRows; h += kHalf) {
      uint4 v[kHalf];
      uint32_t ok[kHalf];
#pragma unroll
      for (int i = 0; i < kHalf; ++i) {
        const uint64_t x = xl + (uint64_t)(h + i) * kRowBytes;
        v[i] = make_uint4(0u, 0u, 0u, 0u);
        ok[i] = 0u;
        if (x < A.hi && x + 16u > A.lo) {          // the chunk holds a byte of the buffer: inside its pages
          v[i] = *reinterpret_cast<const uint4*>(A.base + x);
          ok[i] = valid16(x, A.lo, A.hi);
        }
      }
#pragma unroll
      for (int i = 0; i < kHalf; ++i) {
        const uint64_t x = xl + (uint64_t)(h + i) * kRowBytes;
        const uint32_t nl = mask16(v[i], kKeyNl) & ok[i];
        const uint32_t cr = PASS == 1 ? mask16(v[i], kKeyCr) & ok[i] : 0u;
        if ((nl | cr) == 0u) continue;
        // the first segment at or after the cursor that reaches beyond x
        uint64_t a = seg, b = s1;
        while (a < b) {
          const uint64_t m = a + ((b - a) >> 1);
          if (A.shi[m] - A.obj0 > x) b = m;
          else a = m + 1;
        }
        uint64_t s = a;
        while (s < s1) {
          const uint64_t l = A.slo[s] - A.obj0;
          if (l >= x + 16u) break;
          const uint64_t hh = A.shi[s] - A.obj0;
          if (hh > l && hh > x) {
            const uint32_t ba = l > x ? (uint32_t)(l - x) : 0u;
            const uint32_t bb = hh - x < 16u ? (uint32_t)(hh - x) : 16u;
            const uint32_t bits = (0xFFFFu >> (16u - bb)) & (0xFFFFu << ba);
            uint32_t n1 = nl & bits;
            const uint64_t k = s - s0;
            if (PASS == 1) {
              const uint32_t cn = (uint32_t)__popc(n1), cc = (uint32_t)__popc(cr & bits);
              if (k < (uint64_t)kSlots) {
                if (cn) {
                  atomicAdd(&s_a[k], cn);
                  atomicMin(&s_c[k], (uint32_t)(x - x0) + (uint32_t)__builtin_ctz(n1));
                }
                if (cc) atomicAdd(&s_b[k], cc);
              } else {
                if (cn) {
                  atomicAdd(A.o0 + s, (unsigned long long)cn);
                  atomicMin(A.o2 + s, (unsigned long long)(A.obj0 + x + (uint32_t)__builtin_ctz(n1)));
                }
                if (cc) atomicAdd(A.o1 + s, (unsigned long long)cc);
              }
            } else if (n1) {
              const uint64_t org = A.sorg[s];
              const uint32_t wid = A.swid[s];
              uint32_t c2 = 0, last = 0;
              while (n1) {
                const uint32_t bit = (uint32_t)__builtin_ctz(n1);
                n1 &= n1 - 1u;
                if (off_grid(A.obj0 + x + bit, org, wid)) {
                  ++c2;
                  last = bit + 1u;
                }
              }
              if (c2) {
                if (k < (uint64_t)kSlots) {
                  atomicAdd(&s_a[k], c2);
                  atomicMax(&s_b[k], (uint32_t)(x - x0) + last);
                } else {
                  atomicAdd(A.o0 + s, (unsigned long long)c2);
                  atomicMax(A.o1 + s, (unsigned long long)(A.obj0 + x + last - 1u));
                }
              }
            }
          }
          if (hh >= x + 16u) break;
          ++s;
        }
        seg = s;
      }
    }
    // ---- flush the touched slots (the range's segments, at most kSlots) and leave them initialised
    wave_sync();
    const uint64_t nk = s1 - s0 < (uint64_t)kSlots ? s1 - s0 : (uint64_t)kSlots;
    for (uint64_t k = lane; k < nk; k += kWave) {
      const uint32_t a = s_a[k], b = s_b[k];
      if (PASS == 1) {
        const uint32_t c = s_c[k];
        if (a) {
          atomicAdd(A.o0 + s0 + k, (unsigned long long)a);
          atomicMin(A.o2 + s0 + k, (unsigned long long)(A.obj0 + x0 + c));
          s_a[k] = 0u;
          s_c[k] = kNone32;
        }
        if (b) {
          atomicAdd(A.o1 + s0 + k, (unsigned long long)b);
          s_b[k] = 0u;
        }
      } else if (a) {
        atomicAdd(A.o0 + s0 + k, (unsigned long long)a);
        atomicMax(A.o1 + s0 + k, (unsigned long long)(A.obj0 + x0 + b - 1u));
        s_a[k] = 0u;
        s_b[k] = 0u;
      }
    }
    wave_sync();
  }
}

struct NameArgs {
  const uint8_t* buf;
  uint64_t buf_len, buf_base;
  const unsigned long long* start;
  const unsigned long long* end;     // length launch
  const unsigned long long* off;     // copy launch
  uint32_t* len;
  uint64_t n;
  uint8_t* out;
  uint64_t out_cap;
};

// COPY 0: one lane per header, the length of its name.  COPY 1: one wave per header, its name bytes to out + off.
template <int COPY>
__global__ void __launch_bounds__(256) fai_name_kernel(NameArgs A) {
  if (COPY == 0) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= A.n) return;
    const uint64_t top = A.buf_base + A.buf_len;
    uint64_t p = A.start[i] + 1u, e = A.end[i];
    if (e > top) e = top;
    uint64_t q = p;
    if (p >= A.buf_base + 1u) {
      for (; q < e; ++q) {
        const uint8_t c = A.buf[q - A.buf_base];
        if (c == ' ' || c == '\t' || c == '\r' || c == '\n') break;
      }
    }
    const uint64_t len = q - p;
    A.len[i] = len > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)len;
  } else {
    const uint64_t i = (uint64_t)blockIdx.x * (blockDim.x / kWave) + (threadIdx.x / kWave);
    if (i >= A.n) return;
    const uint64_t p = A.start[i] + 1u, o = A.off[i];
    const uint32_t len = A.len[i];
    if (p < A.buf_base) return;
    for (uint32_t j = threadIdx.x % kWave; j < len; j += kWave) {
      const uint64_t src = p + j - A.buf_base;
      if (src < A.buf_len && o + j < A.out_cap && o + j >= o) A.out[o + j] = A.buf[src];
    }
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
      return fail(DFAI_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));        \
  } while (0)

}  // namespace

struct dfai_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  int grid = 0;                       // one-wave workgroups of the persistent grid
};

extern "C" {

int dfai_abi_version(void) { return DFAI_ABI_VERSION; }

const char* dfai_last_error(void) { return g_err.c_str(); }

int dfai_ctx_create(int device, void* stream, dfai_ctx** out) {
  if (!out) return fail(DFAI_ERR_INVALID, "null out");
  *out = nullptr;
  int n = 0;
  HIPCHK(hipGetDeviceCount(&n));
  if (device < 0 || device >= n) return fail(DFAI_ERR_INVALID, "device " + std::to_string(device) + " out of range");
  HIPCHK(hipSetDevice(device));
  hipDeviceProp_t prop;
  HIPCHK(hipGetDeviceProperties(&prop, device));
  int occ = 0, occ2 = 0;
  HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, fai_count_kernel<1>, kWave, 0));
  HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ2, fai_count_kernel<2>, kWave, 0));
  if (occ2 < occ) occ = occ2;
  if (occ < 1) return fail(DFAI_ERR_HIP, "fai_count_kernel: no resident workgroup per CU");
  if (occ > kMaxWavesPerCU) occ = kMaxWavesPerCU;
  dfai_ctx* c = new dfai_ctx();
  c->device = device;
  c->stream = (hipStream_t)stream;
  // the grid need not be resident (no workgroup waits on another); this size merely fills the chip
  c->grid = prop.multiProcessorCount * occ;
  *out = c;
  return DFAI_OK;
}

int dfai_ctx_destroy(dfai_ctx* c) {
  if (!c) return DFAI_OK;
  (void)hipSetDevice(c->device);
  (void)hipStreamSynchronize(c->stream);
  delete c;
  return DFAI_OK;
}

// The launch behind both passes.  pass 1: o0 nl, o1 cr, o2 first; pass 2: o0 off, o1 lastoff.
static int count_launch(dfai_ctx* c, int pass, const uint8_t* d_buf, uint64_t buf_len, uint64_t buf_base,
                        const uint64_t* d_lo, const uint64_t* d_hi, const uint64_t* d_origin,
                        const uint32_t* d_width, uint64_t n, uint64_t* o0, uint64_t* o1, uint64_t* o2) {
  if (!c) return fail(DFAI_ERR_INVALID, "null ctx");
  if (buf_len && !d_buf) return fail(DFAI_ERR_INVALID, "null buffer");
  if (buf_base + buf_len < buf_base) return fail(DFAI_ERR_INVALID, "the buffer wraps the offset space");
  if (n >= (1ull << 40)) return fail(DFAI_ERR_INVALID, "too many segments");
  if (n && (!d_lo || !d_hi || !d_origin || !o0 || !o1 || (pass == 1 && !o2) || (pass == 2 && !d_width)))
    return fail(DFAI_ERR_INVALID, "null segment or output array");
  if (((uintptr_t)d_lo | (uintptr_t)d_hi | (uintptr_t)d_origin | (uintptr_t)o0 | (uintptr_t)o1 | (uintptr_t)o2) & 7u)
    return fail(DFAI_ERR_INVALID, "misaligned segment or output array");
  if ((uintptr_t)d_width & 3u) return fail(DFAI_ERR_INVALID, "misaligned width array");
  HIPCHK(hipSetDevice(c->device));
  if (n == 0) return DFAI_OK;
  HIPCHK(hipMemsetAsync(o0, 0, n * sizeof(uint64_t), c->stream));
  HIPCHK(hipMemsetAsync(o1, 0, n * sizeof(uint64_t), c->stream));
  if (pass == 1) HIPCHK(hipMemsetAsync(o2, 0xFF, n * sizeof(uint64_t), c->stream));
  if (buf_len == 0) return DFAI_OK;
  const uint64_t shift = (uint64_t)((uintptr_t)d_buf & 15u);
  CountArgs a;
  a.base = (const uint8_t*)((uintptr_t)d_buf - (uintptr_t)shift);
  a.lo = shift;
  a.hi = shift + buf_len;
  a.obj0 = buf_base - shift;
  a.nranges = (a.hi + kRangeBytes - 1) / kRangeBytes;
  a.slo = (const unsigned long long*)d_lo;
  a.shi = (const unsigned long long*)d_hi;
  a.sorg = (const unsigned long long*)d_origin;
  a.swid = d_width;
  a.n = n;
  a.o0 = (unsigned long long*)o0;
  a.o1 = (unsigned long long*)o1;
  a.o2 = (unsigned long long*)o2;
  const unsigned grid = (unsigned)(a.nranges < (uint64_t)c->grid ? a.nranges : (uint64_t)c->grid);
  if (pass == 1) hipLaunchKernelGGL((fai_count_kernel<1>), dim3(grid), dim3(kWave), 0, c->stream, a);
  else hipLaunchKernelGGL((fai_count_kernel<2>), dim3(grid), dim3(kWave), 0, c->stream, a);
  HIPCHK(hipGetLastError());
  return DFAI_OK;
}

int dfai_count_async(dfai_ctx* c, const uint8_t* d_buf, uint64_t buf_len, uint64_t buf_base, const uint64_t* d_lo,
                     const uint64_t* d_hi, const uint64_t* d_origin, uint64_t n, uint64_t* d_nl, uint64_t* d_cr,
                     uint64_t* d_first) {
  return count_launch(c, 1, d_buf, buf_len, buf_base, d_lo, d_hi, d_origin, nullptr, n, d_nl, d_cr, d_first);
}

int dfai_offgrid_async(dfai_ctx* c, const uint8_t* d_buf, uint64_t buf_len, uint64_t buf_base, const uint64_t* d_lo,
                       const uint64_t* d_hi, const uint64_t* d_origin, const uint32_t* d_width, uint64_t n,
                       uint64_t* d_off, uint64_t* d_lastoff) {
  return count_launch(c, 2, d_buf, buf_len, buf_base, d_lo, d_hi, d_origin, d_width, n, d_off, d_lastoff, nullptr);
}

static int name_launch(dfai_ctx* c, int copy, const uint8_t* d_buf, uint64_t buf_len, uint64_t buf_base,
                       const uint64_t* d_start, const uint64_t* d_end, const uint64_t* d_off, uint32_t* d_len,
                       uint64_t n, uint8_t* d_out, uint64_t out_cap) {
  if (!c) return fail(DFAI_ERR_INVALID, "null ctx");
  if (buf_len && !d_buf) return fail(DFAI_ERR_INVALID, "null buffer");
  if (buf_base + buf_len < buf_base) return fail(DFAI_ERR_INVALID, "the buffer wraps the offset space");
  if (n >= (1ull << 31) * 4) return fail(DFAI_ERR_INVALID, "too many headers for one launch");
  if (n && (!d_start || !d_len || (copy ? !d_off || (out_cap && !d_out) : !d_end)))
    return fail(DFAI_ERR_INVALID, "null header or output array");
  if ((((uintptr_t)d_start | (uintptr_t)d_end | (uintptr_t)d_off) & 7u) || ((uintptr_t)d_len & 3u))
    return fail(DFAI_ERR_INVALID, "misaligned header or output array");
  HIPCHK(hipSetDevice(c->device));
  if (n == 0) return DFAI_OK;
  NameArgs a;
  a.buf = d_buf;
  a.buf_len = buf_len;
  a.buf_base = buf_base;
  a.start = (const unsigned long long*)d_start;
  a.end = (const unsigned long long*)d_end;
  a.off = (const unsigned long long*)d_off;
  a.len = d_len;
  a.n = n;
  a.out = d_out;
  a.out_cap = out_cap;
  if (copy) hipLaunchKernelGGL((fai_name_kernel<1>), dim3((unsigned)((n + 3) / 4)), dim3(256), 0, c->stream, a);
  else hipLaunchKernelGGL((fai_name_kernel<0>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, a);
  HIPCHK(hipGetLastError());
  return DFAI_OK;
}

int dfai_name_len_async(dfai_ctx* c, const uint8_t* d_buf, uint64_t buf_len, uint64_t buf_base,
                        const uint64_t* d_start, const uint64_t* d_end, uint64_t n, uint32_t* d_len) {
  return name_launch(c, 0, d_buf, buf_len, buf_base, d_start, d_end, nullptr, d_len, n, nullptr, 0);
}

int dfai_name_copy_async(dfai_ctx* c, const uint8_t* d_buf, uint64_t buf_len, uint64_t buf_base,
                         const uint64_t* d_start, const uint32_t* d_len, const uint64_t* d_off, uint64_t n,
                         uint8_t* d_out, uint64_t out_cap) {
  return name_launch(c, 1, d_buf, buf_len, buf_base, d_start, nullptr, d_off, const_cast<uint32_t*>(d_len), n, d_out,
                     out_cap);
}

int dfai_geometry(dfai_ctx* c, int* range_bytes, int* slots, int* grid_waves) {
  if (!c) return fail(DFAI_ERR_INVALID, "null ctx");
  if (range_bytes) *range_bytes = kRangeBytes;
  if (slots) *slots = kSlots;
  if (grid_waves) *grid_waves = c->grid;
  return DFAI_OK;
}

}  // extern "C"
