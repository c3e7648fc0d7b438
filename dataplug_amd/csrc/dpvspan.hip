// dpvspan.hip — MI355X (gfx950, CDNA4) record ends of the lines of a VCF body + the C ABI of libdpvspan.so
// (include/dpvspan.h, which holds the definition).
//
// vspan_span_kernel: one lane per line.  The lane walks its line from the start as aligned 16-byte chunks (four
// guarded dwords where a chunk crosses the buffer's first or last dword), the next chunk loaded before the current
// one is looked at.  A dword that holds no '\t' and no '\n' (carry-free zero-byte masks) is passed over whole outside
// INFO, and inside INFO too while the walk is in an entry other than the END entry and the dword holds no ';'; the
// others go byte by byte through a small state: the tab count, field 4's start and length, and inside
// field 8 the position in an "END=" match at an entry's start, then the digits of its value.  The walk stops at an
// empty field 4, at field 8's end, at the line's end or at the buffer's end.  One lane may walk a REF of tens of
// kilobytes or an INFO of kilobytes while the other 63 of its wave idle: accepted for this version.
// vspan_blockmax_kernel: one lane per line, kRounds rounds of kBlock lines a workgroup.  The lines' slots never
// decrease along the lanes, so a wave reduces the ends of equal slots with shuffles (a segmented max) and only a
// segment's first lane touches the slot: a plain store for K = 1, one atomicMax otherwise.  Counts, lowest indices and
// the largest span are kept per lane over the rounds, reduced in the wave, then across the waves in LDS, and one lane
// of the workgroup does the atomics on the result words.
// No workgroup ever waits on another: no look-back, no spin, no flag, no ticket -- only atomics on slots and result
// words that are initialised on the stream at every launch.  Loads are plain loads with compiler-placed waits; outputs
// are ordinary vector stores and atomics.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "../../include/dpvspan.h"

namespace {

constexpr int kWave = 64;
constexpr int kBlock = 256;                        // lines per workgroup of the span kernel
constexpr int kRounds = 4;                         // the block-max kernel: kBlock * kRounds lines per workgroup
constexpr int kMaxLines = kBlock * kRounds;

struct SpanArgs {
  const uint8_t* base;         // 16-byte aligned; the coordinates below are relative to it
  uint64_t lo, hi;             // the buffer's bytes below the object's end: coordinates [lo, hi), lo in 0..15
  uint64_t buf_base;           // object offset of coordinate lo
  uint32_t eof;                // coordinate hi is the object's end: a line that reaches it ends there
  const unsigned long long* starts;
  const uint32_t* pos_in;
  uint64_t n;
  uint32_t* end;
  uint8_t* flags;
};

struct Chunk {
  uint32_t w[4];
};

// the 16 bytes at coordinate a (a multiple of 16); dwords wholly outside [lo, hi) rounded out to dwords read as 0
__host__ __device__ __forceinline__ Chunk load_chunk(const uint8_t* base, uint64_t a, uint64_t lo, uint64_t hi) {
  Chunk c;
  if (a >= (lo & ~3ull) && a + 16 <= ((hi + 3) & ~3ull)) {
    const uint4 v = *reinterpret_cast<const uint4*>(base + a);
    c.w[0] = v.x, c.w[1] = v.y, c.w[2] = v.z, c.w[3] = v.w;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const uint64_t q = a + 4 * k;
      c.w[k] = (q + 4 > lo && q < hi) ? *reinterpret_cast<const uint32_t*>(base + q) : 0u;
    }
  }
  return c;
}

// 0x80 in every byte of v that is zero, exactly (no carry crosses a byte)
__host__ __device__ __forceinline__ uint32_t zero_bytes(uint32_t v) {
  return ~(((v & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | v | 0x7F7F7F7Fu);
}

// rec_end and the flags of the line that starts at coordinate c in [lo, hi), with POS = pos
__host__ __device__ __forceinline__ void span_line(const uint8_t* base, uint64_t lo, uint64_t hi, bool eof, uint64_t c,
                                                   uint32_t pos, uint32_t& out_end, uint32_t& out_flags) {
  uint32_t tabs = 0;             // tabs seen: the walk is in field tabs + 1
  uint64_t f4 = 0, reflen = 0;   // field 4's first coordinate, its length once tab 4 or the line's end is seen
  uint32_t m = 0;                // inside INFO: 0..3 bytes of "END=" matched at an entry's start, 4 in its value,
                                 // 5 in another entry, 6 the END entry is behind
  uint64_t val = 0;
  uint32_t nd = 0, bad = 0, counts = 0;
  uint32_t stop = 0;             // 1 MISSING_REF, 2 field 8's end, 3 the line's end
  uint64_t e = hi;               // the line's end, where it is seen
  uint64_t a = c & ~15ull;
  Chunk cur = load_chunk(base, a, lo, hi);
  while (!stop && a < hi) {
    const uint64_t an = a + 16;
    Chunk nxt;
    nxt.w[0] = nxt.w[1] = nxt.w[2] = nxt.w[3] = 0;
    if (an < hi) nxt = load_chunk(base, an, lo, hi);     // in flight while this chunk is looked at
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const uint64_t q0 = a + 4 * k;
      if (stop || q0 + 4 <= c || q0 >= hi) continue;
      const uint32_t w = cur.w[k];
      const bool whole = q0 >= c && q0 + 4 <= hi;
      // no tab and no newline: nothing to see outside INFO, nor inside it in an entry that is not the END entry
      // (states 5 and 6) unless a ';' ends that entry
      if (whole && (zero_bytes(w ^ 0x09090909u) | zero_bytes(w ^ 0x0A0A0A0Au)) == 0 &&
          (tabs != 7 || (m >= 5 && zero_bytes(w ^ 0x3B3B3B3Bu) == 0)))
        continue;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const uint64_t q = q0 + j;
        if (stop || q < c || q >= hi) continue;
        const uint32_t b = (w >> (8 * j)) & 0xFFu;
        if (b == '\n') {
          stop = 3;
          e = q;
        } else if (b == '\t') {
          ++tabs;
          if (tabs == 3) {
            f4 = q + 1;
          } else if (tabs == 4) {
            reflen = q - f4;
            if (reflen == 0) stop = 1;
          } else if (tabs == 7) {
            m = 0;
          } else if (tabs == 8) {
            stop = 2;
          }
        } else if (tabs == 7) {
          if (b == ';') {
            if (m == 4) {
              counts = !bad && nd >= 1u && val <= (uint64_t)VSPAN_END_MAX && val >= pos;
              m = 6;
            } else if (m != 6) {
              m = 0;
            }
          } else if (m < 4) {
            m = (b == ((0x3D444E45u >> (8 * m)) & 0xFFu)) ? m + 1 : 5u;   // 'E' 'N' 'D' '='
          } else if (m == 4) {
            if (b - '0' < 10u && nd < 10u) {
              val = val * 10u + (b - '0');
              ++nd;
            } else {
              bad = 1;                             // a non-digit, or an eleventh digit
            }
          }
        }
      }
    }
    cur = nxt;
    a = an;
  }
  if (!stop && !eof) {                             // the buffer ended first
    out_end = 0;
    out_flags = VSPAN_TRUNCATED;
    return;
  }
  if (stop != 1 && stop != 2) {                    // the line's end: its '\n' or the object's end
    if (tabs < 3) {
      stop = 1;
    } else if (tabs == 3) {
      reflen = e - f4;
      if (reflen == 0) stop = 1;
    }
  }
  if (stop == 1) {
    out_end = 0;
    out_flags = VSPAN_MISSING_REF;
    return;
  }
  if (m == 4) counts = !bad && nd >= 1u && val <= (uint64_t)VSPAN_END_MAX && val >= pos;   // the entry ended INFO
  if (counts) {
    out_end = (uint32_t)val;
    out_flags = VSPAN_FROM_END;
  } else {
    const uint64_t r = (uint64_t)pos + reflen - 1;
    out_end = r > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)r;
    out_flags = 0;
  }
}

__global__ void __launch_bounds__(kBlock) vspan_span_kernel(SpanArgs A) {
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= A.n) return;
  const uint64_t s = A.starts[i];
  uint32_t end = 0, fl = VSPAN_TRUNCATED;          // a start outside the buffer (or at / past the object's end)
  if (s >= A.buf_base && s - A.buf_base < A.hi - A.lo)
    span_line(A.base, A.lo, A.hi, A.eof != 0, s - A.buf_base + A.lo, A.pos_in[i], end, fl);
  A.end[i] = end;
  A.flags[i] = (uint8_t)fl;
}

struct MaxArgs {
  const uint32_t* end;
  const uint8_t* flags;
  const uint32_t* pos;
  uint64_t n, ordinal0, slot0;   // slot0 = ordinal0 / every
  uint32_t mask, shift;          // every - 1, log2(every)
  uint32_t* blockmax;
  unsigned long long* res;
};

__device__ __forceinline__ uint64_t shfl_down_u64(uint64_t v, int d) {
  return (uint64_t)__shfl_down((long long)v, d, kWave);
}

__global__ void __launch_bounds__(kBlock) vspan_blockmax_kernel(MaxArgs A) {
  __shared__ unsigned long long sh[kBlock / kWave][DVS_R_WORDS];
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  uint64_t n_mis = 0, n_tru = 0, n_end = 0, span = 0, min_mis = DVS_NONE, min_tru = DVS_NONE;
  for (int r = 0; r < kRounds; ++r) {              // no lane leaves early: the shuffles want the whole wave
    const uint64_t i = ((uint64_t)blockIdx.x * kRounds + r) * kBlock + threadIdx.x;
    const bool in = i < A.n;
    const uint32_t f = in ? A.flags[i] : 0u;
    uint32_t v = in ? A.end[i] : 0u;
    const uint64_t slot = in ? ((A.ordinal0 + i) >> A.shift) - A.slot0 : DVS_NONE;
    if (in) {
      if (f & VSPAN_MISSING_REF) {
        ++n_mis;
        if (i < min_mis) min_mis = i;
      }
      if (f & VSPAN_TRUNCATED) {
        ++n_tru;
        if (i < min_tru) min_tru = i;
      }
      if (f & VSPAN_FROM_END) ++n_end;
      if (!(f & (VSPAN_MISSING_REF | VSPAN_TRUNCATED))) {
        const uint32_t p = A.pos[i];
        if (v >= p && (uint64_t)(v - p) > span) span = v - p;
      }
    }
    if (A.mask == 0) {                             // K = 1: every line is its own slot
      if (in) A.blockmax[slot] = v;
      continue;
    }
    const uint64_t before = (uint64_t)__shfl_up((long long)slot, 1, kWave);
    const bool head = in && (lane == 0 || before != slot);
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {          // the slots never decrease along the lanes: a segmented max
      const uint32_t ov = (uint32_t)__shfl_down((int)v, d, kWave);
      const uint64_t os = shfl_down_u64(slot, d);
      if (lane + d < kWave && os == slot && ov > v) v = ov;
    }
    if (head && v) atomicMax(A.blockmax + slot, v);
  }
#pragma unroll
  for (int d = kWave / 2; d > 0; d >>= 1) {
    n_mis += shfl_down_u64(n_mis, d);
    n_tru += shfl_down_u64(n_tru, d);
    n_end += shfl_down_u64(n_end, d);
    const uint64_t s2 = shfl_down_u64(span, d), a2 = shfl_down_u64(min_mis, d), b2 = shfl_down_u64(min_tru, d);
    span = s2 > span ? s2 : span;
    min_mis = a2 < min_mis ? a2 : min_mis;
    min_tru = b2 < min_tru ? b2 : min_tru;
  }
  if (lane == 0) {
    sh[wave][DVS_R_MISSING] = n_mis;
    sh[wave][DVS_R_TRUNCATED] = n_tru;
    sh[wave][DVS_R_FROM_END] = n_end;
    sh[wave][DVS_R_MAX_SPAN] = span;
    sh[wave][DVS_R_MIN_MISSING] = min_mis;
    sh[wave][DVS_R_MIN_TRUNCATED] = min_tru;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < kBlock / kWave; ++w) {
      n_mis += sh[w][DVS_R_MISSING];
      n_tru += sh[w][DVS_R_TRUNCATED];
      n_end += sh[w][DVS_R_FROM_END];
      if (sh[w][DVS_R_MAX_SPAN] > span) span = sh[w][DVS_R_MAX_SPAN];
      if (sh[w][DVS_R_MIN_MISSING] < min_mis) min_mis = sh[w][DVS_R_MIN_MISSING];
      if (sh[w][DVS_R_MIN_TRUNCATED] < min_tru) min_tru = sh[w][DVS_R_MIN_TRUNCATED];
    }
    if (n_mis) {
      atomicAdd(A.res + DVS_R_MISSING, (unsigned long long)n_mis);
      atomicMin(A.res + DVS_R_MIN_MISSING, (unsigned long long)min_mis);
    }
    if (n_tru) {
      atomicAdd(A.res + DVS_R_TRUNCATED, (unsigned long long)n_tru);
      atomicMin(A.res + DVS_R_MIN_TRUNCATED, (unsigned long long)min_tru);
    }
    if (n_end) atomicAdd(A.res + DVS_R_FROM_END, (unsigned long long)n_end);
    if (span) atomicMax(A.res + DVS_R_MAX_SPAN, (unsigned long long)span);
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
      return fail(DVS_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));         \
  } while (0)

}  // namespace

struct dvs_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
};

extern "C" {

int dvs_abi_version(void) { return DVS_ABI_VERSION; }

const char* dvs_last_error(void) { return g_err.c_str(); }

int dvs_ctx_create(int device, void* stream, dvs_ctx** out) {
  if (!out) return fail(DVS_ERR_INVALID, "null out");
  *out = nullptr;
  int n = 0;
  HIPCHK(hipGetDeviceCount(&n));
  if (device < 0 || device >= n) return fail(DVS_ERR_INVALID, "device " + std::to_string(device) + " out of range");
  HIPCHK(hipSetDevice(device));
  dvs_ctx* c = new dvs_ctx();
  c->device = device;
  c->stream = (hipStream_t)stream;
  *out = c;
  return DVS_OK;
}

int dvs_ctx_destroy(dvs_ctx* c) {
  if (!c) return DVS_OK;
  (void)hipSetDevice(c->device);
  (void)hipStreamSynchronize(c->stream);
  delete c;
  return DVS_OK;
}

int dvs_span_async(dvs_ctx* c, const uint8_t* d_buf, uint64_t buf_len, uint64_t buf_base, uint64_t size,
                   const uint64_t* d_starts, uint64_t n, const uint32_t* d_pos, uint32_t* d_end, uint8_t* d_flags) {
  if (!c) return fail(DVS_ERR_INVALID, "null ctx");
  if (buf_len && !d_buf) return fail(DVS_ERR_INVALID, "null buffer");
  if (buf_base + buf_len < buf_base) return fail(DVS_ERR_INVALID, "the buffer wraps the offset space");
  if (n >= (1ull << 32)) return fail(DVS_ERR_INVALID, "too many lines for one launch");
  if (n && (!d_starts || !d_pos || !d_end || !d_flags)) return fail(DVS_ERR_INVALID, "null line or output array");
  if (((uintptr_t)d_starts & 7u) || (((uintptr_t)d_pos | (uintptr_t)d_end) & 3u))
    return fail(DVS_ERR_INVALID, "misaligned line or output array");
  HIPCHK(hipSetDevice(c->device));
  if (n == 0) return DVS_OK;
  const uint64_t shift = (uint64_t)((uintptr_t)d_buf & 15u);
  uint64_t len = buf_len;                          // the buffer's bytes below the object's end
  if (size <= buf_base) len = 0;
  else if (size - buf_base < len) len = size - buf_base;
  SpanArgs a;
  a.base = (const uint8_t*)((uintptr_t)d_buf - (uintptr_t)shift);
  a.lo = shift;
  a.hi = shift + len;
  a.buf_base = buf_base;
  a.eof = (size >= buf_base && buf_base + len == size) ? 1u : 0u;
  a.starts = (const unsigned long long*)d_starts;
  a.pos_in = d_pos;
  a.n = n;
  a.end = d_end;
  a.flags = d_flags;
  hipLaunchKernelGGL(vspan_span_kernel, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, c->stream, a);
  HIPCHK(hipGetLastError());
  return DVS_OK;
}

int dvs_blockmax_async(dvs_ctx* c, const uint32_t* d_end, const uint8_t* d_flags, const uint32_t* d_pos, uint64_t n,
                       uint64_t ordinal0, uint32_t every, uint32_t* d_blockmax, uint64_t* d_result) {
  if (!c) return fail(DVS_ERR_INVALID, "null ctx");
  if (every == 0 || (every & (every - 1))) return fail(DVS_ERR_INVALID, "every must be a power of two");
  if (n >= (1ull << 32)) return fail(DVS_ERR_INVALID, "too many lines for one launch");
  if (ordinal0 + n < ordinal0) return fail(DVS_ERR_INVALID, "the ordinals wrap");
  if (!d_result) return fail(DVS_ERR_INVALID, "null result");
  if (n && (!d_end || !d_flags || !d_pos || !d_blockmax)) return fail(DVS_ERR_INVALID, "null line or slot array");
  if (((uintptr_t)d_result & 7u) || (((uintptr_t)d_end | (uintptr_t)d_pos | (uintptr_t)d_blockmax) & 3u))
    return fail(DVS_ERR_INVALID, "misaligned line, slot or result array");
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipMemsetAsync(d_result, 0, DVS_R_MIN_MISSING * sizeof(uint64_t), c->stream));
  HIPCHK(hipMemsetAsync(d_result + DVS_R_MIN_MISSING, 0xFF, (DVS_R_WORDS - DVS_R_MIN_MISSING) * sizeof(uint64_t),
                        c->stream));
  if (n == 0) return DVS_OK;
  MaxArgs a;
  a.end = d_end;
  a.flags = d_flags;
  a.pos = d_pos;
  a.n = n;
  a.ordinal0 = ordinal0;
  a.mask = every - 1u;
  a.shift = (uint32_t)__builtin_ctz(every);
  a.slot0 = ordinal0 >> a.shift;
  a.blockmax = d_blockmax;
  a.res = (unsigned long long*)d_result;
  const uint64_t slots = ((ordinal0 + n - 1) >> a.shift) - a.slot0 + 1;
  HIPCHK(hipMemsetAsync(d_blockmax, 0, slots * sizeof(uint32_t), c->stream));
  hipLaunchKernelGGL(vspan_blockmax_kernel, dim3((unsigned)((n + kMaxLines - 1) / kMaxLines)), dim3(kBlock), 0,
                     c->stream, a);
  HIPCHK(hipGetLastError());
  return DVS_OK;
}

int dvs_geometry(dvs_ctx* c, int* span_lines, int* blockmax_lines) {
  if (!c) return fail(DVS_ERR_INVALID, "null ctx");
  if (span_lines) *span_lines = kBlock;
  if (blockmax_lines) *blockmax_lines = kMaxLines;
  return DVS_OK;
}

}  // extern "C"
