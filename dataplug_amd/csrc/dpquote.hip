// dpquote.hip — MI355X (gfx950, CDNA4) quote-aware CSV record index + the C ABI of libdpquote.so (include/dpquote.h).
//
// One kernel, one pass over the bytes (DESIGN.md §Quote-aware record index).  A 256-lane workgroup claims 64 KiB
// tiles from a global ticket; each of its 4 waves owns 16 KiB of the tile, 16 rows of one 16-byte chunk per lane:
//   phase A  per chunk a quote mask and a newline mask (16 bits each), the in-chunk prefix XOR of the quote mask, the
//            lane's exclusive quote parity in the row from one ballot; the newlines kept if the wave is entered
//            outside / inside a quoted field stay in one VGPR per row, the bytes themselves are dropped;
//   scan     the wave summaries (parity, kept0, kept1) compose into the tile's; wave 0 publishes it as an AGG
//            descriptor and resolves the tile's incoming (state, output base) by a decoupled look-back over the
//            descriptors of the tiles before it, 64 per step, then publishes the inclusive PREFIX;
//   phase B  every lane keeps nl & ~(inside ^ state_in) and stores its offsets at base + exclusive popcount scan.
// The house rules of dpscan.hip hold: tiles are claimed from the ticket by running workgroups only (a wait only ever
// depends on a tile that a running or finished workgroup owns: no co-residency assumption); every inter-workgroup
// wait is bounded in time (20 s of the realtime counter, DQ_ERR_TIMEOUT, the waiters are released); the ticket, the
// result words and the descriptors are zeroed per launch on the stream; outputs are ordinary vector stores.
//
// Three output forms of the one kernel template: uint32 and uint64 object offsets (tiles start at the 16-byte boundary
// at or below the range's first byte), and the blocked form u16b (dq_records_blocked_async): tiles lie on the object's
// 64 KiB grid, so a record end's uint16 low word is its position in the tile and the block table entry of a tile is
// the exclusive base its look-back resolves anyway.
//
// Escape-aware variant (second template parameter, dq_records_esc_async / dq_records_esc_blocked_async): a byte that
// follows an unescaped escape byte is literal.  The "this byte is escaped" bit is resolved before the masks are
// summarized -- escaped quotes leave the quote mask, under scope "all" escaped newlines leave the newline mask -- so
// the summaries, the descriptors, the look-back and phase B are those of the plain kernel.  Inside a chunk the escaped
// bytes come from one add-carry over the escape mask; across the lanes of a row from two ballots (all-escape chunks
// pass the incoming bit on, every other chunk sets it to the parity of its trailing escape run); across rows from
// scalar work on those ballots; and at its 16 KiB start a wave reads the chunks just before it, walking further back
// only while they hold nothing but escape bytes (at most DQ_ESCAPE_RUN_MAX bytes, then DQ_ERR_ESCAPE_RUN: no wait).

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <type_traits>

#include "../../include/dpquote.h"

namespace {

constexpr int kWave = 64;
constexpr int kWaves = 4;
constexpr int kThreads = kWave * kWaves;           // 256
constexpr int kRowBytes = kWave * 16;              // one 16-byte chunk per lane
constexpr int kRows = 16;                          // rows per wave
constexpr int kHalf = kRows / 2;                   // rows per load batch (32 VGPRs of destinations)
constexpr int kWaveBytes = kRowBytes * kRows;      // 16 KiB
constexpr int kTileBytes = kWaveBytes * kWaves;    // 64 KiB
constexpr int kMaxBlocksPerCU = 8;                 // 32 waves per CU
static_assert(kWaveBytes <= 0xFFFF, "wave counts are packed in 16 bits");

constexpr uint32_t kSel12 = 0x0C0C0C0Cu;           // v_perm selector that yields 0x00
constexpr uint32_t kErrTimeout = 1u;
constexpr uint32_t kErrOverflow = 2u;
constexpr uint32_t kErrEscapeRun = 4u;
constexpr uint32_t kOddBits = 0xAAAAAAAAu;
// a wave's walk back over all-escape chunks: whole windows of 64 chunks, then the one chunk beyond the bound
constexpr uint32_t kEscWindows = (uint32_t)(DQ_ESCAPE_RUN_MAX / (64 * 16));
static_assert(DQ_ESCAPE_RUN_MAX % (64 * 16) == 0 && DQ_ESCAPE_RUN_MAX >= (1 << 16) + 16,
              "the bound is whole windows and at least a tile plus a chunk");

// Descriptor word (one 64-bit atomic store, zero = not published):
//   AGG     bits 0..23 kept0, 24..47 kept1, 48 parity  -- the tile as a function of its incoming state
//   PREFIX  bits 0..47 record ends up to and including the tile, 48 the state after it
constexpr uint64_t kStatAgg = 1ull << 62;
constexpr uint64_t kStatPrefix = 2ull << 62;
constexpr uint64_t kCountMask = 0xFFFFFFFFFFFFull;

// control words at the head of the workspace (uint64 each), descriptors follow at kCtrlWords
constexpr int kCtrlTicket = 0, kCtrlErr = 1, kCtrlOut = 2, kCtrlQuotes = 3, kCtrlNewlines = 4;
constexpr int kCtrlToggles = 5;                      // escape-aware launches: the quotes that are not escaped
constexpr int kCtrlWords = 8;

constexpr uint64_t kWaitTicks = 100000000ull * 20;   // 20 s of the 100 MHz realtime counter
constexpr uint32_t kPollCheck = 255u;                // check the clock every 256 polls
__device__ __forceinline__ bool wait_expired(uint32_t spins, uint64_t& t0) {
  if ((spins & kPollCheck) != kPollCheck) return false;
  const uint64_t t = __builtin_amdgcn_s_memrealtime();
  if (t0 == 0) {
    t0 = t;
    return false;
  }
  return t - t0 > kWaitTicks;
}

struct QuoteArgs {
  const uint8_t* base;         // 16-byte aligned; coordinates below are relative to it (blocked form: it may lie
                               // before the allocation; only chunks that hold a byte of [lo, hi) are loaded)
  uint64_t lo, hi;             // the bytes to scan: [lo, hi), lo in 0..15 (blocked form: 0..65535)
  uint64_t obj0;               // object offset of coordinate 0 (mod 2^64: only coordinates >= lo are emitted)
  uint64_t ntiles;
  uint32_t key_q, key_nl;      // match4 keys of the quote byte and of '\n'
  uint32_t carry;
  void* out;
  uint64_t cap;
  unsigned long long* table;   // blocked form: ntiles entries, the record ends of the launch before each tile
  unsigned long long* ctrl;    // kCtrlWords control words, then ntiles descriptors
  // escape-aware launches only
  uint32_t key_e;              // match4 key of the escape byte
  uint32_t esc_carry;          // 1: the byte at lo is escaped
  uint32_t esc_nl;             // 0xFFFF: an escaped '\n' is no record end (scope "all"); 0: scope "quoted"
};

// 0x00 in every byte of w that equals the key's pattern byte, 0xFF in every other byte (exact).
__device__ __forceinline__ uint32_t match4(uint32_t w, uint32_t key) {
  return __builtin_amdgcn_perm(0xFFFFFFFFu, 0xFFFFFFFFu, w ^ key);
}
// match4 bytes of a lane's 4 dwords -> 16-bit mask, bit i = byte i matched (four independent v_dot4_i32_i8 with
// weights 1, 2, 4, 8: each subtracts the non-matching weights from 15, the first one carrying the +0xFFFF)
__device__ __forceinline__ uint32_t mask16(const uint4& v, uint32_t key) {
  const int d0 = __builtin_amdgcn_sdot4((int)match4(v.x, key), 0x08040201, 0xFFFF, false);
  const int d1 = __builtin_amdgcn_sdot4((int)match4(v.y, key), 0x08040201, 0, false);
  const int d2 = __builtin_amdgcn_sdot4((int)match4(v.z, key), 0x08040201, 0, false);
  const int d3 = __builtin_amdgcn_sdot4((int)match4(v.w, key), 0x08040201, 0, false);
  const uint32_t lo = ((uint32_t)d1 << 4) + (uint32_t)d0;
  const uint32_t hi = ((uint32_t)d3 << 4) + (uint32_t)d2;
  return ((hi << 8) + lo) & 0xFFFFu;
}
// the bytes of the 16-byte chunk at coordinate x that lie in [lo, hi), as 16 bits (the chunk overlaps the range:
// x < hi and x + 16 > lo, whatever lo is)
__device__ __forceinline__ uint32_t valid16(uint64_t x, uint64_t lo, uint64_t hi) {
  const uint32_t a = lo > x ? (uint32_t)(lo - x) : 0u;              // < 16
  const uint32_t b = hi - x < 16u ? (uint32_t)(hi - x) : 16u;       // 1..16
  return (0xFFFFu >> (16u - b)) & (0xFFFFu << a);
}
// Escape bytes e of a chunk (16 bits) and the bit `in` of the byte that is escaped on entry (at most one bit, zero
// for none): the add-carry over runs of escape bytes.  With c = esc_code(e, in), the escaped bytes are
// (c ^ (e | in)) & 0xFFFF and bit 15 of c & e says that the byte after the chunk is escaped.
__device__ __forceinline__ uint32_t esc_code(uint32_t e, uint32_t in) {
  const uint32_t pot = e & ~in;                    // escape bytes that are not escaped by the carry
  return (((pot << 1) | kOddBits) - pot) ^ kOddBits;
}
// A chunk as the row chain sees it: a = all 16 bytes are escape bytes (16 is even: the incoming bit passes through),
// t = the bit it hands on otherwise (the parity of its trailing escape run).  The chunk that holds the byte at lo
// starts the chain: its incoming bit is the launch's esc_carry, at that byte, and it never passes anything through.
struct EscChunk {
  uint32_t e, in0, a, t;
  bool first;
};
__device__ __forceinline__ EscChunk esc_chunk(const uint4& v, uint32_t ok, uint64_t x, const QuoteArgs& A) {
  EscChunk c;
  c.e = mask16(v, A.key_e) & ok;
  c.first = x <= A.lo && A.lo < x + 16u;
  c.in0 = c.first ? A.esc_carry << (uint32_t)(A.lo - x) : 0u;
  c.a = (c.e == 0xFFFFu && !c.first) ? 1u : 0u;
  c.t = ((esc_code(c.e, c.in0) & c.e) >> 15) & 1u;
  return c;
}
__device__ __forceinline__ uint32_t mbcnt(uint64_t m) {
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}
__device__ __forceinline__ uint32_t wave_sum(uint32_t x) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) x += (uint32_t)__shfl_xor((int)x, d, kWave);
  return x;
}
__device__ __forceinline__ uint64_t readlane64(uint64_t x, int l) {
  const uint32_t lo = __builtin_amdgcn_readlane((int)(uint32_t)x, l);
  const uint32_t hi = __builtin_amdgcn_readlane((int)(uint32_t)(x >> 32), l);
  return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ uint64_t ld_desc(unsigned long long* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_desc(unsigned long long* p, uint64_t v) {
  __hip_atomic_store(p, (unsigned long long)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// A byte range as a function of its incoming state: the parity of its quotes, and the newlines kept when it is
// entered outside (k0) / inside (k1) a quoted field.  then(a, b): a, then b -- associative.
struct Sum {
  uint32_t par;
  uint64_t k0, k1;
};
__device__ __forceinline__ Sum then(const Sum& a, const Sum& b) {
  Sum r;
  r.par = a.par ^ b.par;
  r.k0 = a.k0 + (a.par ? b.k1 : b.k0);
  r.k1 = a.k1 + (a.par ? b.k0 : b.k1);
  return r;
}

struct Shared {
  uint32_t tile;
  uint32_t abort;
  uint32_t state_in;
  uint32_t pad;
  unsigned long long base;
  uint32_t wpar[kWaves], wk0[kWaves], wk1[kWaves], wq[kWaves];
};

// The tile's incoming state and output base: walk the descriptors before `tile` 64 at a time, nearest first, up to
// the nearest PREFIX.  Wave 0 only, result wave-uniform.  Returns false when a wait expired (here or elsewhere).
__device__ __forceinline__ bool look_back(const QuoteArgs& A, uint64_t tile, int lane, uint32_t& state_in,
                                          uint64_t& base) {
  unsigned long long* desc = A.ctrl + kCtrlWords;
  unsigned int* err = reinterpret_cast<unsigned int*>(A.ctrl + kCtrlErr);
  Sum f{0u, 0ull, 0ull};                           // tiles (window end, tile) composed so far
  int64_t j = (int64_t)tile - 1;                   // nearest tile of the window
  uint32_t spins = 0;
  uint64_t t0 = 0;
  for (;;) {
    const int64_t idx = j - lane;
    // before tile 0: the launch's own incoming state
    const uint64_t d = idx >= 0 ? ld_desc(desc + idx) : (kStatPrefix | ((uint64_t)A.carry << 48));
    const uint32_t st = (uint32_t)(d >> 62);
    const uint64_t pm = __ballot(st == 2u);
    const uint64_t nm = __ballot(st == 0u);
    const int first_p = pm ? (int)__builtin_ctzll(pm) : 64;
    const uint64_t below = first_p == 64 ? ~0ull : ((1ull << first_p) - 1ull);
    if (nm & below) {                              // a tile nearer than the first PREFIX is not published yet
      ++spins;
      if ((spins & kPollCheck) == kPollCheck &&
          (__hip_atomic_load(err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & kErrTimeout))
        return false;
      if (wait_expired(spins, t0)) {
        if (lane == 0) atomicOr(err, kErrTimeout);
        return false;
      }
      __builtin_amdgcn_s_sleep(2);
      continue;
    }
    for (int l = 0; l < first_p; ++l) {            // AGG descriptors, nearest first: each goes in front
      const uint64_t a = readlane64(d, l);
      const Sum s{(uint32_t)(a >> 48) & 1u, a & 0xFFFFFFull, (a >> 24) & 0xFFFFFFull};
      f = then(s, f);
    }
    if (first_p < 64) {
      const uint64_t p = readlane64(d, first_p);
      const uint32_t s = (uint32_t)(p >> 48) & 1u;
      state_in = s ^ f.par;
      base = (p & kCountMask) + (s ? f.k1 : f.k0);
      return true;
    }
    j -= 64;
  }
}

// Is the byte at coordinate xw, the wave's first, escaped?  Wave-uniform.  Lane l reads the (l + 1)-th chunk before
// xw -- like every load of the kernel only if the chunk holds a byte of [lo, hi) -- and the nearest chunk that is not
// all escape bytes decides; chunks below lo are not read and decide 0, but the chunk of lo is nearer and always
// decides.  After kEscWindows windows of nothing but escape bytes one more chunk is looked at: a run that covers it
// too is beyond DQ_ESCAPE_RUN_MAX and ends the launch with kErrEscapeRun (no wait: descriptors are published as usual).
__device__ __forceinline__ uint32_t wave_esc_in(const QuoteArgs& A, uint64_t xw, int lane) {
  if (xw <= A.lo || xw >= A.hi) return 0u;         // the chain starts in this wave, or the wave holds no byte
  for (uint32_t it = 0;; ++it) {
    const uint64_t back = ((uint64_t)it * kWave + (uint64_t)lane + 1u) * 16u;
    uint32_t ca = 0u, ct = 0u;
    if (back <= xw) {
      const uint64_t x = xw - back;                // x < xw < hi
      if (x < A.hi && x + 16u > A.lo) {            // the chunk holds a byte of [lo, hi): inside the buffer's pages
        const uint4 v = *reinterpret_cast<const uint4*>(A.base + x);
        const EscChunk c = esc_chunk(v, valid16(x, A.lo, A.hi), x, A);
        ca = c.a;
        ct = c.t;
      }
    }
    const uint64_t ba = __ballot(ca != 0u), bt = __ballot(ct != 0u);
    if (it == kEscWindows) {
      if (ba & 1ull) {
        if (lane == 0) atomicOr(reinterpret_cast<unsigned int*>(A.ctrl + kCtrlErr), kErrEscapeRun);
        return 0u;
      }
      return (uint32_t)bt & 1u;
    }
    const uint64_t stop = ~ba;
    if (stop) return (uint32_t)(bt >> __builtin_ctzll(stop)) & 1u;
  }
}

// OUT64: 0 uint32 offsets, 1 uint64 offsets, 2 uint16 low words + the 64 KiB block table (tiles on the object's grid)
// ESC: 1 honours the escape byte (key_e, esc_carry, esc_nl)
template <int OUT64, int ESC>
__global__ void __launch_bounds__(kThreads) quote_kernel(QuoteArgs A) {
  __shared__ Shared S;
  using OutT = typename std::conditional<OUT64 == 1, uint64_t,
                                         typename std::conditional<OUT64 == 2, uint16_t, uint32_t>::type>::type;
  OutT* const out = reinterpret_cast<OutT*>(A.out);
  unsigned long long* const desc = A.ctrl + kCtrlWords;
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  uint32_t overflow = 0;

  for (;;) {
    if (threadIdx.x == 0) S.tile = atomicAdd(reinterpret_cast<unsigned int*>(A.ctrl + kCtrlTicket), 1u);
    __syncthreads();
    const uint64_t tile = S.tile;
    if (tile >= A.ntiles) break;                   // workgroup-uniform
    const uint64_t x0 = tile * kTileBytes + (uint64_t)wave * kWaveBytes + (uint64_t)lane * 16u;

    // ---- phase A: masks, in-wave parity, the newlines kept under either incoming state
    uint32_t km[kRows];                            // bits 0..15 kept if the wave is entered outside, 16..31 inside
    uint32_t run = 0;                              // parity of the wave's rows so far (wave-uniform)
    uint32_t cnt = 0, nq = 0;                      // per lane: kept0 | kept1 << 16; quotes (ESC: | unescaped << 16)
    uint32_t erow = 0;                             // ESC: is the row's first byte escaped (wave-uniform)
    if (ESC) erow = wave_esc_in(A, x0 - (uint64_t)lane * 16u, lane);
#pragma unroll
    for (int h = 0; h < kRows; h += kHalf) {
      uint4 v[kHalf];
      uint32_t ok[kHalf];
#pragma unroll
      for (int r = 0; r < kHalf; ++r) {
        const uint64_t x = x0 + (uint64_t)(h + r) * kRowBytes;
        v[r] = make_uint4(0u, 0u, 0u, 0u);
        ok[r] = 0u;
        // (blocked form: the chunks of a first tile's leading rows and waves lie wholly below lo and stay zero)
        if (x < A.hi && x + 16u > A.lo) {          // the chunk holds a byte of [lo, hi): inside the buffer's pages
          v[r] = *reinterpret_cast<const uint4*>(A.base + x);
          ok[r] = valid16(x, A.lo, A.hi);
        }
      }
#pragma unroll
      for (int r = 0; r < kHalf; ++r) {
        uint32_t q = mask16(v[r], A.key_q) & ok[r];
        uint32_t n = mask16(v[r], A.key_nl) & ok[r];
        if (ESC) {
          const EscChunk c = esc_chunk(v[r], ok[r], x0 + (uint64_t)(h + r) * kRowBytes, A);
          const uint64_t ba = __ballot(c.a != 0u), bt = __ballot(c.t != 0u);
          // the bit of the nearest lane below that is not all escape bytes, or the row's
          const uint64_t stop = ~ba & ((1ull << lane) - 1ull);
          uint32_t in = stop ? (uint32_t)(bt >> (63 - __builtin_clzll(stop))) & 1u : erow;
          if (c.first) in = c.in0;                 // the chunk of lo: esc_carry, at that byte
          const uint32_t escaped = (esc_code(c.e, in) ^ (c.e | in)) & 0xFFFFu;
          nq += (uint32_t)__popc(q) << 16;         // the quote bytes; below, the low half counts the unescaped ones
          q &= ~escaped;
          n &= ~(escaped & A.esc_nl);
          if (~ba) erow = (uint32_t)(bt >> (63 - __builtin_clzll(~ba))) & 1u;   // the next row's, scalar
        }
        uint32_t px = q;                           // bit i: parity of the chunk's quotes in bytes 0..i
        px ^= px << 1;
        px ^= px << 2;
        px ^= px << 4;
        px ^= px << 8;
        const uint64_t b = __ballot(__popc(q) & 1);
        const uint32_t before = (mbcnt(b) ^ run) & 1u;           // parity of the wave's quotes before this chunk
        const uint32_t inside = (px ^ (0u - before)) & 0xFFFFu;  // per byte, if the wave is entered outside
        const uint32_t k0 = n & ~inside, k1 = n & inside;
        km[h + r] = k0 | (k1 << 16);
        cnt += (uint32_t)__popc(k0) | ((uint32_t)__popc(k1) << 16);
        nq += (uint32_t)__popc(q);
        run ^= (uint32_t)__popcll(b) & 1u;
      }
    }
    cnt = wave_sum(cnt);                           // <= 16384 per half: no carry between the halves
    nq = wave_sum(nq);
    if (lane == 0) {
      S.wpar[wave] = run;
      S.wk0[wave] = cnt & 0xFFFFu;
      S.wk1[wave] = cnt >> 16;
      S.wq[wave] = nq;
    }
    __syncthreads();

    // ---- the tile's summary, its look-back, its descriptors (wave 0)
    if (wave == 0) {
      Sum t{0u, 0ull, 0ull};
      uint32_t tq = 0, tn = 0, tt = 0;
#pragma unroll
      for (int w = 0; w < kWaves; ++w) {
        t = then(t, Sum{S.wpar[w], S.wk0[w], S.wk1[w]});
        if (ESC) {
          tq += S.wq[w] >> 16;
          tt += S.wq[w] & 0xFFFFu;
        } else tq += S.wq[w];
        tn += S.wk0[w] + S.wk1[w];
      }
      uint32_t state_in = A.carry;
      uint64_t base = 0;
      bool ok = true;
      if (tile != 0) {
        if (lane == 0) st_desc(desc + tile, kStatAgg | ((uint64_t)t.par << 48) | (t.k1 << 24) | t.k0);
        ok = look_back(A, tile, lane, state_in, base);
        if (!ok) {
          state_in = 0;
          base = 0;
        }
      }
      const uint64_t incl = base + (state_in ? t.k1 : t.k0);
      if (lane == 0) {
        // (after a timeout the value is wrong, but a published PREFIX releases every tile waiting on this one)
        st_desc(desc + tile, kStatPrefix | ((uint64_t)(state_in ^ t.par) << 48) | (incl & kCountMask));
        S.state_in = state_in;
        S.base = base;
        S.abort = ok ? 0u : 1u;
        if (OUT64 == 2) A.table[tile] = base;      // the record ends before the tile: its entry of the block table
        if (tq) atomicAdd(A.ctrl + kCtrlQuotes, (unsigned long long)tq);
        if (tn) atomicAdd(A.ctrl + kCtrlNewlines, (unsigned long long)tn);
        if (ESC && tt) atomicAdd(A.ctrl + kCtrlToggles, (unsigned long long)tt);
        if (tile + 1 == A.ntiles) A.ctrl[kCtrlOut] = incl;
      }
    }
    __syncthreads();

    // ---- phase B: the wave's incoming state and base, then the offsets
    if (S.abort) continue;                         // workgroup-uniform: the next claim ends or skips likewise
    uint32_t st = S.state_in;
    uint64_t wbase = S.base;
    for (int w = 0; w < wave; ++w) {
      wbase += st ? S.wk1[w] : S.wk0[w];
      st ^= S.wpar[w];
    }
    const uint32_t sh = st ? 16u : 0u;
#pragma unroll
    for (int r = 0; r < kRows; ++r) {
      uint32_t kept = (km[r] >> sh) & 0xFFFFu;
      const uint32_t c = (uint32_t)__popc(kept);   // 0..16
      uint32_t ex = 0, total = 0;
      const uint64_t any = __ballot(c != 0u);
      if (any == 0ull) continue;                   // wave-uniform
      if (__ballot(c > 1u) == 0ull) {              // common: at most one per lane
        ex = mbcnt(any);
        total = (uint32_t)__popcll(any);
      } else {
#pragma unroll
        for (int bit = 0; bit < 5; ++bit) {
          const uint64_t m = __ballot((c >> bit) & 1u);
          ex += mbcnt(m) << bit;
          total += (uint32_t)__popcll(m) << bit;
        }
      }
      uint64_t i = wbase + ex;
      const uint64_t off = A.obj0 + x0 + (uint64_t)r * kRowBytes;
      while (kept) {
        const uint64_t o = off + (uint32_t)__builtin_ctz(kept);
        kept &= kept - 1u;
        if (OUT64 == 0 && (o >> 32)) overflow = 1u;
        else if (OUT64 == 2) {                     // obj0 is a multiple of 64 KiB: the low word of the offset is the
          if (i < A.cap) out[i] = (OutT)(uint32_t)o;   // byte's position in its tile (32-bit arithmetic is enough)
        } else if (i < A.cap) out[i] = (OutT)o;
        ++i;
      }
      wbase += total;
    }
  }
  if (OUT64 == 0 && overflow) atomicOr(reinterpret_cast<unsigned int*>(A.ctrl + kCtrlErr), kErrOverflow);
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
      return fail(DQ_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));          \
  } while (0)

}  // namespace

struct dq_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  int grid = 0;                       // workgroups of the persistent grid (the plain instantiations)
  int grid_esc[3] = {0, 0, 0};        // ... of the escape-aware instantiation of each output form
  unsigned long long* d_ws = nullptr; // control words + descriptors (grow-only)
  uint64_t ws_words = 0;
  unsigned long long* h_res = nullptr;  // pinned copy of the control words
  bool in_flight = false;
  bool count_only = false;            // cap = 0 with d_out = NULL: no capacity error
  bool escaped = false;               // the launch in flight is an escape-aware one
  uint64_t cap = 0;
};

extern "C" {

int dq_abi_version(void) { return DQ_ABI_VERSION; }

const char* dq_last_error(void) { return g_err.c_str(); }

int dq_ctx_create(int device, void* stream, dq_ctx** out) {
  if (!out) return fail(DQ_ERR_INVALID, "null out");
  *out = nullptr;
  int n = 0;
  HIPCHK(hipGetDeviceCount(&n));
  if (device < 0 || device >= n) return fail(DQ_ERR_INVALID, "device " + std::to_string(device) + " out of range");
  HIPCHK(hipSetDevice(device));
  hipDeviceProp_t prop;
  HIPCHK(hipGetDeviceProperties(&prop, device));
  int occ = 0;
  HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, quote_kernel<0, 0>, kThreads, 0));
  int occ1 = 0;
  HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ1, quote_kernel<1, 0>, kThreads, 0));
  if (occ1 < occ) occ = occ1;
  int occ2 = 0;
  HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ2, quote_kernel<2, 0>, kThreads, 0));
  if (occ2 < occ) occ = occ2;
  if (occ < 1) return fail(DQ_ERR_HIP, "quote_kernel: no resident workgroup per CU");
  if (occ > kMaxBlocksPerCU) occ = kMaxBlocksPerCU;
  // the escape-aware instantiations size their own grids: a lower occupancy there does not shrink the grid above
  int occ_esc[3] = {0, 0, 0};
  HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ_esc[0], quote_kernel<0, 1>, kThreads, 0));
  HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ_esc[1], quote_kernel<1, 1>, kThreads, 0));
  HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ_esc[2], quote_kernel<2, 1>, kThreads, 0));
  for (int f = 0; f < 3; ++f) {
    if (occ_esc[f] < 1) return fail(DQ_ERR_HIP, "quote_kernel (escape): no resident workgroup per CU");
    if (occ_esc[f] > kMaxBlocksPerCU) occ_esc[f] = kMaxBlocksPerCU;
  }
  dq_ctx* c = new dq_ctx();
  c->device = device;
  c->stream = (hipStream_t)stream;
  // the grid need not be resident (tiles are claimed by running workgroups); this size merely fills the chip
  c->grid = prop.multiProcessorCount * occ;
  for (int f = 0; f < 3; ++f) c->grid_esc[f] = prop.multiProcessorCount * occ_esc[f];
  hipError_t e = hipHostMalloc((void**)&c->h_res, kCtrlWords * sizeof(unsigned long long), hipHostMallocDefault);
  if (e != hipSuccess) {
    delete c;
    return fail(DQ_ERR_HIP, std::string("hipHostMalloc: ") + hipGetErrorString(e));
  }
  *out = c;
  return DQ_OK;
}

int dq_ctx_destroy(dq_ctx* c) {
  if (!c) return DQ_OK;
  (void)hipSetDevice(c->device);
  (void)hipStreamSynchronize(c->stream);
  if (c->d_ws) (void)hipFree(c->d_ws);
  if (c->h_res) (void)hipHostFree(c->h_res);
  delete c;
  return DQ_OK;
}

// The escape arguments of a launch; `on` = false is the plain kernel.
struct EscSpec {
  bool on;
  uint32_t escape, esc_carry, flags;
};

// The launch behind every entry point.  form: 0 uint32, 1 uint64 (coordinate 0 = the 16-byte boundary at or below
// the device address of `begin`), 2 blocked (coordinate 0 = object offset begin & ~0xFFFF, d_table required).
static int records_launch(dq_ctx* c, const uint8_t* d_buf, uint64_t buf_len, uint64_t buf_base, uint64_t begin,
                          uint64_t end, uint32_t quote, uint32_t carry, void* d_out, int form, uint64_t cap,
                          uint64_t* d_table, uint64_t table_cap, const EscSpec& esc = EscSpec{false, 0u, 0u, 0u}) {
  if (!c) return fail(DQ_ERR_INVALID, "null ctx");
  if (c->in_flight) return fail(DQ_ERR_INVALID, "a launch is in flight: collect it with dq_records_result");
  if (begin > end || begin < buf_base || end - buf_base > buf_len)
    return fail(DQ_ERR_INVALID, "[begin, end) outside the buffer");
  if (end > begin && !d_buf) return fail(DQ_ERR_INVALID, "null buffer");
  if (quote > 255u || quote == 10u) return fail(DQ_ERR_INVALID, "quote must be a byte other than '\\n'");
  if (carry > 1u) return fail(DQ_ERR_INVALID, "carry must be 0 or 1");
  if (esc.on) {
    if (esc.escape > 255u || esc.escape == 10u || esc.escape == quote)
      return fail(DQ_ERR_INVALID, "escape must be a byte other than the quote and '\\n'");
    if (esc.esc_carry > 1u) return fail(DQ_ERR_INVALID, "esc_carry must be 0 or 1");
    if (esc.flags & ~(uint32_t)DQ_ESC_SCOPE_QUOTED) return fail(DQ_ERR_INVALID, "unknown escape flags");
  }
  if (cap && !d_out) return fail(DQ_ERR_INVALID, "null output with cap > 0");
  if (form < 0 || form > 2) return fail(DQ_ERR_INVALID, "out_u64 must be 0 or 1");
  if (cap && ((uintptr_t)d_out & (form == 1 ? 7u : form == 2 ? 1u : 3u)))
    return fail(DQ_ERR_INVALID, "misaligned output");

  const uint64_t len = end - begin;
  const uintptr_t p = (uintptr_t)d_buf + (uintptr_t)(begin - buf_base);
  uint64_t shift, ntiles, obj0;
  if (form == 2) {
    // tiles on the object's 64 KiB grid: coordinate 0 may lie before the allocation (never dereferenced there)
    if (len && ((p ^ begin) & 15u))
      return fail(DQ_ERR_INVALID, "blocked form: the device address of `begin` must be congruent to begin mod 16");
    if ((uintptr_t)d_table & 7u) return fail(DQ_ERR_INVALID, "misaligned block table");
    shift = len ? (begin & 0xFFFFu) : 0u;
    obj0 = begin & ~(uint64_t)0xFFFFu;
    ntiles = len ? ((end - 1) >> 16) - (begin >> 16) + 1 : 0u;
    if (ntiles && !d_table) return fail(DQ_ERR_INVALID, "null block table");
    if (table_cap < ntiles)
      return fail(DQ_ERR_INVALID, "block table capacity " + std::to_string(table_cap) + " below " +
                                      std::to_string(ntiles) + " tiles");
  } else {
    shift = len ? (uint64_t)(p & 15u) : 0u;
    obj0 = begin - shift;
    ntiles = len ? (shift + len + kTileBytes - 1) / kTileBytes : 0u;
  }
  if (ntiles >= 0xFFFF0000ull) return fail(DQ_ERR_INVALID, "range too large for one launch");
  HIPCHK(hipSetDevice(c->device));
  const uint64_t words = kCtrlWords + ntiles;
  if (words > c->ws_words) {
    HIPCHK(hipStreamSynchronize(c->stream));
    if (c->d_ws) HIPCHK(hipFree(c->d_ws));
    c->d_ws = nullptr;
    c->ws_words = 0;
    const uint64_t want = words + words / 4 + 1024;
    HIPCHK(hipMalloc((void**)&c->d_ws, want * sizeof(unsigned long long)));
    c->ws_words = want;
  }
  HIPCHK(hipMemsetAsync(c->d_ws, 0, words * sizeof(unsigned long long), c->stream));
  if (ntiles) {
    QuoteArgs a;
    a.base = (const uint8_t*)(p - (uintptr_t)shift);
    a.lo = shift;
    a.hi = shift + len;
    a.obj0 = obj0;
    a.ntiles = ntiles;
    a.key_q = (quote * 0x01010101u) ^ kSel12;
    a.key_nl = 0x0A0A0A0Au ^ kSel12;
    a.carry = carry;
    a.out = d_out;
    a.cap = cap;
    a.table = (unsigned long long*)d_table;
    a.ctrl = c->d_ws;
    a.key_e = esc.on ? (esc.escape * 0x01010101u) ^ kSel12 : 0u;
    a.esc_carry = esc.on ? esc.esc_carry : 0u;
    a.esc_nl = esc.on && !(esc.flags & DQ_ESC_SCOPE_QUOTED) ? 0xFFFFu : 0u;
    const uint64_t full = (uint64_t)(esc.on ? c->grid_esc[form] : c->grid);
    const unsigned grid = (unsigned)(ntiles < full ? ntiles : full);
    if (esc.on) {
      if (form == 2) hipLaunchKernelGGL((quote_kernel<2, 1>), dim3(grid), dim3(kThreads), 0, c->stream, a);
      else if (form == 1) hipLaunchKernelGGL((quote_kernel<1, 1>), dim3(grid), dim3(kThreads), 0, c->stream, a);
      else hipLaunchKernelGGL((quote_kernel<0, 1>), dim3(grid), dim3(kThreads), 0, c->stream, a);
    } else if (form == 2) hipLaunchKernelGGL((quote_kernel<2, 0>), dim3(grid), dim3(kThreads), 0, c->stream, a);
    else if (form == 1) hipLaunchKernelGGL((quote_kernel<1, 0>), dim3(grid), dim3(kThreads), 0, c->stream, a);
    else hipLaunchKernelGGL((quote_kernel<0, 0>), dim3(grid), dim3(kThreads), 0, c->stream, a);
    HIPCHK(hipGetLastError());
  }
  HIPCHK(hipMemcpyAsync(c->h_res, c->d_ws, kCtrlWords * sizeof(unsigned long long), hipMemcpyDeviceToHost,
                        c->stream));
  c->cap = cap;
  c->count_only = cap == 0 && !d_out;
  c->in_flight = true;
  c->escaped = esc.on;
  return DQ_OK;
}

int dq_records_async(dq_ctx* c, const uint8_t* d_buf, uint64_t buf_len, uint64_t buf_base, uint64_t begin,
                     uint64_t end, uint32_t quote, uint32_t carry, void* d_out, int out_u64, uint64_t cap) {
  if (out_u64 != 0 && out_u64 != 1) return fail(DQ_ERR_INVALID, "out_u64 must be 0 or 1");
  return records_launch(c, d_buf, buf_len, buf_base, begin, end, quote, carry, d_out, out_u64, cap, nullptr, 0);
}

int dq_records_blocked_async(dq_ctx* c, const uint8_t* d_buf, uint64_t buf_len, uint64_t buf_base, uint64_t begin,
                             uint64_t end, uint32_t quote, uint32_t carry, uint16_t* d_low, uint64_t cap,
                             uint64_t* d_table, uint64_t table_cap) {
  return records_launch(c, d_buf, buf_len, buf_base, begin, end, quote, carry, d_low, 2, cap, d_table, table_cap);
}

int dq_records_esc_async(dq_ctx* c, const uint8_t* d_buf, uint64_t buf_len, uint64_t buf_base, uint64_t begin,
                         uint64_t end, uint32_t quote, uint32_t carry, uint32_t escape, uint32_t esc_carry,
                         uint32_t flags, void* d_out, int out_u64, uint64_t cap) {
  if (out_u64 != 0 && out_u64 != 1) return fail(DQ_ERR_INVALID, "out_u64 must be 0 or 1");
  return records_launch(c, d_buf, buf_len, buf_base, begin, end, quote, carry, d_out, out_u64, cap, nullptr, 0,
                        EscSpec{true, escape, esc_carry, flags});
}

int dq_records_esc_blocked_async(dq_ctx* c, const uint8_t* d_buf, uint64_t buf_len, uint64_t buf_base,
                                 uint64_t begin, uint64_t end, uint32_t quote, uint32_t carry, uint32_t escape,
                                 uint32_t esc_carry, uint32_t flags, uint16_t* d_low, uint64_t cap,
                                 uint64_t* d_table, uint64_t table_cap) {
  return records_launch(c, d_buf, buf_len, buf_base, begin, end, quote, carry, d_low, 2, cap, d_table, table_cap,
                        EscSpec{true, escape, esc_carry, flags});
}

int dq_records_esc_result(dq_ctx* c, uint64_t* n_out, uint64_t* n_quotes, uint64_t* n_newlines,
                          uint64_t* n_toggles) {
  // (a plain launch toggles at every quote byte)
  if (c && c->in_flight && n_toggles) {
    const bool escaped = c->escaped;
    const int rc = dq_records_result(c, n_out, n_quotes, n_newlines);
    *n_toggles = c->h_res[escaped ? kCtrlToggles : kCtrlQuotes];
    return rc;
  }
  return dq_records_result(c, n_out, n_quotes, n_newlines);
}

int dq_records_result(dq_ctx* c, uint64_t* n_out, uint64_t* n_quotes, uint64_t* n_newlines) {
  if (!c) return fail(DQ_ERR_INVALID, "null ctx");
  if (!c->in_flight) return fail(DQ_ERR_INVALID, "no launch in flight");
  c->in_flight = false;
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipStreamSynchronize(c->stream));
  const uint32_t err = (uint32_t)c->h_res[kCtrlErr];
  if (n_out) *n_out = c->h_res[kCtrlOut];
  if (n_quotes) *n_quotes = c->h_res[kCtrlQuotes];
  if (n_newlines) *n_newlines = c->h_res[kCtrlNewlines];
  if (err & kErrTimeout) return fail(DQ_ERR_TIMEOUT, "a look-back wait exceeded its bound: results invalid");
  if (err & kErrEscapeRun)
    return fail(DQ_ERR_ESCAPE_RUN, "a run of escape bytes longer than DQ_ESCAPE_RUN_MAX: results invalid");
  if (err & kErrOverflow) return fail(DQ_ERR_OVERFLOW, "a record end lies at an offset >= 2^32 (uint32 output)");
  if (c->h_res[kCtrlOut] > c->cap && !c->count_only)
    return fail(DQ_ERR_CAPACITY, "output capacity " + std::to_string(c->cap) + " below " +
                                     std::to_string(c->h_res[kCtrlOut]) + " record ends");
  return DQ_OK;
}

int dq_geometry(dq_ctx* c, int* grid, int* tile_bytes) {
  if (!c) return fail(DQ_ERR_INVALID, "null ctx");
  if (grid) *grid = c->grid;
  if (tile_bytes) *tile_bytes = kTileBytes;
  return DQ_OK;
}

}  // extern "C"
