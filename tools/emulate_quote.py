"""Lane-exact numpy model of quote_kernel<0|1|2> (dataplug_amd/csrc/dpquote.hip), for CPU validation.

The kernel as written, not the definition (tests/_quote_model.py): the host arithmetic of dq_records_async, 64 KiB
tiles of 4 waves x 16 rows x 64 lanes x 16-byte chunks, match4 as a v_perm_b32 byte table, mask16 as four signed-byte
dot products with the +0xFFFF accumulator, valid16, the in-chunk prefix XOR, the ballot of odd chunks, the packed
per-lane counts, the wave / tile summaries, the 64-bit descriptor words, the 64-lane look-back window and both
phase-B scan paths.  Phase A and phase B are vectorised over every chunk of the launch (arrays of shape tiles x
waves x rows x lanes); the look-back runs tile by tile on Python integers.

What the hardware decides by timing -- which descriptors a tile finds published when it looks back -- is an argument
here: a *schedule* hands every look-back its descriptor snapshots (``SCHEDULES``).  ``mutate=`` switches on one
deliberate defect (``MUTANTS``); tests/test_quote_model.py uses it to show that its cases would notice each of them.

    prepare(...)  -> Prepared      host arithmetic, the launch's view of memory, phase A, the tile summaries
    finish(P,...) -> result        look-back under a schedule, phase B, the result words
    run(...)      = finish(prepare(...))

The blocked form u16b (quote_kernel<2>, dq_records_blocked_async) is asked for by keyword: ``host_args(...,
blocked=True)`` / ``prepare(..., blocked=True)`` lay the tiles on the object's 64 KiB grid (coordinate 0 = object
offset begin & ~0xFFFF, lo up to 65535), and ``finish(..., fmt="u16b")`` / ``run(..., fmt="u16b")`` return
``(low, table, n_out, n_quotes, n_newlines, err_bits)``: the uint16 low words and the block table (each tile's
exclusive base).  ``BLOCKED_MUTANTS`` are the deliberate defects of that code; tests/test_quote_blocked_model.py.

The escape-aware instantiations (quote_kernel<.., 1>, dq_records_esc_async / dq_records_esc_blocked_async) are asked
for by keyword too: ``prepare(..., escape=92, esc_carry=0, escape_scope="all")`` / ``run(...)`` with the same
keywords model the escape mask, the add-carry escaped mask (``esc_code``), the two ballots per row (all-escape chunks,
trailing-run parity), the scalar row chain, the wave's walk back over the chunks before it with its bound
(``ERR_ESCAPE_RUN``) and ``esc_carry`` applied at the byte ``lo``.  The result tuples keep their shape; the number of
unescaped quotes is ``Prepared.n_toggles`` and ``stats["n_toggles"]``.  ``ESCAPE_MUTANTS`` are the deliberate defects
of that code; tests/test_quote_escape_model.py.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Callable, List, Optional, Tuple

import numpy as np

# ------------------------------------------------------------------------------------------ the kernel's constants
WAVE, WAVES, ROWS = 64, 4, 16
ROW_BYTES = WAVE * 16
WAVE_BYTES = ROW_BYTES * ROWS
TILE_BYTES = WAVE_BYTES * WAVES
SEL12 = 0x0C0C0C0C
CTRL_WORDS = 8
DOT_WEIGHTS = 0x08040201
DOT_ACC0 = 0xFFFF

AGG_K1_SHIFT, AGG_PAR_SHIFT = 24, 48
AGG_K_MASK = 0xFFFFFF
PREFIX_STATE_SHIFT = 48
COUNT_MASK = 0xFFFFFFFFFFFF
STATUS_SHIFT = 62
STAT_AGG, STAT_PREFIX = 1 << STATUS_SHIFT, 2 << STATUS_SHIFT

ERR_TIMEOUT, ERR_OVERFLOW = 1, 2          # the kernel's bits of the error word
ERR_CAPACITY = 4                          # the model's bit for dq_records_result's check n_out > cap
ERR_STRAY = 8                             # the model's bit for a store beyond every newline (only a mutant does it)
ERR_ESCAPE_RUN = 16                       # the model's bit for the kernel's kErrEscapeRun (its bit 4 is taken above)
MAX_TILES = 0xFFFF0000

ODD_BITS = 0xAAAAAAAA
ESCAPE_RUN_MAX = 1 << 20                  # include/dpquote.h DQ_ESCAPE_RUN_MAX
ESC_WINDOWS = ESCAPE_RUN_MAX // (WAVE * 16)
ESC_SCOPE_QUOTED = 1

MUTANTS = ("then_swapped", "window_drops_f", "base_swapped", "ignore_carry", "no_run", "valid_hi_plus_one",
           "unsigned_dot", "agg_k1_shift16")

# deliberate defects of the blocked form only (they change nothing in the uint32 / uint64 forms)
BLOCKED_MUTANTS = ("table_inclusive", "low_from_shifted", "table_skip_tile0")

# deliberate defects of the escape-aware code only (they change nothing without ``escape=``)
ESCAPE_MUTANTS = ("escaped_quote_toggles", "all_escape_resets", "esc_carry_at_chunk_start", "wave_flag_zero",
                  "all_keeps_escaped_newlines")

M32 = 0xFFFFFFFF
M64 = (1 << 64) - 1
CANARY = 0xEEEEEEEEEEEEEEEE


def _check_mutant(mutate):
    if mutate is not None and mutate not in MUTANTS and mutate not in BLOCKED_MUTANTS and \
            mutate not in ESCAPE_MUTANTS:
        raise ValueError(f"mutate={mutate!r}: one of {MUTANTS + BLOCKED_MUTANTS + ESCAPE_MUTANTS}")


# ------------------------------------------------------------------------------------------ instructions
def v_perm_byte(s0: int, s1: int, sel: int) -> int:
    """One result byte of v_perm_b32 D, S0, S1, selector byte ``sel``: 0..3 a byte of S1, 4..7 a byte of S0, 8..11
    the sign of one 16-bit half replicated, 12 the constant 0x00, 13 and above 0xFF."""
    if sel <= 3:
        return (s1 >> (8 * sel)) & 0xFF
    if sel <= 7:
        return (s0 >> (8 * (sel - 4))) & 0xFF
    if sel <= 11:
        src, bit = ((s1, 15), (s1, 31), (s0, 15), (s0, 31))[sel - 8]
        return 0xFF if (src >> bit) & 1 else 0x00
    return 0x00 if sel == 12 else 0xFF


# __builtin_amdgcn_perm(0xFFFFFFFF, 0xFFFFFFFF, selector): the result byte for every selector byte
PERM_FF = np.array([v_perm_byte(M32, M32, s) for s in range(256)], np.uint8)


def match4(w: np.ndarray, key: int) -> np.ndarray:
    """match4 of uint32 words ``w``: the four result bytes of each word (last axis, byte 0 first)."""
    x = (np.ascontiguousarray(w, "<u4") ^ np.uint32(key)).view(np.uint8).reshape(w.shape + (4,))
    return PERM_FF[x]


def sdot4(a_bytes: np.ndarray, b: int, c, unsigned: bool = False) -> np.ndarray:
    """v_dot4_i32_i8 without clamp: the signed bytes of a (last axis) times the signed bytes of ``b``, plus ``c``, as
    the uint32 bit pattern of the int32 result."""
    a = a_bytes.astype(np.int64) if unsigned else a_bytes.view(np.int8).astype(np.int64)
    bb = np.array([(b >> (8 * i)) & 0xFF for i in range(4)], np.uint8)
    bw = bb.astype(np.int64) if unsigned else bb.view(np.int8).astype(np.int64)
    return ((a * bw).sum(-1) + np.asarray(c, np.int64)) & M32


def mask16(v: np.ndarray, key: int, mutate: Optional[str] = None) -> np.ndarray:
    """mask16 of chunks ``v`` (uint32, last axis = the uint4's x, y, z, w): bit i = byte i of the chunk matched."""
    d = sdot4(match4(v, key), DOT_WEIGHTS, np.array([DOT_ACC0, 0, 0, 0], np.int64), mutate == "unsigned_dot")
    lo = ((d[..., 1] << 4) + d[..., 0]) & M32
    hi = ((d[..., 3] << 4) + d[..., 2]) & M32
    return ((hi << 8) + lo) & 0xFFFF


def valid16(x: np.ndarray, lo: int, hi: int, mutate: Optional[str] = None) -> np.ndarray:
    """valid16 of chunks at coordinates ``x`` that overlap [lo, hi) (x < hi and x + 16 > lo)."""
    a = np.where(lo > x, lo - x, 0)
    rest = hi - x + (1 if mutate == "valid_hi_plus_one" else 0)
    b = np.where(rest < 16, rest, 16)
    return (0xFFFF >> (16 - b)) & ((0xFFFF << a) & M32)


_P8 = np.array([bin(i).count("1") for i in range(256)], np.int64)


def popc(x: np.ndarray) -> np.ndarray:
    x = np.asarray(x, np.int64)
    return _P8[x & 0xFF] + _P8[(x >> 8) & 0xFF] + _P8[(x >> 16) & 0xFF] + _P8[(x >> 24) & 0xFF]


def mbcnt(pred: np.ndarray) -> np.ndarray:
    """mbcnt(ballot(pred)) for every lane (last axis): the lanes below it whose predicate holds."""
    p = pred.astype(np.int64)
    return np.cumsum(p, axis=-1) - p


def popcll_ballot(pred: np.ndarray) -> np.ndarray:
    """popcll(ballot(pred)): wave-uniform, the lane axis dropped."""
    return pred.astype(np.int64).sum(-1)


# ------------------------------------------------------------------------------------------ escape bytes
def esc_code(e: np.ndarray, inb: np.ndarray) -> np.ndarray:
    """esc_code of escape masks ``e`` and entry bits ``inb`` (32-bit arithmetic): with c the result, the escaped bytes
    are (c ^ (e | inb)) & 0xFFFF and bit 15 of c & e says that the byte after the chunk is escaped."""
    e, inb = np.asarray(e, np.int64), np.asarray(inb, np.int64)
    pot = e & ~inb & M32
    return ((((pot << 1) & M32) | ODD_BITS) - pot) & M32 ^ ODD_BITS


def esc_chunks(e: np.ndarray, x: np.ndarray, lo: int, esc_carry: int, mutate: Optional[str] = None):
    """esc_chunk of chunks at coordinates ``x`` with (valid) escape masks ``e``: (first, in0, a, t)."""
    first = (x <= lo) & (lo < x + 16)
    at = 0 if mutate == "esc_carry_at_chunk_start" else np.where(first, lo - x, 0)
    in0 = np.where(first, (esc_carry << at) & M32, 0)
    a = (e == 0xFFFF) & ~first
    if mutate == "all_escape_resets":
        a = np.zeros_like(a)
    t = ((esc_code(e, in0) & e) >> 15) & 1
    return first, in0, a, t


def wave_esc_in(a_flat: np.ndarray, t_flat: np.ndarray, xw: int, lo: int, hi: int, mutate: Optional[str] = None):
    """wave_esc_in of the wave that starts at coordinate ``xw``: (is its first byte escaped, error).  ``a_flat`` and
    ``t_flat`` are the a / t bits of every chunk of the launch by chunk index (chunks the kernel does not load: 0)."""
    if xw <= lo or xw >= hi or mutate == "wave_flag_zero":
        return 0, 0
    c0 = xw >> 4
    lanes = np.arange(WAVE)
    it = 0
    while True:
        idx = c0 - (it * WAVE + lanes + 1)               # back <= xw  <=>  idx >= 0
        ok = idx >= 0
        ca = np.where(ok, a_flat[np.where(ok, idx, 0)], 0)
        ct = np.where(ok, t_flat[np.where(ok, idx, 0)], 0)
        if it == ESC_WINDOWS:
            return (0, 1) if ca[0] else (int(ct[0]), 0)
        stop = np.nonzero(ca == 0)[0]
        if len(stop):
            return int(ct[stop[0]]), 0                   # ctz of ~ba: the nearest chunk that is not all escape bytes
        it += 1


def escape_phase(e, x, q, n, a: "Args", mutate: Optional[str] = None):
    """The escape-aware part of phase A over every chunk ([tiles, waves, rows, lanes]): the quote and newline masks
    with the escaped bytes taken out, the raw quote counts, and the error flag of the walk back."""
    T = e.shape[0]
    first, in0, ca, ct = esc_chunks(e, x, a.lo, a.esc_carry, mutate)
    a_flat, t_flat = ca.reshape(-1).astype(np.int64), ct.reshape(-1).astype(np.int64)
    erow = np.zeros((T, WAVES), np.int64)
    err = 0
    # a wave walks back only if the chunk before it is all escape bytes: the others read their flag off that chunk
    for t in range(T):
        for w in range(WAVES):
            erow[t, w], bad = wave_esc_in(a_flat, t_flat, t * TILE_BYTES + w * WAVE_BYTES, a.lo, a.hi, mutate)
            err |= bad
    lanes = np.arange(WAVE)
    inb = np.zeros_like(e)
    for r in range(ROWS):
        na = ~ca[:, :, r, :].astype(bool)                # lanes that are not all escape bytes
        # highest lane below each lane that is not all-escape (63 - clzll(stop)), -1 for none
        cand = np.where(na, lanes, -1)
        upto = np.maximum.accumulate(cand, axis=-1)      # highest such lane <= each lane
        below = np.concatenate([np.full(upto.shape[:-1] + (1,), -1), upto[..., :-1]], axis=-1)
        tr = ct[:, :, r, :]
        chain = np.where(below >= 0, np.take_along_axis(tr, np.maximum(below, 0), axis=-1), erow[:, :, None])
        inb[:, :, r, :] = chain
        top = upto[..., -1]
        erow = np.where(top >= 0, np.take_along_axis(tr, np.maximum(top, 0)[..., None], axis=-1)[..., 0], erow)
    inb = np.where(first, in0, inb)
    escaped = (esc_code(e, inb) ^ (e | inb)) & 0xFFFF
    raw = popc(q)
    if mutate != "escaped_quote_toggles":
        q = q & ~escaped
    nl_mask = 0 if mutate == "all_keeps_escaped_newlines" else a.esc_nl
    n = n & ~(escaped & nl_mask)
    return q, n, raw, err


# ------------------------------------------------------------------------------------------ summaries, descriptors
@dataclass(frozen=True)
class Sum:
    par: int
    k0: int
    k1: int


IDENT = Sum(0, 0, 0)


def then(a: Sum, b: Sum) -> Sum:
    return Sum(a.par ^ b.par, a.k0 + (b.k1 if a.par else b.k0), a.k1 + (b.k0 if a.par else b.k1))


def pack_agg(t: Sum, mutate: Optional[str] = None) -> int:
    sh = 16 if mutate == "agg_k1_shift16" else AGG_K1_SHIFT
    return (STAT_AGG | (t.par << AGG_PAR_SHIFT) | (t.k1 << sh) | t.k0) & M64


def unpack_agg(a: int, mutate: Optional[str] = None) -> Sum:
    sh = 16 if mutate == "agg_k1_shift16" else AGG_K1_SHIFT
    return Sum((a >> AGG_PAR_SHIFT) & 1, a & AGG_K_MASK, (a >> sh) & AGG_K_MASK)


def pack_prefix(state: int, count: int) -> int:
    return STAT_PREFIX | (state << PREFIX_STATE_SHIFT) | (count & COUNT_MASK)


def unpack_prefix(p: int) -> Tuple[int, int]:
    """(state after the tile, record ends up to and including it)."""
    return (p >> PREFIX_STATE_SHIFT) & 1, p & COUNT_MASK


def status(d: int) -> int:
    return (d >> STATUS_SHIFT) & 3


# ------------------------------------------------------------------------------------------ look-back
def look_back_window(desc: List[int], j: int, f: Sum, carry: int, mutate: Optional[str] = None):
    """One iteration of look_back()'s loop over a snapshot ``desc`` of the descriptor array: lane l reads tile j - l
    (before tile 0 the virtual PREFIX that carries the launch's incoming state).  Returns ("spin",) when a tile nearer
    than the first PREFIX is unpublished, ("next", f, j - 64) when the window holds no PREFIX, and
    ("done", state_in, base) otherwise."""
    virt = STAT_PREFIX | ((0 if mutate == "ignore_carry" else carry) << PREFIX_STATE_SHIFT)
    d = [desc[j - lane] if j - lane >= 0 else virt for lane in range(WAVE)]
    pm = sum(1 << lane for lane in range(WAVE) if status(d[lane]) == 2)
    nm = sum(1 << lane for lane in range(WAVE) if status(d[lane]) == 0)
    first_p = (pm & -pm).bit_length() - 1 if pm else 64
    below = M64 if first_p == 64 else (1 << first_p) - 1
    if nm & below:
        return ("spin",)
    for lane in range(first_p):                          # AGG descriptors, nearest first: each goes in front
        s = unpack_agg(d[lane], mutate)
        f = then(f, s) if mutate == "then_swapped" else then(s, f)
    if first_p < 64:
        s, count = unpack_prefix(d[first_p])
        pick1 = (not s) if mutate == "base_swapped" else bool(s)
        return ("done", s ^ f.par, count + (f.k1 if pick1 else f.k0))
    return ("next", IDENT if mutate == "window_drops_f" else f, j - WAVE)


def look_back(tile: int, carry: int, snapshots: Callable[[int], List[int]], mutate: Optional[str] = None):
    """look_back() of ``tile``: (state_in, base, windows read, descriptors composed, spins).  ``snapshots(n)`` is the
    descriptor array as the n-th read of this look-back finds it."""
    f, j = IDENT, tile - 1
    reads = windows = spins = 0
    while True:
        desc = snapshots(reads)
        reads += 1
        r = look_back_window(desc, j, f, carry, mutate)
        if r[0] == "spin":
            spins += 1
            if spins > 1000:
                raise RuntimeError(f"tile {tile}: the schedule never publishes what the look-back waits for")
            continue
        windows += 1
        if r[0] == "done":
            return r[1], r[2], windows, spins
        f, j = r[1], r[2]


# ------------------------------------------------------------------------------------------ schedules
# A schedule is a callable (tile, read, agg, prefix) -> descriptor snapshot for tiles 0..tile-1, where agg[i] and
# prefix[i] are the words tile i publishes (the tiles resolve in order in the model, so prefix[i] is known) and
# ``read`` counts this look-back's reads of the array.  Snapshots stay realisable: a PREFIX of tile i is shown only
# when every tile before i shows at least its AGG, because tile i's own look-back had to complete first.  The one
# exception is tile 0: the kernel never publishes an AGG for it (it starts from ``carry`` without a look-back), so on
# hardware every chain ends at tile 0's PREFIX at the latest and the virtual PREFIX before tile 0 is never selected.
# ``all_agg`` shows tile 0's summary as an AGG all the same, which is the only way to walk into the virtual PREFIX.
def sequential(tile, read, agg, prefix):
    return list(prefix[:tile])


def all_agg(tile, read, agg, prefix):
    return list(agg[:tile])


def chain_to_tile0(tile, read, agg, prefix):
    """The deepest chain the hardware can produce: tile 0's PREFIX, every other predecessor an AGG."""
    return [prefix[0]] + list(agg[1:tile])


def random(seed: int, p_prefix: Optional[float] = None, p_spin: float = 0.3):
    """Each predecessor but tile 0 independently AGG or PREFIX (a PREFIX with probability ``p_prefix``, by default
    2^-(1 + seed mod 8): chains of a few tiles for seed 0, of more than a window for seed 5); with probability
    ``p_spin`` the first read finds one of the AGGs nearer than the first PREFIX still unpublished (a spin), the next
    read finds it published."""
    if p_prefix is None:
        p_prefix = 0.5 ** (1 + seed % 8)

    def sched(tile, read, agg, prefix):
        rng = np.random.default_rng([seed, tile])
        is_p = rng.random(tile) < p_prefix
        is_p[0] = True
        d = [prefix[i] if is_p[i] else agg[i] for i in range(tile)]
        nearest_p = max(i for i in range(tile) if is_p[i])
        if rng.random() < p_spin and nearest_p < tile - 1 and read == 0:
            d[int(rng.integers(nearest_p + 1, tile))] = 0
        return d
    return sched


WINDOW_EDGE_LANES = (63, 0, 1, 64)


def window_edge(lane: Optional[int] = None):
    """The first PREFIX exactly ``lane`` descriptors before the nearest one (lane 64: the first lane of the second
    window), AGGs nearer; ``lane=None`` cycles through WINDOW_EDGE_LANES with the tile index.  A tile with fewer
    predecessors walks to tile 0's PREFIX."""
    def sched(tile, read, agg, prefix):
        ln = WINDOW_EDGE_LANES[tile % len(WINDOW_EDGE_LANES)] if lane is None else lane
        p = max(0, tile - 1 - ln)
        return list(prefix[:p + 1]) + list(agg[p + 1:tile])
    return sched


SCHEDULES = {"sequential": sequential, "all_agg": all_agg, "chain_to_tile0": chain_to_tile0,
             "window_edge": window_edge()}


def get_schedule(s):
    if callable(s):
        return s
    if s in SCHEDULES:
        return SCHEDULES[s]
    name, _, arg = str(s).partition(":")
    if name == "random" and arg:
        return random(int(arg))
    if name == "window_edge" and arg:
        return window_edge(int(arg))
    raise ValueError(f"schedule {s!r}: one of {sorted(SCHEDULES)}, 'random:SEED', 'window_edge:LANE' or a callable")


# ------------------------------------------------------------------------------------------ host side
@dataclass(frozen=True)
class Args:
    """QuoteArgs as dq_records_async (dq_records_blocked_async with ``blocked``) derives them; ``base_addr`` is the
    16-byte aligned device address of coordinate 0 (blocked: possibly below the buffer, never loaded from there)."""
    base_addr: int
    shift: int
    lo: int
    hi: int
    obj0: int
    ntiles: int
    key_q: int
    key_nl: int
    key_e: int = 0                   # the escape-aware launches (``escape`` is None otherwise)
    esc_carry: int = 0
    esc_nl: int = 0
    escape: Optional[int] = None


def host_args(dev_addr: int, buf_len: int, buf_base: int, begin: int, end: int, quote: int = 34,
              blocked: bool = False, escape: Optional[int] = None, esc_carry: int = 0,
              escape_scope: str = "all") -> Args:
    if escape is not None:
        if not 0 <= escape <= 255 or escape == 10 or escape == quote:
            raise ValueError("escape must be a byte other than the quote and '\\n'")
        if esc_carry not in (0, 1):
            raise ValueError("esc_carry must be 0 or 1")
        if escape_scope not in ("all", "quoted"):
            raise ValueError("escape_scope must be 'all' or 'quoted'")
    if begin > end or begin < buf_base or end - buf_base > buf_len:
        raise ValueError("[begin, end) outside the buffer")
    if not 0 <= quote <= 255 or quote == 10:
        raise ValueError("quote must be a byte other than '\\n'")
    n = end - begin
    p = dev_addr + (begin - buf_base)
    if blocked:                                          # tiles on the object's 64 KiB grid
        if n and (p ^ begin) & 15:
            raise ValueError("blocked form: the device address of begin must be congruent to begin mod 16")
        shift = (begin & 0xFFFF) if n else 0
        obj0 = begin & ~0xFFFF
        ntiles = ((end - 1) >> 16) - (begin >> 16) + 1 if n else 0
    else:
        shift = (p & 15) if n else 0
        obj0 = (begin - shift) & M64
        ntiles = (shift + n + TILE_BYTES - 1) // TILE_BYTES if n else 0
    if ntiles >= MAX_TILES:
        raise ValueError("range too large for one launch")
    if escape is None:
        return Args(p - shift, shift, shift, shift + n, obj0, ntiles,
                    ((quote * 0x01010101) & M32) ^ SEL12, 0x0A0A0A0A ^ SEL12)
    return Args(p - shift, shift, shift, shift + n, obj0, ntiles,
                ((quote * 0x01010101) & M32) ^ SEL12, 0x0A0A0A0A ^ SEL12,
                ((escape * 0x01010101) & M32) ^ SEL12, esc_carry, 0xFFFF if escape_scope == "all" else 0, escape)


@dataclass
class Prepared:
    args: Args
    mutate: Optional[str]
    km: np.ndarray                   # [tiles, waves, rows, lanes]: kept if entered outside | inside << 16
    wpar: np.ndarray                 # [tiles, waves], as Shared holds them
    wk0: np.ndarray
    wk1: np.ndarray
    wq: np.ndarray
    tiles: List[Sum] = field(default_factory=list)
    n_quotes: int = 0
    n_newlines: int = 0
    blocked: bool = False            # tiles on the object's 64 KiB grid (quote_kernel<2>)
    n_toggles: int = 0               # escape-aware launches: the quotes that are not escaped (else n_quotes)
    esc_err: int = 0                 # escape-aware launches: the walk back met a run beyond ESCAPE_RUN_MAX


def launch_memory(buf: np.ndarray, dev_addr: int, a: Args, outside: bytes) -> np.ndarray:
    """The bytes of every 16-byte chunk the kernel loads, by coordinate: the chunks that hold a byte of [lo, hi).
    Bytes of those chunks that lie outside the buffer are whatever memory holds there: the pattern ``outside``.
    Chunks the kernel does not load stay zero, like its registers."""
    mem = np.zeros(a.ntiles * TILE_BYTES, np.uint8)
    if a.ntiles == 0:
        return mem
    first, top = a.lo & ~15, (a.hi + 15) & ~15           # the loaded chunks are coordinates [first, top); first = 0
    pat = np.resize(np.frombuffer(outside, np.uint8), 16)            # unless the form is blocked (lo up to 65535)
    mem[first:first + 16] = pat                          # [lo, hi) is inside the buffer: only the first and the
    mem[top - 16:top] = pat                              # last chunk can reach beyond it
    c0 = dev_addr - a.base_addr                          # coordinate of buf[0]
    x0, x1 = max(first, c0), min(top, c0 + len(buf))
    mem[x0:x1] = buf[x0 - c0:x1 - c0]
    return mem


def prepare(buf, dev_addr: int = 0, buf_base: int = 0, begin: Optional[int] = None, end: Optional[int] = None,
            quote: int = 34, mutate: Optional[str] = None, outside: bytes = b'"\n',
            blocked: bool = False, escape: Optional[int] = None, esc_carry: int = 0,
            escape_scope: str = "all") -> Prepared:
    """Host arithmetic, phase A and the tile summaries of one launch over ``buf`` (the buffer's bytes, object bytes
    [buf_base, buf_base + len(buf))) placed at device address ``dev_addr``; only dev_addr mod 16 matters."""
    _check_mutant(mutate)
    buf = np.asarray(buf, np.uint8)
    begin = buf_base if begin is None else begin
    end = buf_base + len(buf) if end is None else end
    a = host_args(dev_addr, len(buf), buf_base, begin, end, quote, blocked, escape, esc_carry, escape_scope)
    T = a.ntiles
    shape = (T, WAVES, ROWS, WAVE)
    if T == 0:
        z = np.zeros((0, WAVES), np.int64)
        return Prepared(a, mutate, np.zeros(shape, np.int64), z, z, z, z, blocked=blocked)
    mem = launch_memory(buf, dev_addr, a, outside)
    v = mem.view("<u4").reshape(shape + (4,))
    x = (np.arange(T * WAVES * ROWS * WAVE, dtype=np.int64) * 16).reshape(shape)     # x0 + row * kRowBytes
    loaded = (x < a.hi) & (x + 16 > a.lo)
    ok = np.where(loaded, valid16(np.where(loaded, x, a.lo), a.lo, a.hi, mutate), 0)
    q = mask16(v, a.key_q, mutate) & ok
    n = mask16(v, a.key_nl, mutate) & ok
    raw, esc_err = None, 0
    if a.escape is not None:
        q, n, raw, esc_err = escape_phase(mask16(v, a.key_e, mutate) & ok, x, q, n, a, mutate)
    px = q.copy()
    for s in (1, 2, 4, 8):
        px ^= (px << s) & M32
    odd = (popc(q) & 1) == 1                             # the ballot b of every row
    row_par = popcll_ballot(odd) & 1                     # [T, W, R]
    run_before = (np.cumsum(row_par, axis=-1) - row_par) & 1         # run when the row starts
    before = mbcnt(odd) & 1 if mutate == "no_run" else (mbcnt(odd) ^ run_before[..., None]) & 1
    inside = (px ^ ((0 - before) & M32)) & 0xFFFF
    k0, k1 = n & ~inside, n & inside
    km = k0 | (k1 << 16)
    cnt = (popc(k0) | (popc(k1) << 16)).sum(2) & M32     # per lane over the rows
    cnt = cnt.sum(-1) & M32                              # wave_sum
    nq = popc(q).sum(2).sum(-1) & M32
    if raw is not None:                                  # packed per lane: the quote bytes << 16 | the unescaped ones
        nq = (nq + ((raw.sum(2).sum(-1) << 16) & M32)) & M32
    P = Prepared(a, mutate, km, row_par.sum(-1) & 1, cnt & 0xFFFF, cnt >> 16, nq, blocked=blocked)
    for t in range(T):
        s = IDENT
        for w in range(WAVES):
            s = then(s, Sum(int(P.wpar[t, w]), int(P.wk0[t, w]), int(P.wk1[t, w])))
        P.tiles.append(s)
    P.n_quotes = int(P.wq.sum())                         # the atomicAdds of tq and tn
    P.n_toggles = P.n_quotes
    if raw is not None:                                  # wave 0 unpacks the halves before it adds the waves up
        P.n_quotes, P.n_toggles, P.esc_err = int((P.wq >> 16).sum()), int((P.wq & 0xFFFF).sum()), esc_err
    P.n_newlines = int((P.wk0 + P.wk1).sum())
    return P


# ------------------------------------------------------------------------------------------ look-back, phase B
def resolve(P: Prepared, carry: int, schedule="sequential", mutate: Optional[str] = None):
    """The incoming (state, base) of every tile and the PREFIX words, by look-back under ``schedule``; stats."""
    sched = get_schedule(schedule)
    T = P.args.ntiles
    agg = [pack_agg(t, mutate) for t in P.tiles]
    prefix: List[int] = []
    state_in, base = [0] * T, [0] * T
    stats = {"max_windows": 0, "spins": 0, "windows": [0] * T}
    for t in range(T):
        s, b = carry, 0
        if t != 0:
            s, b, windows, spins = look_back(t, carry, lambda n, t=t: sched(t, n, agg, prefix), mutate)
            stats["windows"][t] = windows
            stats["max_windows"] = max(stats["max_windows"], windows)
            stats["spins"] += spins
        state_in[t], base[t] = s, b
        incl = b + (P.tiles[t].k1 if s else P.tiles[t].k0)
        prefix.append(pack_prefix(s ^ P.tiles[t].par, incl))
    n_out = unpack_prefix(prefix[-1])[1] if T else 0     # ctrl[kCtrlOut] = incl of the last tile
    return state_in, base, n_out, stats


def phase_b(P: Prepared, state_in, base, u64: bool, cap: int, out: np.ndarray, u16b: bool = False,
            mutate: Optional[str] = None) -> int:
    """The stores of phase B into ``out`` (entries at or beyond ``cap`` are never written); returns the overflow
    flag and the number of stores that fell beyond ``out`` itself.  ``u16b``: the low words of the blocked form."""
    T = P.args.ntiles
    if T == 0:
        return 0, 0
    st = np.asarray(state_in, np.int64)                  # the wave's incoming state and base
    wbase = np.zeros((T, WAVES), np.int64)
    wst = np.zeros((T, WAVES), np.int64)
    b = np.asarray(base, np.int64).copy()
    for w in range(WAVES):
        wbase[:, w], wst[:, w] = b, st
        b = b + np.where(st != 0, P.wk1[:, w], P.wk0[:, w])
        st = st ^ P.wpar[:, w]
    sh = np.where(wst != 0, 16, 0)[:, :, None, None]
    kept = (P.km >> sh) & 0xFFFF
    c = popc(kept)                                       # 0..16
    one = (c != 0)
    single = ~(c > 1).any(-1)                            # __ballot(c > 1u) == 0
    ex1, tot1 = mbcnt(one), popcll_ballot(one)
    ex5, tot5 = np.zeros_like(c), np.zeros_like(tot1)
    for bit in range(5):
        m = ((c >> bit) & 1) != 0
        ex5 += mbcnt(m) << bit
        tot5 += popcll_ballot(m) << bit
    ex = np.where(single[..., None], ex1, ex5)
    total = np.where(single, tot1, tot5)                 # a row with any == 0 adds 0 either way
    row_base = wbase[:, :, None] + np.cumsum(total, axis=-1) - total
    i0 = (row_base[..., None] + ex).reshape(-1)          # the lane's first index
    if cap == 0 and (u64 or u16b):
        return 0, 0                                      # nothing is stored and nothing can overflow
    bits = np.unpackbits(kept.astype("<u2").reshape(-1, 1).view(np.uint8), axis=1, bitorder="little")
    ch, bit = np.nonzero(bits)                           # chunk by chunk, lowest bit first: the while (kept) loop
    cc = c.reshape(-1)
    first = np.cumsum(cc) - cc
    i = i0[ch] + (np.arange(len(ch)) - first[ch])
    o = np.uint64(P.args.obj0) + (ch.astype(np.uint64) * np.uint64(16) + bit.astype(np.uint64))   # mod 2^64
    over = (o >> np.uint64(32)) != 0 if not (u64 or u16b) else np.zeros(len(o), bool)
    if u16b and mutate == "low_from_shifted":            # the coordinate of the other forms: from the 16-byte boundary
        o = o - np.uint64(P.args.lo & ~15)               # at or below the first byte, not from the 64 KiB one
    w = ~over & (i < cap)
    stray = w & (i >= len(out))                          # beyond every possible count: only a mutant stores there
    w &= ~stray
    if u16b:
        out[i[w]] = (o[w] & np.uint64(0xFFFF)).astype(np.uint16)
    else:
        out[i[w]] = o[w] if u64 else (o[w] & np.uint64(M32)).astype(np.uint32)
    return int(over.any()), int(stray.sum())


def table_stores(P: Prepared, state_in, base, table: np.ndarray, mutate: Optional[str] = None) -> None:
    """Wave 0's block table stores of the blocked form: table[tile] = the tile's exclusive base, after its
    look-back, for every tile of the launch (0 for tile 0) -- whatever ``cap`` is."""
    for t in range(P.args.ntiles):
        if mutate == "table_skip_tile0" and t == 0:
            continue
        v = base[t]
        if mutate == "table_inclusive":
            v += P.tiles[t].k1 if state_in[t] else P.tiles[t].k0
        table[t] = v


def finish(P: Prepared, carry: int = 0, u64: bool = True, cap: Optional[int] = None, schedule="sequential",
           mutate: Optional[str] = None, stats: Optional[dict] = None, fmt: Optional[str] = None):
    """(offsets, n_out, n_quotes, n_newlines, err_bits) of the prepared launch.  ``cap=None`` is room for every
    newline; ``cap=0`` is the count-only launch (no capacity error).  ``offsets`` are the first min(n_out, cap)
    entries of the output array; ``stats`` receives the look-back statistics and the whole output array
    ("out_raw", CANARY where nothing was stored).

    ``fmt="u16b"`` (a launch prepared with ``blocked=True``): (low, table, n_out, n_quotes, n_newlines, err_bits),
    the uint16 low words below ``cap`` and the ``ntiles`` block table entries; ``stats`` also receives the whole
    table array ("table_raw", CANARY beyond the tiles)."""
    if fmt not in (None, "u16b"):
        raise ValueError(f"fmt={fmt!r}: None (the uint32 / uint64 forms, by u64=) or 'u16b'")
    u16b = fmt == "u16b"
    if u16b != P.blocked:
        raise ValueError("fmt='u16b' goes with a launch prepared with blocked=True, and only with it")
    _check_mutant(mutate)
    if carry not in (0, 1):
        raise ValueError("carry must be 0 or 1")
    mutate = mutate or P.mutate
    state_in, base, n_out, st = resolve(P, carry, schedule, mutate)
    count_only = cap == 0
    cap = P.n_newlines if cap is None else cap
    dt = np.uint16 if u16b else (np.uint64 if u64 else np.uint32)
    out = np.full(min(cap, P.n_newlines) + 64, CANARY & (2 ** (8 * np.dtype(dt).itemsize) - 1), dt)
    overflow, stray = phase_b(P, state_in, base, u64, cap, out, u16b, mutate)
    err = ERR_OVERFLOW if overflow else 0
    if n_out > cap and not count_only:
        err |= ERR_CAPACITY
    if stray:
        err |= ERR_STRAY
    if P.esc_err:
        err |= ERR_ESCAPE_RUN
    if stats is not None:
        stats.update(st, out_raw=out, state_in=state_in, base=base, n_toggles=P.n_toggles)
    if u16b:
        table = np.full(P.args.ntiles + 8, CANARY, np.uint64)
        table_stores(P, state_in, base, table, mutate)
        if stats is not None:
            stats.update(table_raw=table)
        return out[:min(n_out, cap)], table[:P.args.ntiles], n_out, P.n_quotes, P.n_newlines, err
    return out[:min(n_out, cap)], n_out, P.n_quotes, P.n_newlines, err


def run(buf, dev_addr: int = 0, buf_base: int = 0, begin: Optional[int] = None, end: Optional[int] = None,
        quote: int = 34, carry: int = 0, u64: bool = True, cap: Optional[int] = None, schedule="sequential",
        mutate: Optional[str] = None, outside: bytes = b'"\n', stats: Optional[dict] = None,
        fmt: Optional[str] = None, escape: Optional[int] = None, esc_carry: int = 0, escape_scope: str = "all"):
    """One launch, as ScanContext.records_async + records_result see it:
    (offsets, n_out, n_quotes, n_newlines, err_bits); with ``fmt="u16b"`` as ``form="u16b"`` does:
    (low, table, n_out, n_quotes, n_newlines, err_bits)."""
    if fmt not in (None, "u16b"):
        raise ValueError(f"fmt={fmt!r}: None (the uint32 / uint64 forms, by u64=) or 'u16b'")
    return finish(prepare(buf, dev_addr, buf_base, begin, end, quote, mutate, outside, fmt == "u16b", escape,
                          esc_carry, escape_scope), carry, u64, cap, schedule, mutate, stats, fmt)
