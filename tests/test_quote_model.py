"""Lane-exact numpy model of quote_kernel (tools/emulate_quote.py) against the definition (tests/_quote_model.py),
without a GPU: the kernel's bit formulas, its descriptor words, both phase-B scan paths and -- the part no GPU test
can steer -- the decoupled look-back under schedules chosen here: every predecessor a PREFIX, none, random mixes, and
the first PREFIX on either side of a 64-descriptor window edge.  tests/test_gpu_quote.py pins the model's idea of the
instructions to the hardware; the look-back's multi-window paths are shown correct here only.  Every deliberate defect
of ``emulate_quote.MUTANTS`` must make at least one case below disagree with the definition."""
import os
import re
import sys

import numpy as np
import pytest

from _quote_cases import ALPHABET, mixed_0_1_16, odd_tiles, one_lane_16
from _quote_model import record_ends

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))
import emulate_quote as emu  # noqa: E402

T = emu.TILE_BYTES
LOOKBACK_TILES = 130
SCHEDULES = ["sequential", "all_agg", "chain_to_tile0", "window_edge"] + \
    [f"window_edge:{ln}" for ln in emu.WINDOW_EDGE_LANES] + [f"random:{s}" for s in range(6)]
PHASE_A_MUTANTS = ("no_run", "valid_hi_plus_one", "unsigned_dot")


def agrees(buf, lo, hi, buf_base=0, mis=0, carry=0, u64=True, quote=34, schedule="sequential", mutate=None):
    """The model's launch over buffer bytes [lo, hi) equals the definition: offsets, n_out and both counts."""
    got, n_out, nq, nn, err = emu.run(buf, dev_addr=4096 + mis, buf_base=buf_base, begin=buf_base + lo,
                                      end=buf_base + hi, quote=quote, carry=carry, u64=u64, schedule=schedule,
                                      mutate=mutate)
    exp, eq, en = record_ends(buf[lo:hi], base=buf_base + lo, quote=quote, carry=carry)
    return (got.dtype == (np.uint64 if u64 else np.uint32) and err == 0 and (n_out, nq, nn) == (len(exp), eq, en)
            and np.array_equal(got.astype(np.uint64), exp))


# ------------------------------------------------------------------------------------------ the instructions
def test_perm_table_is_zero_for_selector_12_only():
    assert emu.PERM_FF[0x0C] == 0 and np.all(np.delete(emu.PERM_FF, 0x0C) == 0xFF)
    assert emu.v_perm_byte(0x44332211, 0x88776655, 0) == 0x55 and emu.v_perm_byte(0x44332211, 0x88776655, 7) == 0x44
    assert emu.v_perm_byte(0, 0x80000000, 9) == 0xFF and emu.v_perm_byte(0, 0x80000000, 8) == 0x00


@pytest.mark.parametrize("pos", range(16))
def test_mask16_every_quote_byte_against_every_data_byte(pos):
    rng = np.random.default_rng(pos)
    chunks = rng.integers(0, 256, (256, 16), dtype=np.uint8)         # the other 15 bytes: anything
    chunks[:, pos] = np.arange(256)                                  # every data byte at this position
    v = chunks.view("<u4")
    for q in range(256):                                             # (10 is the newline key itself)
        key = ((q * 0x01010101) & 0xFFFFFFFF) ^ emu.SEL12
        exp = ((chunks == q) << np.arange(16)).sum(1)
        got = emu.mask16(v, key)
        assert np.array_equal(got, exp), (pos, q)
        assert np.array_equal((got >> pos) & 1, np.arange(256) == q)
    assert emu.host_args(0, 16, 0, 0, 16, 11).key_nl == 0x0A0A0A0A ^ emu.SEL12


def test_valid16_is_the_bytes_inside_the_range():
    for lo in (0, 3, 15):
        for hi in range(lo + 1, 70):
            x = np.arange(0, 80, 16)
            x = x[(x < hi) & (x + 16 > lo)]
            exp = [sum(1 << i for i in range(16) if lo <= xi + i < hi) for xi in x]
            assert list(emu.valid16(x, lo, hi)) == exp, (lo, hi)


def test_host_arguments():
    a = emu.host_args(dev_addr=0x7F0005, buf_len=5000, buf_base=1000, begin=1007, end=1007 + 4096, quote=0x0C)
    assert (a.shift, a.lo, a.hi, a.ntiles) == (12, 12, 12 + 4096, 1) and a.base_addr == 0x7F0000
    assert a.obj0 == 1007 - 12 and a.key_q == 0 and a.key_nl == 0x06060606
    assert emu.host_args(5, 100, 0, 0, 100).obj0 == (1 << 64) - 5            # coordinate 0 lies before the object
    assert emu.host_args(5, 100, 0, 40, 40).ntiles == 0
    assert emu.host_args(15, 2 * T, 0, 0, 2 * T - 15).ntiles == 2 and emu.host_args(15, 2 * T, 0, 0, 2 * T - 14).ntiles == 3
    for bad in ((0, 10, 5, 4, 9), (0, 10, 5, 5, 16)):
        with pytest.raises(ValueError):
            emu.host_args(*bad)
    with pytest.raises(ValueError):
        emu.host_args(0, 10, 0, 0, 10, quote=10)


# ------------------------------------------------------------------------------------------ lengths and placement
LENGTHS = (0, 1, 15, 16, 17, T - 1, T, T + 1, 2 * T + 5)


def padded(n, seed):
    """n + 40 bytes of ALPHABET; outside [7, 7 + n) quotes and newlines alternate."""
    buf = ALPHABET[np.random.default_rng(seed).integers(0, 4, n + 40)].copy()
    pad = np.resize(np.frombuffer(b'\n"', np.uint8), n + 40)
    buf[:7], buf[7 + n:] = pad[:7], pad[7 + n:]
    return buf


def placement_cases(mutate=None):
    """(label, agrees) of every length x device-address offset x carry x width, the range inside its buffer."""
    for n in LENGTHS:
        buf = padded(n, n)
        for mis in (0, 5, 15):
            for carry in (0, 1):
                for u64 in (True, False):
                    yield (n, mis, carry, u64), agrees(buf, 7, 7 + n, buf_base=1_000_003, mis=mis, carry=carry,
                                                       u64=u64, schedule="all_agg" if carry else "sequential",
                                                       mutate=mutate)
        yield (n, "head"), agrees(buf[7:], 0, n, mis=0, mutate=mutate)


def test_lengths_and_placement():
    bad = [label for label, ok in placement_cases() if not ok]
    assert bad == []


@pytest.mark.parametrize("quote", [0x00, 0x0C, 0x80, 0xFF, 39])
def test_unusual_quote_bytes(quote):
    rng = np.random.default_rng(quote)
    buf = np.array([quote, 10, 0, 0x0C, 0x80, 0xFF, 97, 34], np.uint8)[rng.integers(0, 8, T + 77)]
    for mis in (0, 11):
        for carry in (0, 1):
            assert agrees(buf, 3, T + 50, buf_base=9, mis=mis, carry=carry, quote=quote)


# ------------------------------------------------------------------------------------------ look-back
@pytest.fixture(scope="module")
def many_tiles():
    """130 tiles, every one of odd quote parity; phase A once (it depends on neither the carry nor the schedule)."""
    buf = odd_tiles((LOOKBACK_TILES - 1) * T + 12345, T, seed=7)
    P = emu.prepare(buf)
    assert P.args.ntiles == LOOKBACK_TILES and all(t.par == 1 for t in P.tiles)
    assert len({(t.k0, t.k1) for t in P.tiles}) > 100 and sum(t.k0 != t.k1 for t in P.tiles) > 100
    return buf, P, {c: record_ends(buf, carry=c) for c in (0, 1)}


def lookback_agrees(many, carry, schedule, mutate=None, stats=None):
    _, P, model = many
    exp, eq, en = model[carry]
    got, n_out, nq, nn, err = emu.finish(P, carry=carry, schedule=schedule, mutate=mutate, stats=stats)
    return err == 0 and (n_out, nq, nn) == (len(exp), eq, en) and np.array_equal(got, exp)


@pytest.mark.parametrize("carry", [0, 1])
@pytest.mark.parametrize("schedule", SCHEDULES)
def test_every_schedule_gives_the_definition(many_tiles, schedule, carry):
    st = {}
    assert lookback_agrees(many_tiles, carry, schedule, stats=st)
    last = st["windows"][LOOKBACK_TILES - 1]
    if schedule in ("all_agg", "chain_to_tile0"):
        assert last == 3                                 # tiles 128..65, 64..1, then tile 0 / the virtual PREFIX
    if schedule == "window_edge:64":
        assert last == 2 and st["windows"][65] == 2 and st["windows"][64] == 1
    if schedule in ("window_edge:63", "window_edge:0", "window_edge:1", "sequential"):
        assert st["max_windows"] == 1
    if schedule == "window_edge":
        assert sorted(set(st["windows"][65:])) == [1, 2]
    if schedule == "random:5":
        assert st["max_windows"] >= 2 and st["spins"] > 0


def test_look_back_window_steps():
    """One window at a time: spin, next, done; the virtual PREFIX carries the launch's state."""
    s = [emu.Sum(1, 5, 2), emu.Sum(1, 1, 7), emu.Sum(0, 3, 3)]
    agg = [emu.pack_agg(x) for x in s]
    assert [emu.unpack_agg(a) for a in agg] == s
    assert emu.look_back_window([agg[0], 0, agg[2]], 2, emu.IDENT, 0) == ("spin",)
    assert emu.look_back_window([0, emu.pack_prefix(1, 100), agg[2]], 2, emu.IDENT, 0) == ("done", 1, 103)
    f = emu.then(s[0], emu.then(s[1], s[2]))
    assert emu.look_back_window(agg, 2, emu.IDENT, 1) == ("done", 1 ^ f.par, f.k1)
    assert emu.look_back_window(agg, 2, emu.IDENT, 0) == ("done", f.par, f.k0)
    many = [agg[i % 3] for i in range(70)]
    kind, f64, j = emu.look_back_window(many, 69, emu.IDENT, 0)
    assert (kind, j) == ("next", 5) and f64.par == sum(s[i % 3].par for i in range(6, 70)) % 2


# ------------------------------------------------------------------------------------------ descriptor extremes
def test_descriptor_fields_at_their_extremes():
    full = emu.Sum(1, 65536, 65536)
    a = emu.pack_agg(full)
    assert a >> 62 == 1 and emu.unpack_agg(a) == full and a < 1 << 64
    p = emu.pack_prefix(1, (1 << 48) - 1)
    assert p >> 62 == 2 and emu.unpack_prefix(p) == (1, (1 << 48) - 1)
    assert emu.unpack_prefix(emu.pack_prefix(0, (1 << 48) + 5)) == (0, 5)

    nl = np.full(T, 10, np.uint8)
    P = emu.prepare(nl)
    assert P.tiles == [emu.Sum(0, 65536, 0)] and list(P.wk0[0]) == [16384] * 4
    assert emu.finish(P, carry=0)[1] == T and emu.finish(P, carry=1)[1] == 0
    qnl = nl.copy()
    qnl[0] = 34
    assert emu.prepare(qnl).tiles == [emu.Sum(1, 0, 65535)]
    two = np.concatenate([qnl, nl])                      # the second tile is entered inside: its kept1 = 0 counts
    for sched in ("sequential", "all_agg"):
        assert agrees(two, 0, 2 * T, schedule=sched) and agrees(two, 0, 2 * T, carry=1, schedule=sched)

    q = np.full(T, 34, np.uint8)
    P = emu.prepare(q)
    assert P.tiles == [emu.Sum(0, 0, 0)] and P.n_quotes == T and list(P.wq[0]) == [16384] * 4
    assert emu.prepare(q[:T - 1]).tiles == [emu.Sum(1, 0, 0)]
    assert agrees(np.concatenate([q[:T - 1], nl]), 0, 2 * T - 1, mis=1, schedule="all_agg")


def test_prefix_count_carries_into_the_high_bits():
    n = LOOKBACK_TILES * T
    nl = np.full(n, 10, np.uint8)
    P = emu.prepare(nl)
    for sched in ("sequential", "all_agg", "window_edge:64"):
        st = {}
        assert emu.finish(P, carry=0, cap=0, schedule=sched, stats=st)[1:] == (n, 0, n, 0)
        assert st["base"][LOOKBACK_TILES - 1] == n - T > 1 << 23
        assert emu.finish(P, carry=1, cap=0, schedule=sched)[1:] == (0, 0, n, 0)
    nl[0] = 34
    P = emu.prepare(nl)
    assert emu.finish(P, carry=1, cap=0, schedule="all_agg")[1:] == (n - 1, 1, n - 1, 0)
    assert emu.finish(P, carry=0, cap=0, schedule="all_agg")[1:] == (0, 1, n - 1, 0)


# ------------------------------------------------------------------------------------------ phase B
def phase_b_cases(mutate=None):
    for name, buf in (("one_lane_16", one_lane_16(T + 4000, 1)), ("mixed_0_1_16", mixed_0_1_16(T + 4000, 2))):
        for mis in (0, 9):
            for carry in (0, 1):
                yield (name, mis, carry), agrees(buf, 2, len(buf) - 1, buf_base=11, mis=mis, carry=carry,
                                                 u64=bool(carry), mutate=mutate)


def test_phase_b_scan_paths():
    buf = one_lane_16(8192, 1)
    chunks = (buf[:8192].reshape(-1, 64, 16) == 10).sum(2)           # newlines per row and lane
    assert np.all((chunks == 16).sum(1) == 1) and np.all((chunks == 0).sum(1) == 63)
    chunks = (mixed_0_1_16(1 << 16, 2).reshape(-1, 64, 16) == 10).sum(2)
    assert set(np.unique(chunks)) == {0, 1, 16}
    assert np.any(np.all(chunks <= 1, 1) & np.any(chunks == 1, 1))              # one-ballot rows occur as well
    assert [label for label, ok in phase_b_cases() if not ok] == []


def test_cap_clips_the_stores_not_the_count():
    buf = ALPHABET[np.random.default_rng(4).integers(0, 4, T + 4096)]
    for carry in (0, 1):
        exp, eq, en = record_ends(buf, base=50, carry=carry)
        n = len(exp)
        for u64 in (True, False):
            for cap in (0, 1, n - 1, n):
                st = {}
                got, n_out, nq, nn, err = emu.run(buf, buf_base=50, carry=carry, u64=u64, cap=cap, stats=st)
                assert (n_out, nq, nn) == (n, eq, en)
                assert err == (emu.ERR_CAPACITY if 0 < cap < n else 0)
                assert np.array_equal(got.astype(np.uint64), exp[:cap])
                raw = st["out_raw"]
                assert len(raw) > cap and np.all(raw[cap:] == raw.dtype.type(emu.CANARY & (2 ** (8 * raw.itemsize) - 1)))


def test_uint32_overflow_flag():
    base = (1 << 32) - 100
    buf = np.full(300, 10, np.uint8)
    got, n_out, _, _, err = emu.run(buf, buf_base=base, u64=False)
    assert err == emu.ERR_OVERFLOW and n_out == 300
    assert np.array_equal(got[:100], np.arange(base, 1 << 32, dtype=np.uint64).astype(np.uint32))
    assert agrees(buf, 0, 300, buf_base=base, u64=True)
    assert agrees(buf, 0, 100, buf_base=base, u64=False)             # wholly below 2^32
    assert agrees(buf, 0, 100, buf_base=base, mis=13, u64=False)


# ------------------------------------------------------------------------------------------ mutants
def killers(many, mutate):
    """The cases above that disagree with the definition under ``mutate``, lazily."""
    if mutate not in PHASE_A_MUTANTS:                    # look-back and descriptor defects: the 130 tiles
        yield from (("look-back", s, c) for s in SCHEDULES for c in (0, 1) if not lookback_agrees(many, c, s, mutate))
    yield from (("placement",) + label for label, ok in placement_cases(mutate) if not ok)
    yield from (("phase B",) + label for label, ok in phase_b_cases(mutate) if not ok)


@pytest.mark.parametrize("mutate", emu.MUTANTS)
def test_every_mutant_is_killed(many_tiles, mutate):
    first = next(killers(many_tiles, mutate), None)      # the first case that notices is enough
    print(mutate, "killed by", first)
    assert first is not None, f"the defect {mutate!r} changes no result of this file: add the case that notices it"


def test_unknown_mutant_and_schedule_are_refused():
    with pytest.raises(ValueError):
        emu.run(np.zeros(4, np.uint8), mutate="none")
    with pytest.raises(ValueError):
        emu.run(np.zeros(T + 1, np.uint8), schedule="lucky")


# ------------------------------------------------------------------------------------------ drift guard
def kernel_constants(text):
    """The constants of dpquote.hip that the model copies, read out of its source."""
    def one(pattern, base=10):
        m = re.findall(pattern, text)
        assert len(m) == 1, (pattern, m)
        return int(m[0], base)
    agg = re.findall(r"kStatAgg \| \(\(uint64_t\)t\.par << (\d+)\) \| \(t\.k1 << (\d+)\) \| t\.k0\)", text)
    unp = re.findall(r"Sum s\{\(uint32_t\)\(a >> (\d+)\) & 1u, a & 0x([0-9A-Fa-f]+)ull, \(a >> (\d+)\) & 0x([0-9A-Fa-f]+)ull\}",
                     text)
    assert len(agg) == 1 and len(unp) == 1, (agg, unp)
    return {
        "WAVE": one(r"constexpr int kWave = (\d+);"),
        "WAVES": one(r"constexpr int kWaves = (\d+);"),
        "ROWS": one(r"constexpr int kRows = (\d+);"),
        "CTRL_WORDS": one(r"constexpr int kCtrlWords = (\d+);"),
        "SEL12": one(r"constexpr uint32_t kSel12 = 0x([0-9A-Fa-f]+)u;", 16),
        "COUNT_MASK": one(r"constexpr uint64_t kCountMask = 0x([0-9A-Fa-f]+)ull;", 16),
        "STAT_AGG": 1 << one(r"constexpr uint64_t kStatAgg = 1ull << (\d+);"),
        "STAT_PREFIX": 2 << one(r"constexpr uint64_t kStatPrefix = 2ull << (\d+);"),
        "STATUS_SHIFT": one(r"const uint32_t st = \(uint32_t\)\(d >> (\d+)\);"),
        "AGG_PAR_SHIFT": (int(agg[0][0]), int(unp[0][0])),
        "AGG_K1_SHIFT": (int(agg[0][1]), int(unp[0][2])),
        "AGG_K_MASK": (int(unp[0][1], 16), int(unp[0][3], 16)),
        "PREFIX_STATE_SHIFT": (one(r"kStatPrefix \| \(\(uint64_t\)\(state_in \^ t\.par\) << (\d+)\)"),
                               one(r"kStatPrefix \| \(\(uint64_t\)A\.carry << (\d+)\)"),
                               one(r"const uint32_t s = \(uint32_t\)\(p >> (\d+)\) & 1u;")),
        "DOT_WEIGHTS": tuple(int(x, 16) for x in re.findall(r"__builtin_amdgcn_sdot4\([^,]+, key\), 0x([0-9A-Fa-f]+),", text)),
        "DOT_ACC": tuple(int(x, 16) for x in re.findall(r"__builtin_amdgcn_sdot4\([^,]+, key\), 0x[0-9A-Fa-f]+, (?:0x)?([0-9A-Fa-f]+),", text)),
    }


def model_constants():
    return {
        "WAVE": emu.WAVE, "WAVES": emu.WAVES, "ROWS": emu.ROWS, "CTRL_WORDS": emu.CTRL_WORDS, "SEL12": emu.SEL12,
        "COUNT_MASK": emu.COUNT_MASK, "STAT_AGG": emu.STAT_AGG, "STAT_PREFIX": emu.STAT_PREFIX,
        "STATUS_SHIFT": emu.STATUS_SHIFT, "AGG_PAR_SHIFT": (emu.AGG_PAR_SHIFT,) * 2,
        "AGG_K1_SHIFT": (emu.AGG_K1_SHIFT,) * 2, "AGG_K_MASK": (emu.AGG_K_MASK,) * 2,
        "PREFIX_STATE_SHIFT": (emu.PREFIX_STATE_SHIFT,) * 3, "DOT_WEIGHTS": (emu.DOT_WEIGHTS,) * 4,
        "DOT_ACC": (emu.DOT_ACC0, 0, 0, 0),
    }


def kernel_source():
    with open(os.path.join(REPO, "dataplug_amd", "csrc", "dpquote.hip")) as f:
        return f.read()


def test_model_constants_are_the_kernels():
    assert kernel_constants(kernel_source()) == model_constants()
    assert emu.TILE_BYTES == emu.WAVE * 16 * emu.ROWS * emu.WAVES == 1 << 16


@pytest.mark.parametrize("old,new", [
    ("constexpr int kRows = 16;", "constexpr int kRows = 8;"),
    ("constexpr int kWaves = 4;", "constexpr int kWaves = 8;"),
    ("constexpr int kCtrlWords = 8;", "constexpr int kCtrlWords = 16;"),
    ("kSel12 = 0x0C0C0C0Cu", "kSel12 = 0x0D0D0D0Du"),
    ("(t.k1 << 24)", "(t.k1 << 32)"),
    ("(a >> 24) & 0xFFFFFFull", "(a >> 16) & 0xFFFFFFull"),
    ("(uint64_t)A.carry << 48", "(uint64_t)A.carry << 49"),
    ("0x08040201, 0xFFFF, false", "0x08040201, 0xFFF, false"),
])
def test_drift_guard_notices_an_edited_kernel(old, new):
    text = kernel_source()
    assert text.count(old) >= 1
    edited = text.replace(old, new, 1)
    assert kernel_constants(edited) != model_constants()

