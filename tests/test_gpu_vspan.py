"""vspan_span_kernel and vspan_blockmax_kernel (libdpvspan.so) through the C ABI, every output array bit-equal to the
definition's byte loop (tests/_vspan_loop.py), with sentinel entries on both sides of every output array.  The lines
of a workgroup come from dvs_geometry."""
import ctypes
import functools

import numpy as np
import pytest

import _vcfpos_loop as P
import _vspan_loop as L
from _vspan_cases import BIG_REF, CASES, line
from dataplug_amd.scan import _vspan

pytestmark = pytest.mark.gpu

BASE = 1_000_003                                         # an odd buf_base
S32, S8, S64 = 0xDEADBEEF, 0xAB, 0x0123456789ABCDEF      # the sentinels around the output arrays
POISON = b"\tEND=7;\t\n"                                 # behind the buffer: bytes that would end a field or a line


@pytest.fixture(scope="module")
def geo(ctx):
    g = ctx.vspan_geometry()
    assert g[0] >= 64 and g[1] >= g[0] and g[0] % 64 == 0 and g[1] % 64 == 0
    return g


def launch(ctx, buf: bytes, starts, pos, base=BASE, size=None, mis=0, ordinal0=0, every=1):
    """One span launch and one block-max launch over ``buf`` = object bytes from ``base``, at device alignment ``mis``:
    (end, flags, slots, result words), after the sentinels around each array were found untouched."""
    v, h = ctx._vspan_ctx()
    n = len(starts)
    size = base + len(buf) if size is None else size
    ns = L.n_slots(ordinal0, n, every)
    d = ctx.workspace("vspan_test_in", len(buf) + 160)
    assert d.ptr % 16 == 0
    ctx.h2d(d.ptr, np.frombuffer(b"\t" * mis + buf + POISON * 8, np.uint8))
    ws = ctx.workspace("vspan_test_lines", 12 * n + 64)
    d_starts, d_pos = ws.ptr, ws.ptr + 8 * n + 8
    if n:
        ctx.h2d(d_starts, np.asarray(starts, np.uint64))
        ctx.h2d(d_pos, np.asarray(pos, np.uint32))
    wo = ctx.workspace("vspan_test_out", 4 * (n + 2) + (n + 2) + 8 + 4 * (ns + 2) + 8 * (_vspan.R_WORDS + 2) + 64)
    d_end = wo.ptr
    d_flags = d_end + 4 * (n + 2)
    d_max = (d_flags + n + 2 + 7) & ~7
    d_res = (d_max + 4 * (ns + 2) + 7) & ~7
    ctx.h2d(d_end, np.full(n + 2, S32, np.uint32))
    ctx.h2d(d_flags, np.full(n + 2, S8, np.uint8))
    ctx.h2d(d_max, np.full(ns + 2, S32, np.uint32))
    ctx.h2d(d_res, np.full(_vspan.R_WORDS + 2, S64, np.uint64))
    p = ctypes.c_void_p
    _vspan.check(v.dvs_span_async(h, p(d.ptr + mis), len(buf), base, size, p(d_starts), n, p(d_pos), p(d_end + 4),
                                  p(d_flags + 1)))
    _vspan.check(v.dvs_blockmax_async(h, p(d_end + 4), p(d_flags + 1), p(d_pos), n, ordinal0, every, p(d_max + 4),
                                      p(d_res + 8)))
    end = ctx.d2h(np.empty(n + 2, np.uint32), d_end)
    flags = ctx.d2h(np.empty(n + 2, np.uint8), d_flags)
    slots = ctx.d2h(np.empty(ns + 2, np.uint32), d_max)
    res = ctx.d2h(np.empty(_vspan.R_WORDS + 2, np.uint64), d_res)
    assert end[0] == end[-1] == S32 and flags[0] == flags[-1] == S8, "a line output's sentinel was written"
    assert slots[0] == slots[-1] == S32 and res[0] == res[-1] == S64, "a slot's or a result word's sentinel was written"
    return end[1:-1].tolist(), flags[1:-1].tolist(), slots[1:-1].tolist(), res[1:-1].tolist()


@functools.lru_cache(maxsize=8)
def lines_of(buf: bytes, base: int, size: int):
    """(starts, POS) of the lines of ``buf`` by the position loop, computed once per buffer."""
    starts = [base + s for s in P.line_starts(buf, 0)]
    return starts, P.loop_parse(buf, base, size, starts)[0]


@functools.lru_cache(maxsize=8)
def want_span(buf: bytes, base: int, size: int, starts: tuple, pos: tuple):
    return L.loop_span(buf, base, size, starts, pos)


def check(ctx, buf: bytes, starts=None, pos=None, base=BASE, size=None, mis=0, ordinal0=0, every=1):
    size = base + len(buf) if size is None else size
    if starts is None:
        starts, pos = lines_of(buf, base, size)
    elif pos is None:
        pos = P.loop_parse(buf, base, size, starts)[0]
    end, flags, slots, res = launch(ctx, buf, starts, pos, base, size, mis, ordinal0, every)
    w_end, w_flags = want_span(buf, base, size, tuple(starts), tuple(pos))
    for g, w, name in ((end, w_end, "end"), (flags, w_flags, "flags")):
        assert g == w, (name, mis, [(i, a, b) for i, (a, b) in enumerate(zip(g, w)) if a != b][:5])
    w_slots, w = L.loop_blockmax(w_end, w_flags, pos, ordinal0, every)
    assert slots == w_slots and len(slots) == L.n_slots(ordinal0, len(starts), every), (ordinal0, every)
    assert res == [w["n_missing"], w["n_truncated"], w["n_from_end"], w["max_span"], w["min_missing"],
                   w["min_truncated"]], (ordinal0, every)
    return end, flags, slots, res


def test_hand_written_lines_at_every_alignment(ctx):
    closed = [c for c in CASES if c[1].endswith(b"\n")]
    opened = [c for c in CASES if not c[1].endswith(b"\n")]
    assert len(opened) >= 2 and len(closed) >= 35
    for tail in [None] + opened:                                         # an unterminated line ends its own object
        cases = closed + ([tail] if tail else [])
        buf = b"".join(c[1] for c in cases)
        for mis in range(4):                                             # every byte alignment of every line's start
            end, flags, _, _ = check(ctx, buf, mis=mis, every=2)
            assert end == [c[3] for c in cases] and flags == [c[4] for c in cases]
    # the same lines, their four alignments inside one dword-aligned buffer
    for pad in range(4):
        buf = b"x" * pad + b"\n" + b"".join(c[1] for c in closed)
        check(ctx, buf, starts=[BASE + s for s in P.line_starts(buf, 0)][1:], every=128)


def body_lines(n: int, seed: int = 0) -> bytes:
    """``n`` lines of 83 bytes: reference blocks, REF of a few bases and the odd far END."""
    rng = np.random.default_rng(seed)
    v = rng.integers(0, 1 << 30, (n, 3))
    out = []
    for i in range(n):
        p = 1000 + 7 * i
        info = (b"END=%d" % (p + int(v[i, 0] % 90)), b"DP=%d" % int(v[i, 0] % 90), b"X=1;END=%d" % (p + 10**5))[
            0 if v[i, 1] % 8 < 5 else 1 if v[i, 1] % 8 < 7 else 2]
        row = b"chr1\t%d\t.\t%s\tC\t.\t.\t%s\tGT\t" % (p, b"ACGT"[:1 + int(v[i, 2] % 4)], info)
        out.append(row + b"0" * (82 - len(row)) + b"\n")
    assert all(len(x) == 83 for x in out)
    return b"".join(out)


def test_line_counts_around_the_geometry_and_every_block_phase(ctx, geo):
    counts = sorted({1} | {c for g in geo for c in (g - 1, g, g + 1, 2 * g + 1)})
    for n in counts:
        buf = body_lines(n, seed=n)
        for every in (1, 2, 128):
            for ordinal0 in sorted({0, 1, every - 1, every, 3 * every + 5}):
                _, _, slots, res = check(ctx, buf, ordinal0=ordinal0, every=every)
                assert len(slots) == (ordinal0 + n - 1) // every - ordinal0 // every + 1
                assert res[0] == res[1] == 0 and (n < 20 or res[3] == 10**5)
    assert launch(ctx, b"", [], [], ordinal0=9, every=4) == ([], [], [], [0, 0, 0, 0, L.NONE, L.NONE])


def test_long_ref_and_long_info_among_short_lines(ctx):
    short = body_lines(150, seed=3)
    big_ref = line(2001, BIG_REF, info=b"DP=3")
    big_info = line(2002, b"AC", info=b"N=" + b"v" * 5000 + b";END=777777")
    buf = short[:83 * 70] + big_ref + short[83 * 70:83 * 100] + big_info + short[83 * 100:]
    for mis in (0, 3):
        end, flags, slots, res = check(ctx, buf, mis=mis, every=128)
        assert end[70] == 2001 + 70_000 - 1 and flags[70] == 0 and end[101] == 777777 and flags[101] == L.FROM_END
        assert res[3] == 777777 - 2002 and len(end) == 152


def test_buffers_that_end_inside_a_line(ctx):
    rows = body_lines(40, seed=5)
    last = line(5000, b"ACGTACGT", info=b"NS=3;END=6000")
    obj = rows + last + rows                                             # the object goes on behind the buffer
    size = BASE + len(obj)
    at = len(rows)
    cuts = {"field 8": at + last.index(b"END=") + 6, "field 4": at + last.index(b"ACGTACGT") + 3,
            "the newline": at + len(last)}
    for mis in (0, 1, 2, 3):
        for name, cut in cuts.items():
            end, flags, _, res = check(ctx, obj[:cut], size=size, mis=mis, every=2)
            want = (6000, L.FROM_END) if name == "the newline" else (0, L.TRUNCATED)
            assert (end[40], flags[40]) == want and flags[:40] == L.loop_span(rows, 0, len(rows),
                                                                             P.line_starts(rows, 0), [0] * 40)[1]
            assert res[1] == (name != "the newline") and res[5] == (L.NONE if name == "the newline" else 40)
        # every cut of the last line: the buffer's last dword is partial in three of four
        for cut in range(at + 1, at + len(last) + 1):
            check(ctx, obj[:cut], size=size, mis=mis, every=128)
    # the object itself ends there: a line's end, not a truncation
    end, flags, _, _ = check(ctx, obj[:cuts["field 8"]], every=2)
    assert (end[40], flags[40]) == (5007, 0)                             # END=60 lies below POS: REF decides


def test_starts_outside_the_buffer_and_an_empty_launch(ctx):
    buf = body_lines(10, seed=6)
    starts = [BASE + s for s in P.line_starts(buf, 0)]
    far = starts + [BASE + len(buf), BASE + len(buf) + 1, BASE + 2**40, 2**63]
    pos = P.loop_parse(buf, BASE, BASE + 2**41, starts)[0] + [5, 5, 5, 5]
    for mis in (0, 2):
        end, flags, _, res = check(ctx, buf, starts=far, pos=pos, size=BASE + 2**41, mis=mis, every=4)
        assert end[-4:] == [0] * 4 and flags[-4:] == [L.TRUNCATED] * 4 and res[1] == 4 and res[5] == 10
    below = [BASE - 1, 0] + starts                                       # starts in front of the buffer
    end, flags, _, _ = check(ctx, buf, starts=below, pos=[9, 9] + pos[:10], every=1)
    assert flags[:2] == [L.TRUNCATED] * 2
    v, h = ctx._vspan_ctx()
    assert v.dvs_blockmax_async(h, None, None, None, 0, 0, 3, None, ctypes.c_void_p(8)) == _vspan.DVS_ERR_INVALID
    assert b"power of two" in v.dvs_last_error()
