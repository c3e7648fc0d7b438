"""libdpquote.so's record-end kernel through ScanContext.records, bit-exact against the numpy model
(tests/_quote_model.py): every length around the chunk / tile edges, contents that put quotes and newlines on those
edges, both incoming states, unaligned ranges inside larger buffers, the output modes, capacity, and context reuse.
With T, G = tile bytes, grid: the largest case hands more than one tile to a workgroup (a look-back deeper than one).

The last two tests pin the lane-exact model of the kernel (tools/emulate_quote.py) to the hardware: every quote byte
against every data byte in every chunk position (v_perm_b32 and the signed v_dot4_i32_i8 as the model reads them), and
the kernel's offsets, counts and capacity error equal to the model's.  Nothing here tries to steer how the hardware
schedules workgroups: which descriptors a look-back finds published is left to timing on a GPU, so the look-back's
walks across 64-descriptor windows are shown correct on the CPU only, by tests/test_quote_model.py over schedules the
hardware cannot be made to produce on demand."""
import os
import sys

import numpy as np
import pytest

import _escape_cases as C
from _escape_loop import blocked
from _quote_cases import every_value_every_position, one_lane_16
from _quote_model import record_ends
from dataplug_amd.scan import DPCapacityError, DPScanError, ScanContext

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import emulate_quote as emu  # noqa: E402

pytestmark = pytest.mark.gpu

ALPHABET = np.frombuffer(b'"\n,a', np.uint8)
# mostly text, one quote and one newline in 32: records of ~32 bytes, quoted stretches across several of them
SPARSE = np.frombuffer(b'"\n,,' + b"a" * 28, np.uint8)


@pytest.fixture(scope="module")
def geo(ctx):
    t, g = ctx.quote_geometry()
    assert t > 0 and t % 1024 == 0 and g > 0
    return t, g


def _run(ctx, buf: np.ndarray, lo: int, hi: int, buf_base: int = 0, carry: int = 0, u64: bool = True, mis: int = 0,
         cap=None, quote: int = 34):
    """records of buffer bytes [lo, hi) -- object bytes [buf_base + lo, buf_base + hi) -- with the buffer placed
    ``mis`` bytes past a 16-byte boundary; checked against the model."""
    d = ctx.workspace("quote_in", len(buf) + 64)
    if len(buf):
        ctx.h2d(d.ptr + mis, buf)
    got, _, nq, nn, _, _ = ctx.records(d.ptr + mis, len(buf), buf_base, buf_base + lo, buf_base + hi, quote=quote,
                                       carry=carry, form="u64" if u64 else "u32", cap=cap)
    exp, eq, en = record_ends(buf[lo:hi], base=buf_base + lo, quote=quote, carry=carry)
    assert got.dtype == (np.uint64 if u64 else np.uint32)
    assert (nq, nn) == (eq, en)
    assert len(got) == len(exp) and np.array_equal(got.astype(np.uint64), exp)
    return got


def test_lengths_random_alphabet_both_states(ctx, geo):
    t, _ = geo
    rng = np.random.default_rng(1)
    for n in (0, 1, 15, 16, 17, t - 1, t, t + 1, 2 * t + 5):
        buf = ALPHABET[rng.integers(0, 4, n + 40)]
        for carry in (0, 1):
            _run(ctx, buf, 0, n, carry=carry)                                  # aligned, the buffer's head
            _run(ctx, buf, 7, 7 + n, buf_base=1_000_003, carry=carry, mis=5)   # unaligned range, odd base


def test_many_tiles_per_workgroup(ctx, geo):
    t, g = geo
    n = min(3 * g * t + 12345, 256 << 20)
    assert n > g * t, "the ticket must hand some workgroup a second tile"
    rng = np.random.default_rng(2)
    buf = SPARSE[rng.integers(0, 32, n + 16, dtype=np.uint8)]
    _run(ctx, buf, 3, 3 + n, buf_base=77, carry=1, mis=9)


def test_uniform_contents(ctx, geo):
    t, _ = geo
    n = 2 * t + 5
    for byte in (34, 10, 97):
        buf = np.full(n, byte, np.uint8)
        for carry in (0, 1):
            got = _run(ctx, buf, 0, n, carry=carry)
            assert len(got) == (n if byte == 10 and carry == 0 else 0)


def test_quotes_and_newlines_on_the_edges(ctx, geo):
    t, _ = geo
    n = 2 * t + 100
    for mis in (0, 11):
        # a quote as the last byte of a tile, '\n' as the first byte of the next: suppressed, the one after "..." kept
        buf = np.full(n, 97, np.uint8)
        buf[t - 1], buf[t], buf[t + 5], buf[t + 7] = 34, 10, 34, 10
        got = _run(ctx, buf, 0, n, mis=mis)
        assert list(got) == [t + 7]
        assert list(_run(ctx, buf, 0, n, carry=1, mis=mis)) == [t]
        # "" across a 16-byte chunk edge, a wave-row edge (1 KiB), a wave edge (16 KiB) and a tile edge, a newline
        # after each: the pair toggles twice, every newline is kept; under carry 1 none is
        buf = np.full(n, 97, np.uint8)
        edges = (16, 1024, 16384, t, t + 16384, 2 * t)
        for e in edges:
            buf[e - 1], buf[e], buf[e + 3] = 34, 34, 10
        assert list(_run(ctx, buf, 0, n, mis=mis)) == [e + 3 for e in edges]
        assert len(_run(ctx, buf, 0, n, carry=1, mis=mis)) == 0
        # the same pairs shifted so that they straddle the kernel's edges when the range starts mid-chunk
        assert len(_run(ctx, buf, 13, n - 3, buf_base=29, mis=mis)) == len(edges)


def test_one_quote_suppresses_everything_after_it(ctx, geo):
    t, _ = geo
    n = 3 * t + 17
    buf = np.full(n, 10, np.uint8)
    buf[0] = 34
    assert len(_run(ctx, buf, 0, n)) == 0
    assert len(_run(ctx, buf, 0, n, carry=1)) == n - 1
    assert len(_run(ctx, buf, 1, n)) == n - 1                       # the quote outside the range does not count
    assert len(_run(ctx, buf, 0, n, quote=39)) == n - 1             # another quote byte: '"' is plain text


def test_uint32_output_and_overflow(ctx, geo):
    t, _ = geo
    rng = np.random.default_rng(3)
    buf = ALPHABET[rng.integers(0, 4, t + 333)]
    a = _run(ctx, buf, 0, len(buf), buf_base=12345, u64=True)
    b = _run(ctx, buf, 0, len(buf), buf_base=12345, u64=False)
    assert np.array_equal(a, b.astype(np.uint64))
    base = (1 << 32) - 100                                          # the range crosses 2^32
    buf = np.full(300, 10, np.uint8)
    with pytest.raises(OverflowError):
        _run(ctx, buf, 0, 300, buf_base=base, u64=False)
    got = _run(ctx, buf, 0, 300, buf_base=base, u64=True)
    assert int(got[-1]) == base + 299 and int(got[0]) == base
    _run(ctx, buf, 0, 100, buf_base=base, u64=False)                # wholly below 2^32: fine as uint32


def test_capacity_and_count_only(ctx, geo):
    t, _ = geo
    rng = np.random.default_rng(4)
    buf = ALPHABET[rng.integers(0, 4, t + 4096)]
    exp, eq, en = record_ends(buf, base=50)
    assert len(exp) > 1000
    d = ctx.workspace("quote_in", len(buf) + 64)
    ctx.h2d(d.ptr, buf)
    counts = ctx.records(d.ptr, len(buf), 50, 50, 50 + len(buf), form="count")
    assert (counts.n, counts.n_quotes, counts.n_newlines) == (len(exp), eq, en)
    assert ctx.records(d.ptr, len(buf), 50, 50, 50 + len(buf), carry=1, form="count").n == \
        len(record_ends(buf, base=50, carry=1)[0])
    cap = 777
    canary = np.full(len(exp) + 64, 0xEEEEEEEEEEEEEEEE, np.uint64)
    out = ctx.workspace("quote_canary", canary.nbytes)
    ctx.h2d(out.ptr, canary)
    ctx.records_async(d.ptr, len(buf), 50, 50, 50 + len(buf), quote=34, carry=0, form="u64", d_out=out.ptr, cap=cap)
    with pytest.raises(DPCapacityError) as ei:
        ctx.records_result()
    assert ei.value.needed == len(exp) and (ei.value.n_quotes, ei.value.n_newlines) == (eq, en)
    back = ctx.d2h(np.empty_like(canary), out.ptr)
    assert np.array_equal(back[:cap], exp[:cap])
    assert np.array_equal(back[cap:], canary[cap:]), "written at or beyond cap"
    got = ctx.records(d.ptr, len(buf), 50, 50, 50 + len(buf), cap=1).ends        # the wrapper retries with the count
    assert np.array_equal(got, exp)


def test_bad_arguments_are_refused(ctx):
    d = ctx.workspace("quote_in", 4096)
    for kw in ({"quote": 10}, {"quote": 300}, {"carry": 2}):
        with pytest.raises(DPScanError):
            ctx.records(d.ptr, 100, 0, 0, 100, **kw)
    with pytest.raises(DPScanError):
        ctx.records(d.ptr, 100, 10, 5, 50)                          # begins before the buffer
    with pytest.raises(DPScanError):
        ctx.records(d.ptr, 100, 10, 20, 111)                        # ends past it
    assert len(ctx.records(d.ptr, 100, 10, 60, 60).ends) == 0       # empty range


def test_reuse_of_one_context_and_two_contexts(ctx, geo):
    t, _ = geo
    rng = np.random.default_rng(5)
    big = ALPHABET[rng.integers(0, 4, 5 * t + 3)]
    small = ALPHABET[rng.integers(0, 4, t + 9)]
    first = _run(ctx, big, 0, len(big))
    _run(ctx, small, 0, len(small), carry=1)                        # fewer tiles: the earlier descriptors are stale
    again = _run(ctx, big, 0, len(big))
    assert np.array_equal(first, again)
    other = ScanContext(0)
    try:
        assert np.array_equal(_run(other, big, 0, len(big)), first)
        assert np.array_equal(_run(ctx, big, 0, len(big)), first)
        assert np.array_equal(_run(other, small, 2, len(small), carry=1, mis=3),
                              record_ends(small[2:], base=2, carry=1)[0])
    finally:
        other.close()


# ------------------------------------------------------------------------------------------ the one launch path
@pytest.fixture(scope="module")
def three_tiles(ctx, geo):
    """3 tiles + 17 bytes of quotes, escape bytes and newlines as object bytes [5, ..) at a device address 5 past a
    16-byte boundary: the smallest input with a tile boundary, a look-back and a ragged tail; \\" across both inner
    tile edges."""
    t, _ = geo
    d = C.random_five(3 * t + 17, 31)
    for edge in (t - 5, 2 * t - 5):                      # the buffer offsets of both inner tile edges, in every form
        d[edge - 2:edge] = (ord("a"), C.E)
        C.after_run(d, edge)
    c = C.case(d, begin=5, base=5, carry=1, name="three_tiles")
    dev = ctx.workspace("quote_records_in", len(d) + 64)
    ctx.h2d(dev.ptr + 5, d)
    plain = record_ends(d, base=5, carry=1)
    want = {None: plain + (plain[1],), C.E: C.expect(c)}  # a plain launch toggles at every quote byte
    assert want[C.E][3] < want[C.E][1] and not np.array_equal(want[C.E][0], plain[0])
    assert min(len(want[None][0]), len(want[C.E][0])) > 1000
    return c, dev.ptr + 5, want


@pytest.mark.parametrize("escape", [None, C.E])
@pytest.mark.parametrize("form", ["count", "u32", "u64", "u16b"])
def test_records_equals_the_definition_in_every_form(ctx, three_tiles, form, escape):
    c, addr, want = three_tiles
    d, begin, end = c["buf"], c["begin"], c["end"]
    ends, nq, nn, tog = want[escape]
    r = ctx.records(addr, len(d), c["base"], begin, end, carry=c["carry"], escape=escape, form=form)
    assert (r.n, r.n_quotes, r.n_newlines, r.toggles) == (len(ends), nq, nn, tog)
    if escape is None:
        assert r.toggles == r.n_quotes
    if form == "count":
        assert r.ends is None and r.table is None
    elif form == "u16b":
        low, table = blocked(ends, begin, end)
        assert r.ends.dtype == np.uint16 and r.table.dtype == np.uint64 and len(table) == 4
        assert np.array_equal(r.ends, low) and np.array_equal(r.table, table)
    else:
        assert r.ends.dtype == (np.uint64 if form == "u64" else np.uint32) and r.table is None
        assert np.array_equal(r.ends.astype(np.uint64), ends)
    if form == "u64":                                    # started too small: one relaunch, the same offsets
        again = ctx.records(addr, len(d), c["base"], begin, end, carry=c["carry"], escape=escape, cap=1)
        assert np.array_equal(again.ends, r.ends) and again[2:] == r[2:]


# ------------------------------------------------------------------------------------------ the lane-exact model
def _run_both(ctx, buf, lo, hi, **kw):
    """_run (the kernel against the definition), then the lane model of the same launch against the kernel."""
    got = _run(ctx, buf, lo, hi, **kw)
    mis, base = kw.get("mis", 0), kw.get("buf_base", 0)
    addr = ctx.workspace("quote_in", len(buf) + 64).ptr + mis
    off, n_out, nq, nn, err = emu.run(buf, dev_addr=addr, buf_base=base, begin=base + lo, end=base + hi,
                                      quote=kw.get("quote", 34), carry=kw.get("carry", 0), u64=kw.get("u64", True))
    assert err == 0 and n_out == len(got) and off.dtype == got.dtype and np.array_equal(off, got)
    assert (nq, nn) == record_ends(buf[lo:hi], quote=kw.get("quote", 34))[1:]
    return got


def test_every_quote_byte_against_every_data_byte(ctx):
    data = every_value_every_position(4096)
    mis, lo = 5, 7
    shift = (mis + lo) % 16                              # chunk position of the range's first byte
    seen = np.zeros((256, 16), bool)
    seen[data, (shift + np.arange(4096)) % 16] = True
    assert seen.all(), "every byte value in every position of a 16-byte chunk"
    buf = np.empty(4096 + 40, np.uint8)
    buf[lo:lo + 4096] = data
    for quote in range(256):
        if quote == 10:
            continue
        pad = np.resize(np.array([quote, 10], np.uint8), 40)         # the bytes around the range: quotes and newlines
        buf[:lo], buf[lo + 4096:] = pad[:lo], pad[lo:]
        for carry in (0, 1):
            _run_both(ctx, buf, lo, lo + 4096, buf_base=1_000_003, carry=carry, mis=mis, quote=quote)


def test_kernel_equals_lane_model(ctx, geo):
    t, _ = geo
    assert t == emu.TILE_BYTES
    rng = np.random.default_rng(6)
    for n in (t - 1, t + 1, 3 * t + 17):
        for name, buf in (("alphabet", ALPHABET[rng.integers(0, 4, n + 40)]), ("one_lane_16", one_lane_16(n + 40, n))):
            for mis in (0, 11):
                for carry in (0, 1):
                    for u64 in (True, False):
                        _run_both(ctx, buf, 7, 7 + n, buf_base=29, carry=carry, u64=u64, mis=mis)
    # a capacity below the count: the stores below cap, the count and the capacity error as the model has them
    buf = ALPHABET[rng.integers(0, 4, t + 4096)]
    d = ctx.workspace("quote_in", len(buf) + 64)
    ctx.h2d(d.ptr + 11, buf)
    for u64 in (True, False):
        cap = 777
        off, n_out, nq, nn, err = emu.run(buf, dev_addr=d.ptr + 11, buf_base=50, carry=1, u64=u64, cap=cap)
        assert err == emu.ERR_CAPACITY and n_out > cap and len(off) == cap
        canary = np.full(n_out + 64, 0xEEEEEEEE, off.dtype)
        out = ctx.workspace("quote_canary", canary.nbytes)
        ctx.h2d(out.ptr, canary)
        ctx.records_async(d.ptr + 11, len(buf), 50, 50, 50 + len(buf), quote=34, carry=1,
                          form="u64" if u64 else "u32", d_out=out.ptr, cap=cap)
        with pytest.raises(DPCapacityError) as ei:
            ctx.records_result()
        assert (ei.value.needed, ei.value.n_quotes, ei.value.n_newlines) == (n_out, nq, nn)
        back = ctx.d2h(np.empty_like(canary), out.ptr)
        assert np.array_equal(back[:cap], off) and np.array_equal(back[cap:], canary[cap:])
