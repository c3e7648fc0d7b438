"""GPU: the scan kernels on the built edge cases of _scan_cases.py, bit-exact against the oracle.

Every FASTA case runs through both forms (map + placement; one-pass) in uint32 and uint64 into an output workspace
filled with a canary; every newline case through line_kernel and the one-pass kernel in all four output forms; the
find cases through dp_find_delim.  test_scan_cases_cpu.py proves each case has the property it is named for."""
import numpy as np
import pytest

import _scan_cases as sc
from dataplug_amd.scan.objects import ByteOffsets
from oracle import dpref

pytestmark = pytest.mark.gpu

CANARY = 0xA5
# bytes round the uploaded buffer, inside the workspace: a kernel that reads past either end finds '>' and newlines
TEMPT = np.frombuffer(b"A\n>A\n>A\n>A\n>A\n>A", np.uint8)
assert len(TEMPT) == 16


def _upload(ctx, name, buf: np.ndarray, shift: int, tempt=TEMPT) -> int:
    """``buf`` at device address = shift mod 16, tempting bytes before and after it; returns its device pointer."""
    ws = ctx.workspace(name, 16 + len(buf) + 64)
    ctx.h2d(ws.ptr, np.concatenate([tempt[:shift], buf, tempt]))
    assert ws.ptr % 16 == 0
    return ws.ptr + shift


def _canary_out(ctx, nbytes: int):
    """(workspace, output pointer 16 bytes into it, total bytes), all bytes CANARY."""
    total = 16 + ((nbytes + 15) & ~15) + 64
    ws = ctx.workspace("e_out", total)
    ctx.h2d(ws.ptr, np.full(total, CANARY, np.uint8))
    return ws, ws.ptr + 16, total


def _read_out(ctx, ws, total, dtype):
    raw = ctx.d2h(np.empty(total, np.uint8), ws.ptr)
    assert (raw[:16] == CANARY).all(), "the 16 bytes before the output were written"
    return raw[16:].view(dtype)


# ---------------------------------------------------------------------------------------------- FASTA
def _run_fasta(ctx, case, a, d_in, buf_len, plan, u64, expect):
    pairs, cend, pending, unresolved = expect
    dtype = np.uint64 if u64 else np.uint32
    count = len(pairs)
    cap = count + 8
    ws, d_out, total = _canary_out(ctx, 2 * cap * np.dtype(dtype).itemsize)
    chunks = np.ascontiguousarray(np.asarray(plan, np.uint64).reshape(-1))
    ctx.fasta_index_async(d_in, buf_len, 0, len(a), chunks, d_out, u64, cap)
    n, got_pending, got_cend = ctx.fasta_result(len(plan))
    out = _read_out(ctx, ws, total, dtype)
    canary = dtype(int.from_bytes(bytes([CANARY]) * np.dtype(dtype).itemsize, "little"))
    assert n == count
    got = out[:2 * count].reshape(-1, 2).astype(np.uint64)
    want = pairs.copy()
    for i in unresolved:                                  # a pending header's end slot is not the kernels' to write
        want[i, 1] = np.uint64(canary)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert not len(bad), (len(bad), bad[:4], got[bad[:4]], want[bad[:4]])
    assert got_cend.tolist() == cend
    assert got_pending.tolist() == pending
    assert (out[2 * count:] == canary).all(), "elements past the last pair were written"


def _fasta_case(ctx, case, forms=(0, 1)):
    a = case.data
    buf_len = case.extra.get("buf_len", len(a))
    # after a buffer that stops short of its object come the object's next bytes (not the kernels' to read)
    tail = TEMPT if buf_len == len(a) else np.concatenate([a[buf_len:buf_len + 16], TEMPT])[:16]
    d_in = _upload(ctx, "e_in", a[:buf_len], case.shift, tail)
    expects = [sc.fasta_expect(a, plan, buf_len, dpref.fasta_pairs) for plan in case.plans]
    try:
        for form in forms:
            ctx.set_form(fasta=form)
            for plan, expect in zip(case.plans, expects):
                for u64 in (False, True):
                    try:
                        _run_fasta(ctx, case, a, d_in, buf_len, plan, u64, expect)
                    except AssertionError as e:
                        raise AssertionError(f"{case.name} form={form} u64={u64} plan={plan[:4]}: {e}") from e
                    if case.extra.get("retry"):           # a capacity below the count: clamped stores, then the retry
                        p2, pend2, cend2 = ctx.fasta_index(d_in, buf_len, 0, len(a), plan, u64=u64,
                                                           cap=max(1, len(expect[0]) // 3))
                        assert np.array_equal(p2.astype(np.uint64), expect[0]), (case.name, form, u64, "retry")
                        assert cend2.tolist() == expect[1] and pend2.tolist() == expect[2]
    finally:
        ctx.set_form(fasta=0)


@pytest.mark.parametrize("case", sc.cases_of("fasta"), ids=lambda c: c.name)
def test_fasta_edge(ctx, case):
    _fasta_case(ctx, case)


# ---------------------------------------------------------------------------------------------- newline
def _rebuild(r, mode, first):
    """uint64 offsets from an out_mode 3 or 4 result (as test_gpu_scan.py's _rebuild)."""
    if mode == 3:
        low, _, _, tab = r
        blk = np.searchsorted(tab.astype(np.int64), np.arange(len(low)), side="right").astype(np.uint64) - np.uint64(1)
        return ((blk + np.uint64(first >> 16)) << np.uint64(16)) | low.astype(np.uint64)
    low, _, _, tab, sub = r
    return ByteOffsets(low, sub, tab, first >> 8, first >> 16).to_u64()


def _run_delim_canary(ctx, d_in, n, base, ranges, delim, k, add, carry, mode, expect):
    want, nd, ends = expect
    dtype = np.uint64 if mode == 1 else np.uint32
    cap = len(want) + 8
    ws, d_out, total = _canary_out(ctx, cap * np.dtype(dtype).itemsize)
    rg = np.ascontiguousarray(np.asarray(ranges, np.uint64).reshape(-1))
    ctx.delim_ranges_async(d_in, n, base, rg, delim, k, add, carry, d_out, mode, cap)
    got_n, got_nd, got_ends = ctx.delim_ranges_result(len(ranges))
    out = _read_out(ctx, ws, total, dtype)
    canary = dtype(int.from_bytes(bytes([CANARY]) * np.dtype(dtype).itemsize, "little"))
    assert (got_n, got_nd, got_ends.tolist()) == (len(want), nd, ends)
    assert np.array_equal(out[:got_n].astype(np.uint64), want)
    assert (out[got_n:] == canary).all(), "entries past the last one were written"


def _run_delim_blocked(ctx, d_in, n, base, ranges, delim, mode, expect):
    want, nd, ends = expect
    r = ctx.delim_ranges(d_in, n, base, ranges, delim=delim, out_mode=mode)
    low, got_nd, got_ends, tab = r[:4]
    assert (len(low), got_nd, got_ends.tolist()) == (len(want), nd, ends)
    first, last = ranges[0][0], ranges[-1][1]
    assert np.array_equal(_rebuild(r, mode, first), want)
    if last > first:
        b64 = np.arange(first >> 16, ((last - 1) >> 16) + 1, dtype=np.uint64) << np.uint64(16)
        assert np.array_equal(tab[1:], np.searchsorted(want, b64[1:]).astype(np.uint64))
        if mode == 4:
            b256 = np.arange(first >> 8, ((last - 1) >> 8) + 1, dtype=np.uint64) << np.uint64(8)
            assert np.array_equal(r[4][1:], (np.searchsorted(want, b256[1:]) & 0xFFFF).astype(np.uint16))


@pytest.mark.parametrize("case", sc.cases_of("delim"), ids=lambda c: c.name)
def test_newline_edge(ctx, case):
    a = case.data
    base, delim = case.shift, case.extra["delim"]
    (ranges,) = case.plans
    tempt = np.full(16, delim, np.uint8)                   # delimiters right before and after the buffer
    d_in = _upload(ctx, "e_in", a, case.shift, tempt)
    select = case.extra.get("select", [(1, 0, 0)])
    try:
        for form in (1, 3):                                # line_kernel, the one-pass kernel
            ctx.set_form(delim=form)
            for k, add, carry in select:
                expect = sc.delim_expect(a, base, ranges, delim, k, add, carry, dpref.delim)
                for mode in (1, 0):
                    try:
                        _run_delim_canary(ctx, d_in, len(a), base, ranges, delim, k, add, carry, mode, expect)
                    except AssertionError as e:
                        raise AssertionError(f"{case.name} form={form} mode={mode} k={k} add={add} carry={carry}: {e}") from e
                    assert ctx.last_delim_form() == form
                if (k, add) == (1, 0) and carry == 0:
                    for mode in (3, 4):
                        try:
                            _run_delim_blocked(ctx, d_in, len(a), base, ranges, delim, mode, expect)
                        except AssertionError as e:
                            raise AssertionError(f"{case.name} form={form} mode={mode}: {e}") from e
    finally:
        ctx.set_form(delim=0)


# ---------------------------------------------------------------------------------------------- find
@pytest.mark.parametrize("case", sc.cases_of("find"), ids=lambda c: c.name)
def test_find_edge(ctx, case):
    a = case.data
    L, delim = case.extra["buf_len"], case.extra["delim"]
    (start,) = case.plans
    # the byte after the buffer (a[L]) and delimiters before and after it live in the workspace's padding
    d_in = _upload(ctx, "e_find", a, case.shift, np.full(16, delim, np.uint8))
    assert ctx.find_delim(d_in, L, 0, start, delim) == sc.find_expect(a, L, start, delim)
    base = 1 << 33                                        # the same buffer as a window far into an object
    want = sc.find_expect(a, L, start, delim)
    assert ctx.find_delim(d_in, L, base, base + start, delim) == (want + base if want >= 0 else -1)
