"""fq_read_kernel, fq_scan_kernel and fq_sample_kernel (libdpfq.so) through the C ABI, bit-equal to the definition's
byte loop (tests/_fastq_loop.py).  G, the reads of a workgroup, and W, the lanes of the scan, come from dfq_geometry;
every output array is preset to a guard byte and checked one entry beyond what the launch owns."""
import ctypes

import numpy as np
import pytest

import _fastq_loop as L

pytestmark = pytest.mark.gpu

BASE = 1_000_003                                         # an odd buf_base
GUARD = 0xAB
G32, G64 = int.from_bytes(bytes([GUARD]) * 4, "little"), int.from_bytes(bytes([GUARD]) * 8, "little")
Z = b"@\n\n+\n\n"                                        # the 6-byte read of zero bases


def rd(name, seq, qual=None, eol=b"\n"):
    qual = b"I" * len(seq) if qual is None else qual
    return b"@" + name + eol + seq + eol + b"+" + eol + qual + eol


@pytest.fixture(scope="module")
def geo(ctx):
    return ctx.fq_geometry()


def obj(nreads, real=()):
    """``nreads`` reads: 6-byte empty ones, with the reads at the indices ``real`` = {index: bytes} instead."""
    real = dict(real)
    return b"".join(real.get(r, Z) for r in range(nreads))


def starts_of(data, base=0):
    """The line starts by construction-free means: numpy over the bytes (the loop checks them in the small cases)."""
    a = np.frombuffer(data, np.uint8)
    s = np.concatenate([[0], np.flatnonzero(a == 10) + 1])
    return (s[s < len(data)] + base).astype(np.uint64)


def launch(ctx, buf: bytes, starts, skip, n, last_end, read0=0, every=1, base=BASE, size=None, mis=0, smis=0,
           lens=None):
    """The three launches over ``buf`` = object bytes from ``base``; ``mis`` / ``smis`` misalign the buffer and the
    starts (by bytes / by one entry).  ``lens``: fq_sample_kernel reads this len[] instead of the read kernel's."""
    from dataplug_amd.scan import _fq
    f, h = ctx._fq_ctx()
    g = ctx.fq_geometry()[0]
    size = base + len(buf) if size is None else size
    nb = -(-n // g)
    ns = -(-(read0 + n) // every) - -(-read0 // every)
    d = ctx.workspace("fq_test_in", len(buf) + 96)
    ctx.h2d(d.ptr, np.full(len(buf) + 96, ord("@"), np.uint8))           # a read beyond the buffer would find an '@'
    if len(buf):
        ctx.h2d(d.ptr + mis, np.frombuffer(buf, np.uint8))
    st = np.asarray(starts, np.uint64)
    ws = ctx.workspace("fq_test_starts", 8 * len(st) + 64)
    d_starts = ws.ptr + 8 * smis
    if len(st):
        ctx.h2d(d_starts, st)
    sizes = [("res", 8 * _fq.R_WORDS), ("smp", 16 * (ns + 1)), ("block", 8 * (nb + 1)), ("len", 4 * (n + 1)),
             ("flags", n + 1)]
    off, total = {}, 0
    for name, nbytes in sizes:
        off[name] = total
        total += (nbytes + 15) & ~15
    out = ctx.workspace("fq_test_out", total)
    ctx.h2d(out.ptr, np.full(total, GUARD, np.uint8))
    p = ctypes.c_void_p
    at = lambda name: p(out.ptr + off[name])
    _fq.check(f.dfq_reads_async(h, p(d.ptr + mis), len(buf), base, size, p(d_starts), skip, n, int(last_end),
                                at("len"), at("flags"), at("block"), at("res")))
    if lens is not None:
        ctx.h2d(out.ptr + off["len"], np.asarray(lens, np.uint32))
        blk = np.asarray(lens, np.uint64)
        blk = np.array([blk[i:i + g].sum(dtype=np.uint64) for i in range(0, n, g)], np.uint64)
        ctx.h2d(out.ptr + off["block"], blk)
    _fq.check(f.dfq_scan_async(h, at("block"), nb, at("res")))
    _fq.check(f.dfq_sample_async(h, p(d_starts), skip, at("len"), at("block"), n, read0, every, at("smp")))
    raw = ctx.d2h(np.empty(total, np.uint8), out.ptr)
    view = lambda name, t, k: raw[off[name]:off[name] + k * np.dtype(t).itemsize].view(t)
    return dict(res=view("res", np.uint64, _fq.R_WORDS).tolist(), smp=view("smp", np.uint64, 2 * (ns + 1)),
                block=view("block", np.uint64, nb + 1), len=view("len", np.uint32, n + 1),
                flags=view("flags", np.uint8, n + 1), ns=ns, nb=nb, g=g)


def check(ctx, data: bytes, skip=0, read0=0, every=1, base=BASE, mis=0, smis=0, starts=None, n=None, size=None):
    """Launch over the whole reads of ``data`` behind its first ``skip`` lines and compare every output with the
    loop."""
    st = starts_of(data, base) if starts is None else np.asarray(starts, np.uint64)
    n = (len(st) - skip) // 4 if n is None else n
    t = skip + 4 * n
    if t < len(st):
        last_end = int(st[t]) - 1
    else:
        last_end = base + len(data) - (1 if data.endswith(b"\n") else 0)
    r = launch(ctx, data, st[:t], skip, n, last_end, read0, every, base, size, mis, smis)
    lens, flags = L.loop_launch(data, base, base + len(data) if size is None else size, st.tolist(), skip, n, last_end)
    assert r["len"][:n].tolist() == lens and int(r["len"][n]) == G32
    assert r["flags"][:n].tolist() == flags and int(r["flags"][n]) == GUARD
    assert r["res"] == L.loop_result(lens, flags)
    g = r["g"]
    sums = [sum(lens[i:i + g]) for i in range(0, n, g)]
    assert r["block"][:r["nb"]].tolist() == [sum(sums[:i]) for i in range(len(sums))] and int(r["block"][r["nb"]]) == G64
    want = L.loop_samples(st.tolist(), skip, lens, read0, every)
    assert r["ns"] == len(want)
    assert r["smp"][:2 * r["ns"]].reshape(-1, 2).tolist() == [list(w) for w in want]
    assert r["smp"][2 * r["ns"]:].tolist() == [G64, G64]
    return r, lens, flags


def read_counts(geo):
    g, w = geo
    return [0, 1, 2, g - 1, g, g + 1, 2 * g + 1, w * g - 1, w * g, w * g + 1, 2 * w * g + 3]


@pytest.mark.parametrize("which", range(11))
def test_read_counts_around_a_workgroup_and_the_scan_width(ctx, geo, which):
    g, w = geo
    for nreads in read_counts(geo)[which:which + 1]:
        real = {r: rd(b"r%d" % r, b"ACGT" * (1 + r % 5)) for r in (0, 1, g - 1, g, nreads // 2, nreads - 2, nreads - 1)
                if 0 <= r < nreads}
        data = obj(nreads, real)
        assert len(data) < 4 << 20
        for every in ((1, 64) if nreads <= 2 * g + 1 else (64,)):
            r, lens, flags = check(ctx, data, every=every)
            assert len(lens) == nreads and not any(flags)
        if nreads and nreads <= 2 * g + 1:                               # the loop's own index agrees with the launch
            pairs, nr, b, mn, mx = L.loop_index(data, 1)
            assert (nr, b, mn, mx) == (nreads, sum(lens), min(lens), max(lens))
            assert [p[1] for p in pairs[:-1]] == [sum(lens[:i]) for i in range(nreads)]


@pytest.mark.parametrize("every", [1, 2, 64, 1 << 20])
def test_skip_read0_and_sampling_slots(ctx, geo, every):
    g, _ = geo
    nreads = 2 * g + 1
    data = obj(nreads, {r: rd(b"x", b"AC" * (r % 7)) for r in range(0, nreads, 3)})
    for skip in range(4):
        body = b"junk\n" * skip + data                                   # lines of a read begun before the launch
        for read0 in sorted({0, 1, every - 1, every, every + 1, 3 * every, 3 * every + 5}):
            for smis in (0, 1):
                check(ctx, body, skip=skip, read0=read0, every=every, smis=smis)
        check(ctx, body + b"@tail\nAC\n", skip=skip, read0=7, every=every)      # lines behind the last whole read


@pytest.mark.parametrize("mis", range(16))
def test_buffer_misalignment_and_the_last_byte(ctx, mis):
    reads = [rd(b"n%d" % i, b"ACGTN" * (i % 9), eol=b"\r\n" if i % 2 else b"\n") for i in range(150)]
    data = b"".join(reads)
    for base in (0, 1, BASE, (1 << 33) + 5):
        check(ctx, data, base=base, mis=mis, every=2)
    check(ctx, data[:-1], mis=mis)                                       # the last read ends at the buffer's last byte
    check(ctx, data[:-2] if data.endswith(b"\r\n") else data[:-1], mis=mis)
    # the object ends inside the buffer: the bytes at and behind `size` are not the object's
    r, lens, flags = check(ctx, data, mis=mis, size=BASE + len(data) - len(reads[-1]) + 1)
    assert flags[-1] == L.KINDS.index("bad_separator") and not any(flags[:-1])
    # starts outside the buffer read nothing
    far = [0, 1, 2, 3, BASE + len(data) + 5, BASE + len(data) + 9, 1 << 62, (1 << 62) + 4]
    r, lens, flags = check(ctx, data, mis=mis, starts=far, n=2)
    assert flags == [1, 1]


def test_crlf_mixed_endings_and_zero_length_reads(ctx):
    crlf = b"".join(rd(b"c%d" % i, b"ACGT" * (i % 4), eol=b"\r\n") for i in range(70))
    r, lens, flags = check(ctx, crlf)
    assert lens[:5] == [0, 4, 8, 12, 0] and not any(flags)
    mixed = b"@a\r\nACGT\n+\r\nIIII\r\n" + b"@b\nACGT\r\n+\nIIII\n" + b"@c\nACG\r\n+\nIIII\n" + b"\r\nA\n+\nI\n" + \
        b"@d\n\r\n+\n\n" + b"@e\nA\n\r\n\r\n" + b"@q\nAC\n+@\n@+\n"
    r, lens, flags = check(ctx, mixed)
    assert lens == [4, 4, 3, 1, 0, 1, 2] and flags == [0, 0, 3, 1, 0, 2, 0]
    check(ctx, mixed[:-1])


def test_each_error_kind_at_the_first_read_the_last_and_a_wave_boundary(ctx, geo):
    g, _ = geo
    nreads = 2 * g + 70
    bad = {1: b"a\n\n+\n\n", 2: b"@\n\n-\n\n", 3: b"@\nA\n+\n\n"}
    for kind, body in bad.items():
        for where in ([0], [nreads - 1], [63], [64], [g - 1, g], [65, 64, g + 64, nreads - 1]):
            r, lens, flags = check(ctx, obj(nreads, {i: body for i in where}), every=64)
            assert r["res"][0] == len(where) and r["res"][3] == min(where)
            assert [i for i, f in enumerate(flags) if f] == sorted(where) and set(flags) == {0, kind}
    r, lens, flags = check(ctx, obj(nreads, {5: bad[3], 4: bad[2], 200: bad[1], 3: b"x\nA\n-\n\n"}))
    assert flags[3:6] == [1, 2, 3] and r["res"][0] == 4 and r["res"][3] == 3


def test_min_and_max_length_words(ctx, geo):
    g, _ = geo
    for nreads, real in ((1, {0: rd(b"a", b"ACGT")}), (g + 1, {g: rd(b"a", b"A" * 300)}),
                         (3 * g, {i: rd(b"a", b"A" * (5 + i % 3)) for i in range(3 * g)}),
                         (3 * g, {i: rd(b"a", b"A" * (9 if i != g + 65 else 2)) for i in range(3 * g)})):
        r, lens, flags = check(ctx, obj(nreads, real))
        assert r["res"][1] == max(lens) and r["res"][4] == min(lens)
    r, _, _ = check(ctx, b"")                                            # no reads: the words as initialised
    assert r["res"] == [0, 0, 0, L.NONE, L.NONE]


def test_sample_sums_carry_past_32_bits(ctx):
    data = obj(3)
    st = starts_of(data, BASE)
    big = [0xFFFFFFF0] * 3
    for every in (1, 2):
        r = launch(ctx, data, st, 0, 3, BASE + len(data) - 1, read0=0, every=every, lens=big)
        want = L.loop_samples(st.tolist(), 0, big, 0, every)
        assert want[-1][1] == 2 * 0xFFFFFFF0 > 1 << 32
        assert r["smp"][:2 * r["ns"]].reshape(-1, 2).tolist() == [list(w) for w in want]
        assert r["res"][2] == 3 * 0xFFFFFFF0 and r["block"][0] == 0


def test_scan_loops_over_more_blocks_than_lanes(ctx, geo):
    from dataplug_amd.scan import _fq
    g, w = geo
    f, h = ctx._fq_ctx()
    rng = np.random.default_rng(3)
    for nb in (1, w - 1, w, w + 1, 3 * w + 7):
        v = rng.integers(0, 1 << 40, nb + 1, dtype=np.uint64)
        v[nb] = G64
        d = ctx.workspace("fq_test_scan", 8 * (nb + 1) + 64)
        ctx.h2d(d.ptr + 48, v)
        ctx.h2d(d.ptr, np.full(8 * _fq.R_WORDS, GUARD, np.uint8))
        _fq.check(f.dfq_scan_async(h, ctypes.c_void_p(d.ptr + 48), nb, ctypes.c_void_p(d.ptr)))
        got = ctx.d2h(np.empty(nb + 1, np.uint64), d.ptr + 48)
        res = ctx.d2h(np.empty(_fq.R_WORDS, np.uint64), d.ptr).tolist()
        ex = np.concatenate([[0], np.cumsum(v[:nb], dtype=np.uint64)]).astype(np.uint64)
        assert got[:nb].tolist() == ex[:nb].tolist() and int(got[nb]) == G64
        assert res == [G64, G64, int(ex[nb]), G64, G64]                  # only the bases word is written


def test_fastq_lines_and_reads_own_the_lines_of_a_part(ctx):
    """The device layer's two calls on one resident buffer: as the only part, and as a middle part whose last line is
    incomplete and whose first lines belong to a read begun before it."""
    from dataplug_amd import synth
    data = synth.fastq_long(300, seed=4, len_min=10, len_max=3000).tobytes()
    pairs, nr, b, mn, mx = L.loop_index(data, 8)
    d = ctx.workspace("fq_test_in", len(data) + 96)
    ctx.h2d(d.ptr, np.frombuffer(data, np.uint8))
    assert ctx.fastq_lines(d.ptr, len(data), 0, 0, len(data), len(data), first=True, cap=16) == 4 * nr
    p = ctx.fastq_reads(0, 0, 8)
    assert (p.n_reads, p.bases, p.min_len, p.max_len, p.first_malformed, p.closed) == (nr, b, mn, mx, None, True)
    assert p.samples.tolist() == [list(x) for x in pairs[:-1]] and p.edge_lines.tolist() == [0]
    ln = L.lines_of(data)
    lo, hi = ln[4 * 50 + 1][0] + 3, ln[4 * 250 + 2][0] + 1               # from inside a line to inside another
    n = ctx.fastq_lines(d.ptr + lo, hi - lo, lo, lo, hi, len(data))
    assert n == (4 * 250 + 2) - (4 * 50 + 1)
    p = ctx.fastq_reads(2, 51, 8)                                        # lines 50*4+2, +3 in front: skip 2
    assert (p.n_reads, p.read0, p.closed) == (199, 51, False)
    assert p.edge_lines.tolist() == [0, 1, 2, 2 + 4 * 199, 3 + 4 * 199, 4 + 4 * 199]
    assert p.edge_starts.tolist() == [ln[i][0] for i in (202, 203, 204, 1000, 1001, 1002)]
    base = sum(x[2] for x in ln[1:4 * 51:4])
    assert p.samples.tolist() == [[o, c - base] for o, c in pairs[7:32]] and p.bases == sum(x[2] for x in ln[205:1000:4])
