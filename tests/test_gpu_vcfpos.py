"""vpos_parse_kernel, vpos_reduce_kernel and vpos_name_kernel (libdpvpos.so) through the C ABI, bit-equal to the
definition's byte loop (tests/_vcfpos_loop.py).  The lines of a workgroup come from dvp_geometry."""
import ctypes

import numpy as np
import pytest

import _vcfpos_loop as L

pytestmark = pytest.mark.gpu

BASE = 1_000_003                                         # an odd buf_base
GUARD = 0xAB
REST = b"rs1\tA\tC\t9\tPASS\tNS=3\n"


def row(chrom, pos, rest=REST):
    chrom = chrom if isinstance(chrom, bytes) else chrom.encode()
    pos = pos if isinstance(pos, bytes) else b"%d" % pos
    return chrom + b"\t" + pos + b"\t" + rest


@pytest.fixture(scope="module")
def geo(ctx):
    return ctx.vpos_geometry()


def parse(ctx, buf: bytes, starts, base=BASE, size=None, mis=0, poison=b"\t7\t7\t"):
    """One parse launch over ``buf`` = object bytes from ``base``; the device bytes behind the buffer hold a tab, a
    digit and a tab, so a read beyond buf_len would resolve a prefix the definition calls unresolved."""
    n = len(starts)
    size = base + len(buf) if size is None else size
    d = ctx.workspace("vpos_test_in", len(buf) + 96)
    ctx.h2d(d.ptr + mis, np.frombuffer(buf + poison * 8, np.uint8))
    ws = ctx.workspace("vpos_test_starts", 8 * n + 16)
    if n:
        ctx.h2d(ws.ptr, np.asarray(starts, np.uint64))
    ctx.vcf_parse(d.ptr + mis, len(buf), base, size, ws.ptr, n)
    s = ctx._vp
    got = (ctx.d2h(np.empty(n, np.uint32), s["d_pos"]).tolist(), ctx.d2h(np.empty(n, np.uint16), s["d_clen"]).tolist(),
           ctx.d2h(np.empty(n, np.uint8), s["d_flags"]).tolist())
    return got


def check_parse(ctx, body: bytes, base=BASE, mis=0, starts=None, size=None):
    starts = [base + s for s in L.line_starts(body, 0)] if starts is None else starts
    got = parse(ctx, body, starts, base, size, mis)
    want = L.loop_parse(body, base, base + len(body) if size is None else size, starts)
    for g, w, name in zip(got, want, ("pos", "clen", "flags")):
        assert g == w, (name, [i for i, (a, b) in enumerate(zip(g, w)) if a != b][:5])
    return got


def check_reduce(ctx, parsed, ordinal0, every, cap=4096):
    pos, clen, flags = parsed
    r = ctx.vcf_positions(ordinal0, every, run_cap=cap)
    smp, runs, res = L.loop_reduce(pos, clen, flags, ordinal0, every)
    none = lambda v: None if v == L.NONE else v
    assert r.samples.tolist() == smp
    assert list(zip(r.run_line.tolist(), r.run_pos.tolist(), map(len, r.names), r.run_last_line.tolist(),
                    r.run_last.tolist())) == runs
    assert (r.n_malformed, r.first_malformed, r.n_unsorted, r.first_unsorted, r.first_pos, r.last_pos) == \
        (res["n_malformed"], none(res["min_malformed"]), res["n_unsorted"], none(res["min_unsorted"]),
         res["first_pos"], res["last_pos"])
    return r


def edge_counts(geo):
    g = set()
    for w in {64, geo[0], geo[1]}:
        g |= {w - 1, w, w + 1}
    return sorted(g | {1, 63, 64, 65, 2 * max(geo) + 1})


def test_line_counts_and_contig_changes_at_every_edge(ctx, geo):
    """Line counts around a wave and a workgroup, the contig changing exactly at each edge (and not changing), and an
    order violation on each edge."""
    for n in edge_counts(geo):
        for change in sorted({0, 63, 64, 65, geo[0] - 1, geo[0], geo[0] + 1, n - 1}):
            if not 0 <= change < n:
                continue
            rows = [row("chr1" if i < change else "chr2", 100 + i if i != change else 50) for i in range(n)]
            body = b"".join(rows)
            got = check_parse(ctx, body)
            r = check_reduce(ctx, got, 0, 1)
            assert len(r.names) == (1 if change == 0 else 2) and r.names[-1] == b"chr2"
        body = b"".join(row("chrQ", 7 if i in (63, 64, geo[0]) else 9) for i in range(n))    # equal CHROM across edges
        r = check_reduce(ctx, check_parse(ctx, body), 5, 4)
        assert r.names == [b"chrQ"] and r.run_offset.tolist() == [BASE]
        assert r.first_unsorted == (63 if n > 63 else None)


def test_chrom_compare_and_pos_forms(ctx):
    names = [b"chr1", b"chr2", b"chr", b"chr1", b"chr10", b"chr1", b"chr\x80", b"chr\xff", b"chr\xff", b"\x80", b"a" * 300,
             b"a" * 299 + b"b", b"a" * 300, b"x", b"x"]
    body = b"".join(row(nm, 5) for nm in names)
    _, clen, flags = check_parse(ctx, body)
    assert flags == [0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 1] and clen[10] == 300
    pos = [b"0", b"7", b"42", b"123", b"1234", b"12345", b"123456", b"1234567", b"12345678", b"123456789",
           b"2147483647", b"0000000000", b"0000000042", b"007",
           b"2147483648", b"4294967296", b"9999999999", b"00000000012", b"12345678901", b"", b"12a", b"-1", b" 1", b"1 ",
           b"1\r"]
    body = b"".join(row("c", p) for p in pos) + b"\tc\t5\n" + b"c\t5\n" + b"c 5 x\n" + b"\n" + b"c\t\t\n" + row("c", 9)
    got = check_parse(ctx, body)
    assert got[2][:14] == [0] + [1] * 13 and got[2][14:-1] == [2] * (len(got[2]) - 15)
    assert got[2][-1] == 1 and len(got[2]) == 31                          # "c\t\t" is malformed, its first field is c
    r = check_reduce(ctx, got, 0, 1)
    assert r.first_malformed == 14 and r.n_malformed == len(got[2]) - 15
    assert r.first_unsorted == 11 and r.n_unsorted == 2                   # 0000000000 behind 2147483647, 007 behind 42
    # crlf line endings, an unterminated last line, '\n' as the buffer's last byte
    check_parse(ctx, (row("1", 5) + row("1", 6)).replace(b"\n", b"\r\n"))
    check_parse(ctx, row("1", 5) + row("1", 6)[:-1])
    check_parse(ctx, row("1", 5) + b"1\t6")                               # the prefix reaches the object's end
    several = b"".join(row("1", p) for p in (9, 8, 7, 7, 6)) + b"bad\n" + row("1", 1) + b"bad\n"
    r = check_reduce(ctx, check_parse(ctx, several), 3, 2)
    assert (r.first_unsorted, r.n_unsorted, r.first_malformed, r.n_malformed) == (1, 3, 5, 2)


def test_prefix_limit(ctx):
    for t2 in (1022, 1023, 1024, 1025):
        for clen in (1, t2 - 2, t2 - 11):
            line = b"c" * clen + b"\t" + b"0" * (t2 - clen - 2) + b"7\t" + b"q\n"
            assert line.index(b"\t", clen + 1) == t2
            got = check_parse(ctx, row("c", 1) + line + row("c" * clen, 8))
            assert got[2][1] == (2 if t2 >= 1024 or t2 - clen - 1 > 10 else 0), (t2, clen)


@pytest.mark.parametrize("mis", range(16))
def test_alignment_base_and_buffer_end(ctx, mis):
    rng = np.random.default_rng(mis)
    rows = [row(b"chr%d" % (i // 7), 10 * i + int(rng.integers(0, 9))) for i in range(150)]
    body = b"".join(rows)
    for base in (0, 1, BASE, (1 << 33) + 5):
        check_reduce(ctx, check_parse(ctx, body, base=base, mis=mis), 0, 2)
    # the last line's prefix ends exactly at the buffer end: resolved by the buffer's last byte, and cut one short
    tail = b"chr21\t1234\t"
    for cut in range(len(tail)):
        got = check_parse(ctx, body + tail[:len(tail) - cut], mis=mis)
        assert got[2][-1] == (1 if cut == 0 else 2), cut
    # the object ends inside the buffer: bytes at and behind `size` are not the object's
    size = BASE + len(body) + 8
    got = check_parse(ctx, body + tail + b"x\n", mis=mis, size=size, starts=[BASE + len(rows[0]), BASE + len(body)])
    assert got[2] == [0, 2]
    # starts outside the buffer read nothing and are malformed
    got = check_parse(ctx, body, mis=mis, starts=[0, BASE - 1, BASE, BASE + len(body) - 1, BASE + len(body),
                                                  BASE + len(body) + 3, 1 << 62, 2**64 - 1])
    assert got[2] == [2, 2, 0, 2, 2, 2, 2, 2]


def raw_reduce(ctx, pos, clen, flags, ordinal0, every, cap):
    """dvp_reduce_async on uploaded parse outputs with every output byte preset to GUARD."""
    from dataplug_amd.scan import _vpos
    v, h = ctx._vpos_ctx()
    n = len(pos)
    ns = -(-(ordinal0 + n) // every) - -(-ordinal0 // every)
    inp = ctx.workspace("vpos_test_lines", 8 * n + 64)
    d_pos, d_clen, d_flags = inp.ptr, inp.ptr + 4 * n, inp.ptr + 6 * n
    for d, a, t in ((d_pos, pos, np.uint32), (d_clen, clen, np.uint16), (d_flags, flags, np.uint8)):
        ctx.h2d(d, np.asarray(a, t))
    nb = 64 + 20 * (cap + 1) + 4 * (ns + 1) + 64
    out = ctx.workspace("vpos_test_out", nb)
    ctx.h2d(out.ptr, np.full(nb, GUARD, np.uint8))
    d_res, d_runs = out.ptr, out.ptr + 64
    d_ends = d_runs + 8 * (cap + 1)
    d_rcl = d_ends + 8 * (cap + 1)
    d_smp = d_rcl + 4 * (cap + 1)
    p = ctypes.c_void_p
    _vpos.check(v.dvp_reduce_async(h, p(d_pos), p(d_clen), p(d_flags), n, ordinal0, every, p(d_smp), p(d_runs),
                                   p(d_ends), p(d_rcl), cap, p(d_res)))
    raw = ctx.d2h(np.empty(nb, np.uint8), out.ptr)
    off = lambda d: d - out.ptr
    return dict(res=raw[:64].view(np.uint64), runs=raw[off(d_runs):off(d_ends)].view(np.uint64),
                ends=raw[off(d_ends):off(d_rcl)].view(np.uint64), rcl=raw[off(d_rcl):off(d_smp)].view(np.uint32),
                smp=raw[off(d_smp):off(d_smp) + 4 * (ns + 1)].view(np.uint32), ns=ns)


@pytest.mark.parametrize("every", [1, 128])
def test_sampling_slots_and_guard(ctx, geo, every):
    guard32 = int.from_bytes(bytes([GUARD]) * 4, "little")
    for n in (1, 127, 128, 129, 2 * geo[1] + 3):
        pos = list(range(1000, 1000 + n))
        for ordinal0 in (0, every - 1, every, every + 1):
            r = raw_reduce(ctx, pos, [1] * n, [0] + [1] * (n - 1), ordinal0, every, 8)
            want = [pos[i] for i in range(n) if (ordinal0 + i) % every == 0]
            assert r["ns"] == len(want) and r["smp"][:-1].tolist() == want and int(r["smp"][-1]) == guard32
            assert r["res"].tolist() == [1, 0, 0, pos[0], pos[-1], 1, L.NONE, L.NONE]
            assert r["runs"].tolist() == [pos[0]] + [int.from_bytes(bytes([GUARD]) * 8, "little")] * 8


def test_run_cap_reports_the_count_and_the_retry_succeeds(ctx, geo):
    n = 3 * geo[1] + 5
    rows = [row(b"c%d" % (i // 3), i) for i in range(n)]                 # a run every three lines
    body = b"".join(rows)
    parsed = check_parse(ctx, body)
    smp, runs, res = L.loop_reduce(*parsed, 0, 1)
    m = res["n_runs"]
    guard64 = int.from_bytes(bytes([GUARD]) * 8, "little")
    r = raw_reduce(ctx, *parsed, 0, 1, m - 1)
    assert int(r["res"][0]) == m == int(r["res"][5]) and int(r["runs"][-1]) == guard64 == int(r["ends"][-1])
    assert int(r["rcl"][-1]) == int.from_bytes(bytes([GUARD]) * 4, "little")
    assert set(r["runs"][:-1].tolist()) < {(a << 32) | p for a, p, _, _, _ in runs}        # real runs, one missing
    r = raw_reduce(ctx, *parsed, 0, 1, m)
    assert sorted(r["runs"][:-1].tolist()) == [(a << 32) | p for a, p, _, _, _ in runs]
    assert sorted(r["ends"][:-1].tolist()) == [(b << 32) | q for _, _, _, b, q in runs]
    got = check_reduce(ctx, parsed, 0, 1, cap=m - 1)                     # the device layer retries with the count
    assert got.names == [b"c%d" % k for k in range(m)]
    assert got.run_offset.tolist() == [BASE + sum(map(len, rows[:3 * k])) for k in range(m)]


def test_long_lines_between_short_ones(ctx):
    long_ = row("chrL", 77, b"x" * 100_000 + b"\n")
    body = (row("chrL", 5) + b"a\tb\n\n" + long_ + b"1\t2\t\n" + long_ + long_ + b"abcde" + b"\n" + row("chrL", 78)) * 3
    got = check_parse(ctx, body)
    check_reduce(ctx, got, 127, 128)
    assert got[0].count(77) == 9 and got[2].count(2) == 9


def test_vcf_lines_puts_line_zero_in_front_and_drops_a_start_at_size(ctx):
    from dataplug_amd import synth
    data = synth.vcf_sorted(300_007, seed=2, contigs=3).tobytes()
    bo = len(synth.VCF_HEADER)
    d = ctx.workspace("vpos_test_in", len(data) + 96)
    ctx.h2d(d.ptr, np.frombuffer(data, np.uint8))
    starts = L.line_starts(data, bo)
    assert ctx.vcf_lines(d.ptr, len(data), 0, bo, len(data), len(data), first=True, cap=16) == len(starts)
    r = ctx.vcf_positions(0, 128)
    smp, contigs, n = L.loop_index(data, bo, 128)
    assert r.samples.tolist() == smp and r.names == [c[0] for c in contigs]
    assert r.run_offset.tolist() == [c[3] for c in contigs] and r.first_offset == bo
    mid = starts[len(starts) // 2]                                       # a later part: no line 0, the rest the same
    assert ctx.vcf_lines(d.ptr, len(data), 0, mid - 1, len(data), len(data)) == len(starts) - len(starts) // 2
    assert ctx.vcf_positions(len(starts) // 2, 128).samples.tolist() == \
        [s for k, s in enumerate(smp) if k * 128 >= len(starts) // 2]
