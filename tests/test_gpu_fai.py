"""fai_count_kernel and fai_name_kernel (libdpfai.so) through ScanContext, against numpy counts over the same
segments (the definition in include/dpfai.h).  R (the range a wave takes), K (its LDS slots) and the grid come from
dfai_geometry."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NONE = np.uint64(0xFFFFFFFFFFFFFFFF)
BASE = 1_000_003                                         # an odd buf_base


@pytest.fixture(scope="module")
def geo(ctx):
    return ctx.fai_geometry()


def noisy(n, seed, p_nl=0.06, p_cr=0.03):
    """Random bytes over all 256 values with extra '\\n' and '\\r'."""
    rng = np.random.default_rng(seed)
    d = rng.integers(0, 256, n, dtype=np.uint8)
    u = rng.random(n)
    d[u < p_nl] = 10
    d[(u >= p_nl) & (u < p_nl + p_cr)] = 13
    return d


def ref_pass1(data, base, lo, hi):
    nl, cr, first = [], [], []
    for a, b in zip(lo, hi):
        s = data[int(a) - base:int(b) - base]
        w = np.flatnonzero(s == 10)
        nl.append(len(w))
        cr.append(int(np.count_nonzero(s == 13)))
        first.append(int(a) + int(w[0]) if len(w) else int(NONE))
    return np.array(nl, np.uint64), np.array(cr, np.uint64), np.array(first, np.uint64)


def ref_pass2(data, base, lo, hi, origin, width):
    off, last = [], []
    for a, b, o, w in zip(lo, hi, origin, width):
        p = int(a) + np.flatnonzero(data[int(a) - base:int(b) - base] == 10).astype(np.int64)
        bad = p[(p - int(o) + 1) % int(w) != 0] if int(w) else p
        off.append(len(bad))
        last.append(int(bad[-1]) if len(bad) else 0)
    return np.array(off, np.uint64), np.array(last, np.uint64)


def put(ctx, data, mis=0):
    buf = ctx.workspace("fai_test_in", len(data) + 64)
    if len(data):
        ctx.h2d(buf.ptr + mis, data)
    return buf.ptr + mis


def check(ctx, data, segs, mis=0, widths=(), origin=None, base=BASE):
    """Both passes over ``segs`` [(lo, hi), ...] (object offsets) against numpy; returns pass 1's arrays."""
    lo = np.array([s[0] for s in segs], np.uint64)
    hi = np.array([s[1] for s in segs], np.uint64)
    org = lo if origin is None else np.asarray(origin, np.uint64)
    d = put(ctx, data, mis)
    got = ctx.fai_counts(d, len(data), base, lo, hi, org)
    exp = ref_pass1(data, base, lo, hi)
    for g, e, name in zip(got, exp, ("nl", "cr", "first")):
        assert g.dtype == np.uint64 and np.array_equal(g, e), (name, np.flatnonzero(g != e)[:5])
    for w in widths:
        wid = np.full(len(segs), w, np.uint32) if np.isscalar(w) else np.asarray(w, np.uint32)
        got2 = ctx.fai_counts(d, len(data), base, lo, hi, org, width=wid)
        exp2 = ref_pass2(data, base, lo, hi, org, wid)
        for g, e, name in zip(got2, exp2, ("off", "lastoff")):
            assert np.array_equal(g, e), (name, w, np.flatnonzero(g != e)[:5])
    return got


def cuts_to_segs(cuts, gap=0):
    cuts = sorted(set(int(c) for c in cuts))
    return [(a, max(a, b - gap)) for a, b in zip(cuts[:-1], cuts[1:])]


@pytest.mark.parametrize("mis", [0, 5])
def test_lengths_and_alignment(ctx, geo, mis):
    R = geo[0]
    for n in (0, 1, 15, 16, 17, R - 1, R, R + 1, 2 * R + 5):
        data = noisy(n, 100 + n)
        check(ctx, data, [(BASE, BASE + n)], mis, widths=(1, 3))          # one segment over the whole buffer
        rng = np.random.default_rng(n)
        cuts = np.concatenate([[0, n], rng.integers(0, n + 1, 9)]) + BASE
        check(ctx, data, cuts_to_segs(cuts), mis, widths=(2,))            # abutting segments
        check(ctx, data, cuts_to_segs(cuts, gap=1), mis, widths=(61,))    # gaps (and empty segments)


def test_bytes_above_0x7f_are_not_miscounted(ctx, geo):
    R = geo[0]
    data = np.resize(np.arange(256, dtype=np.uint8), 2 * R + 256)         # every value at every position mod 16
    nl, cr, _ = check(ctx, data, [(BASE, BASE + len(data))])
    assert nl[0] == np.count_nonzero(data == 10) and cr[0] == np.count_nonzero(data == 13)
    check(ctx, data, cuts_to_segs(BASE + np.arange(0, len(data) + 1, 37)))
    data = np.full(R + 100, 0x8A, np.uint8)                               # '\n' | 0x80 everywhere
    data[[0, 17, R - 1, R + 99]] = 10
    data[[5, R]] = 0x8D
    nl, cr, first = check(ctx, data, [(BASE, BASE + len(data))])
    assert (nl[0], cr[0], first[0]) == (4, 0, BASE)


def test_segment_edges(ctx, geo):
    R = geo[0]
    n = 2 * R + 100
    data = noisy(n, 7, p_nl=0.5, p_cr=0.2)
    edges = list(range(4096 - 1, 4096 + 18)) + [R - 1, R, R + 1]
    for mis in (0, 5):
        # the chunk edges of the device address lie at object offset BASE - mis + 16 j
        e0 = [BASE - mis + e for e in edges]
        cuts = [BASE] + e0 + [BASE + n]
        check(ctx, data, cuts_to_segs(cuts), mis, widths=(1, 2))          # abutting, 1-byte segments among them
        segs = cuts_to_segs(cuts, gap=1)
        segs = sorted(segs + [(a, a) for a, _ in segs[::3]])              # empty segments between them
        check(ctx, data, segs, mis, widths=(3,))
    # a '\n' as the first and as the last byte of a segment, and in the gaps just outside it
    data = np.full(n, 65, np.uint8)
    segs = [(BASE + 10, BASE + 50), (BASE + R - 7, BASE + R + 9), (BASE + R + 30, BASE + R + 31)]
    for a, b in segs:
        data[[a - BASE - 1, a - BASE, b - BASE - 1, b - BASE]] = 10
    nl, cr, first = check(ctx, data, segs, widths=(4,))
    assert nl.tolist() == [2, 2, 1] and first.tolist() == [s[0] for s in segs]
    data[:] = 65
    for a, b in segs:
        data[[a - BASE - 1, b - BASE]] = 10                               # only outside: nothing is counted
    nl, cr, first = check(ctx, data, segs)
    assert nl.tolist() == [0, 0, 0] and (first == NONE).all()


@pytest.mark.parametrize("mult", ["K+1", "3K"])
def test_more_segments_in_a_range_than_slots(ctx, geo, mult):
    R, K, _ = geo
    nseg = K + 1 if mult == "K+1" else 3 * K
    step = R // (nseg + 1)
    assert step >= 2
    data = noisy(3 * R, 11, p_nl=0.3, p_cr=0.1)
    # all of them inside the second range of the (aligned) buffer, with gaps of one byte, then one large segment
    segs = [(BASE + R + 8 + i * step, BASE + R + 8 + (i + 1) * step - 1) for i in range(nseg)]
    assert segs[-1][1] <= BASE + 2 * R - 8
    segs.append((BASE + 2 * R + 20, BASE + 3 * R))
    for mis in (0, 5):
        nl, _, _ = check(ctx, data, segs, mis, widths=(2, 5))
        assert int(nl[K:nseg].sum()) > 0                                  # the overflow path counted something


def test_a_wave_takes_a_second_range(ctx, geo):
    R, _, waves = geo
    n = min(2 * waves * R + 12345, 256 << 20)
    rng = np.random.default_rng(5)
    data = rng.integers(0, 256, n, dtype=np.uint8)
    data[::61][rng.random(len(data[::61])) < 0.97] = 10                   # mostly regular lines of width 61
    check(ctx, data, [(BASE + 3, BASE + n - 2)], mis=5, widths=(61,))


def test_pass2_widths_origins_and_lastoff(ctx, geo):
    R = geo[0]
    n = 3 * R + 50
    data = noisy(n, 21, p_nl=0.1)
    segs = cuts_to_segs([BASE, BASE + 700, BASE + R + 3, BASE + 2 * R + 11, BASE + n], gap=2)
    org = [max(0, a - d) for (a, _), d in zip(segs, (0, 333, 5 * R, 1))]  # origin < lo: a clipped part
    check(ctx, data, segs, widths=(1, 2, 61, R + 7), origin=org)
    check(ctx, data, [(BASE, BASE + n)], mis=5, widths=(1, 2, 61, R + 7), origin=[BASE - 12345])
    # lastoff at a segment's last byte, and elsewhere
    body = np.full(n, 67, np.uint8)
    a, b = BASE + 40, BASE + 40 + 61 * 300 + 10                           # 300 full lines, a short one with a break
    body[a - BASE + 60:b - BASE:61] = 10
    body[b - BASE - 1] = 10
    c, d = BASE + 2 * R, BASE + 2 * R + 61 * 20
    body[c - BASE + 60:d - BASE:61] = 10
    body[c - BASE + 61 * 7 + 30] = 10                                     # a short middle line
    lo, hi = np.array([a, c], np.uint64), np.array([b, d], np.uint64)
    dp = put(ctx, body)
    off, last = ctx.fai_counts(dp, n, BASE, lo, hi, lo, width=np.array([61, 61], np.uint32))
    assert off.tolist() == [1, 1] and last.tolist() == [b - 1, c + 61 * 7 + 30]
    body[c - BASE + 61 * 7 + 30] = 67
    body[c - BASE + 61 * 3 + 5] = 10
    body[c - BASE + 61 * 4 + 5] = 10                                      # the next break is on the grid again
    dp = put(ctx, body)
    off, last = ctx.fai_counts(dp, n, BASE, lo, hi, lo, width=np.array([61, 61], np.uint32))
    assert off.tolist() == [1, 2] and last.tolist() == [b - 1, c + 61 * 4 + 5]


def test_two_parts_merge_to_the_whole_and_launches_repeat(ctx, geo):
    R = geo[0]
    n = 3 * R + 77
    data = noisy(n, 31)
    segs = cuts_to_segs(BASE + np.array([0, 5, 900, R - 1, R + 40, 2 * R + 333, n]), gap=1)
    lo = np.array([s[0] for s in segs], np.uint64)
    hi = np.array([s[1] for s in segs], np.uint64)
    wid = np.full(len(segs), 7, np.uint32)
    whole1 = check(ctx, data, segs)
    dp = put(ctx, data)
    whole2 = ctx.fai_counts(dp, n, BASE, lo, hi, lo, width=wid)
    again1 = ctx.fai_counts(dp, n, BASE, lo, hi, lo)                      # per-launch initialisation
    again2 = ctx.fai_counts(dp, n, BASE, lo, hi, lo, width=wid)
    assert all(np.array_equal(a, b) for a, b in zip(whole1 + whole2, again1 + again2))
    cut = R + 4321
    parts = []
    for a, b in ((0, cut), (cut, n)):
        plo = np.clip(lo, BASE + a, BASE + b).astype(np.uint64)
        phi = np.clip(hi, BASE + a, BASE + b).astype(np.uint64)
        keep = phi > plo
        dp = put(ctx, data[a:b], mis=3)
        r1 = ctx.fai_counts(dp, b - a, BASE + a, plo[keep], phi[keep], lo[keep])
        r2 = ctx.fai_counts(dp, b - a, BASE + a, plo[keep], phi[keep], lo[keep], width=wid[keep])
        full = [np.zeros(len(segs), np.uint64) for _ in range(5)]
        full[2][:] = NONE
        for f, r in zip(full, r1 + r2):
            f[keep] = r
        parts.append(full)
    p, q = parts
    merged = (p[0] + q[0], p[1] + q[1], np.minimum(p[2], q[2]), p[3] + q[3], np.maximum(p[4], q[4]))
    assert (lo < BASE + cut).any() and (hi > BASE + cut).any() and ((lo < BASE + cut) & (hi > BASE + cut)).any()
    for m, w, name in zip(merged, whole1 + whole2, ("nl", "cr", "first", "off", "lastoff")):
        assert np.array_equal(m, w), name


def test_names(ctx):
    rng = np.random.default_rng(3)
    names, parts, starts, ends = [], [], [], []
    pos = 0
    stops = [b" ", b"\t", b"\r", b"\n"]
    for i, ln in enumerate((1, 63, 64, 65, 1000, 7, 12)):
        name = bytes(rng.integers(33, 127, ln, dtype=np.uint8).tolist()).replace(b">", b"x")
        stop = stops[i % 4]
        line = b">" + name + stop + (b"" if stop == b"\n" else b"rest of the line\n")
        names.append(name)
        starts.append(BASE + pos)
        ends.append(BASE + pos + len(line))
        parts += [line, b"ACGT\nAC\n"]
        pos += len(line) + 8
    last = b"last_header_runs_to_the_end"
    parts.append(b">" + last)
    names.append(last)
    starts.append(BASE + pos)
    ends.append(BASE + pos + 1 + len(last))
    data = np.frombuffer(b"".join(parts), np.uint8)
    for mis in (0, 5):
        dp = put(ctx, data, mis)
        lens, packed = ctx.fai_names(dp, len(data), BASE, starts, ends)
        assert lens.tolist() == [len(x) for x in names]
        assert packed.tobytes() == b"".join(names)
    # a header clipped by the buffer's end: the name stops there
    s1 = starts[1]
    lens, packed = ctx.fai_names(put(ctx, data), s1 - BASE + 37, BASE, [s1], [s1 + 37])
    assert lens.tolist() == [36] and packed.tobytes() == names[1][:36]
    assert ctx.fai_names(put(ctx, data), len(data), BASE, [], [])[0].shape == (0,)
