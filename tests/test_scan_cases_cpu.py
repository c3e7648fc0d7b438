"""The scan kernels' edge-case table (_scan_cases.py) on the CPU: its geometry is the kernels', every case has the
property it is named for (computed from the oracle's index and the bytes), and every threshold value is present."""
import os
import re

import numpy as np
import pytest

import _scan_cases as sc
from oracle import cpu_ref, dpref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------- drift guard
def kernel_source() -> str:
    with open(os.path.join(REPO, "dataplug_amd", "csrc", "dpscan.hip")) as f:
        return f.read()


def kernel_constants(src: str) -> dict:
    """Every ``constexpr <integer type> kName = <expression of earlier constants>;`` of dpscan.hip, evaluated."""
    env = {}
    for name, expr in re.findall(r"^constexpr\s+(?:int|uint32_t|uint64_t)\s+(k\w+)\s*=\s*([^;]+);", src, re.M):
        e = re.sub(r"\((?:uint32_t|uint64_t|int)\)", "", expr)
        e = re.sub(r"\b(\d+)(?:ull|u)\b", r"\1", e).replace("/", "//")
        try:
            env[name] = int(eval(e, {"__builtins__": {}}, dict(env)))
        except Exception:
            pass
    return env


def mirrored(k: dict, src: str) -> dict:
    """The table's constants as dpscan.hip states them."""
    words = re.search(r"uint4 sw0 = uint4\{0u, 0u, 0u, 0u\}((?:, sw\d+ = sw0)*);", src)
    assert words, "the prefetched spill words sw0.. of fasta_place_block"
    n_words = 1 + words.group(1).count("= sw0")
    assert not re.search(rf"\bsw{n_words}\b", src)
    k0 = {int(x) for x in re.findall(r"for \(uint32_t k0 = (\d+)u; k0 < nev; k0 \+= 8u\)", src)}
    assert k0 == {8 * n_words}, "the events read after the prefix start where the prefetched words end"
    assert f"if (nev > {8 * (n_words - 1)}u) sw{n_words - 1} = " in src
    return dict(LANE=k["kRowBytes"] // k["kWave"], ROW=k["kRowBytes"], BUF=k["kBufBytes"], RANGE=k["kWaveBytes"],
                GROUP_RANGES=k["kMapWaves"], UNIT_RANGES=k["kDataWaves"], PLACE_BLOCK=k["kPlaceBlock"],
                STAGE_BYTES=k["kStageBytes"], SPILL_CAP=k["kSpillCap"], PREFETCH_EVENTS=8 * n_words,
                LINE_CAP=k["kLineCap"], DENSE_MAX=k["kDenseMax"], UNIT=k["kUnitBytes"])


def test_constants_are_the_kernels():
    src = kernel_source()
    assert mirrored(kernel_constants(src), src) == dict(
        LANE=sc.LANE, ROW=sc.ROW, BUF=sc.BUF, RANGE=sc.RANGE, GROUP_RANGES=sc.GROUP_RANGES, UNIT_RANGES=sc.UNIT_RANGES,
        PLACE_BLOCK=sc.PLACE_BLOCK, STAGE_BYTES=sc.STAGE_BYTES, SPILL_CAP=sc.SPILL_CAP,
        PREFETCH_EVENTS=sc.PREFETCH_EVENTS, LINE_CAP=sc.LINE_CAP, DENSE_MAX=sc.DENSE_MAX, UNIT=sc.UNIT)
    assert sc.GROUP == sc.GROUP_RANGES * sc.RANGE and sc.BLOCK == sc.PLACE_BLOCK * sc.RANGE
    # the thresholds the table is built round are the constants +- 1 (+- 2 for the event counts, which come in pairs)
    assert set(sc.F_COUNT_EVENTS) == {c + d for c in (sc.PREFETCH_EVENTS, sc.SPILL_CAP, sc.DENSE_MAX) for d in range(-2, 3)}
    assert set(sc.D_COUNT_DELIMS) == {0, 1, sc.RANGE} | {c + d for c in (sc.LINE_CAP, sc.DENSE_MAX) for d in (-1, 0, 1)}
    assert set(sc.F_RUN_PAIRS) == {sc.STAGE_BYTES // b + d for b in (8, 16) for d in (-1, 0, 1)}


def test_drift_guard_sees_an_edit():
    """The guard reads the value from the source: the same source with one constant edited no longer matches."""
    src = kernel_source()
    want = mirrored(kernel_constants(src), src)
    for old, new, key in (("kLineCap = 640;", "kLineCap = 648;", "LINE_CAP"), ("kSpillCap = 512;", "kSpillCap = 256;", "SPILL_CAP"),
                          ("kStageBytes = 128u << 10;", "kStageBytes = 64u << 10;", "STAGE_BYTES"),
                          ("kDataWaves = 15;", "kDataWaves = 14;", "UNIT_RANGES")):
        assert old in src
        edited = src.replace(old, new)
        got = mirrored(kernel_constants(edited), edited)
        assert got[key] != want[key] and {k for k in got if got[k] != want[k]} >= {key}


# ---------------------------------------------------------------------------------------------- case properties
def _starts_ends(pairs, shift):
    """aligned coordinates of every header's '>' and of its last byte"""
    return pairs[:, 0].astype(np.int64) + shift, pairs[:, 1].astype(np.int64) - 1 + shift


def _check_fasta(c, a):
    s, n = c.shift, len(a)
    buf_len = c.extra.get("buf_len", n)
    exps = []
    for plan in c.plans:
        assert all(0 <= c0 <= c1 <= buf_len for c0, c1 in plan), (c.name, plan)
        exp = dpref.fasta_pairs(a, plan)
        pairs, cend, pending, unresolved = sc.fasta_expect(a, plan, buf_len, dpref.fasta_pairs)
        assert np.array_equal(pairs, exp) and cend[-1] == len(exp), c.name
        if n <= 1 << 20 and len(plan) <= 64:
            ref = [p for c0, c1 in plan for p in cpu_ref.fasta_chunk_pairs(a.tobytes(), c0, c1)]
            assert np.array_equal(np.asarray(ref, np.uint64).reshape(-1, 2), exp), c.name
        exps.append((exp, pending, unresolved))
    exp = exps[0][0]
    st, en = _starts_ends(exp, s)
    kind = c.prop[0]
    if kind == "events_in_range":
        _, r, ev = c.prop
        got = int(np.count_nonzero(st // sc.RANGE == r) + np.count_nonzero(en // sc.RANGE == r))
        assert got == ev, (c.name, got)
        assert all(a[e - s] == sc.NL for e in en), c.name
    elif kind.endswith("_byte_of"):
        byte, where = kind.split("_")[:2]
        B = c.extra["boundary"]
        b = c.prop[1]
        if b == "object":
            assert B - s == n
        elif b == "chunk":
            assert c.plans[0][0][1] == B - s
        else:
            size = sc.boundary_size(b)
            larger = [sc.boundary_size(x) for x in sc.BOUNDARIES[:7] if sc.boundary_size(x) > size]
            assert B % size == 0 and all(B % g for g in larger if g % size == 0 and b not in ("unit", "group")), c.name
        p = (B - 1 if where == "last" else B) - s
        emitted = [bool(np.any(e[0][:, 0] == p)) for e in exps]
        if byte == "gt":
            assert a[p] == sc.GT and a[p - 1] != sc.NL
            fol = c.prop[2]
            assert (fol == "followed_by_end" and p + 1 == n) or a[p + 1] == {"followed_by_A": sc.A_, "followed_by_nl": sc.NL}[fol]
            one_chunk = [plan for plan in c.plans if len(plan) == 1]
            for plan, em in zip(c.plans, emitted):
                cut_after = any(c1 == p + 1 for _, c1 in plan) and len(plan) > 1
                assert em == (fol == "followed_by_A" and not cut_after), (c.name, plan)
            assert one_chunk or b == "chunk"
        else:
            assert a[p] == sc.NL
            for e, plan in zip(exps, c.plans):
                assert np.any(e[0][:, 1] == p + 1), c.name           # it ends a header
                if p + 1 < n:
                    assert np.any(e[0][:, 0] == p + 1), c.name       # and the '>' right after it starts one
    elif kind == "header_spans_ranges":
        k = c.prop[1]
        h0, nl = c.extra["header"]
        i = int(np.flatnonzero(exp[:, 0] == h0)[0])
        assert int(exp[i, 1]) == nl + 1 and (nl + s) // sc.RANGE - (h0 + s) // sc.RANGE + 1 == k
        inner = np.flatnonzero(a[h0 + 1:nl] == sc.GT) + h0 + 1
        assert len(inner) >= 1 and not np.isin(inner, exp[:, 0]).any()
        mid = c.extra["mid"]
        cut = exps[1][0]
        nxt = int(inner[inner >= mid][0])
        assert h0 < mid < nl and np.any(cut[:, 0] == nxt) and len(cut) == len(exp) + 1
        short, pending, unresolved = exps[2]
        assert int(short[-1, 0]) == h0 and int(short[-1, 1]) == nl + 1 and pending == [-1] and not unresolved
    elif kind == "pairs_in_block":
        _, b0, p0, b1, p1 = c.prop
        blk = st // sc.BLOCK
        assert int(np.count_nonzero(blk == b0)) == p0 and int(np.count_nonzero(blk == b1)) == p1 and len(exp) == p0 + p1
        per_range = np.bincount((st // sc.RANGE).astype(np.int64)) * 2
        assert per_range.max() <= sc.SPILL_CAP, "no dense range: the run is staged or copied, not rescanned"
        if c.extra["pending_into_block1"]:
            i = int(np.flatnonzero(blk == b0)[-1])
            assert en[i] // sc.BLOCK == b1
    elif kind == "cuts_at":
        _, size, ds = c.prop
        cuts = {c0 + s for c0, _ in c.plans[0][1:]}
        want = {(d % size) for d in ds}
        assert {x % size for x in cuts} == want and len(cuts) >= 2 * len(ds), c.name
    elif kind == "chunks_in_one_lane":
        inside = [(c0, c1) for c0, c1 in c.plans[0] if c1 > c0 and (c0 + s) // sc.LANE == (c1 - 1 + s) // sc.LANE
                  and (c0 + s) // sc.LANE == sc.RANGE // sc.LANE]
        assert len(inside) == c.prop[1], c.name
    elif kind == "one_byte_chunk":
        ones = [(c0, c1) for c0, c1 in c.plans[0] if c1 == c0 + 1]
        assert len(ones) == 1 and a[ones[0][0]] == {"gt": sc.GT, "nl": sc.NL}[c.prop[1]] and c.plans[1] == ones
        assert len(exps[1][0]) == 0
    elif kind == "empty_chunks":
        plan = c.plans[0]
        assert sum(1 for c0, c1 in plan if c0 == c1) == c.prop[1] and plan[0][0] == plan[0][1] and plan[-1][0] == plan[-1][1]
        assert len(exps[1][0]) == 0
    elif kind == "first_chunk_start":
        assert c.plans[0][0][0] == c.prop[1] and 1 <= c.prop[1] <= 15
    elif kind == "resolve":
        v = c.prop[1]
        hi = c.extra["chunk_hi"]
        for (e, pending, unresolved), plan in zip(exps, c.plans):
            assert plan[-1][1] == hi and int(e[-1, 0]) < hi <= int(e[-1, 1]) - 1 or v.startswith("absent")
            nl_in_buf = np.flatnonzero(a[hi:buf_len] == sc.NL)
            if v == "nl_at_chunk_hi":
                assert a[hi] == sc.NL and int(e[-1, 1]) == hi + 1 and not unresolved
            elif v == "nl_at_chunk_hi_plus_1":
                assert a[hi] != sc.NL and a[hi + 1] == sc.NL and int(e[-1, 1]) == hi + 2 and not unresolved
            elif v == "nl_on_buffer_last_byte":
                assert buf_len < n and nl_in_buf.tolist() == [buf_len - 1 - hi] and int(e[-1, 1]) == buf_len and not unresolved
            elif v == "absent_buffer_ends_object":
                assert buf_len == n and not len(nl_in_buf) and int(e[-1, 1]) == n and not unresolved
            else:
                assert buf_len < n and not len(nl_in_buf) and a[buf_len] == sc.NL
                assert unresolved == [len(e) - 1] and pending[-1] == len(e) - 1 and pending[:-1] == [-1] * (len(plan) - 1)
    else:
        raise AssertionError(f"{c.name}: unknown property {c.prop}")


def _check_delim(c, a):
    s = c.shift
    d = c.extra["delim"]
    (ranges,) = c.plans
    assert all(s <= lo <= hi <= s + len(a) for lo, hi in ranges), c.name
    full, nd, ends = sc.delim_expect(a, s, ranges, d, 1, 0, 0, dpref.delim)
    ref = np.concatenate([cpu_ref.delim_index(a, lo - s, hi - s, d) for lo, hi in ranges]) + np.uint64(s)
    assert np.array_equal(full, ref) and nd == len(full) and ends[-1] == nd, c.name
    kind = c.prop[0]
    if kind == "delims_in_range":
        _, r, cnt = c.prop
        per = np.bincount((full // np.uint64(sc.RANGE)).astype(np.int64), minlength=r + 2)
        assert per[r] == cnt, (c.name, per[r])
        assert all(0 < per[q] < 30 for q in range(r + 2) if q != r), "sparse neighbours: a non-trivial prefix"
        if "first" in c.name and cnt:
            assert full[per[:r].sum()] == max(r * sc.RANGE, s) and np.all(np.diff(full[per[:r].sum():][:cnt]) == 1)
        if "last" in c.name and cnt:
            assert full[per[:r + 1].sum() - 1] == (r + 1) * sc.RANGE - 1
        if "lane" in c.name:
            lanes = np.bincount(((full[per[:r].sum():][:cnt] - np.uint64(r * sc.RANGE)) // np.uint64(sc.LANE)).astype(np.int64))
            assert len(lanes) == min(cnt, sc.RANGE // sc.LANE) and lanes.max() - lanes.min() <= 1
    elif kind == "boundary_launch":
        _, P, lo, hi = c.prop
        assert a[P - 1 - s] == d and a[P - s] == d and [(lo, hi)] == ranges
        assert lo in (s, P - 1, P, P + 1) and hi in (s + len(a), P - 1, P, P + 1) or (lo >> 8 == (hi - 1) >> 8 and nd == 1)
    elif kind == "selects":
        _, k, carry, target = c.prop
        for kk, add, cc in c.extra["select"]:
            out, _, _ = sc.delim_expect(a, s, ranges, d, kk, add, cc, dpref.delim)
            assert (kk, cc) == (k, carry) and target + add in out.tolist(), c.name
        i = int(np.flatnonzero(full == target)[0])
        r = target // sc.RANGE
        first, last = full[i - 1] // np.uint64(sc.RANGE) != r, full[i + 1] // np.uint64(sc.RANGE) != r
        assert first or last, c.name
        assert ("first" in c.name) == bool(first) and ("group-1" in c.name) == (r == sc.GROUP_RANGES)
    elif kind == "selects_none":
        _, k, carry, count = c.prop
        assert count == nd and k > carry + nd
        assert all(len(sc.delim_expect(a, s, ranges, d, kk, add, cc, dpref.delim)[0]) == 0 for kk, add, cc in c.extra["select"])
    elif kind == "delim_byte":
        assert nd == 16 and {int(x) % 16 for x in full} == set(range(16)) and d == c.prop[1]
    else:
        raise AssertionError(f"{c.name}: unknown property {c.prop}")


def _check_find(c, a):
    s, d, L = c.shift, c.extra["delim"], c.extra["buf_len"]
    _, m, scenario = c.prop
    (f,) = c.plans
    assert len(a) == L + 1 and (f + s) % 16 == m
    got = sc.find_expect(a, L, f, d)
    step = lambda p: ((p + s) - ((f + s) & ~15)) // sc.ROW      # which 1 KiB step of wave_find holds buffer byte p
    want = {"at_from": f, "before_from": -1, "last_byte": L - 1, "past_buf_len": -1}.get(scenario, got)
    assert got == want, c.name
    if scenario == "at_from":
        assert a[f] == d
    else:
        assert a[f - 1] == d and a[f] != d
    if scenario == "past_buf_len":
        assert a[L] == d
    if scenario in ("second_step", "third_step"):
        assert step(got) == {"second_step": 1, "third_step": 2}[scenario]


_CHECK = {"fasta": _check_fasta, "delim": _check_delim, "find": _check_find}


@pytest.mark.parametrize("family", list(sc.CASES))
def test_every_case_has_its_property(family):
    for c in sc.CASES[family]:
        _CHECK[c.kind](c, c.data)


def test_small_and_large_sizes():
    """Only the cases about the 16 MiB placement block (and the header of 1025 ranges) are large; the rest fit 1 MiB."""
    for c in sc.ALL:
        big = c.name.startswith(("F-run", "F-pending-1025", "F-last-byte-block"))
        n = len(c.data) if big or c.kind != "find" else sc.FIND_LEN + 1
        assert (16 << 20) < n <= (18 << 20) if big else n <= 1 << 20, (c.name, n)


def test_every_threshold_is_in_the_table():
    have = set()
    for c in sc.ALL:
        p = c.prop
        if p[0] == "events_in_range":
            have.add(("events", p[2], p[1]))
        elif p[0] == "pairs_in_block":
            have.add(("pairs", p[2]))
        elif p[0] == "delims_in_range":
            have.add(("delims", p[2], p[1]))
        elif p[0].endswith("_byte_of"):
            have.add((p[0], p[1]) + p[2:])
        elif p[0] == "from_mod16":
            have.add(("find", p[2], c.shift, c.extra["delim"], p[1]))
        elif p[0] == "header_spans_ranges":
            have.add(("spans", p[1]))
        elif p[0] == "resolve":
            have.add(("resolve", p[1], c.shift))
        elif p[0] == "delim_byte":
            have.add(("byte", p[1]))
        elif p[0] == "boundary_launch":
            have.add(("launch", p[1], p[2] - p[1] if abs(p[2] - p[1]) <= 1 else None, p[3] - p[1] if abs(p[3] - p[1]) <= 1 else None))
        elif p[0] == "selects":
            have.add(("select", p[1], c.name.split("-", 3)[3]))
        elif p[0] == "first_chunk_start":
            have.add(("first_chunk", p[1]))
    want = {("events", e, r) for e in (30, 31, 32, 33, 34, 510, 511, 512, 513, 514, 1022, 1023, 1024, 1025, 1026)
            for r in (0, 15, 16)}
    want |= {("pairs", p) for p in (16383, 16384, 16385, 8191, 8192, 8193, 1)}
    want |= {("delims", d, r) for d in (0, 1, 639, 640, 641, 1023, 1024, 1025, 16384) for r in (0, 15, 16)}
    for b in ("lane", "row", "buffer", "range", "group", "unit", "block", "chunk"):
        want |= {(f"gt_{w}_byte_of", b, f"followed_by_{f}") for w in ("last", "first") for f in ("A", "nl")}
        want |= {(f"nl_{w}_byte_of", b) for w in ("last", "first")}
    want |= {("gt_last_byte_of", "object", "followed_by_end"), ("nl_last_byte_of", "object")}
    want |= {("find", sn, s, v, m) for sn in sc.FIND_SCENARIOS for s in (0, 5, 15) for v in (0x00, 0x0A, 0x0C, 0x80, 0xFF)
             for m in range(16)}
    want |= {("spans", k) for k in (2, 17, 1025)}
    want |= {("resolve", v, s) for v in sc.RESOLVE_VARIANTS for s in (0, 5, 15)}
    want |= {("byte", v) for v in (0x00, 0x0A, 0x0C, 0x80, 0xFF)}
    want |= {("launch", P, d, None) for P in (256, 65536) for d in (-1, 0, 1)}
    want |= {("launch", P, None, d) for P in (256, 65536) for d in (-1, 0, 1)}
    want |= {("select", k, t) for k in (2, 3, 4) for t in ("first-of-range-3", "last-of-range-3", "first-of-group-1")}
    want |= {("first_chunk", k) for k in range(1, 16)}
    assert want <= have, sorted(want - have, key=str)[:10]
    names = {c.name for c in sc.ALL}
    assert {"F-chunks-range-pm1", "F-chunks-lane-pm1", "F-chunks-two-in-a-lane", "F-chunks-three-in-a-lane",
            "F-chunks-one-byte-gt", "F-chunks-one-byte-nl", "F-chunks-empty", "D-select-k-beyond-count"} <= names
    assert any(c.extra.get("pending_into_block1") for c in sc.CASES["F-run"])
    assert {c.prop[4] for c in sc.CASES["F-run"]} >= {0, 1, 3}
