"""The VCF position index without a GPU: the definition's byte loop (tests/_vcfpos_loop.py) on hand-written bodies,
libdpvpos.so's ABI and ISA-guard stamp, scan/vpos.py's merge and the object layer's chain over a numpy-backed fake of
the device layer whose launches are computed by the loop, and fetch_region and the two strategies over a memory store.
tests/test_gpu_vcfpos*.py run the kernels."""
import ctypes
import json
import os
import re
import threading

import numpy as np
import pytest

import _vcfpos_loop as L
from _vcfpos_model import FakeDevices, parts_by_cuts
from dataplug_amd import build as B
from dataplug_amd import synth
from dataplug_amd.cloudobject import CloudObject
from dataplug_amd.formats.genomics import vcf as fvcf
from dataplug_amd.scan import _vpos
from dataplug_amd.scan import objects as scan_objects
from dataplug_amd.scan import vpos
from dataplug_amd.scan.vpos import VcfFormatError
from dataplug_amd.storage import MemoryStore

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEAD = synth.VCF_HEADER
BO = len(HEAD)


def row(chrom, pos, rest=b"rs1\tA\tC\t9\tPASS\tNS=3\n"):
    chrom = chrom if isinstance(chrom, bytes) else chrom.encode()
    pos = pos if isinstance(pos, bytes) else b"%d" % pos
    return chrom + b"\t" + pos + b"\t" + rest


# ------------------------------------------------------------------------------------------------ the loop, by hand
def test_loop_lines_and_terminators():
    d = row("1", 5) + row("1", 7)[:-1]                                   # an unterminated last line is a line
    assert L.loop_index(d, 0, 1) == ([5, 7], [(b"1", 0, 2, 0, len(d), 5, 7)], 2)
    d = row("1", 5) + row("1", 7)                                        # '\n' as the last byte: no empty line follows
    assert L.line_starts(d, 0) == [0, len(row("1", 5))] and L.loop_index(d, 0, 1)[2] == 2
    assert L.loop_index(d, len(d), 1) == ([], [], 0)                     # an empty body has no lines
    crlf = d.replace(b"\n", b"\r\n")                                     # \r\n: the '\r' lies behind t2
    assert L.loop_index(crlf, 0, 2) == ([5], [(b"1", 0, 2, 0, len(crlf), 5, 7)], 2)
    assert L.parse_line(b"1\t5\r\n", 0) is None                          # ... unless POS is the last field


@pytest.mark.parametrize("pos, ok", [(b"0", True), (b"2147483647", True), (b"2147483648", False),
                                      (b"00000000012", False), (b"0000000012", True), (b"", False), (b"12a", False),
                                      (b"-1", False), (b" 1", False), (b"9999999999", False)])
def test_loop_pos_field(pos, ok):
    r = L.parse_line(row("chrX", pos), 0)
    assert (r == (b"chrX", int(pos))) if ok else r is None


def test_loop_malformed_classes_and_prefix_limit():
    assert L.parse_line(b"\t5\tx\n", 0) is None                          # an empty CHROM
    assert L.parse_line(b"chr1\t55\n", 0) is None                        # one tab only
    assert L.parse_line(b"chr1 55 x\n", 0) is None
    assert L.parse_line(b"chr1\t55", 0) is None                          # the prefix reaches the object's end
    for t2, ok in ((1023, True), (1024, False)):                         # the second tab at prefix offset 1023 / 1024
        chrom = b"c" * (t2 - 3)
        line = chrom + b"\t77\tq\n"
        assert line.index(b"\t", len(chrom) + 1) == t2
        assert (L.parse_line(line, 0) == (chrom, 77)) is ok
    hi = bytes([0x80, 0xFF, 0xC3, 0xA9])                                 # CHROM bytes >= 0x80
    assert L.parse_line(row(hi, 3), 0) == (hi, 3)
    with pytest.raises(L.LoopError) as e:
        L.loop_index(row("1", 5) + b"oops\n" + row("1", 2), 0)
    assert (e.value.kind, e.value.ordinal, e.value.offset) == ("malformed", 1, len(row("1", 5)))


def test_loop_order_and_split_contig():
    a, b = row("1", 5), row("1", 5)
    assert L.loop_index(a + b + row("2", 1), 0, 1)[1] == [(b"1", 0, 2, 0, len(a + b), 5, 5),
                                                          (b"2", 2, 1, len(a + b), len(a + b) + len(row("2", 1)), 1, 1)]
    with pytest.raises(L.LoopError) as e:
        L.loop_index(a + row("1", 4), 0)
    assert (e.value.kind, e.value.ordinal, e.value.offset) == ("unsorted", 1, len(a))
    with pytest.raises(L.LoopError) as e:                                # a contig that reappears
        L.loop_index(a + row("2", 1) + row("1", 9), 0)
    assert (e.value.kind, e.value.ordinal) == ("split contig", 2)
    with pytest.raises(L.LoopError) as e:                                # the first offending line wins
        L.loop_index(a + row("2", 1) + row("2", 0) + b"bad\n" + row("1", 9), 0)
    assert (e.value.kind, e.value.ordinal) == ("unsorted", 2)


def test_loop_parse_flags():
    d = row("ab", 5) + row("ab", 3) + row("abc", 3) + row("ab", 1) + b"ab\n" + row("ab", 2) + b"ab\tx\n" + row("ab", 2)
    st = L.line_starts(d, 0)
    pos, clen, flags = L.loop_parse(d, 0, len(d), st)
    assert pos == [5, 3, 3, 1, 0, 2, 0, 2] and clen == [2, 2, 3, 2, 0, 2, 0, 2]
    assert flags == [0, 1, 0, 0, 2, 0, 2, 1]                             # the first field of a malformed line counts
    smp, runs, res = L.loop_reduce(pos, clen, flags, 3, 2)
    assert smp == [3, 1, 2, 2] and res["n_runs"] == 6 and res["min_malformed"] == 4 and res["n_malformed"] == 2
    assert res["min_unsorted"] == 1 and res["n_unsorted"] == 1 and runs[0] == (0, 5, 2, 1, 3)


# ------------------------------------------------------------------------------------------------ ABI, stamp
def test_header_table_exports_and_stamp_agree():
    raw = open(os.path.join(REPO, "include", "dpvpos.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    fns = sorted(set(re.findall(r"\b(dvp_[a-z0-9_]+)\s*\(", text)))
    assert sorted(n for n, _, _ in _vpos.SIGNATURES) == fns
    for name, _, args in _vpos.SIGNATURES:                               # the argument counts
        decl = re.search(r"\b%s\s*\(([^)]*)\)" % name, text).group(1).strip()
        assert len(args) == (0 if decl in ("", "void") else decl.count(",") + 1), name
    assert os.path.exists(_vpos.LIB_PATH), f"{_vpos.LIB_PATH} missing: run __graft_entry__.build()"
    lib = ctypes.CDLL(_vpos.LIB_PATH)
    assert [f for f in fns if not hasattr(lib, f)] == []
    assert _vpos.load().dvp_abi_version() == _vpos.ABI_VERSION == 1
    assert int(re.search(r"#define VPOS_PREFIX_MAX (\d+)", raw).group(1)) == _vpos.VPOS_PREFIX_MAX == L.PREFIX_MAX
    words = dict(re.findall(r"#define DVP_R_(\w+) (\d+)", raw))
    assert {k: int(v) for k, v in words.items()} == {
        "RUNS": _vpos.R_RUNS, "MALFORMED": _vpos.R_MALFORMED, "UNSORTED": _vpos.R_UNSORTED,
        "FIRST_POS": _vpos.R_FIRST_POS, "LAST_POS": _vpos.R_LAST_POS, "RUN_ENDS": _vpos.R_RUN_ENDS,
        "MIN_MALFORMED": _vpos.R_MIN_MALFORMED, "MIN_UNSORTED": _vpos.R_MIN_UNSORTED, "WORDS": _vpos.R_WORDS}
    with open(B.stamp_path(B.VPOS_OUT)) as f:
        rep = json.load(f)
    assert rep["result"] == "ok" and rep["guard_enforced"] is True and rep["arch"] == "gfx950"
    assert rep["so_sha256"] == B.sha256_file(B.VPOS_OUT) and rep["src_sha256"] == B.sha256_file(B.VPOS_SRC)
    assert rep["scratch"] == [] and rep["n_violations"] == 0 and rep["missing_kernels"] == []
    assert {k.split("<")[0] for k in rep["kernels"]} == set(B.VPOS_REQUIRED)


def test_loader_refuses_a_missing_library(tmp_path):
    from dataplug_amd.scan._lib import DPScanUnavailable
    with pytest.raises(DPScanUnavailable):
        _vpos.load(str(tmp_path / "missing.so"))
    bare = tmp_path / "libdpvpos.so"
    bare.write_bytes(open(_vpos.LIB_PATH, "rb").read())                  # the library without its stamp
    with pytest.raises(DPScanUnavailable):
        _vpos.load(str(bare))


# ------------------------------------------------------------------------------------------------ the fake device layer
# (tests/_vcfpos_model.py: FakeContext, FakeDevices, parts_by_cuts)
def _mem(name):
    MemoryStore._named.pop(name, None)
    return {"endpoint_url": f"memory://{name}"}


def _co(data: bytes, key: str, cfg):
    co = CloudObject.from_s3(fvcf.VCF, f"s3://data/{key}", fetch=False, s3_config=cfg)
    try:
        co.storage.head_bucket(Bucket="data")
    except Exception:
        co.storage.create_bucket(Bucket="data")
    co.storage.put_object(Body=data, Bucket="data", Key=key)
    return CloudObject.from_s3(fvcf.VCF, f"s3://data/{key}", s3_config=cfg)


def want_index(data, bo, every):
    smp, contigs, n = L.loop_index(data, bo, every)
    return L.samples_bytes(smp), L.contigs_text(contigs), n


def got_index(parts, size):
    smp, names, rows, n = vpos.merge_parts(parts, size)
    return smp.astype("<u4").tobytes(), vpos.contigs_text(names, rows), n


@pytest.fixture(scope="module")
def small():
    return HEAD + synth.vcf_sorted(40_000, seed=3, contigs=5).tobytes()[BO:]


@pytest.mark.parametrize("every", [1, 2, 128])
def test_merge_random_cuts(small, every):
    rng = np.random.default_rng(every)
    want = want_index(small, BO, every)
    for nparts in range(1, 6):
        for _ in range(6):
            cuts = rng.integers(BO, len(small), nparts - 1).tolist()
            assert got_index(parts_by_cuts(small, BO, cuts, every), len(small)) == want, cuts
    names, rows = vpos.parse_contigs(want[1])
    assert vpos.contigs_text(names, rows) == want[1] and len(names) == 5


def test_merge_run_spanning_three_parts_and_line_edges():
    d = b"".join(row("1", p) for p in range(1, 40)) + b"".join(row("2", p) for p in (3, 3, 9))
    w = len(row("1", 1))
    want = want_index(d, 0, 4)
    for cuts in ([5 * w + 3, 20 * w], [w, 2 * w], [w - 1, w, w + 1], [len(d) - 1], [39 * w, 39 * w + 1]):
        parts = parts_by_cuts(d, 0, cuts, 4)
        assert got_index(parts, len(d)) == want, cuts
    assert [p.n for p in parts_by_cuts(d, 0, [3, 5], 4)][:2] == [1, 0]   # a part without any line start


def test_merge_errors_across_part_boundaries():
    a = b"".join(row("1", p) for p in (5, 6, 7))
    w = len(row("1", 5))
    bad = a + row("1", 6) + row("1", 9)                                  # the order violation is the part's first line
    for cuts in ([3 * w - 1], [3 * w - 1, 4 * w - 1], [w]):
        with pytest.raises(VcfFormatError) as e:
            vpos.merge_parts(parts_by_cuts(bad, 0, cuts, 2), len(bad))
        assert (e.value.kind, e.value.ordinal, e.value.offset) == ("unsorted", 3, 3 * w) and "unsorted" in str(e.value)
    split = a + row("2", 1) + row("1", 8)
    for cuts in ([], [4 * w - 1], [2 * w, 4 * w - 1]):
        with pytest.raises(VcfFormatError) as e:
            vpos.merge_parts(parts_by_cuts(split, 0, cuts, 2), len(split))
        assert (e.value.kind, e.value.ordinal, e.value.offset) == ("split contig", 4, 4 * w)
    mal = a + b"1\tx\tq\n" + row("1", 1) + b"zz\n"                        # the lowest of several, across kinds
    for cuts in ([], [3 * w], [3 * w + 7]):
        with pytest.raises(VcfFormatError) as e:
            vpos.merge_parts(parts_by_cuts(mal, 0, cuts, 2), len(mal))
        assert (e.value.kind, e.value.ordinal, e.value.offset) == ("malformed", 3, 3 * w)
    assert isinstance(e.value, ValueError)


@pytest.mark.parametrize("devs", [[0], [0, 0, 0]])
def test_pos_index_object_chains_the_parts(monkeypatch, small, devs):
    layer = FakeDevices(monkeypatch, devs)
    co = _co(small, "s.vcf", _mem(f"vpos_cpu_obj{len(devs)}"))
    smp, names, rows, n = scan_objects.pos_index_object(co, BO, 8, part_bytes=7000, halo=1024)
    assert (smp.astype("<u4").tobytes(), vpos.contigs_text(names, rows), n) == want_index(small, BO, 8)
    red = sorted(c[1:] for c in layer.calls if c[0] == "reduce" and c[1] is not None)
    assert len(red) >= 5 and [r[1] for r in red] == list(np.cumsum([0] + [r[2] for r in red])[:-1])   # ordinal0 chain
    assert all(hi - lo <= 7000 + 1024 for lo, hi in layer.fetches)
    with pytest.raises(ValueError):
        scan_objects.pos_index_object(co, BO, 3)
    assert scan_objects.pos_index_object(co, len(small), 8)[3] == 0


def test_a_part_that_raises_releases_the_chain(monkeypatch, small):
    """One early part fails before it publishes its line count; the later parts, on other workers, have counted and
    wait for it: they must be released, and the caller must see the failure itself."""
    import time
    layer = FakeDevices(monkeypatch, [0, 0, 0])
    co = _co(small, "f.vcf", _mem("vpos_cpu_fail"))
    want = want_index(small, BO, 8)
    run = lambda: scan_objects.pos_index_object(co, BO, 8, part_bytes=7000, halo=1024)
    t0 = time.perf_counter()
    smp, names, rows, n = run()
    healthy = time.perf_counter() - t0
    assert (smp.astype("<u4").tobytes(), vpos.contigs_text(names, rows), n) == want
    parts = scan_objects.line_parts(BO, len(small), 3, 7000)
    assert len(parts) >= 5
    result = {}

    def call():
        try:
            result["value"] = run()
        except BaseException as e:
            result["error"] = e

    layer.fail_at = {parts[1][0]}                        # part 1 never publishes its count: parts 2.. wait for it
    del layer.calls[:]
    th = threading.Thread(target=call, daemon=True)
    th.start()
    # a guard against a hang, not a speed: a released waiter notices the failure at its next 50 ms poll; 200 times
    # the healthy run and at least 20 s leaves a loaded machine two orders of magnitude
    th.join(max(20.0, 200 * healthy))
    assert not th.is_alive(), "pos_index_object hangs when a part fails"
    assert "value" not in result and isinstance(result["error"], OSError)
    assert "fake: the part's launch failed" in str(result["error"]), "the caller must see the cause, not a waiter"
    counted = {c[1] for c in layer.calls if c[0] == "lines"}
    assert parts[2][0] in counted and parts[1][0] not in counted        # a later part had counted and was waiting
    assert not [c for c in layer.calls if c[0] == "reduce" and c[2] > 0]     # and none past part 0 went on to reduce
    layer.fail_at = set()
    scan_objects.release_workers()                       # the workers are idle again: this returns
    smp, names, rows, n = run()
    assert (smp.astype("<u4").tobytes(), vpos.contigs_text(names, rows), n) == want


# ------------------------------------------------------------------------------------------------ plugin over a store
def indexed(monkeypatch, data, key, name, every, devs=(0, 0)):
    FakeDevices(monkeypatch, list(devs))
    monkeypatch.setattr(scan_objects, "line_index_object", lambda co, begin=0, end=None, **kw: np.array(
        [p for p in range(begin, len(data)) if data[p] == 10], np.uint64))
    co = _co(data, key, _mem(name))
    co.preprocess(extra_args={"pos_index": True, "pos_index_every": every, "index_format": "u64"})
    return co


def py_filter(data, chrom, start, end):
    return L.loop_region(data, BO, chrom, start, end)


@pytest.mark.parametrize("every", [1, 2, 128])
def test_plugin_stores_and_queries(monkeypatch, every):
    body = b"".join(row("chrA", p) for p in [1, 1, 2, 5, 5, 5, 5, 9] + list(range(10, 400, 3)))
    body += b"".join(row(b"chr\xc3\xa9", p) for p in range(7, 300, 2)) + row("chrZ", 2147483647)[:-1]
    data = HEAD + body
    co = indexed(monkeypatch, data, "q.vcf", f"vpos_cpu_plugin{every}", every)
    smp, ctg, n = want_index(data, BO, every)
    meta = co.meta_path.bucket
    get = lambda k: co.storage.get_object(Bucket=meta, Key=k)["Body"].read()
    assert get("q.vcf.pos") == smp and get("q.vcf.contigs") == ctg
    a = co.attributes
    assert (a.pos_index_key, a.pos_index_every, a.contigs_key, a.num_contigs, a.num_body_lines) == \
        ("q.vcf.pos", every, "q.vcf.contigs", 3, n)
    names, rows = fvcf.load_contigs(co)
    assert names == [b"chrA", b"chr\xc3\xa9", b"chrZ"] and int(rows["num_lines"].sum()) == n
    lines = L.lines_of(data, BO)
    # regions that begin or end on a sample line, equal POS straddling a sample, an empty region, a whole contig
    regions = [("chrA", None, None), ("chrA", 5, 5), ("chrA", 1, 1), ("chrA", 2, 9), ("chrA", 6, 8), ("chrA", 400, None),
               ("chrA", None, 0), ("chrA", 13, 16), (b"chr\xc3\xa9", 7, 7), (b"chr\xc3\xa9", 100, 201),
               (b"chr\xc3\xa9", None, 50), ("chrZ", None, None), ("chrZ", 2147483647, 2147483647), ("chrZ", 1, 5)]
    for k in range(0, n, max(every, 37)):                                # regions whose ends are sample lines' POS
        c, p = L.parse_line(data, lines[k][0])
        regions += [(c, p, p + 4), (c, max(0, p - 4), p)]
    got_gets = []
    real = co.storage.get_object

    def spy(**kw):
        if kw["Bucket"] == "data":
            a, b = map(int, kw["Range"][6:].split("-"))
            got_gets.append(b + 1 - a)
        return real(**kw)
    monkeypatch.setattr(co.storage, "get_object", spy)
    for chrom, s, e in regions:
        del got_gets[:]
        cb = chrom if isinstance(chrom, bytes) else chrom.encode()
        want = py_filter(data, cb, s, e)
        assert fvcf.fetch_region(co, chrom, s, e) == want, (chrom, s, e)
        fetched = list(got_gets)
        del got_gets[:]
        r0, r1, (c0, c1), raw = fvcf.region_range(co, chrom, s, e)       # what the regions strategy calls
        assert fetched == ([c1 - c0] if c1 > c0 else [])                 # fetch_region: one ranged GET, the candidates
        assert data[r0:r1] == want and raw is None
        # the strategy reads at most the two boundary sample intervals, and nothing for a side that is open
        assert len(got_gets) <= (s is not None) + (e is not None)
        # the candidates: at most the matching lines plus the sample intervals they touch
        row_ = rows[names.index(cb)]
        span = max(len(x) for x in [want] + [b""])
        worst = max(e_ - s_ for s_, e_ in lines)
        assert all(g <= (every + 1) * worst for g in got_gets)
        assert c1 - c0 <= span + 2 * every * worst and c0 >= int(row_["offset"]) and c1 <= int(row_["end"])
    with pytest.raises(KeyError):
        fvcf.fetch_region(co, "chrQ", 1, 2)
    monkeypatch.setattr(co.storage, "get_object", real)
    sl = co.partition(fvcf.partition_contigs_strategy)
    head = get("q.vcf").decode() + "\n"
    assert [s.get() for s in sl] == [head + py_filter(data, nm, None, None).decode("utf-8") for nm in names]
    sl = co.partition(fvcf.partition_regions_strategy, regions=regions[:10])
    assert [s.get() for s in sl] == [head + py_filter(data, c if isinstance(c, bytes) else c.encode(), s, e).decode()
                                     for c, s, e in regions[:10]]
    assert sl[6].body[0] == sl[6].body[1]                                # an empty region gives an empty body
    # an object that changed after it was indexed: an error that says so, not an IndexError
    broken = bytearray(data)
    at = lines[2][0]                                                    # the first line with POS >= 2
    broken[at:at + 6] = b"chrA x"
    co.storage.put_object(Body=bytes(broken), Bucket="data", Key="q.vcf")
    with pytest.raises(ValueError, match=f"byte {at} .*does not match its position index"):
        fvcf.fetch_region(co, "chrA", 2, 9)


def test_without_pos_index_nothing_changes_and_errors_keep_the_line_index(monkeypatch):
    data = HEAD + b"".join(row("1", p) for p in (4, 5, 3, 9))
    FakeDevices(monkeypatch, [0])
    monkeypatch.setattr(scan_objects, "line_index_object", lambda co, begin=0, end=None, **kw: np.array(
        [p for p in range(begin, len(data)) if data[p] == 10], np.uint64))
    cfg = _mem("vpos_cpu_plain")
    co = _co(data, "p.vcf", cfg)
    co.preprocess(extra_args={"index_format": "u64"})
    keys = sorted(o["Key"] for o in co.storage.list_objects_v2(Bucket=co.meta_path.bucket)["Contents"])
    assert keys == ["p.vcf", "p.vcf.attrs", "p.vcf.lines"]
    with pytest.raises(KeyError):
        fvcf.load_contigs(co)
    plain = {k: co.storage.get_object(Bucket=co.meta_path.bucket, Key=k)["Body"].read() for k in keys}
    cb = _co(data, "b.vcf", cfg)
    with pytest.raises(VcfFormatError) as e:
        cb.preprocess(extra_args={"index_format": "u64", "pos_index": True})
    w = len(row("1", 4))
    assert (e.value.kind, e.value.ordinal, e.value.offset) == ("unsorted", 2, BO + 2 * w)
    cb = CloudObject.from_s3(fvcf.VCF, "s3://data/b.vcf", s3_config=cfg)
    got = {k: cb.storage.get_object(Bucket=cb.meta_path.bucket, Key=k.replace("p.vcf", "b.vcf"))["Body"].read()
           for k in keys}
    assert got["p.vcf"] == plain["p.vcf"] and got["p.vcf.lines"] == plain["p.vcf.lines"]
    assert len(cb.partition(fvcf.partition_num_chunks, num_chunks=2)) == 2
    with pytest.raises(ValueError):
        _co(data, "c.vcf", cfg).preprocess(extra_args={"pos_index": True, "line_index": False})


def test_vcf_sorted_is_exact_sorted_and_seeded():
    a = synth.vcf_sorted(100_003, seed=9, contigs=4)
    assert len(a) == 100_003 and a[-1] == 10 and a[:BO].tobytes() == HEAD
    assert np.array_equal(a, synth.vcf_sorted(100_003, seed=9, contigs=4))
    assert not np.array_equal(a, synth.vcf_sorted(100_003, seed=10, contigs=4))
    smp, contigs, n = L.loop_index(a.tobytes(), BO, 1)
    assert [c[0] for c in contigs] == [b"chr1", b"chr2", b"chr3", b"chr4"] and n > 1000
    assert sum(x == y for x, y in zip(smp, smp[1:])) > n // 20          # some equal neighbours
    big = synth.vcf_sorted(3_000_017, seed=1, contigs=2, block=100_003)  # several copies of the tile per contig
    assert L.loop_index(big.tobytes(), BO, 128)[1][0][6] > 10**6
