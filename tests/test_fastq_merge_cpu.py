"""The FASTQ read index without a GPU: libdpfq.so's ABI and ISA-guard stamp; scan/fastq.py's merge, the object
layer's chain and the FASTQ plugin over a numpy stand-in for the per-part device step (tests/_fastq_model.py), equal to
the definition's byte loop (tests/_fastq_loop.py); the two strategies and fetch_reads over a memory store against an
index built by the loop.  tests/test_gpu_fastq*.py run the kernels."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

import _fastq_loop as L
import _fastq_model as M
from dataplug_amd import build as B
from dataplug_amd import synth
from dataplug_amd.cloudobject import CloudObject
from dataplug_amd.formats.genomics import fastq as ffq
from dataplug_amd.scan import _fq
from dataplug_amd.scan import fastq
from dataplug_amd.scan import objects as scan_objects
from dataplug_amd.scan.fastq import FastqFormatError
from dataplug_amd.storage import MemoryStore

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ ABI, stamp
def test_header_table_exports_and_stamp_agree():
    raw = open(os.path.join(REPO, "include", "dpfq.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    fns = sorted(set(re.findall(r"\b(dfq_[a-z0-9_]+)\s*\(", text)))
    assert sorted(n for n, _, _ in _fq.SIGNATURES) == fns
    for name, _, args in _fq.SIGNATURES:                                 # the argument counts
        decl = re.search(r"\b%s\s*\(([^)]*)\)" % name, text).group(1).strip()
        assert len(args) == (0 if decl in ("", "void") else decl.count(",") + 1), name
    assert os.path.exists(_fq.LIB_PATH), f"{_fq.LIB_PATH} missing: run __graft_entry__.build()"
    lib = ctypes.CDLL(_fq.LIB_PATH)
    assert [f for f in fns if not hasattr(lib, f)] == []
    assert _fq.load().dfq_abi_version() == _fq.ABI_VERSION == 1
    words = dict(re.findall(r"#define DFQ_R_(\w+) (\d+)", raw))
    assert {k: int(v) for k, v in words.items()} == {
        "MALFORMED": _fq.R_MALFORMED, "MAX_LEN": _fq.R_MAX_LEN, "BASES": _fq.R_BASES,
        "MIN_MALFORMED": _fq.R_MIN_MALFORMED, "MIN_LEN": _fq.R_MIN_LEN, "WORDS": _fq.R_WORDS}
    kinds = {k: int(v) for k, v in re.findall(r"#define DFQ_(WELL_FORMED|BAD_\w+|LENGTH_MISMATCH) (\d+)u", raw)}
    assert kinds == {"WELL_FORMED": 0, "BAD_HEADER": 1, "BAD_SEPARATOR": 2, "LENGTH_MISMATCH": 3}
    assert [k.upper() if k else None for k in L.KINDS[1:]] == ["BAD_HEADER", "BAD_SEPARATOR", "LENGTH_MISMATCH"]
    assert fastq.KINDS[1:] == L.KINDS[1:] + ("truncated",)
    with open(B.stamp_path(B.FQ_OUT)) as f:
        rep = json.load(f)
    assert rep["result"] == "ok" and rep["guard_enforced"] is True and rep["arch"] == "gfx950"
    assert rep["so_sha256"] == B.sha256_file(B.FQ_OUT) and rep["src_sha256"] == B.sha256_file(B.FQ_SRC)
    assert rep["scratch"] == [] and rep["n_violations"] == 0 and rep["missing_kernels"] == []
    assert {k.split("<")[0] for k in rep["kernels"]} == set(B.FQ_REQUIRED)


def test_loader_refuses_a_missing_library(tmp_path):
    from dataplug_amd.scan._lib import DPScanUnavailable
    with pytest.raises(DPScanUnavailable):
        _fq.load(str(tmp_path / "missing.so"))
    bare = tmp_path / "libdpfq.so"
    bare.write_bytes(open(_fq.LIB_PATH, "rb").read())                    # the library without its stamp
    with pytest.raises(DPScanUnavailable):
        _fq.load(str(bare))


# ------------------------------------------------------------------------------------------------ inputs
def _long(seed, crlf=False, n=40):
    """~200 KB of log-uniform reads."""
    return synth.fastq_long(n, seed=seed, len_min=20, len_max=20_000, crlf=crlf).tobytes()


@pytest.fixture(scope="module")
def inputs():
    short = synth.fastq(60, seed=5, read_len=50).tobytes()
    one = synth.fastq_long(1, seed=6, len_min=75_000, len_max=75_000).tobytes()       # one read of 150 KB
    mid = L.read_ranges(short)[30][0]
    return {"long": _long(1), "crlf": _long(2, crlf=True), "open": _long(3)[:-1],
            "one_long_read": short[:mid] + one + short[mid:]}


@pytest.fixture(scope="module")
def wants(inputs):
    return {(name, k): L.loop_index(d, k) for name, d in inputs.items() for k in (1, 4, 64)}


def got_index(data, cuts, every):
    get = lambda q: data[q]
    idx = fastq.merge_parts(M.parts_by_cuts(data, cuts, every), len(data), every, get)
    return ([tuple(map(int, p)) for p in idx.samples.tolist()], idx.num_reads, idx.num_bases, idx.min_read_len,
            idx.max_read_len)


def even_cuts(size, part):
    return list(range(part, size, part))


# ------------------------------------------------------------------------------------------------ the merge
@pytest.mark.parametrize("name", ["long", "crlf", "open", "one_long_read"])
@pytest.mark.parametrize("part", [64, 4 << 10, 64 << 10])
def test_merge_equals_the_loop(inputs, wants, name, part):
    data = inputs[name]
    assert 150_000 < len(data) < 600_000
    for every in (1, 4, 64):
        assert got_index(data, even_cuts(len(data), part), every) == wants[name, every], (name, part, every)


def test_merge_random_cuts_and_line_edges(inputs, wants):
    data = inputs["long"]
    rng = np.random.default_rng(7)
    nl = [p for p in range(len(data)) if data[p] == 10]
    for nparts in (1, 2, 3, 9):
        for _ in range(4):
            cuts = rng.integers(0, len(data), nparts - 1).tolist()
            assert got_index(data, cuts, 4) == wants["long", 4], cuts
    for p in (nl[0], nl[3], nl[4], nl[len(nl) // 2], nl[-1]):            # cuts right at, before and behind a '\n'
        for cuts in ([p], [p + 1], [p, p + 1], [p - 1, p, p + 1]):
            cuts = [c for c in cuts if 0 < c < len(data)]
            assert got_index(data, cuts, 4) == wants["long", 4], cuts
    parts = M.parts_by_cuts(inputs["one_long_read"], even_cuts(len(inputs["one_long_read"]), 4 << 10), 4)
    assert sum(1 for p in parts if p.n_lines == 0) >= 30                 # parts without any line start are legal


def test_small_objects_every_cut():
    z = b"@\n\n+\n\n"
    for data in (z, z + b"@a\nAC\n+\nII\n" + z, z * 2 + b"@a\nAC\n+\nII", b"@a\r\nAC\r\n+\r\nII\r\n" * 2):
        want = L.loop_index(data, 2)
        for c in range(1, len(data)):
            assert got_index(data, [c], 2) == want
            assert got_index(data, [c, min(len(data) - 1, c + 2)], 2) == want
    assert fastq.merge_parts([], 0, 64, None) == fastq.empty_index()
    assert L.index_bytes(L.loop_index(b"")[0]) == fastq.samples_bytes(fastq.empty_index().samples)


def broken(data, where, how):
    """``data`` with one byte of read ``where`` changed: its '@', its '+', or a quality byte turned into a '\\n'."""
    s, e = L.read_ranges(data)[where]
    ln = [x for x in L.lines_of(data) if s <= x[0] < e]
    p = {"bad_header": ln[0][0], "bad_separator": ln[2][0]}.get(how)
    if how == "length_mismatch":                                         # the sequence line loses its last base
        return data[:ln[1][1] - 1] + data[ln[1][1]:]
    return data[:p] + b"x" + data[p + 1:]


@pytest.mark.parametrize("how", ["bad_header", "bad_separator", "length_mismatch"])
def test_errors_in_a_device_read_an_edge_read_and_the_last_partial_read(inputs, how):
    data = inputs["long"]
    part = 16 << 10
    cuts = even_cuts(len(data), part)
    parts = M.parts_by_cuts(data, cuts, 4)
    lines_before = np.cumsum([0] + [p.n_lines for p in parts])
    dev = [p for p in parts if p.n_reads >= 2]
    in_device = dev[1].read0 + dev[1].n_reads - 1                        # the last read a device step handles
    in_edge = next(r for r in range(40) if not any(p.read0 <= r < p.read0 + p.n_reads for p in parts))
    for where in (in_device, in_edge):
        bad = broken(data, where, how)
        with pytest.raises(L.LoopError) as le:
            L.loop_index(bad, 4)
        assert (le.value.kind, le.value.read) == (how, where)
        with pytest.raises(FastqFormatError) as e:
            fastq.merge_parts(M.parts_by_cuts(bad, even_cuts(len(bad), part), 4), len(bad), 4, lambda q: bad[q])
        assert (e.value.kind, e.value.read, e.value.offset) == (how, where, le.value.offset), where
        assert isinstance(e.value, ValueError) and str(where) in str(e.value)
    assert int(lines_before[-1]) == 160
    # the last, partial read: truncated, unless a malformed read comes first
    s, e = L.read_ranges(data)[-1]
    cut = data[:s + (e - s) // 2]
    with pytest.raises(FastqFormatError) as e:
        fastq.merge_parts(M.parts_by_cuts(cut, even_cuts(len(cut), part), 4), len(cut), 4, lambda q: cut[q])
    assert (e.value.kind, e.value.read, e.value.offset) == ("truncated", 39, s)
    bad = broken(cut, in_device, how)
    with pytest.raises(FastqFormatError) as e:
        fastq.merge_parts(M.parts_by_cuts(bad, even_cuts(len(bad), part), 4), len(bad), 4, lambda q: bad[q])
    assert (e.value.kind, e.value.read) == (how, in_device)


# ------------------------------------------------------------------------------------------------ object layer, plugin
def _mem(name):
    MemoryStore._named.pop(name, None)
    return {"endpoint_url": f"memory://{name}"}


def _co(data: bytes, key: str, cfg):
    co = CloudObject.from_s3(ffq.FASTQ, f"s3://data/{key}", fetch=False, s3_config=cfg)
    try:
        co.storage.head_bucket(Bucket="data")
    except Exception:
        co.storage.create_bucket(Bucket="data")
    co.storage.put_object(Body=data, Bucket="data", Key=key)
    return CloudObject.from_s3(ffq.FASTQ, f"s3://data/{key}", s3_config=cfg)


def pairs_of(idx):
    return [tuple(map(int, p)) for p in idx.samples.tolist()]


@pytest.mark.parametrize("devs", [[0], [0, 0, 0]])
def test_reads_index_object_chains_the_parts(monkeypatch, inputs, wants, devs):
    layer = M.ModelDevices(monkeypatch, devs)
    data = inputs["one_long_read"]
    co = _co(data, "r.fastq", _mem(f"fq_cpu_obj{len(devs)}"))
    gets = []
    real = co.storage.get_object
    monkeypatch.setattr(co.storage, "get_object", lambda **kw: (gets.append(kw.get("Range")), real(**kw))[1])
    idx = scan_objects.reads_index_object(co, 4, part_bytes=5000)
    assert (pairs_of(idx), *idx[1:]) == wants["one_long_read", 4]
    reads = sorted(c[1:] for c in layer.calls if c[0] == "reads" and c[1] is not None)
    lines = sorted(c[1:] for c in layer.calls if c[0] == "lines")
    assert len(lines) >= 30 and sorted(layer.fetches) == [(lo, hi) for lo, hi, _ in lines]    # no halo is fetched
    before = np.cumsum([0] + [n for _, _, n in lines if n])[:-1]
    assert [(r[1], r[2]) for r in reads] == [((-int(b)) % 4, -(-int(b) // 4)) for b in before]
    single = [g for g in gets if g and re.fullmatch(r"bytes=(\d+)-\1", g)]
    assert 0 < len(single) <= 14 * len(lines)                            # the edge reads' bytes, one at a time
    with pytest.raises(ValueError):
        scan_objects.reads_index_object(co, 3)


def test_a_part_that_raises_releases_the_chain(monkeypatch, inputs):
    import threading
    data = inputs["long"]
    layer = M.ModelDevices(monkeypatch, [0, 0, 0])
    co = _co(data, "f.fastq", _mem("fq_cpu_fail"))
    parts = scan_objects.line_parts(0, len(data), 3, 30_000)
    layer.fail_at = {parts[1][0]}                        # part 1 never publishes its count: parts 2.. wait for it
    result = {}

    def call():
        try:
            result["value"] = scan_objects.reads_index_object(co, 4, part_bytes=30_000)
        except BaseException as e:
            result["error"] = e

    th = threading.Thread(target=call, daemon=True)
    th.start()
    th.join(30.0)                                        # a guard against a hang: a released waiter polls every 50 ms
    assert not th.is_alive(), "reads_index_object hangs when a part fails"
    assert "value" not in result and "model: the part's launch failed" in str(result["error"])
    assert not [c for c in layer.calls if c[0] == "reads" and c[3] > 0]      # none past part 0 went on
    layer.fail_at = set()
    scan_objects.release_workers()
    assert pairs_of(scan_objects.reads_index_object(co, 4, part_bytes=30_000)) == L.loop_index(data, 4)[0]


def indexed(monkeypatch, data, key, name, every, part_bytes=5000):
    M.ModelDevices(monkeypatch, [0, 0])
    real = scan_objects.reads_index_object
    monkeypatch.setattr(scan_objects, "reads_index_object", lambda co, k, **kw: real(co, k, part_bytes=part_bytes, **kw))
    co = _co(data, key, _mem(name))
    co.preprocess(extra_args={"reads_index_every": every})
    return co


def meta_keys(co):
    return sorted(o["Key"] for o in co.storage.list_objects_v2(Bucket=co.meta_path.bucket).get("Contents", []))


@pytest.mark.parametrize("every", [1, 4, 64])
def test_plugin_stores_the_loops_index_and_attributes(monkeypatch, inputs, wants, every):
    data = inputs["long"]
    co = indexed(monkeypatch, data, "p.fastq", f"fq_cpu_plugin{every}", every)
    pairs, r, b, mn, mx = wants["long", every]
    got = co.storage.get_object(Bucket=co.meta_path.bucket, Key="p.fastq.fqi")["Body"].read()
    assert got == L.index_bytes(pairs)
    a = co.attributes
    assert (a.reads_index_key, a.reads_index_every, a.num_reads, a.num_bases, a.min_read_len, a.max_read_len) == \
        ("p.fastq.fqi", every, r, b, mn, mx)
    smp = ffq.load_read_samples(co)
    assert smp.dtype.names == ("offset", "bases") and list(zip(smp["offset"].tolist(), smp["bases"].tolist())) == pairs


def test_plugin_error_stores_nothing_and_names_the_read(monkeypatch, inputs):
    data = broken(inputs["long"], 17, "bad_separator")
    M.ModelDevices(monkeypatch, [0, 0])
    co = _co(data, "e.fastq", _mem("fq_cpu_error"))
    with pytest.raises(L.LoopError) as le:
        L.loop_index(data)
    with pytest.raises(ffq.FastqFormatError) as e:
        co.preprocess()
    assert (e.value.kind, e.value.read, e.value.offset) == ("bad_separator", 17, le.value.offset)
    assert meta_keys(co) == []
    co = CloudObject.from_s3(ffq.FASTQ, "s3://data/e.fastq", s3_config={"endpoint_url": "memory://fq_cpu_error"})
    with pytest.raises(KeyError, match="preprocess it as"):
        ffq.load_read_samples(co)


def test_empty_object(monkeypatch):
    co = indexed(monkeypatch, b"", "z.fastq", "fq_cpu_empty", 64)
    assert co.storage.get_object(Bucket=co.meta_path.bucket, Key="z.fastq.fqi")["Body"].read() == bytes(16)
    assert co.attributes.num_reads == 0 and ffq.fetch_reads(co, 0, 0) == b""
    sl = co.partition(ffq.partition_bases_strategy, num_chunks=3)
    assert [(s.range_0, s.range_1, s.num_reads) for s in sl] == [(0, 0, 0)] * 3


# ------------------------------------------------------------------------------------------------ strategies, fetch
def loop_indexed(data, key, name, every):
    """A FASTQ object whose stored index and attributes were written from the byte loop's result."""
    from dataplug_amd.preprocessing.handler import upload_metadata
    from dataplug_amd.preprocessing.metadata import PreprocessingMetadata
    pairs, r, b, mn, mx = L.loop_index(data, every)
    co = _co(data, key, _mem(name))
    co.storage.create_bucket(Bucket=co.meta_path.bucket)
    co.storage.put_object(Body=L.index_bytes(pairs), Bucket=co.meta_path.bucket, Key=key + ".fqi")
    upload_metadata(co, PreprocessingMetadata(attributes={
        "reads_index_key": key + ".fqi", "reads_index_every": every, "num_reads": r, "num_bases": b,
        "min_read_len": mn, "max_read_len": mx}))
    co = CloudObject.from_s3(ffq.FASTQ, f"s3://data/{key}", s3_config={"endpoint_url": f"memory://{name}"})
    co.fetch()
    return co, pairs, r, b


@pytest.mark.parametrize("every", [1, 4, 16, 64])                      # R = 40: R % K is 0, 0, 8 and 40
@pytest.mark.parametrize("n", [1, 3, 7, 64])
def test_strategies_tile_the_object_at_read_starts(inputs, every, n):
    data = inputs["long"]
    co, pairs, r, b = loop_indexed(data, "s.fastq", f"fq_cpu_strat{every}_{n}", every)
    starts = {s for s, _ in L.read_ranges(data)} | {len(data)}
    s_count = len(pairs) - 1
    widest = max(b1 - b0 for (_, b0), (_, b1) in zip(pairs, pairs[1:]))
    for strategy in (ffq.partition_reads_strategy, ffq.partition_bases_strategy):
        sl = co.partition(strategy, num_chunks=n)
        assert len(sl) == n and sl[0].range_0 == 0 and sl[-1].range_1 == len(data)
        assert all(a.range_1 == c.range_0 for a, c in zip(sl, sl[1:]))   # the slices tile [0, size)
        assert all(s.range_0 in starts for s in sl)
        assert sum(s.num_reads for s in sl) == r and sum(s.num_bases for s in sl) == b
        assert all(s.num_reads >= 0 and s.first_read <= r for s in sl)
        assert [s.first_read for s in sl] == list(np.cumsum([0] + [s.num_reads for s in sl])[:-1])
        for s in sl:
            text = s.get()
            assert text.encode() == data[s.range_0:s.range_1]
            assert text.count("\n") == 4 * s.num_reads
        if n > s_count:
            assert sum(1 for s in sl if s.range_0 == s.range_1) >= n - s_count      # n > S: empty slices
        if strategy is ffq.partition_bases_strategy:
            # each boundary is the sample nearest to its target i * B / n, so it misses it by at most half the widest
            # sample interval's bases, and a slice's bases differ from B / n by at most that whole interval
            assert all(abs(s.num_bases - b / n) <= widest for s in sl), [s.num_bases for s in sl]
        else:
            assert [s.first_read for s in sl] == [((i * s_count) // n) * every for i in range(n)]
            assert sl[-1].first_read + sl[-1].num_reads == r             # R % K reads in the last slice too


@pytest.mark.parametrize("n", [1, 2, 3, 8])
def test_a_cut_at_the_closing_sample_begins_at_read_r(n):
    """Four reads of 4 bases and one of 400, K = 4: R = 5, S = 2, R % K = 1, and the last sample interval holds nearly
    all bases, so the bases strategy puts cuts before the last one on the closing sample, which stands for read 5."""
    a = b"@a\nACGT\n+\nIIII\n"
    data = a * 4 + b"@b\n" + b"A" * 400 + b"\n+\n" + b"I" * 400 + b"\n"
    co, pairs, r, b = loop_indexed(data, "c.fastq", f"fq_cpu_closing{n}", 4)
    assert pairs == [(0, 0), (60, 16), (len(data), 416)] and (r, b) == (5, 416)
    for strategy in (ffq.partition_reads_strategy, ffq.partition_bases_strategy):
        sl = co.partition(strategy, num_chunks=n)
        assert len(sl) == n and all(s.num_reads >= 0 for s in sl)
        assert sum(s.num_reads for s in sl) == 5 and sum(s.num_bases for s in sl) == 416
        assert [s.first_read for s in sl] == list(np.cumsum([0] + [s.num_reads for s in sl])[:-1])
        assert all(s.get().count("\n") == 4 * s.num_reads for s in sl)
    if n == 3:                                                           # targets 139 and 277: samples 1 and 2
        assert [(s.range_0, s.range_1, s.first_read, s.num_reads) for s in sl] == \
            [(0, 60, 0, 4), (60, len(data), 4, 1), (len(data), len(data), 5, 0)]


def test_bases_strategy_picks_the_nearest_sample_and_the_lower_on_a_tie():
    # reads of 0, 4, 4, 0, 8 bases: cumulative bases at the samples (K = 1) 0 0 4 8 8 16
    z, a = b"@\n\n+\n\n", b"@a\nACGT\n+\nIIII\n"
    data = z + a + a + z + b"@b\nACGTACGT\n+\nIIIIIIII\n"
    co, pairs, r, b = loop_indexed(data, "t.fastq", "fq_cpu_tie", 1)
    assert [p[1] for p in pairs] == [0, 0, 4, 8, 8, 16]
    sl = co.partition(ffq.partition_bases_strategy, num_chunks=2)        # target 8: samples 3 and 4 tie, 3 wins
    assert [(s.first_read, s.num_reads, s.num_bases) for s in sl] == [(0, 3, 8), (3, 2, 8)]
    sl = co.partition(ffq.partition_bases_strategy, num_chunks=8)        # targets 2 4 6 8 10 12 14
    assert [s.first_read for s in sl] == [0, 0, 2, 2, 3, 3, 3, 5][:8]
    assert [s.num_bases for s in sl] == [0, 4, 0, 4, 0, 0, 8, 0]


@pytest.mark.parametrize("every", [1, 4, 64])
def test_fetch_reads_equals_a_host_walk(inputs, every):
    data = inputs["long"]
    co, pairs, r, b = loop_indexed(data, "g.fastq", f"fq_cpu_fetch{every}", every)
    rr = L.read_ranges(data)
    want = lambda f, c: data[rr[f][0]:rr[f + c - 1][1]] if c else b""
    k = every
    cases = {(f, c) for f in (0, k - 1, k, k + 1, 2 * k - 1, 2 * k) for c in (0, 1, k - 1, k, k + 1) if f + c <= r}
    cases |= {(r - 1, 1), (r, 0), (0, r), (r - k - 1, k + 1), (max(0, r - 2 * k), 2 * k if 2 * k <= r else r)}
    gets = []
    real = co.storage.get_object
    co.storage.get_object = lambda **kw: (gets.append(kw), real(**kw))[1]
    for f, c in sorted(x for x in cases if x[0] >= 0 and x[1] >= 0):
        del gets[:]
        assert ffq.fetch_reads(co, f, c) == want(f, c), (f, c)
        data_gets = [g for g in gets if g["Key"] == "g.fastq"]
        assert len(data_gets) == (1 if c else 0)
        if c:
            lo, hi = pairs[f // k][0], pairs[-(-(f + c) // k)][0]
            assert data_gets[0]["Range"] == f"bytes={lo}-{hi - 1}"
    for f, c in ((0, r + 1), (r, 1), (-1, 1), (1, -1)):
        with pytest.raises(IndexError):
            ffq.fetch_reads(co, f, c)
