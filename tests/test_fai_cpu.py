"""The faidx-compatible FASTA index without a GPU: the definition's byte loop (tests/_fai_loop.py) on hand-written
objects, the count formulas of include/dpfai.h against the loop, libdpfai.so's ABI and ISA-guard stamp, and the
object and plugin layers (part clipping and merging, the stored text, fetch_region, partition_bases_strategy) over a
numpy-backed fake of the device layer.  tests/test_gpu_fai*.py run the kernels."""
import ctypes
import json
import os
import pickle
import re

import numpy as np
import pytest

from _fai_loop import loop_fai, loop_text
from _fai_model import FakeDevices, header_pairs, np_names, np_pass1, np_pass2
from dataplug_amd import build as B
from dataplug_amd.cloudobject import CloudObject
from dataplug_amd.formats.genomics import fasta as ffasta
from dataplug_amd.scan import _fai
from dataplug_amd.scan import fai as sfai
from dataplug_amd.scan import objects as scan_objects
from dataplug_amd.scan.fai import FaiFormatError
from dataplug_amd.storage import MemoryStore

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = 0xFFFFFFFFFFFFFFFF


# ------------------------------------------------------------------------------------------------ the loop, by hand
HAND = (b">s1 desc\nACGT\nACGT\nAC\n"                    # LF, a short last line
        b">s2\tx\nACGTA\r\nACGTA\r\nAC\r\n"              # CRLF, the name ends at a tab
        b">s4\n"                                          # an empty body
        b">s5\nACGTACGT\n"                                # one line
        b">s6 x\nAC GT\nAC\tGT\nA\n"                      # spaces and tabs count as bases
        b">s7\nA\nC\nG\n"
        b">s8\nACGT\nACGT\n"                              # full lines only
        b">s9\r\nACG\r\nA\r\n"                            # the header line ends in CRLF too
        b">s10\nACGT\nAC")                                # a last line without a line break
HAND_FAI = (b"s1\t10\t9\t4\t5\n"
            b"s2\t12\t28\t5\t7\n"
            b"s4\t0\t50\t0\t0\n"
            b"s5\t8\t54\t8\t9\n"
            b"s6\t11\t69\t5\t6\n"
            b"s7\t3\t87\t1\t2\n"
            b"s8\t8\t97\t4\t5\n"
            b"s9\t4\t112\t3\t5\n"
            b"s10\t6\t125\t4\t5\n")


def test_loop_on_a_hand_written_object():
    assert loop_text(loop_fai(HAND, header_pairs(HAND))) == HAND_FAI
    one = b">only one\nACGTACGT"                          # a body of one line with no break
    assert loop_text(loop_fai(one, header_pairs(one))) == b"only\t8\t10\t8\t8\n"


IRREGULAR = [
    (b">ok\nAC\n>a\nACGT\nAC\nACGT\n", 1, b"a"),                        # a short middle line
    (b">a\nACGT\nACGTACGTA\nACGT\n", 0, b"a"),                          # over-long, its breaks on multiples of W
    (b">ok\nAC\n>b z\nACGT\r\nACGT\n", 1, b"b"),                        # mixed line endings
    (b">a x\nAC\n>b\nAC\n>a y\nAC\n", 2, b"a"),                         # a duplicate name
    (b">a\nACGT\nACGTA\n", 0, b"a"),                                    # a longer last line
    (b">a\nACGT\nACGTA", 0, b"a"),                                      # ... without its break
]


@pytest.mark.parametrize("data,ordinal,name", IRREGULAR)
def test_each_irregular_class_raises(data, ordinal, name):
    with pytest.raises(FaiFormatError) as ei:
        loop_fai(data, header_pairs(data))
    assert isinstance(ei.value, ValueError) and (ei.value.ordinal, ei.value.name) == (ordinal, name)
    with pytest.raises(FaiFormatError) as ei:
        formulas(data, header_pairs(data))
    assert (ei.value.ordinal, ei.value.name) == (ordinal, name)


# ------------------------------------------------------------------------------------------------ counts in numpy
def formulas(data: bytes, pairs):
    """The .fai rows through the counts and scan.fai.derive: what the GPU path computes, in numpy."""
    d = np.frombuffer(data, np.uint8)
    p = np.asarray(pairs, np.uint64).reshape(-1, 2)
    b, e = sfai.bodies(p, len(data))
    nl, cr, first = np_pass1(d, 0, b, e)
    w = sfai.line_widths(b, e, nl, first)
    off, last = np_pass2(d, 0, b, e, b, np.minimum(w, 0xFFFFFFFF))
    names = sfai.split_names(*np_names(d, 0, p[:, 0], p[:, 1]))
    return names, sfai.derive(b, e, nl, cr, first, off, last, names)


def wrapped(rng, n_seq, lb_max=9, perturb=0.0, drop=0.3):
    """A FASTA of ``n_seq`` wrapped sequences (LF or CRLF per sequence), optionally with random damage."""
    out = []
    for i in range(n_seq):
        lb = int(rng.integers(1, lb_max + 1))
        term = b"\r\n" if rng.random() < 0.3 else b"\n"
        n = int(rng.integers(0, 4 * lb))
        seq = bytes(rng.choice(np.frombuffer(b"ACGT ", np.uint8), n).tolist())
        body = b"".join(seq[k:k + lb] + term for k in range(0, n, lb))
        if body and rng.random() < drop:
            body = body[:-len(term)]                     # the last line without its break
        name = b"q%d" % (i if rng.random() < 0.95 else 0)
        out.append(b">" + name + (b" d" if rng.random() < 0.5 else b"") + term + body)
    raw = bytearray(b"".join(out))
    for _ in range(int(perturb * len(raw))):
        raw[int(rng.integers(0, len(raw)))] = int(rng.choice(np.frombuffer(b">\n\rA ", np.uint8)))
    return bytes(raw)


def test_count_formulas_agree_with_the_loop():
    rng = np.random.default_rng(2024)
    alphabet = np.frombuffer(b">\n\rA ", np.uint8)
    ok = bad = 0
    for it in range(4000):
        if it % 2:
            data = bytes(rng.choice(alphabet, int(rng.integers(0, 40)), p=[0.08, 0.25, 0.07, 0.5, 0.1]).tolist())
        else:
            data = wrapped(rng, int(rng.integers(1, 5)), perturb=0.02 * (it % 4 == 0))
        pairs = header_pairs(data)
        try:
            want = loop_fai(data, pairs)
        except FaiFormatError as e:
            with pytest.raises(FaiFormatError) as ei:
                formulas(data, pairs)
            assert (ei.value.ordinal, ei.value.name) == (e.ordinal, e.name), data
            bad += 1
            continue
        names, rows = formulas(data, pairs)
        assert sfai.fai_text(names, rows) == loop_text(want), data
        assert sfai.parse_fai(loop_text(want))[0] == names
        ok += 1
    assert ok > 800 and bad > 800                        # both sides of the definition were exercised


# ------------------------------------------------------------------------------------------------ ABI, stamp
def test_header_table_exports_and_stamp_agree():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "dpfai.h")).read(), flags=re.S)
    fns = sorted(set(re.findall(r"\b(dfai_[a-z0-9_]+)\s*\(", text)))
    assert sorted(n for n, _, _ in _fai.SIGNATURES) == fns
    assert os.path.exists(_fai.LIB_PATH), f"{_fai.LIB_PATH} missing: run __graft_entry__.build()"
    lib = ctypes.CDLL(_fai.LIB_PATH)
    assert [f for f in fns if not hasattr(lib, f)] == []
    assert _fai.load().dfai_abi_version() == _fai.ABI_VERSION == 1
    with open(B.stamp_path(B.FAI_OUT)) as f:
        rep = json.load(f)
    assert rep["result"] == "ok" and rep["guard_enforced"] is True and rep["arch"] == "gfx950"
    assert rep["so_sha256"] == B.sha256_file(B.FAI_OUT) and rep["src_sha256"] == B.sha256_file(B.FAI_SRC)
    assert rep["scratch"] == [] and rep["n_violations"] == 0 and rep["missing_kernels"] == []
    assert {k.split("<")[0] for k in rep["kernels"]} == set(B.FAI_REQUIRED)


def test_loader_refuses_a_missing_library(tmp_path, monkeypatch):
    from dataplug_amd.scan._lib import DPScanUnavailable
    with pytest.raises(DPScanUnavailable):
        _fai.load(str(tmp_path / "missing.so"))
    bare = tmp_path / "libdpfai.so"
    bare.write_bytes(open(_fai.LIB_PATH, "rb").read())   # the library without its stamp
    with pytest.raises(DPScanUnavailable):
        _fai.load(str(bare))


# ------------------------------------------------------------------------------------------------ fai_index_object
# (tests/_fai_model.py: FakeContext, FakeDevices)
def _mem(name):
    MemoryStore._named.pop(name, None)
    return {"endpoint_url": f"memory://{name}"}


def _co(data: bytes, key: str, cfg):
    co = CloudObject.from_s3(ffasta.FASTA, f"s3://data/{key}", fetch=False, s3_config=cfg)
    try:
        co.storage.head_bucket(Bucket="data")
    except Exception:
        co.storage.create_bucket(Bucket="data")
    co.storage.put_object(Body=data, Bucket="data", Key=key)
    return CloudObject.from_s3(ffasta.FASTA, f"s3://data/{key}", s3_config=cfg)


@pytest.fixture(scope="module")
def genome():
    rng = np.random.default_rng(77)
    parts = [wrapped(rng, 40, lb_max=70, drop=0.0)]
    long_header = b">long" + b"N" * 300 + b" " + b"d" * 500 + b"\n"          # longer than the test's halo
    parts.append(long_header + b"ACGTACGTAC\n" * 700 + b"ACG\n")              # a body over several parts
    parts.append(wrapped(np.random.default_rng(78), 30, lb_max=61, drop=0.0))
    data = b"".join(parts)
    pairs = header_pairs(data)
    # unique names: wrapped() repeats names on purpose
    seen, out, p = {}, bytearray(), 0
    for s, e in pairs:
        out += data[p:s]
        line = data[s:e]
        nm = re.split(rb"[ \t\r\n]", line[1:], maxsplit=1)[0]
        k = seen.get(nm, 0)
        seen[nm] = k + 1
        out += b">" + nm + (b"_%d" % k if k else b"") + line[1 + len(nm):]
        p = e
    out += data[p:]
    data = bytes(out)
    pairs = header_pairs(data)
    return data, pairs, loop_fai(data, pairs)


@pytest.mark.parametrize("devs", [[0], [0, 0, 0]])
def test_fai_index_object_clips_and_merges_the_parts(monkeypatch, genome, devs):
    data, pairs, want = genome
    fake = FakeDevices(monkeypatch, devs)
    co = _co(data, "g.fa", _mem(f"fai_cpu_obj{len(devs)}"))
    names, rows = scan_objects.fai_index_object(co, pairs, part_bytes=1000, halo=64)
    assert sfai.fai_text(names, rows) == loop_text(want)
    parts = scan_objects.line_parts(0, len(data), len(devs), 1000)
    assert len(parts) >= 8
    assert sorted(c[1] for c in fake.calls if c[0] == "pass1") == [lo for lo, _ in parts]
    assert sorted(c[1] for c in fake.calls if c[0] == "pass2") == [lo for lo, _ in parts]
    # every part is fetched with its halo; again for pass 2, as an entry holds several parts here
    assert sorted(set(fake.fetches)) == [(lo, min(len(data), hi + 64)) for lo, hi in parts]
    assert len(fake.fetches) == 2 * len(parts)
    # one part per entry: pass 2 runs on the resident bytes
    fake.fetches.clear()
    names, rows = scan_objects.fai_index_object(co, pairs, part_bytes=1 << 30)
    assert sfai.fai_text(names, rows) == loop_text(want)
    assert len(fake.fetches) == len(scan_objects.line_parts(0, len(data), len(devs)))
    assert scan_objects.fai_index_object(co, np.zeros((0, 2), np.uint64))[0] == []


def test_fai_index_object_reports_the_first_offending_sequence(monkeypatch, genome):
    data, pairs, _ = genome
    FakeDevices(monkeypatch, [0, 0])
    s, e = pairs[len(pairs) // 2]
    broken = data[:e] + b"ACGTACGT\nAC\nACGTACGT\n" + data[e:]
    bp = header_pairs(broken)
    with pytest.raises(FaiFormatError) as want:
        loop_fai(broken, bp)
    co = _co(broken, "b.fa", _mem("fai_cpu_broken"))
    with pytest.raises(FaiFormatError) as got:
        scan_objects.fai_index_object(co, bp, part_bytes=1500, halo=64)
    assert (got.value.ordinal, got.value.name) == (want.value.ordinal, want.value.name)
    assert got.value.ordinal == len(pairs) // 2


# ------------------------------------------------------------------------------------------------ the plugin
@pytest.fixture
def stub_headers(monkeypatch):
    """The GPU header scan replaced by header_pairs over the object's bytes."""
    def fasta_index_object(co, plan, u64=False, **kw):
        raw = co.storage.get_object(Bucket=co.path.bucket, Key=co.path.key)["Body"].read()
        return np.asarray(header_pairs(raw), np.uint64 if u64 else np.uint32).reshape(-1, 2)
    monkeypatch.setattr(scan_objects, "fasta_index_object", fasta_index_object)


def dewrapped(data, pairs):
    seqs = []
    for i, (s, e) in enumerate(pairs):
        end = pairs[i + 1][0] if i + 1 < len(pairs) else len(data)
        seqs.append(data[e:end].replace(b"\n", b"").replace(b"\r", b""))
    return seqs


def test_preprocess_stores_the_text_and_the_strategies_slice_bases(monkeypatch, stub_headers, genome):
    data, pairs, want = genome
    FakeDevices(monkeypatch, [0, 0])
    cfg = _mem("fai_cpu_plugin")
    co = _co(data, "g.fa", cfg)
    co.preprocess(extra_args={"fai": True}, chunk_size=len(data) // 4)
    keys = sorted(c["Key"] for c in co.storage.list_objects_v2(Bucket=co.meta_path.bucket)["Contents"])
    assert keys == ["g.fa", "g.fa.attrs", "g.fa.fai"]
    assert co.storage.get_object(Bucket=co.meta_path.bucket, Key="g.fa.fai")["Body"].read() == loop_text(want)
    seqs = dewrapped(data, pairs)
    assert co.attributes.fai_key == "g.fa.fai" and co.attributes.num_bases == sum(map(len, seqs))
    assert co.attributes.num_sequences == len(pairs)
    names, rows = ffasta.load_fai(co)
    assert names == [r[0] for r in want] and rows["length"].tolist() == [len(s) for s in seqs]
    # fetch_region: 0-based half-open base coordinates, the line breaks stripped
    rng = np.random.default_rng(5)
    for i in rng.integers(0, len(seqs), 60):
        n = len(seqs[i])
        a = int(rng.integers(0, n + 1))
        b = int(rng.integers(a, n + 1))
        assert ffasta.fetch_region(co, names[i], a, b) == seqs[i][a:b], (names[i], a, b)
    big = int(np.argmax(rows["length"]))
    assert ffasta.fetch_region(co, names[big].decode(), 0, len(seqs[big])) == seqs[big]
    with pytest.raises(ValueError):
        ffasta.fetch_region(co, names[0], 0, len(seqs[0]) + 1)
    with pytest.raises(KeyError):
        ffasta.fetch_region(co, b"nope", 0, 0)
    # partition_bases_strategy: equal shares of the bases, the last slice the rest
    allb = b"".join(seqs)
    cum = np.concatenate([[0], np.cumsum([len(s) for s in seqs])])
    for k in (1, 2, 7, 13):
        slices = co.partition(ffasta.partition_bases_strategy, num_chunks=k)
        share = len(allb) // k
        assert len(slices) == k and slices[0].range_0 == 0 and slices[-1].range_1 == len(data)
        for j, s in enumerate(slices):
            g0, g1 = j * share, len(allb) if j == k - 1 else (j + 1) * share
            raw = s.get()
            lines = raw.replace(b"\r", b"").split(b"\n")
            assert b"".join(ln for ln in lines if not ln.startswith(b">")) == allb[g0:g1], (k, j)
            if j:
                assert s.range_0 == slices[j - 1].range_1
            i = int(np.searchsorted(cum, g0, "right")) - 1
            if g0 == cum[i]:
                assert s.header is None and s.offset == 0
            else:
                assert s.header == tuple(int(x) for x in pairs[i]) and s.offset == g0 - cum[i]
                assert lines[0] == data[pairs[i][0]:pairs[i][1]].rstrip(b"\r\n") + b" offset=%d" % s.offset


def test_without_fai_nothing_changes_and_an_irregular_object_keeps_its_header_index(monkeypatch, stub_headers, genome):
    data, pairs, _ = genome
    FakeDevices(monkeypatch, [0])
    cfg = _mem("fai_cpu_plain")
    co = _co(data, "p.fa", cfg)
    co.preprocess(chunk_size=len(data) // 4)
    keys = sorted(c["Key"] for c in co.storage.list_objects_v2(Bucket=co.meta_path.bucket)["Contents"])
    assert keys == ["p.fa", "p.fa.attrs"]
    attrs = pickle.loads(co.storage.get_object(Bucket=co.meta_path.bucket, Key="p.fa.attrs")["Body"].read())
    assert attrs == {"num_sequences": len(pairs)}
    index = co.storage.get_object(Bucket=co.meta_path.bucket, Key="p.fa")["Body"].read()
    assert index == np.asarray(pairs, np.uint32).tobytes()
    with pytest.raises(KeyError):
        ffasta.load_fai(co)
    # an irregular object: FaiFormatError, and the header index is stored as without fai
    e = pairs[3][1]
    broken = data[:e] + b"ACGTACGT\nAC\nACGTACGT\n" + data[e:]
    cb = _co(broken, "b.fa", cfg)
    with pytest.raises(FaiFormatError) as ei:
        cb.preprocess(extra_args={"fai": True}, chunk_size=len(broken) // 4)
    assert ei.value.ordinal == 3
    keys = sorted(c["Key"] for c in cb.storage.list_objects_v2(Bucket=cb.meta_path.bucket)["Contents"])
    assert keys == ["b.fa", "b.fa.attrs", "p.fa", "p.fa.attrs"]
    attrs = pickle.loads(cb.storage.get_object(Bucket=cb.meta_path.bucket, Key="b.fa.attrs")["Body"].read())
    assert attrs == {"num_sequences": len(header_pairs(broken))}
    stored = cb.storage.get_object(Bucket=cb.meta_path.bucket, Key="b.fa")["Body"].read()
    assert stored == np.asarray(header_pairs(broken), np.uint32).tobytes()
