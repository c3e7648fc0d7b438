"""The quote-aware record index without a GPU: libdpquote.so's ABI, ISA-guard stamp and loader refusal, the numpy
model against Python's csv module, and the record partition strategies over an in-memory store with a record index
written from the model (the scan is replaced by a stub, so this checks host logic only; tests/test_gpu_quote*.py run
the kernel).  The last section runs scan.objects.record_index_object itself -- the per-part counts, the carry chain,
the capacity choice and the release of waiting parts after a failure -- over a numpy-backed fake of the device layer."""
import csv as pycsv
import ctypes
import functools
import io
import json
import os
import pickle
import re
import shutil
import threading
import time

import numpy as np
import pytest

import _fake_scan
from _quote_model import record_ends
from dataplug_amd import build as B
from dataplug_amd import synth
from dataplug_amd.cloudobject import CloudObject
from dataplug_amd.formats import _lines
from dataplug_amd.formats.generic import csv as fcsv
from dataplug_amd.scan import _lib, _quote
from dataplug_amd.scan import objects as scan_objects
from dataplug_amd.storage import MemoryStore

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ ABI, stamp, loader
def header_functions():
    text = open(os.path.join(REPO, "include", "dpquote.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(dq_[a-z0-9_]+)\s*\(", text)))


def test_header_table_and_exports_agree():
    fns = header_functions()
    assert sorted(n for n, _, _ in _quote.SIGNATURES) == fns
    assert os.path.exists(_quote.LIB_PATH), f"{_quote.LIB_PATH} missing: run __graft_entry__.build()"
    lib = ctypes.CDLL(_quote.LIB_PATH)
    assert [f for f in fns if not hasattr(lib, f)] == []
    for must in ("dq_abi_version", "dq_last_error", "dq_ctx_create", "dq_ctx_destroy", "dq_records_async",
                 "dq_records_result", "dq_geometry"):
        assert must in fns
    assert _quote.load().dq_abi_version() == _quote.ABI_VERSION == 1


def test_header_documents_the_reference_lines():
    text = open(os.path.join(REPO, "include", "dpquote.h")).read()
    assert "formats/generic/csv.py:52-105" in text
    for code in ("DQ_ERR_CAPACITY", "DQ_ERR_OVERFLOW", "DQ_ERR_TIMEOUT"):
        assert code in text


def test_stamp_is_ok_and_belongs_to_this_build():
    with open(B.stamp_path(B.QUOTE_OUT)) as f:
        rep = json.load(f)
    assert rep["result"] == "ok" and rep["guard_enforced"] is True
    assert rep["so_sha256"] == B.sha256_file(B.QUOTE_OUT), "the stamp belongs to another build of libdpquote.so"
    assert rep["src_sha256"] == B.sha256_file(B.QUOTE_SRC), "libdpquote.so was built from another dpquote.hip: rebuild"
    assert rep["scratch"] == [] and rep["n_violations"] == 0 and rep["missing_kernels"] == []
    assert {k.split("<")[0] for k in rep["kernels"]} == set(B.QUOTE_REQUIRED)
    assert rep["arch"] == "gfx950"


def test_guard_required_argument_keeps_its_default(tmp_path):
    from dataplug_amd import isa_guard
    asm = tmp_path / "x.s"
    asm.write_text("_ZN12_GLOBAL__N_112quote_kernelILi0EEEvNS_9QuoteArgsE:\n\ts_endpgm\n.Lfunc_end0:\n")
    assert isa_guard.verify(str(asm), required=("quote_kernel",))["result"] == "ok"
    rep = isa_guard.verify(str(asm))                         # the default still asks for libdpscan's kernels
    assert rep["result"] == "FAIL" and set(rep["missing_kernels"]) == set(isa_guard.REQUIRED)
    assert isa_guard.verify(str(asm), required=("quote_kernel", "other_kernel"))["missing_kernels"] == ["other_kernel"]


def test_loader_refuses_a_library_without_its_stamp(tmp_path, monkeypatch):
    lib = tmp_path / "libdpquote.so"
    shutil.copyfile(_quote.LIB_PATH, lib)
    with pytest.raises(_lib.DPScanUnavailable, match="no ISA-guard stamp"):
        _quote.load(str(lib))
    (tmp_path / "libdpquote.so.isa.json").write_text(json.dumps({"result": "ok", "so_sha256": "0" * 64}))
    with pytest.raises(_lib.DPScanUnavailable, match="not loaded"):
        _quote.load(str(lib))
    monkeypatch.setattr(_quote, "LIB_PATH", str(tmp_path / "missing.so"))
    monkeypatch.setattr(_quote, "_lib", None)
    with pytest.raises(_lib.DPScanUnavailable, match="not found"):     # no CPU fallback
        _quote.load()


def test_ctx_create_reports_instead_of_crashing():
    lib = _quote.load()
    h = ctypes.c_void_p()
    rc = lib.dq_ctx_create(10 ** 6, None, ctypes.byref(h))             # no such device, with or without a GPU
    assert rc in (_quote.DQ_ERR_INVALID, _quote.DQ_ERR_HIP) and not h.value
    assert lib.dq_last_error()
    assert lib.dq_ctx_create(0, None, None) == _quote.DQ_ERR_INVALID
    assert lib.dq_ctx_destroy(None) == _quote.DQ_OK
    assert lib.dq_records_result(None, None, None, None) == _quote.DQ_ERR_INVALID


# ------------------------------------------------------------------------------------------------ the model
@pytest.fixture(scope="module")
def quoted():
    data = synth.csv_quoted(1 << 20, seed=3)
    return data, record_ends(data)[0]


def test_csv_quoted_is_deterministic_and_exact(quoted):
    data, _ = quoted
    assert len(data) == 1 << 20 and data[-1] == 10
    assert np.array_equal(data, synth.csv_quoted(1 << 20, seed=3))
    assert not np.array_equal(data, synth.csv_quoted(1 << 20, seed=4))
    assert len(synth.csv_quoted(12345, seed=1)) == 12345
    body = data.tobytes()
    assert b'""' in body and b'\n\n' in body and b'a, b' in body


def test_model_agrees_with_the_csv_module(quoted):
    data, ends = quoted
    text = data.tobytes().decode()
    rows = list(pycsv.reader(io.StringIO(text, newline="")))
    assert len(rows) == len(ends) and int(ends[-1]) == len(data) - 1
    assert len(ends) < int(np.count_nonzero(data == 10))               # some newlines are inside quoted fields
    assert {len(r) for r in rows} == {11}
    starts = np.concatenate([[0], ends[:-1].astype(np.int64) + 1])
    for i in range(3000):
        one = list(pycsv.reader(io.StringIO(text[int(starts[i]):int(ends[i]) + 1], newline="")))
        assert one == [rows[i]], i


def test_model_carry_flips_the_kept_set():
    d = np.frombuffer(b'a\n"b\nc"\n"\n', np.uint8)
    assert list(record_ends(d)[0]) == [1, 7]
    assert list(record_ends(d, carry=1)[0]) == [4, 9]
    assert list(record_ends(d, base=100)[0]) == [101, 107]
    assert record_ends(d)[1:] == (3, 4)


# ------------------------------------------------------------------------------------------------ strategies
def _mem(name):
    MemoryStore._named.pop(name, None)
    return {"endpoint_url": f"memory://{name}"}


def _co(data: bytes, key: str, cfg):
    co = CloudObject.from_s3(fcsv.CSV, f"s3://data/{key}", fetch=False, s3_config=cfg)
    try:
        co.storage.head_bucket(Bucket="data")
    except Exception:
        co.storage.create_bucket(Bucket="data")
    co.storage.put_object(Body=data, Bucket="data", Key=key)
    return CloudObject.from_s3(fcsv.CSV, f"s3://data/{key}", s3_config=cfg)


@pytest.fixture
def stub_scan(monkeypatch):
    """The GPU scans replaced by numpy over the object's bytes."""
    calls = []

    def _bytes(co, begin, end):
        raw = co.storage.get_object(Bucket=co.path.bucket, Key=co.path.key)["Body"].read()
        return np.frombuffer(raw, np.uint8)[begin:end]

    def line_index_object(co, begin=0, end=None, delim=10, max_devices=None, part_bytes=8 << 30, fmt="u64"):
        assert fmt == "u64"
        calls.append("lines")
        end = co.size if end is None else end
        return (begin + np.flatnonzero(_bytes(co, begin, end) == delim)).astype(np.uint64)

    def record_index_object(co, begin=0, end=None, quote=34, max_devices=None, part_bytes=8 << 30):
        calls.append("records")
        end = co.size if end is None else end
        return record_ends(_bytes(co, begin, end), base=begin, quote=quote)[0]

    monkeypatch.setattr(scan_objects, "line_index_object", line_index_object)
    monkeypatch.setattr(scan_objects, "record_index_object", record_index_object)
    return calls


def _check_slices(co, data: bytes, slices, n):
    ends = set((record_ends(np.frombuffer(data, np.uint8))[0] + np.uint64(1)).tolist())
    assert len(slices) == n
    assert b"".join(data[s.body[0]:s.body[1]] for s in slices) == data
    pos = 0
    head = (",".join(co.attributes.columns) + "\n").encode()
    for i, s in enumerate(slices):
        assert (s.range_0, s.range_1) == s.body and s.body[0] == pos and s.chunk_id == i and s.num_chunks == n
        pos = s.body[1]
        if s.body[1] > s.body[0]:
            assert s.body[1] in ends or s.body[1] == len(data)
        got = s.get_bytes()
        assert got == (head if s.body[0] != 0 else b"") + data[s.body[0]:s.body[1]]
    assert pos == len(data)


@pytest.mark.parametrize("n", [1, 2, 7, 64])
def test_record_strategies_cut_at_record_ends(stub_scan, n):
    data = synth.csv_quoted(200_000, seed=5).tobytes()
    co = _co(data, f"q{n}.csv", _mem(f"quote_cpu_{n}"))
    co.preprocess(extra_args={"quotechar": '"', "index_format": "u64"})
    assert stub_scan == ["lines", "records"]
    model = record_ends(np.frombuffer(data, np.uint8))[0]
    assert co.attributes.num_records == len(model) and co.attributes.quotechar == '"'
    assert co.attributes.record_index_key == f"q{n}.csv.records"
    raw = co.storage.get_object(Bucket=co.meta_path.bucket, Key=co.attributes.record_index_key)["Body"].read()
    assert np.array_equal(np.frombuffer(raw, "<u8"), model)
    slices = co.partition(fcsv.partition_records_num_chunks, num_chunks=n)
    _check_slices(co, data, slices, n)
    rows = sum(len(list(pycsv.reader(io.StringIO(s.get(), newline="")))) - (1 if s.body[0] else 0)
               for s in slices if s.body[1] > s.body[0])
    assert rows == len(model)
    cs = -(-len(data) // n)
    by_size = co.partition(fcsv.partition_records_chunk_size, chunk_size=cs)
    assert [s.body for s in by_size] == [s.body for s in slices]


def test_snap_definition():
    ends = np.array([4, 9, 10, 30], np.uint64)
    idx = _lines.LineIndex(ends)
    size = 40
    bounds = sorted({0, size} | {int(e) + 1 for e in ends})
    for x in range(0, size + 3):
        assert _lines.snap(idx, size, x) == min([b for b in bounds if b >= x], default=size), x
    assert _lines.snap(_lines.LineIndex(np.zeros(0, np.uint64)), 7, 3) == 7


def test_more_chunks_than_records_single_record_and_no_trailing_newline(stub_scan):
    few = b'a,b\n1,"x\ny"\n2,"z"\n'
    co = _co(few, "few.csv", _mem("quote_cpu_few"))
    co.preprocess(extra_args={"quotechar": '"', "index_format": "u64"})
    assert co.attributes.num_records == 3
    slices = co.partition(fcsv.partition_records_num_chunks, num_chunks=10)
    _check_slices(co, few, slices, 10)
    assert sum(1 for s in slices if s.body[1] > s.body[0]) <= 3
    assert any(s.body[0] == s.body[1] and s.get_bytes() in (b"", b"a,b\n") for s in slices)

    one = b'a,b\n'
    co = _co(one, "one.csv", _mem("quote_cpu_one"))
    co.preprocess(extra_args={"quotechar": '"', "index_format": "u64"})
    _check_slices(co, one, co.partition(fcsv.partition_records_num_chunks, num_chunks=3), 3)

    cut = b'a,b\n1,"x\ny"\n2,"last\nrow"'
    co = _co(cut, "cut.csv", _mem("quote_cpu_cut"))
    co.preprocess(extra_args={"quotechar": '"', "index_format": "u64"})
    assert co.attributes.num_records == 2
    slices = co.partition(fcsv.partition_records_num_chunks, num_chunks=4)
    _check_slices(co, cut, slices, 4)
    assert slices[-1].body[1] == len(cut)


def test_missing_record_index_is_a_key_error_and_default_preprocess_is_unchanged(stub_scan):
    data = synth.csv(50_000, seed=6).tobytes()
    co = _co(data, "plain.csv", _mem("quote_cpu_plain"))
    co.preprocess(extra_args={"index_format": "u64"})
    assert stub_scan == ["lines"]                                      # no record scan unless asked for
    keys = sorted(c["Key"] for c in co.storage.list_objects_v2(Bucket=co.meta_path.bucket)["Contents"])
    assert keys == ["plain.csv", "plain.csv.attrs", "plain.csv.lines"]
    attrs = pickle.loads(co.storage.get_object(Bucket=co.meta_path.bucket, Key="plain.csv.attrs")["Body"].read())
    assert sorted(attrs) == ["columns", "dtypes", "line_index_key", "num_lines"]
    assert attrs["num_lines"] == data.count(b"\n") and attrs["line_index_key"] == "plain.csv.lines"
    with pytest.raises(KeyError, match="quotechar"):
        co.partition(fcsv.partition_records_num_chunks, num_chunks=4)
    with pytest.raises(KeyError, match="quotechar"):
        co.partition(fcsv.partition_records_chunk_size, chunk_size=1000)
    with pytest.raises(ValueError):
        fcsv.preprocess_csv(co, line_index=False, quotechar="\n")


# ------------------------------------------------------------------------------------------------ record_index_object
def _note(c):
    """The fake device layer's launches as these tests read them: ("counts" | "ends", begin, end, carry, cap)."""
    return "counts" if c.form == "count" else "ends", c.begin, c.end, c.carry, c.cap


FakeDevices = functools.partial(_fake_scan.FakeDevices, note=_note)

CHAIN_BYTES, CHAIN_PART = (1 << 18) + 77, 1 << 14


@pytest.fixture(scope="module")
def chain_data():
    data = synth.csv_quoted(CHAIN_BYTES, seed=11)
    return data, record_ends(data)[0]


def _check_chain(fake, data, begin, end, got, min_parts=16, min_inside=3):
    """The result is the definition over [begin, end); every launch had the parity of the quotes before its part."""
    assert got.dtype == np.uint64 and np.array_equal(got, record_ends(data[begin:end], base=begin)[0])
    parts = scan_objects.line_parts(begin, end, 1, CHAIN_PART)
    inside = [int(np.count_nonzero(data[begin:lo] == 34)) & 1 for lo, _ in parts]
    assert len(parts) >= min_parts and sum(inside) >= min_inside
    counts = sorted(c[1:] for c in fake.calls if c[0] == "counts")
    assert counts == [(lo, hi, 0, 0) for lo, hi in parts]               # one count-only launch per part, carry 0
    emits = [c for c in fake.calls if c[0] == "ends"]
    first = {}
    for _, lo, hi, carry, cap in emits:
        assert carry == inside[parts.index((lo, hi))], (lo, carry)
        first.setdefault((lo, hi), cap)
    assert sorted(first) == parts
    for (lo, hi), cap in first.items():                  # sized by the count-only launch only where that is a bound
        n0 = len(record_ends(data[lo:hi])[0])
        assert cap == (max(n0, 1) if not inside[parts.index((lo, hi))] else (hi - lo) // 16 + 1024)
    assert len(emits) == len(parts) + sum(1 for (lo, hi), cap in first.items()
                                          if len(record_ends(data[lo:hi], carry=inside[parts.index((lo, hi))])[0]) > cap)


@pytest.mark.parametrize("devs", [[0], [0, 0, 0]])
def test_record_index_object_chains_the_parts(monkeypatch, chain_data, devs):
    data, model = chain_data
    fake = FakeDevices(monkeypatch, devs)
    co = _co(data.tobytes(), "chain.csv", _mem(f"quote_cpu_chain{len(devs)}"))
    got = scan_objects.record_index_object(co, part_bytes=CHAIN_PART)
    assert np.array_equal(got, model)
    assert scan_objects.line_parts(0, len(data), len(devs), CHAIN_PART) == scan_objects.line_parts(0, len(data), 1, CHAIN_PART)
    _check_chain(fake, data, 0, len(data), got)
    # a sub-range that starts at a record boundary (not at a part boundary of the whole object) and ends mid-record
    fake.calls.clear()
    begin, end = int(model[len(model) // 7]) + 1, len(data) - 1234
    assert begin % CHAIN_PART and data[end - 1] != 10
    _check_chain(fake, data, begin, end, scan_objects.record_index_object(co, begin, end, part_bytes=CHAIN_PART),
                 min_parts=12, min_inside=1)
    assert len(scan_objects.record_index_object(co, 500, 500)) == 0


def test_record_index_object_releases_the_waiting_parts_when_one_fails(monkeypatch, chain_data):
    data, model = chain_data
    fake = FakeDevices(monkeypatch, [0, 0, 0])
    co = _co(data.tobytes(), "fail.csv", _mem("quote_cpu_fail"))
    t0 = time.perf_counter()
    assert np.array_equal(scan_objects.record_index_object(co, part_bytes=CHAIN_PART), model)
    healthy = time.perf_counter() - t0
    parts = scan_objects.line_parts(0, len(data), 3, CHAIN_PART)
    result = {}

    def call():
        try:
            result["value"] = scan_objects.record_index_object(co, part_bytes=CHAIN_PART)
        except BaseException as e:
            result["error"] = e

    fake.fail_counts_at = parts[1][0]                    # part 1 never publishes its count: parts 2.. wait for it
    th = threading.Thread(target=call, daemon=True)
    th.start()
    # a guard against a hang, not a speed: the healthy call above takes tens of milliseconds here, a released waiter
    # notices the failure at its next 50 ms poll; 200 times the healthy run and at least 20 s leaves a loaded machine
    # two orders of magnitude, and a hang still fails the test instead of stalling the suite
    th.join(max(20.0, 200 * healthy))
    assert not th.is_alive(), "record_index_object hangs when a part fails"
    assert "value" not in result and isinstance(result["error"], RuntimeError)
    assert "fake: record_counts failed" in str(result["error"]), "the caller must see the cause, not a released waiter"
    fake.fail_counts_at = None
    scan_objects.release_workers()                       # the workers are idle again: this returns
    fake.calls.clear()
    assert np.array_equal(scan_objects.record_index_object(co, part_bytes=CHAIN_PART), model)
    _check_chain(fake, data, 0, len(data), model)
