"""The u16b record index without a GPU: the additive entry point of libdpquote.so's ABI, record_index_object's
multi-part merge of the parts' (low words, block table) over a numpy-backed fake of the device layer driven by the
definition (tests/_quote_model.py), the stored form's round trip through store_record_index / records_of over the
in-memory store, the record partition strategies on both stored forms, attributes written before the form existed,
and the refusal of other formats.  tests/test_gpu_quote_blocked.py runs the kernel."""
import ctypes
import functools
import threading

import numpy as np
import pytest

import _fake_scan
from _quote_model import record_ends
from dataplug_amd import synth
from dataplug_amd.cloudobject import CloudObject
from dataplug_amd.formats import _lines
from dataplug_amd.formats.generic import csv as fcsv
from dataplug_amd.scan import _quote
from dataplug_amd.scan import objects as scan_objects
from dataplug_amd.scan.objects import BlockedOffsets
from dataplug_amd.storage import MemoryStore

SIZE, PART = (1 << 20) + 77, 100_003


# ------------------------------------------------------------------------------------------------ ABI
def test_blocked_entry_point_is_exported_and_refuses_a_null_context():
    lib = _quote.load()
    assert "dq_records_blocked_async" in [n for n, _, _ in _quote.SIGNATURES]
    rc = lib.dq_records_blocked_async(None, None, 0, 0, 0, 0, 34, 0, None, 0, None, 0)
    assert rc == _quote.DQ_ERR_INVALID and b"ctx" in lib.dq_last_error()
    assert lib.dq_abi_version() == _quote.ABI_VERSION == 1
    assert ctypes.sizeof(ctypes.c_uint64) == 8


# ------------------------------------------------------------------------------------------------ the fake device layer
def _note(c):
    """The fake device layer's emitting launches as these tests read them: (form, begin, end, carry)."""
    return None if c.form == "count" or c.relaunch else (c.form, c.begin, c.end, c.carry)


FakeDevices = functools.partial(_fake_scan.FakeDevices, note=_note)


def _co(data: bytes, key: str, name: str):
    MemoryStore._named.pop(name, None)
    cfg = {"endpoint_url": f"memory://{name}"}
    co = CloudObject.from_s3(fcsv.CSV, f"s3://data/{key}", fetch=False, s3_config=cfg)
    co.storage.create_bucket(Bucket="data")
    co.storage.put_object(Body=data, Bucket="data", Key=key)
    return CloudObject.from_s3(fcsv.CSV, f"s3://data/{key}", s3_config=cfg)


@pytest.fixture(scope="module")
def quoted():
    data = synth.csv_quoted(SIZE, seed=17)
    return data, record_ends(data)[0]


# ------------------------------------------------------------------------------------------------ multi-part merge
@pytest.mark.parametrize("devs", [[0], [0, 0, 0]])
def test_record_index_object_merges_the_parts_tables(monkeypatch, quoted, devs):
    data, model = quoted
    fake = FakeDevices(monkeypatch, devs)
    co = _co(data.tobytes(), "merge.csv", f"quote_blocked_merge{len(devs)}")
    parts = scan_objects.line_parts(0, len(data), len(devs), PART)
    inside = [int(np.count_nonzero(data[:lo] == 34)) & 1 for lo, _ in parts]
    assert len(parts) >= 10 and sum(1 for lo, _ in parts if lo & 0xFFFF) >= 9 and sum(inside) >= 2
    got = scan_objects.record_index_object(co, part_bytes=PART, fmt="u16b")
    assert isinstance(got, BlockedOffsets) and got.low.dtype == np.uint16 and got.table.dtype == np.uint64
    assert got.j0 == 0 and len(got) == len(model) and len(got.table) == ((len(data) - 1) >> 16) + 1
    assert np.array_equal(got.to_u64(), model)
    assert np.array_equal(got.table, np.searchsorted(model, np.arange(len(got.table), dtype=np.uint64) << np.uint64(16)))
    assert sorted(c for c in fake.calls) == [("u16b", lo, hi, c) for (lo, hi), c in zip(parts, inside)]
    fake.calls.clear()
    u64 = scan_objects.record_index_object(co, part_bytes=PART, fmt="u64")
    assert u64.dtype == np.uint64 and np.array_equal(u64, model) and {c[0] for c in fake.calls} == {"u64"}
    assert np.array_equal(scan_objects.record_index_object(co, part_bytes=PART), model)       # the default is uint64

    # a sub-range that begins and ends off every boundary; one part; the empty range; another format
    begin, end = int(model[len(model) // 5]) + 1, len(data) - 4321
    sub = scan_objects.record_index_object(co, begin, end, part_bytes=PART, fmt="u16b")
    assert sub.j0 == begin >> 16 and begin & 0xFFFF and len(sub.table) == ((end - 1) >> 16) - (begin >> 16) + 1
    assert np.array_equal(sub.to_u64(), model[(model >= begin) & (model < end)]) and sub.table[0] == 0
    if len(devs) == 1:
        one = scan_objects.record_index_object(co, begin, end, fmt="u16b")
        assert np.array_equal(one.low, sub.low) and np.array_equal(one.table, sub.table) and one.j0 == sub.j0
    empty = scan_objects.record_index_object(co, 70_000, 70_000, fmt="u16b")
    ref = scan_objects.line_index_object(co, 70_000, 70_000, fmt="u16b")
    assert isinstance(empty, BlockedOffsets) and len(empty) == 0 and empty.j0 == ref.j0 == 1
    assert np.array_equal(empty.table, ref.table) and empty.low.dtype == ref.low.dtype
    for bad in ("u8s", "u32p", "auto", ""):
        with pytest.raises(ValueError):
            scan_objects.record_index_object(co, fmt=bad)


def test_a_failing_part_still_raises_its_own_error(monkeypatch, quoted):
    data, model = quoted
    fake = FakeDevices(monkeypatch, [0, 0, 0])
    co = _co(data.tobytes(), "fail.csv", "quote_blocked_fail")
    parts = scan_objects.line_parts(0, len(data), 3, PART)
    fake.fail_counts_at = parts[1][0]
    result = {}

    def call():
        try:
            result["value"] = scan_objects.record_index_object(co, part_bytes=PART, fmt="u16b")
        except BaseException as e:
            result["error"] = e

    th = threading.Thread(target=call, daemon=True)
    th.start()
    th.join(60.0)                                        # a guard against a hang: a released waiter leaves within 50 ms
    assert not th.is_alive(), "record_index_object hangs when a part fails"
    assert "value" not in result and "fake: record_counts failed" in str(result["error"])
    fake.fail_counts_at = None
    scan_objects.release_workers()
    assert np.array_equal(scan_objects.record_index_object(co, part_bytes=PART, fmt="u16b").to_u64(), model)


# ------------------------------------------------------------------------------------------------ storage, partitions
@pytest.fixture
def stub_scan(monkeypatch):
    """The GPU scans replaced by numpy over the object's bytes; the record index in the asked form."""
    calls = []

    def _bytes(co, begin, end):
        raw = co.storage.get_object(Bucket=co.path.bucket, Key=co.path.key)["Body"].read()
        return np.frombuffer(raw, np.uint8)[begin:end]

    def line_index_object(co, begin=0, end=None, delim=10, max_devices=None, part_bytes=8 << 30, fmt="u64"):
        end = co.size if end is None else end
        return (begin + np.flatnonzero(_bytes(co, begin, end) == delim)).astype(np.uint64)

    def record_index_object(co, begin=0, end=None, quote=34, max_devices=None, part_bytes=8 << 30, fmt="u64"):
        calls.append(fmt)
        end = co.size if end is None else end
        ends = record_ends(_bytes(co, begin, end), base=begin, quote=quote)[0]
        if fmt == "u64":
            return ends
        nt = ((end - 1) >> 16) - (begin >> 16) + 1
        bounds = np.arange(begin >> 16, (begin >> 16) + nt, dtype=np.uint64) << np.uint64(16)
        return BlockedOffsets((ends & np.uint64(0xFFFF)).astype(np.uint16),
                              np.searchsorted(ends, bounds).astype(np.uint64), begin >> 16)

    monkeypatch.setattr(scan_objects, "line_index_object", line_index_object)
    monkeypatch.setattr(scan_objects, "record_index_object", record_index_object)
    return calls


@pytest.fixture
def both_forms(stub_scan, quoted):
    data, model = quoted
    raw = data.tobytes()
    cos = {}
    for form in ("u64", "u16b"):
        co = _co(raw, f"{form}.csv", f"quote_blocked_store_{form}")
        co.preprocess(extra_args={"quotechar": '"', "index_format": "u64", "record_index_format": form})
        cos[form] = co
    assert stub_scan == ["u64", "u16b"]
    return raw, model, cos


def test_storage_round_trip(both_forms):
    raw, model, cos = both_forms
    a64, a16 = cos["u64"].attributes, cos["u16b"].attributes
    assert a16.record_index_dtype == "u16b" and a16.record_index_key == "u16b.csv.records"
    assert a16.record_index_blocks_key == "u16b.csv.records.blocks" and a16.record_index_block0 == 0
    assert a16.num_records == a64.num_records == len(model) and a16.quotechar == '"'
    assert getattr(a64, "record_index_dtype", None) is None and not hasattr(a64, "record_index_blocks_key")
    st = cos["u16b"].storage
    bucket = cos["u16b"].meta_path.bucket
    low = st.get_object(Bucket=bucket, Key=a16.record_index_key)["Body"].read()
    blocks = st.get_object(Bucket=bucket, Key=a16.record_index_blocks_key)["Body"].read()
    assert len(low) == 2 * len(model) and len(blocks) == 8 * (((len(raw) - 1) >> 16) + 1)
    assert np.array_equal(np.frombuffer(low, "<u2"), (model & np.uint64(0xFFFF)).astype(np.uint16))
    assert np.array_equal(BlockedOffsets(np.frombuffer(low, "<u2"), np.frombuffer(blocks, "<u8"), 0).to_u64(), model)
    stored64 = cos["u64"].storage.get_object(Bucket=cos["u64"].meta_path.bucket, Key=a64.record_index_key)["Body"].read()
    assert np.array_equal(np.frombuffer(stored64, "<u8"), model)               # the uint64 form as before

    r64, r16 = _lines.records_of(cos["u64"]), _lines.records_of(cos["u16b"])
    assert r16.count == r64.count == len(model)
    xs = np.unique(np.concatenate([model.astype(np.int64) - 1, model.astype(np.int64), model.astype(np.int64) + 1,
                                   [0, len(raw) - 1, len(raw), len(raw) + 5]]))
    xs = xs[xs >= 0]
    for x in xs.tolist():
        assert r16.nxt(x) == r64.nxt(x) and r16.contains(x) == r64.contains(x), x
    for i in (0, 1, len(model) // 2, len(model) - 1):
        assert r16.value(i) == r64.value(i) == int(model[i])


def test_storage_round_trip_read_block_by_block(both_forms, monkeypatch):
    """The same answers when the index is too large to preload (ranged GETs of entry blocks, decoded by the table)."""
    raw, model, cos = both_forms
    monkeypatch.setattr(_lines, "_PRELOAD_BYTES", 0)
    r64, r16 = _lines.records_of(cos["u64"]), _lines.records_of(cos["u16b"])
    assert r16._arr is None and r64._arr is None
    for x in (0, int(model[0]), int(model[0]) + 1, int(model[9000]) - 1, int(model[9000]), 70_000, 3 << 16,
              int(model[-1]), int(model[-1]) + 1):
        assert r16.nxt(x) == r64.nxt(x) and r16.contains(x) == r64.contains(x), x


def test_partitions_are_identical_from_both_forms(both_forms):
    raw, model, cos = both_forms
    ends = set((model + np.uint64(1)).tolist())
    for n in (1, 2, 7, 64):
        s64 = cos["u64"].partition(fcsv.partition_records_num_chunks, num_chunks=n)
        s16 = cos["u16b"].partition(fcsv.partition_records_num_chunks, num_chunks=n)
        assert [s.body for s in s16] == [s.body for s in s64] and len(s16) == n
        assert b"".join(raw[s.body[0]:s.body[1]] for s in s16) == raw
        assert all(s.body[1] in ends or s.body[1] == s.body[0] for s in s16)
        cs = -(-len(raw) // n)
        z64 = cos["u64"].partition(fcsv.partition_records_chunk_size, chunk_size=cs)
        z16 = cos["u16b"].partition(fcsv.partition_records_chunk_size, chunk_size=cs)
        assert [s.body for s in z16] == [s.body for s in z64] == [s.body for s in s64]
    assert s16[3].get_bytes() == s64[3].get_bytes()


def test_attributes_without_the_dtype_read_as_uint64(quoted):
    """An object preprocessed before the form existed: record_index_key, num_records, quotechar and nothing else."""
    data, model = quoted
    co = _co(data.tobytes(), "legacy.csv", "quote_blocked_legacy")
    key = "legacy.csv.records"
    co.storage.create_bucket(Bucket=co.meta_path.bucket)
    co.storage.put_object(Body=model.astype("<u8").tobytes(), Bucket=co.meta_path.bucket, Key=key)

    class Legacy:
        record_index_key = key
        num_records = len(model)
        quotechar = '"'

    class Obj:
        storage, meta_path, attributes = co.storage, co.meta_path, Legacy()

    r = _lines.records_of(Obj())
    assert r.count == len(model) and r._item == 8
    assert r.nxt(0) == int(model[0]) + 1 and r.contains(int(model[77])) and not r.contains(int(model[77]) + 1)
    # and store_record_index of a plain array writes exactly those attributes
    attrs = _lines.store_record_index(co, model, '"')
    assert attrs == {"record_index_key": key, "num_records": len(model), "quotechar": '"'}


def test_other_record_index_formats_are_refused(stub_scan, quoted):
    data, _ = quoted
    co = _co(data.tobytes(), "bad.csv", "quote_blocked_bad")
    for bad in ("u8s", "u32p", "auto"):
        with pytest.raises(ValueError, match="record_index_format"):
            co.preprocess(extra_args={"quotechar": '"', "index_format": "u64", "record_index_format": bad}, force=True)
        with pytest.raises(ValueError, match="record_index_format"):
            fcsv.preprocess_csv(co, line_index=False, quotechar='"', record_index_format=bad)
    assert stub_scan == []
