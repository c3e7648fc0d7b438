"""The quote-aware record index through the object layer on the GPU: record_index_object over parts that start inside
quoted fields, co.preprocess(extra_args={"quotechar": '"'}) and the record partition strategies over the in-memory
store, and the plain newline path on the same object, unchanged."""
import csv as pycsv
import io

import numpy as np
import pytest

from _quote_model import record_ends
from dataplug_amd import synth
from dataplug_amd.cloudobject import CloudObject
from dataplug_amd.formats.generic import csv as fcsv
from dataplug_amd.scan import objects as so
from dataplug_amd.storage import MemoryStore

pytestmark = pytest.mark.gpu

SIZE = (8 << 20) + 4321
PART = 1 << 19


@pytest.fixture(scope="module")
def quoted():
    data = synth.csv_quoted(SIZE, seed=11)
    return data, record_ends(data)[0]


def _co(data: bytes, key: str, name: str):
    MemoryStore._named.pop(name, None)
    cfg = {"endpoint_url": f"memory://{name}"}
    co = CloudObject.from_s3(fcsv.CSV, f"s3://data/{key}", fetch=False, s3_config=cfg)
    co.storage.create_bucket(Bucket="data")
    co.storage.put_object(Body=data, Bucket="data", Key=key)
    return CloudObject.from_s3(fcsv.CSV, f"s3://data/{key}", s3_config=cfg)


@pytest.mark.parametrize("devices", ["0", "0,0,0"])
def test_record_index_object_over_parts_inside_quotes(monkeypatch, quoted, devices):
    data, model = quoted
    monkeypatch.setenv("DATAPLUG_AMD_DEVICES", devices)
    ndev = len(devices.split(","))
    parts = so.line_parts(0, len(data), ndev, PART)
    before = np.concatenate([[0], np.cumsum(data == 34)])
    inside = sum(int(before[lo]) & 1 for lo, _ in parts)
    assert len(parts) >= 16 and inside >= 3, "the parts must start inside quoted fields for this to test the chaining"
    co = _co(data.tobytes(), "parts.csv", f"gpu_quote_parts_{ndev}")
    got = so.record_index_object(co, part_bytes=PART)
    assert got.dtype == np.uint64 and np.array_equal(got, model)
    assert np.array_equal(so.record_index_object(co), model)                       # one part per device entry
    lo, hi = int(model[10]) + 1, int(model[-10]) + 1                               # a sub-range starting at a record
    assert np.array_equal(so.record_index_object(co, begin=lo, end=hi, part_bytes=PART),
                          model[(model >= lo) & (model < hi)])


def test_preprocess_with_quotechar_and_record_partitions(quoted):
    data, model = quoted
    raw = data.tobytes()
    co = _co(raw, "q.csv", "gpu_quote_dropin")
    co.preprocess(extra_args={"quotechar": '"'})
    at = co.attributes
    assert at.num_records == len(model) and at.quotechar == '"' and at.record_index_key == "q.csv.records"
    stored = co.storage.get_object(Bucket=co.meta_path.bucket, Key=at.record_index_key)["Body"].read()
    assert np.array_equal(np.frombuffer(stored, "<u8"), model)
    assert len(at.columns) == 11 and at.columns[-1] == "Note"
    ends = set((model + np.uint64(1)).tolist())
    for n in (1, 3, 8, 50):
        slices = co.partition(fcsv.partition_records_num_chunks, num_chunks=n)
        assert len(slices) == n
        assert b"".join(raw[s.body[0]:s.body[1]] for s in slices) == raw
        rows = 0
        for s in slices:
            assert s.body[1] in ends or s.body[1] == s.body[0]
            if s.body[1] == s.body[0]:
                continue
            parsed = list(pycsv.reader(io.StringIO(s.get(), newline="")))
            assert parsed[0] == at.columns and {len(r) for r in parsed} == {11}
            rows += len(parsed) - 1
            df = s.get_as_pandas()
            assert len(df) == len(parsed) - 1 and list(df.columns) == at.columns
        assert rows == at.num_records - 1
    by_size = co.partition(fcsv.partition_records_chunk_size, chunk_size=-(-len(raw) // 8))
    assert [s.body for s in by_size] == [s.body for s in co.partition(fcsv.partition_records_num_chunks, num_chunks=8)]


def test_plain_newline_path_is_unchanged(quoted):
    """On an object preprocessed with quotechar, the newline index and partition_num_chunks give what they gave
    before the record index existed: every '\\n', and the reference's slices (oracle/cpu_ref.csv_slice_get)."""
    from dataplug_amd.formats._lines import LineIndex
    from oracle import cpu_ref
    data, _ = quoted
    raw = data.tobytes()
    co = _co(raw, "p.csv", "gpu_quote_plain")
    co.preprocess(extra_args={"quotechar": '"'})
    li = LineIndex.of(co)
    assert np.array_equal(li._fetch(0, li.count), np.flatnonzero(data == 10))
    assert co.attributes.num_lines == int(np.count_nonzero(data == 10))
    assert co.attributes.line_index_dtype == so.line_index_form(co, 0, co.size)
    for n in (4, 25):
        for s in co.partition(fcsv.partition_num_chunks, num_chunks=n):
            assert s.get() == cpu_ref.csv_slice_get(raw, co.attributes.columns, s.range_0, s.range_1, s.chunk_id, n)
