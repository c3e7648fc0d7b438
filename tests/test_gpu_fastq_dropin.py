"""co.preprocess() of an uncompressed FASTQ on the GPU: the stored .fqi and the attributes against the definition's
byte loop (tests/_fastq_loop.py), with the default parts and with 4 KiB parts on two device entries; both strategies
and fetch_reads against host walks; the error path; the sample offsets against the existing newline launch; and a
second preprocess on warm contexts, which allocates nothing."""
import numpy as np
import pytest

import _fastq_loop as L
from dataplug_amd import synth
from dataplug_amd.cloudobject import CloudObject
from dataplug_amd.formats.genomics import fastq as ffq
from dataplug_amd.scan import objects as scan_objects
from dataplug_amd.storage import MemoryStore

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def objs():
    out = {}
    for name, data in (("short", synth.fastq(20_000, seed=31).tobytes()),
                       ("long", synth.fastq_long(2_000, seed=32).tobytes())):
        out[name] = (data, L.loop_index(data, 64), L.read_ranges(data))
    return out


def _co(data, name):
    MemoryStore._named.pop(name, None)
    cfg = {"endpoint_url": f"memory://{name}"}
    co = CloudObject.from_s3(ffq.FASTQ, "s3://data/r.fastq", fetch=False, s3_config=cfg)
    co.storage.create_bucket(Bucket="data")
    co.storage.put_object(Body=data, Bucket="data", Key="r.fastq")
    return CloudObject.from_s3(ffq.FASTQ, "s3://data/r.fastq", s3_config=cfg)


def stored(co):
    found = co.storage.list_objects_v2(Bucket=co.meta_path.bucket).get("Contents", [])
    return {o["Key"]: co.storage.get_object(Bucket=co.meta_path.bucket, Key=o["Key"])["Body"].read() for o in found}


def check_stored(co, want):
    pairs, r, b, mn, mx = want
    assert stored(co)["r.fastq.fqi"] == L.index_bytes(pairs)
    a = co.attributes
    assert (a.reads_index_key, a.reads_index_every, a.num_reads, a.num_bases, a.min_read_len, a.max_read_len) == \
        ("r.fastq.fqi", 64, r, b, mn, mx)


@pytest.mark.parametrize("name", ["short", "long"])
@pytest.mark.parametrize("route", ["memory", "joblib"])
def test_preprocess_stores_the_loops_bytes(objs, name, route):
    data, want, rr = objs[name]
    co = _co(data, f"gpu_fq_{name}_{route}")
    co.preprocess(parallel_config={"backend": "threading"} if route == "joblib" else None,
                  extra_args={"dataplug_devices": [0, 0]})
    check_stored(co, want)
    pairs, r, b = want[0], want[1], want[2]
    for strategy in (ffq.partition_reads_strategy, ffq.partition_bases_strategy):
        sl = co.partition(strategy, num_chunks=7)
        assert sl[0].range_0 == 0 and sl[-1].range_1 == len(data) and sum(s.num_reads for s in sl) == r
        assert all(a.range_1 == c.range_0 for a, c in zip(sl, sl[1:])) and sum(s.num_bases for s in sl) == b
        for s in sl:                                                     # a host walk over the reads of the slice
            assert (s.range_0, s.range_1) == (rr[s.first_read][0], rr[s.first_read + s.num_reads - 1][1])
        assert sl[3].get().encode() == data[sl[3].range_0:sl[3].range_1]
    for f, c in ((0, 1), (63, 2), (64, 64), (r - 65, 65), (r - 1, 1), (1000, 3)):
        assert ffq.fetch_reads(co, f, c) == data[rr[f][0]:rr[f + c - 1][1]], (f, c)
    with pytest.raises(IndexError):
        ffq.fetch_reads(co, r, 1)
    # the existing newline launch: sample j > 0 lies right behind the (4 j K)-th '\n', entry j K - 1 of every fourth
    every4, _ = scan_objects.record_index_bytes(data, every_k=4, emit_add=1)
    assert [p[0] for p in pairs[1:-1]] == [int(every4[64 * j - 1]) for j in range(1, len(pairs) - 1)]


@pytest.mark.parametrize("name", ["short", "long"])
def test_small_parts_on_two_entries(objs, name):
    data, want, rr = objs[name]
    co = _co(data, f"gpu_fq_parts_{name}")
    setattr(co, scan_objects.DEVICES_ATTR, [0, 0])
    idx = scan_objects.reads_index_object(co, 64, part_bytes=4096)
    assert len(scan_objects.line_parts(0, len(data), 2, 4096)) > 1000
    pairs = [tuple(map(int, p)) for p in idx.samples.tolist()]
    assert (pairs, idx.num_reads, idx.num_bases, idx.min_read_len, idx.max_read_len) == want


@pytest.mark.parametrize("how", ["bad_header", "bad_separator", "length_mismatch", "truncated"])
def test_a_malformed_read_raises_and_stores_nothing(objs, how):
    data, want, rr = objs["short"]
    ln = L.lines_of(data[rr[12_345][0]:rr[12_345][1]])
    s = rr[12_345][0]
    if how == "truncated":
        bad = data[:rr[-1][0] + 30]
    elif how == "length_mismatch":
        bad = data[:s + ln[1][1] - 1] + data[s + ln[1][1]:]
    else:
        p = s + ln[0 if how == "bad_header" else 2][0]
        bad = data[:p] + b"x" + data[p + 1:]
    with pytest.raises(L.LoopError) as le:
        L.loop_index(bad, 64)
    assert le.value.kind == how and le.value.read == (len(rr) - 1 if how == "truncated" else 12_345)
    co = _co(bad, f"gpu_fq_bad_{how}")
    with pytest.raises(ffq.FastqFormatError) as e:
        co.preprocess(extra_args={"dataplug_devices": [0, 0]})
    assert (e.value.kind, e.value.read, e.value.offset) == (le.value.kind, le.value.read, le.value.offset)
    assert stored(co) == {}


def test_a_second_preprocess_on_warm_contexts_allocates_nothing(objs):
    from dataplug_amd.scan._lib import alloc_counts
    data, want, _ = objs["long"]
    counts = []
    for k in range(3):
        co = _co(data, f"gpu_fq_warm{k}")
        co.preprocess(extra_args={"dataplug_devices": [0, 0]})
        check_stored(co, want)
        counts.append(alloc_counts())
    assert counts[1] == counts[0] and counts[2] == counts[1]     # the first one here is the warm-up
