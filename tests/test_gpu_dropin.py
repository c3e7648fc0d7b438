"""co.preprocess() drop-in through the HIP path (libdpscan) against the reference's outputs.

FASTA: the sample and the golden fuzz cases (reference-generated), synthetic objects at several chunk
sizes (oracle), the per-chunk joblib route, multi-group splits (DATAPLUG_AMD_DEVICES=0,0,... runs the
multi-GPU grouping on one GPU), and a header line crossing a group boundary (pending-end resolution).
CSV/VCF: the GPU newline index equals the bytes' '\\n' positions and the partitions equal the reference's
get() outputs.  FASTQ.gz: total_lines and per-read ends on the inflated stream, read batches' lines."""
import base64
import gzip
import io
import builtins
import json
import os

import numpy as np
import pytest

from dataplug_amd import synth
from dataplug_amd.cloudobject import CloudObject
from dataplug_amd.entities import get_slices
from dataplug_amd.storage import LoopbackS3Server, MemoryStore

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def server():
    with LoopbackS3Server() as srv:
        yield srv


def _co(fmt, data: bytes, key: str, cfg):
    co = CloudObject.from_s3(fmt, f"s3://data/{key}", fetch=False, s3_config=cfg)
    try:
        co.storage.head_bucket(Bucket="data")
    except Exception:
        co.storage.create_bucket(Bucket="data")
    co.storage.put_object(Body=data, Bucket="data", Key=key)
    return CloudObject.from_s3(fmt, f"s3://data/{key}", s3_config=cfg)


def _index(co):
    return np.frombuffer(co.storage.get_object(Bucket=co.meta_path.bucket, Key=co.meta_path.key)["Body"].read(),
                         np.uint32)


def _lines_u64(co):
    """The stored newline index (index_format "auto": u8s, uint8 low bytes + 256-byte counts + 64 KiB block table, or
    u16b for objects with fewer than one newline per 128 bytes) as uint64 offsets."""
    from dataplug_amd.formats._lines import LineIndex
    from dataplug_amd.scan.objects import line_index_form
    begin = int(getattr(co.attributes, "body_offset", 0) or 0)
    assert co.attributes.line_index_dtype == line_index_form(co, begin, co.size)
    li = LineIndex.of(co)
    return li._fetch(0, li.count)


def _mem(name):
    MemoryStore._named.pop(name, None)
    return {"endpoint_url": f"memory://{name}"}


# ------------------------------------------------------------------------------------------------ FASTA
@pytest.mark.parametrize("parallel_config", [{}, {"backend": "threading", "n_jobs": 4}])
def test_fasta_sample_over_loopback(server, fasta_cases, parallel_config):
    from dataplug_amd.formats.genomics.fasta import FASTA, partition_chunks_strategy
    z = fasta_cases
    i = list(z["kind"]).index("sample")
    data = bytes(z["data"][z["data_off"][i]:z["data_off"][i + 1]])
    co = _co(FASTA, data, f"sample{len(parallel_config)}.fasta", server.storage_config)
    co.preprocess(parallel_config=parallel_config, chunk_size=-(-len(data) // 4))
    assert co.attributes.num_sequences == 9
    assert _index(co).reshape(-1, 2).tolist() == [[0, 60], [236, 296], [473, 533], [709, 769], [946, 1006],
                                                  [1183, 1249], [1426, 1486], [1663, 1721], [1898, 1958]]
    g = [r for r in json.load(open(os.path.join(GOLDEN, "fasta_slices.json"))) if r["object"] == "sample"]
    for rec in g:
        sl = co.partition(partition_chunks_strategy, num_chunks=rec["num_chunks"])
        assert [[s.offset, None if s.header is None else list(s.header), s.range_0, s.range_1] for s in sl] == \
            rec["slices"]
        if "get" in rec:          # the reference's get() outputs, materialized by the batched get_slices
            assert [base64.b64encode(b).decode() for b in get_slices(sl)] == rec["get"]


def test_fasta_golden_cases_batch_and_per_chunk(fasta_cases):
    from dataplug_amd.formats.genomics.fasta import FASTA
    z = fasta_cases
    cfg = _mem("gpu_golden")
    for i in range(0, len(z["chunk_size"]), 7):
        data = bytes(z["data"][z["data_off"][i]:z["data_off"][i + 1]])
        exp = z["expected"][z["expected_off"][i]:z["expected_off"][i + 1]]
        cs = int(z["chunk_size"][i])
        for pc in ({}, {"backend": "sequential"}):
            co = _co(FASTA, data, f"g{i}_{len(pc)}", cfg)
            co.preprocess(parallel_config=pc, chunk_size=cs)
            assert np.array_equal(_index(co), exp), (i, str(z["kind"][i]), cs, pc)
            assert co.attributes.num_sequences == int(z["num_sequences"][i])


@pytest.mark.parametrize("devices", ["0", "0,0", "0,0,0,0,0,0,0,0"])
@pytest.mark.parametrize("div", [1, 4, 9, 64])
def test_fasta_synthetic_groups(monkeypatch, devices, div):
    from oracle import cpu_ref, dpref
    from dataplug_amd.formats.genomics.fasta import FASTA
    monkeypatch.setenv("DATAPLUG_AMD_DEVICES", devices)
    data = synth.fasta(16 << 20, 7 + div)
    cs = -(-len(data) // div)
    co = _co(FASTA, data.tobytes(), f"syn{div}", _mem(f"gpu_syn_{div}_{len(devices)}"))
    co.preprocess(chunk_size=cs)
    exp = dpref.fasta_pairs(data, cpu_ref.chunk_plan(len(data), cs))
    assert np.array_equal(_index(co), exp.reshape(-1).astype(np.uint32))


@pytest.mark.parametrize("devices,div,budget", [("0", 64, 3 << 20), ("0,0,0", 9, 5 << 20), ("0", 1000, 1 << 20)])
def test_fasta_launch_budget_passes(monkeypatch, devices, div, budget):
    """A launch byte budget far below a GPU's group (DATAPLUG_AMD_MAX_LAUNCH_BYTES): each group is scanned
    in several passes of whole chunks; the index still equals the reference's."""
    from oracle import cpu_ref, dpref
    from dataplug_amd.formats.genomics.fasta import FASTA
    monkeypatch.setenv("DATAPLUG_AMD_DEVICES", devices)
    monkeypatch.setenv("DATAPLUG_AMD_MAX_LAUNCH_BYTES", str(budget))
    data = synth.fasta(24 << 20, 70 + div)
    cs = -(-len(data) // div)
    co = _co(FASTA, data.tobytes(), f"bud{div}", _mem(f"gpu_bud_{div}_{len(devices)}"))
    co.preprocess(chunk_size=cs)
    exp = dpref.fasta_pairs(data, cpu_ref.chunk_plan(len(data), cs))
    assert np.array_equal(_index(co), exp.reshape(-1).astype(np.uint32))


@pytest.mark.parametrize("part", [None, (1 << 20) + 13])
@pytest.mark.parametrize("where", ["memory", "loopback"])
def test_fasta_pipelined_fetch_many_parts(server, monkeypatch, part, where):
    """storage -> pinned -> HBM pipeline (objects.fetch_to_device): many ranged-GET parts (ragged last part)
    whose H2D copies are issued as they land, out of order; the index equals the oracle's."""
    from oracle import cpu_ref, dpref
    from dataplug_amd.formats.genomics.fasta import FASTA
    from dataplug_amd.scan import objects
    monkeypatch.setenv("DATAPLUG_AMD_DEVICES", "0")
    if part:
        monkeypatch.setattr(objects, "_GET_PART", part)
    n = (100 << 20) + 4099 if part is None else (16 << 20) + 777
    data = synth.fasta(n, 31)
    cfg = _mem(f"gpu_pipe_{part}") if where == "memory" else server.storage_config
    co = _co(FASTA, data.tobytes(), f"pipe_{part}_{where}", cfg)
    cs = -(-n // 4)
    co.preprocess(chunk_size=cs, force=True)
    exp = dpref.fasta_pairs(data, cpu_ref.chunk_plan(n, cs))
    assert np.array_equal(_index(co), exp.reshape(-1).astype(np.uint32))


def test_fasta_header_crossing_group_boundary(monkeypatch):
    """A header line opened near the end of group 0's last chunk whose '\\n' lies far inside group 1's
    region: group 0's buffer has no newline after it -> pending -> dp_find_delim on later bytes."""
    from oracle import cpu_ref, dpref
    from dataplug_amd.formats.genomics.fasta import FASTA
    monkeypatch.setenv("DATAPLUG_AMD_DEVICES", "0,0")
    n, cs = 1 << 20, 1 << 18                     # 4 chunks -> groups [0,2) [2,4); boundary at 2*cs
    a = np.full(n, ord("A"), np.uint8)
    a[::61] = 10
    a[2 * cs - 300: 2 * cs + 200_000] = ord("x")  # one very long header line across the boundary
    a[2 * cs - 300] = ord(">")
    a[2 * cs - 301] = 10
    a[-1] = 10
    co = _co(FASTA, a.tobytes(), "cross", _mem("gpu_cross"))
    co.preprocess(chunk_size=cs)
    exp = dpref.fasta_pairs(a, cpu_ref.chunk_plan(n, cs))
    got = _index(co).reshape(-1, 2)
    assert np.array_equal(got, exp.astype(np.uint32))
    assert any(e > 2 * cs + 100_000 for _, e in got.tolist())


def test_fasta_quirk_every_chunk_to_eof():
    """chunk_size == num_chunks - 1: every map job reads to EOF, headers repeat (handler.py:36-38)."""
    from oracle import cpu_ref, dpref
    from dataplug_amd.formats.genomics.fasta import FASTA
    cs = 200
    data = synth.fasta(cs * (cs + 1) + 5, 3)
    assert len(data) // cs == cs + 1
    co = _co(FASTA, data.tobytes(), "quirk", _mem("gpu_quirk"))
    co.preprocess(chunk_size=cs)
    exp = dpref.fasta_pairs(data, cpu_ref.chunk_plan(len(data), cs))
    assert len(exp) > 200 * 3
    assert np.array_equal(_index(co), exp.reshape(-1).astype(np.uint32))


# ------------------------------------------------------------------------------------------------ CSV / VCF
def _ref_error(name):
    """The exception class the golden recorded for the reference's get(): a builtin, or the storage
    ClientError (a ranged GET past the end of the object, InvalidRange on S3)."""
    from dataplug_amd.storage.errors import ClientError
    return {"ClientError": ClientError}.get(name) or getattr(builtins, name)


@pytest.mark.parametrize("devices", ["0", "0,0,0"])
def test_csv_line_index_and_partitions(monkeypatch, devices):
    from dataplug_amd.formats.generic import csv as fcsv
    from dataplug_amd.formats._lines import SliceError
    monkeypatch.setenv("DATAPLUG_AMD_DEVICES", devices)
    g = json.load(open(os.path.join(GOLDEN, "csv_slices.json")))["objects"]
    for rec in g:
        data = {"synth_csv": lambda: bytes(synth.csv(1 << 16, 5)), "wide_csv": lambda: bytes(synth.csv_wide(1 << 16, 5))}.get(
            rec["object"], lambda: rec["num_chunks"]["1"][0][2].encode())()
        co = _co(fcsv.CSV, data, rec["object"] + devices, _mem(f"gpu_csv_{rec['object']}_{len(devices)}"))
        co.preprocess()
        assert co.attributes.columns == rec["columns"]
        lines = _lines_u64(co)
        assert np.array_equal(lines, np.flatnonzero(np.frombuffer(data, np.uint8) == 10))
        for n, expected in rec["num_chunks"].items():
            for s, e in zip(co.partition(fcsv.partition_num_chunks, num_chunks=int(n)), expected):
                if isinstance(e[2], dict):
                    with pytest.raises(_ref_error(e[2]["error"])) as ei:   # the reference's class
                        s.get()
                    assert isinstance(ei.value, SliceError)
                else:
                    assert s.get() == e[2]


def test_csv_large_multi_part(monkeypatch):
    from dataplug_amd.formats.generic import csv as fcsv
    monkeypatch.setenv("DATAPLUG_AMD_DEVICES", "0,0,0,0")
    data = synth.csv(96 << 20, 9)
    co = _co(fcsv.CSV, data.tobytes(), "big.csv", _mem("gpu_csv_big"))
    co.preprocess()
    lines = _lines_u64(co)
    assert np.array_equal(lines, np.flatnonzero(data == 10))
    from oracle import cpu_ref
    obj = data.tobytes()
    for s in co.partition(fcsv.partition_num_chunks, num_chunks=25):
        assert s.get() == cpu_ref.csv_slice_get(obj, co.attributes.columns, s.range_0, s.range_1, s.chunk_id, 25)


@pytest.mark.parametrize("devices,fmt", [("0", "u8s"), ("0,0,0", "u8s"), ("0,0", "u16b")])
def test_csv_streamed_index(monkeypatch, devices, fmt):
    """verdict r5 #4: the index stored while later pieces are fetched and scanned (pieces of 7 MiB + 3, each device
    entry's pieces in order on its worker with the next piece's fetch under the previous piece's scan, multipart PUTs
    of 5 MiB parts) is byte-identical to the merged index stored at once, and decodes to every newline of the
    object."""
    from dataplug_amd.formats import _lines
    from dataplug_amd.scan import objects
    from dataplug_amd.formats.generic import csv as fcsv
    monkeypatch.setenv("DATAPLUG_AMD_DEVICES", devices)
    monkeypatch.setattr(_lines, "PART_MIN", 5 << 20)
    data = synth.csv(200 << 20, 13)
    co = _co(fcsv.CSV, data.tobytes(), "streamed.csv", _mem(f"gpu_csv_streamed_{len(devices)}_{fmt}"))
    co2 = _co(fcsv.CSV, b"x", "whole.csv", _mem(f"gpu_csv_whole_{len(devices)}_{fmt}"))
    for c in (co, co2):
        c.storage.create_bucket(Bucket=c.meta_path.bucket)
    a = _lines.index_object(co, 0, fmt, piece_bytes=(7 << 20) + 3)
    whole = objects.line_index_object(co, fmt=fmt)
    b = _lines.store_line_index(co2, whole)
    assert a["num_lines"] == b["num_lines"] == int((data == 10).sum())
    for attr in ("line_index_key", "line_index_blocks_key") + (("line_index_sub_key",) if fmt == "u8s" else ()):
        x = co.storage.get_object(Bucket=co.meta_path.bucket, Key=a[attr])["Body"].read()
        assert x == co2.storage.get_object(Bucket=co2.meta_path.bucket, Key=b[attr])["Body"].read(), attr
    co.preprocess()                                   # the plugin's own call (auto form, one piece at this size)
    assert np.array_equal(_lines_u64(co), np.flatnonzero(data == 10))


def test_streamed_index_dense_pieces(monkeypatch):
    """A piece denser than one newline per 16 bytes (every byte a newline in the middle of the object) overflows the
    streamed launch's first output capacity and is scanned again, sized, before the next piece goes on."""
    from dataplug_amd.formats import _lines
    from dataplug_amd.formats.generic import csv as fcsv
    monkeypatch.setenv("DATAPLUG_AMD_DEVICES", "0")
    monkeypatch.setattr(_lines, "PART_MIN", 5 << 20)
    data = synth.csv(24 << 20, 17)
    data[9 << 20:12 << 20] = 10
    co = _co(fcsv.CSV, data.tobytes(), "dense.csv", _mem("gpu_csv_dense_stream"))
    co.storage.create_bucket(Bucket=co.meta_path.bucket)
    a = _lines.index_object(co, 0, "u8s", piece_bytes=(5 << 20) + 1)
    assert a["num_lines"] == int((data == 10).sum())
    from dataplug_amd.formats._lines import LineIndex
    blocks = np.frombuffer(co.storage.get_object(Bucket=co.meta_path.bucket, Key=a["line_index_blocks_key"])["Body"].read(), "<u8")
    li = LineIndex(storage=co.storage, bucket=co.meta_path.bucket, key=a["line_index_key"], count=a["num_lines"],
                   blocks=blocks, block0=a["line_index_block0"], sub_key=a["line_index_sub_key"],
                   sub0=a["line_index_sub0"])
    assert np.array_equal(li._fetch(0, li.count), np.flatnonzero(data == 10))


@pytest.mark.parametrize("name", ["synth_vcf", "wide_vcf"])
def test_vcf_line_index_and_partitions(monkeypatch, name):
    """Golden VCF slices, incl. rows longer than the padding (the reference's range-expansion path)."""
    from dataplug_amd.formats.genomics import vcf as fvcf
    monkeypatch.setenv("DATAPLUG_AMD_DEVICES", "0,0")
    g = json.load(open(os.path.join(GOLDEN, "vcf_slices.json")))["objects"]
    rec = [r for r in g if r["object"] == name][0]
    data = bytes(synth.vcf(1 << 16, 6) if name == "synth_vcf" else synth.vcf_wide(1 << 16, 6))
    co = _co(fvcf.VCF, data, name + ".vcf", _mem("gpu_" + name))
    co.preprocess()
    assert co.attributes.body_offset == rec["body_offset"] and co.attributes.columns == rec["columns"]
    meta = co.storage.get_object(Bucket=co.meta_path.bucket, Key=co.meta_path.key)["Body"].read().decode()
    assert meta == rec["meta"]
    for n, expected in rec["num_chunks"].items():
        assert [s.get() for s in co.partition(fvcf.partition_num_chunks, num_chunks=int(n))] == \
            [e[2] for e in expected]


# ------------------------------------------------------------------------------------------------ FASTQ.gz
@pytest.mark.parametrize("kind,piece", [("multi", 64 << 20), ("multi", 200_003), ("bgzf", 300_007), ("bgzf", 64 << 20)])
def test_fastq_gz_reads(kind, piece):
    """FASTQ.gz preprocess through the streamed pipeline on the GPU (scan/gzindex.py): pieces of ``piece``
    inflated bytes, so read ends straddle piece boundaries (and gzip member boundaries: two members of
    different levels, or BGZF's 64 KiB members inflated on a thread pool); every read end equals the
    reads' own line ends and the reference's read batches yield every line in order."""
    from dataplug_amd.formats.genomics.fastq import FASTQGZip, load_read_index, partition_reads_batches
    raw = synth.fastq(20_000, seed=4).tobytes()
    if kind == "multi":
        blob = gzip.compress(raw[:1_000_003], 6) + gzip.compress(raw[1_000_003:], 1)     # two members
    else:
        blob = synth.bgzf(raw)
    co = _co(FASTQGZip, blob, f"r_{kind}_{piece}.fastq.gz", _mem(f"gpu_fastq_{kind}_{piece}"))
    co.preprocess(extra_args={"span": 1 << 16, "piece_bytes": piece})
    assert co.attributes.gzip_members == (2 if kind == "multi" else -(-len(raw) // 65280) + 1)
    lines = raw.split(b"\n")[:-1]
    assert co.attributes.total_lines == len(lines) == 80_000
    ends = load_read_index(co)
    nl = np.flatnonzero(np.frombuffer(raw, np.uint8) == 10)
    assert np.array_equal(ends, nl[3::4] + 1)
    batches = co.partition(partition_reads_batches, num_batches=7)
    got = [ln for b in batches for ln in b.get()]
    assert got == [x.decode() for x in lines]


@pytest.mark.parametrize("threads,region", [(16, 1 << 16), (6, 1 << 18)])
def test_fastq_gz_parallel_inflate_on_gpu(threads, region):
    """One ~14 MB gzip member inflated by the parallel engine with small speculative regions (many batches,
    hundreds of region starts) streamed through the GPU newline scan in 1 MB pieces: every read end equals
    the reads' own line ends, the access points and their windows equal the zlib stream index's."""
    from dataplug_amd import gz as gzlib
    from dataplug_amd.scan import get_context
    from dataplug_amd.scan import gzindex
    raw = synth.fastq(60_000, seed=9).tobytes()
    blob = gzip.compress(raw, 6)
    f = io.BytesIO(blob)
    ix = gzindex.index_stream(get_context(0), lambda n: f.read(n), record_lines=4, span=1 << 18,
                              piece_bytes=1_000_003, threads=threads, region_bytes=region)
    nl = np.flatnonzero(np.frombuffer(raw, np.uint8) == 10).astype(np.uint64)
    assert np.array_equal(np.frombuffer(ix.ends.read(), "<u8"), nl[3::4] + np.uint64(1))
    assert ix.newlines == len(nl) and ix.uncompressed_size == len(raw) and ix.members == 1
    _, pts = gzlib.build_index(blob, span=1 << 18)
    assert [r[1] for r in ix.rows] == pts["in_byte"].tolist()
    assert [r[2] for r in ix.rows] == pts["out_byte"].tolist()
    assert [r[6] for r in ix.rows] == pts["bits"].tolist()
    windows = ix.windows.read()
    for r in ix.rows:
        if not r[7]:
            assert windows[r[5]:r[5] + r[4]] == raw[max(0, r[2] - 32768):r[2]]


# ------------------------------------------------------------------------------------------ multi-GPU split
def test_bench_thread_mode_split_on_one_gpu(tmp_path):
    """bench.py --gpus 4 --devices 0,0,0,0: the multi-GPU line's own code (one host thread per GPU, one
    configs[1]-shaped object per worker; the strong point cuts ONE object's 4-chunk plan over the 4 workers
    by the product split, per-group halo) rehearsed on one GPU; every launch is bit-exact against the oracle
    (verified_bit_exact) in both."""
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, os.path.join(repo, "bench.py"), "--full", "--gpus", "4", "--devices", "0,0,0,0",
           "--size", str((48 << 20) + 4096), "--csv-size", str((40 << 20) + 77), "--vcf-size", str((96 << 20) + 5),
           "--steps", "3", "--warmup", "1", "--no-cpu-baseline"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=repo)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["n_gpus"] == 4 and line["verified_bit_exact"] is True
    assert line["config"]["chunks"] == 4 and line["config"]["objects"] == 4
    assert line["config"]["index_dtype"] == "uint32"
    assert line["strong"]["verified_bit_exact"] is True and line["strong"]["gpus_used"] == 4
    assert line["strong"]["chunks"] == 4 and line["strong"]["pieces"] == 4
    assert line["ms_per_step"] * 1e3 >= line["roofline"]["kernel_avg_us"]
    # workers share the GPU: no calibration ratio is reported (it would mix the workers' kernels)
    assert line["roofline"]["measured_peak"] is None and line["roofline"]["frac_of_measured_peak"] is None
    for leg in ("csv", "vcf"):
        sub = line[leg]
        assert "error" not in sub, sub
        assert sub["n_gpus"] == 4 and sub["verified_every_offset"] is True and len(sub["per_gpu"]) == 4
        assert sub["roofline"]["frac"] > 0 and sub["roofline"]["measured_mixed_ref"] is None
    assert line["vcf"]["scaling"] == "strong" and line["csv"]["scaling"] == "weak"
    assert line["peak_rss_gib"] > 0


def test_bench_default_line_carries_the_newline_legs():
    """The driver's command (bench.py, N = 1) at small sizes: ONE line whose headline is the FASTA leg and whose
    csv / vcf sub-objects (BASELINE configs[2] / [3]) carry value, roofline (measured read ceiling and mixed
    reference, behind a barrier), cpu_baseline with the cgroup-derived pool, and every offset verified."""
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, os.path.join(repo, "bench.py"), "--full", "--size", str((64 << 20) + 12), "--csv-size",
           str((72 << 20) + 3), "--vcf-size", str((80 << 20) + 9), "--steps", "3", "--warmup", "1",
           "--e2e-fasta-size", str((48 << 20) + 5), "--e2e-csv-size", str((40 << 20) + 7), "--fastq-tiles", "2"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=repo)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [x for x in r.stdout.splitlines() if x.strip()]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["verified_bit_exact"] is True and line["roofline"]["measured_peak"] > 0
    assert line["cpu_baseline"]["host"]["pool_processes"] == line["cpu_baseline"]["cores"]
    for leg in ("csv", "vcf"):
        sub = line[leg]
        assert "error" not in sub, sub
        assert sub["verified_every_offset"] is True and sub["value"] > 0 and sub["ms_per_step"] > 0
        rf = sub["roofline"]
        assert rf["frac"] > 0 and rf["measured_peak"] > 0 and rf["measured_mixed_ref"] > 0
        assert sub["cpu_baseline"]["value"] > 0 and sub["cpu_baseline"]["cores"] >= 1
        assert rf["kernel"].startswith("line_kernel<DELIM>")         # the default newline form
    # the end-to-end sub-objects (host memory to host memory, every stored index read back and checked)
    e2e = line["e2e"]
    assert "error" not in e2e, e2e
    for kind in ("fasta", "csv"):
        for src in ("memory", "loopback_http"):
            assert e2e[kind][src]["verified"] is True and e2e[kind][src]["value"] > 0, (kind, src, e2e[kind])
        assert e2e[kind]["stages"]["h2d_GiB_per_s"] > 0 and e2e[kind]["stages"]["index_bytes"] > 0
    assert e2e["fits_in_driver_run"] is True
    fq = line["fastq"]
    assert "error" not in fq, fq
    assert fq["verified_every_read_end"] is True and fq["reads"] == 2 * 65536 and fq["gzip_members"] == 1
    assert fq["fits_in_driver_run"] is True
    assert line["bench_wall_s"] > 0


def test_bench_plain_run_is_the_headline_alone_and_dumps_its_outputs(tmp_path):
    """bench.py without --full: the K pipelined steps of the headline leg and nothing else in the line; with
    --dump-outputs the last step's index lands as float64 .npy files and equals the oracle's pairs."""
    import subprocess
    import sys
    from oracle import cpu_ref, dpref
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    size = (24 << 20) + 12
    cmd = [sys.executable, os.path.join(repo, "bench.py"), "--gpus", "1", "--size", str(size), "--steps", "3",
           "--warmup", "1", "--dump-outputs", str(tmp_path / "out")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120, cwd=repo)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [x for x in r.stdout.splitlines() if x.strip()]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["full"] is False and line["steps"] == 3 and line["warmup"] == 1
    assert line["unit"] == "GiB/s" and line["higher_is_better"] is True and line["dtype"] == "u8"
    assert line["value"] > 0 and line["ms_per_step"] > 0
    # value is the object's bytes per timed step; ms_per_step is rounded to 1e-4 ms of a step of 0.01 ms or more
    assert line["value"] == pytest.approx(size / (line["ms_per_step"] / 1e3) / (1 << 30), rel=0.01)
    for moved in ("csv", "vcf", "e2e", "fastq", "cpu_baseline", "roofline", "serialized", "strong"):
        assert moved not in line, moved
    plan = cpu_ref.chunk_plan(size, size // 4)                # bench.py's plan: chunk_size = size / 4, seed 1
    exp = dpref.fasta_pairs(synth.TiledFasta(size, seed=1).bytes_range(0, size), plan)
    got = {f[:-4]: np.load(tmp_path / "out" / f) for f in os.listdir(tmp_path / "out")}
    assert sorted(got) == ["chunk_ends", "count", "pairs", "pending"]
    assert all(a.dtype == np.float64 for a in got.values())
    assert np.array_equal(got["pairs"], exp.astype(np.float64)) and got["count"].tolist() == [len(exp)]
    assert (got["pending"] == -1).all() and len(got["chunk_ends"]) == len(plan) == 4


@pytest.mark.parametrize("workload", ["fasta", "vcf"])
def test_bench_under_torch_distributed_run(workload):
    """The driver's N > 1 launch (python -m torch.distributed.run --nproc-per-node N bench.py --gpus N),
    rehearsed with two ranks on one GPU (--devices 0,0), started as a fresh child before any GPU call in it:
    ONE JSON line from rank 0 with both ranks' results, every launch exact, and no calibration ratio (the
    ranks share the GPU)."""
    import socket
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with socket.socket() as s_:
        s_.bind(("127.0.0.1", 0))
        port = s_.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
           "127.0.0.1", "--master-port", str(port), os.path.join(repo, "bench.py"), "--full", "--gpus", "2",
           "--devices", "0,0", "--workload", workload, "--fasta-size", str(256 << 20), "--legs", "fasta,vcf",
           "--vcf-size", str((200 << 20) + 1),
           "--steps", "3", "--warmup", "1", "--no-cpu-baseline"]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="4")
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=repo, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [x for x in r.stdout.splitlines() if x.strip().startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    line = json.loads(lines[0])
    fasta = line if workload == "fasta" else line["fasta"]
    vcf = line if workload == "vcf" else line["vcf"]
    assert "error" not in fasta and "error" not in vcf
    assert fasta["n_gpus"] == 2 and len(fasta["per_gpu"]) == 2 and fasta["verified_bit_exact"] is True
    assert fasta["strong"]["verified_bit_exact"] is True and fasta["strong"]["gpus_used"] == 2
    assert vcf["n_gpus"] == 2 and len(vcf["per_gpu"]) == 2 and vcf["verified_every_offset"] is True
    assert fasta["roofline"]["frac_of_measured_peak"] is None and vcf["roofline"]["frac_of_measured_peak"] is None


def test_bench_refuses_more_gpus_than_visible():
    import subprocess
    import sys
    from dataplug_amd.scan import device_count
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    n = device_count() + 1
    r = subprocess.run([sys.executable, os.path.join(repo, "bench.py"), "--gpus", str(n), "--steps", "1"],
                       capture_output=True, text=True, timeout=120, cwd=repo)
    assert r.returncode != 0 and "visible" in r.stderr


@pytest.mark.parametrize("u64", [False, True])
def test_device_keyword_and_uint64_index(u64):
    """parallel_config={"dataplug_devices": [0, 0, 0]} runs the three-group split on the GPU box; with
    extra_args={"index_dtype": "uint64"} the stored index is the same pairs as 8-byte words."""
    from oracle import cpu_ref, dpref
    from dataplug_amd.formats.genomics.fasta import FASTA, partition_chunks_strategy
    from dataplug_amd.entities import get_slices
    data = synth.fasta((20 << 20) + 123, 55)
    co = _co(FASTA, data.tobytes(), f"devkw{u64}", _mem(f"gpu_devkw_{u64}"))
    cs = -(-len(data) // 9)
    co.preprocess(chunk_size=cs, parallel_config={"dataplug_devices": [0, 0, 0]},
                  extra_args={"index_dtype": "uint64"} if u64 else None)
    exp = dpref.fasta_pairs(data, cpu_ref.chunk_plan(len(data), cs))
    raw = co.storage.get_object(Bucket=co.meta_path.bucket, Key=co.meta_path.key)["Body"].read()
    got = np.frombuffer(raw, "<u8" if u64 else "<u4").reshape(-1, 2)
    assert np.array_equal(got.astype(np.uint64), exp)
    assert getattr(co.attributes, "index_dtype", "uint32") == ("uint64" if u64 else "uint32")
    slices = co.partition(partition_chunks_strategy, num_chunks=7)
    assert get_slices(slices) == [s.get() for s in slices]
