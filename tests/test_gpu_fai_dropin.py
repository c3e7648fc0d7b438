"""co.preprocess(extra_args={"fai": True}) through the HIP path (libdpscan's header index, libdpfai's counts) on the
memory store, against the definition's byte loop (tests/_fai_loop.py)."""
import pickle

import numpy as np
import pytest

from _fai_loop import loop_fai, loop_text
from dataplug_amd import synth
from dataplug_amd.cloudobject import CloudObject
from dataplug_amd.formats.genomics import fasta as ffasta
from dataplug_amd.scan.fai import FaiFormatError
from dataplug_amd.storage import MemoryStore

pytestmark = pytest.mark.gpu
FAI = {"fai": True, "dataplug_devices": [0, 0]}
# (chunk sizes below are len // k: the map plan has size // chunk_size chunks, and a rounded-up chunk size would leave
# the last quarter of the object without header pairs)


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


def _stored(co, key):
    return co.storage.get_object(Bucket=co.meta_path.bucket, Key=key)["Body"].read()


def _keys(co):
    return sorted(c["Key"] for c in co.storage.list_objects_v2(Bucket=co.meta_path.bucket)["Contents"])


def _pairs(co):
    return ffasta.load_index(co).astype(np.uint64)


def dewrapped(data, pairs):
    seqs = []
    for i, (s, e) in enumerate(pairs):
        end = int(pairs[i + 1][0]) if i + 1 < len(pairs) else len(data)
        seqs.append(data[int(e):end].replace(b"\n", b"").replace(b"\r", b""))
    return seqs


@pytest.fixture(scope="module")
def big():
    """synth.fasta((8 << 20) + 777) preprocessed on the batch route, and the loop's text over the stored pairs."""
    data = synth.fasta((8 << 20) + 777, seed=9).tobytes()
    co = _co(data, "big.fa", _mem("gpu_fai_big"))
    co.preprocess(extra_args=FAI, chunk_size=len(data) // 4)
    pairs = _pairs(co)
    return data, co, pairs, loop_text(loop_fai(data, pairs))


def test_stored_text_equals_the_loops(big):
    data, co, pairs, want = big
    assert _keys(co) == ["big.fa", "big.fa.attrs", "big.fa.fai"]
    assert _stored(co, "big.fa.fai") == want
    assert co.attributes.fai_key == "big.fa.fai" and co.attributes.num_sequences == len(pairs)
    assert co.attributes.num_bases == sum(map(len, dewrapped(data, pairs)))


def test_joblib_route_stores_the_same(big):
    data, co, pairs, want = big
    cj = _co(data, "big.fa", _mem("gpu_fai_big_joblib"))
    cj.preprocess(parallel_config={"backend": "threading", "n_jobs": 4}, extra_args=FAI,
                  chunk_size=len(data) // 4)
    assert _keys(cj) == _keys(co)
    for key in _keys(co):
        assert _stored(cj, key) == _stored(co, key), key


def test_crlf_copy_of_a_small_object():
    data = synth.fasta((256 << 10) + 33, seed=3).tobytes().replace(b"\n", b"\r\n")
    for route, pc in (("batch", {}), ("joblib", {"backend": "sequential"})):
        co = _co(data, "crlf.fa", _mem(f"gpu_fai_crlf_{route}"))
        co.preprocess(parallel_config=pc, extra_args=FAI, chunk_size=len(data) // 3)
        rows = loop_fai(data, _pairs(co))
        assert _stored(co, "crlf.fa.fai") == loop_text(rows), route
        assert rows[0][3] == 60 and rows[0][4] == 62 and b" " not in rows[0][0]


def test_without_fai_the_stored_keys_and_attributes_are_todays(big):
    data, co, pairs, _ = big
    cp = _co(data, "big.fa", _mem("gpu_fai_plain"))
    cp.preprocess(extra_args={"dataplug_devices": [0, 0]}, chunk_size=len(data) // 4)
    assert _keys(cp) == ["big.fa", "big.fa.attrs"]
    assert pickle.loads(_stored(cp, "big.fa.attrs")) == {"num_sequences": len(pairs)}
    assert _stored(cp, "big.fa") == _stored(co, "big.fa")
    with pytest.raises(KeyError):
        ffasta.load_fai(cp)


def test_an_irregular_object_raises_and_keeps_its_header_index():
    good = synth.fasta((128 << 10) + 5, seed=4).tobytes()
    cg = _co(good, "good.fa", _mem("gpu_fai_good"))
    cg.preprocess(extra_args=FAI, chunk_size=len(good) // 2)
    pairs = _pairs(cg)
    e = int(pairs[5][1])
    bad = good[:e] + b"ACGTACGTAC\nACG\n" + good[e:]          # a short line, then the sequence's full lines
    cb = _co(bad, "bad.fa", _mem("gpu_fai_bad"))
    with pytest.raises(FaiFormatError) as ei:
        cb.preprocess(extra_args=FAI, chunk_size=len(bad) // 2)
    assert ei.value.ordinal == 5 and ei.value.name == b"seq5"
    assert _keys(cb) == ["bad.fa", "bad.fa.attrs"]
    assert pickle.loads(_stored(cb, "bad.fa.attrs")) == {"num_sequences": len(pairs)}
    shifted = pairs.copy()
    shifted[6:] += 15
    assert np.array_equal(np.frombuffer(_stored(cb, "bad.fa"), np.uint32).reshape(-1, 2), shifted)
    with pytest.raises(FaiFormatError) as want:
        loop_fai(bad, shifted)
    assert (want.value.ordinal, want.value.name) == (5, b"seq5")


def test_fetch_region_and_base_partitions_agree_with_python_slicing(big):
    data, co, pairs, _ = big
    names, rows = ffasta.load_fai(co)
    seqs = dewrapped(data, pairs)
    rng = np.random.default_rng(1)
    for i in rng.integers(0, len(seqs), 25):
        n = len(seqs[i])
        a = int(rng.integers(0, n + 1))
        b = int(rng.integers(a, n + 1))
        assert ffasta.fetch_region(co, names[i], a, b) == seqs[i][a:b], (i, a, b)
    allb = b"".join(seqs)
    cum = np.concatenate([[0], np.cumsum([len(s) for s in seqs])])
    for k in (3, 8):
        slices = co.partition(ffasta.partition_bases_strategy, num_chunks=k)
        share = len(allb) // k
        assert len(slices) == k and slices[0].range_0 == 0 and slices[-1].range_1 == len(data)
        for j, s in enumerate(slices):
            g0, g1 = j * share, len(allb) if j == k - 1 else (j + 1) * share
            lines = s.get().split(b"\n")
            assert b"".join(ln for ln in lines if not ln.startswith(b">")) == allb[g0:g1], (k, j)
            i = int(np.searchsorted(cum, g0, "right")) - 1
            if g0 == cum[i]:
                assert s.header is None and s.offset == 0
            else:
                assert s.header == (int(pairs[i][0]), int(pairs[i][1])) and s.offset == g0 - cum[i]
