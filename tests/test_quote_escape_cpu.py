"""The escape-aware record index without a GPU: the additive entry points of libdpquote.so's ABI, record_index_object
over a numpy-backed fake of the device layer whose scans are the byte loop (tests/_escape_loop.py) -- parts cut inside
an escape run, right after an odd run and inside a quoted field, the chain fed by toggles, today's calls when no escape
is given -- and preprocess / partition over the in-memory store with the scan stubbed by the loop."""
import csv as pycsv
import functools
import io

import numpy as np
import pytest

import _fake_scan
from _escape_loop import blocked, loop_record_ends
from _quote_model import record_ends
from dataplug_amd import synth
from dataplug_amd.cloudobject import CloudObject
from dataplug_amd.formats.generic import csv as fcsv
from dataplug_amd.scan import _quote
from dataplug_amd.scan import objects as scan_objects
from dataplug_amd.scan.objects import BlockedOffsets
from dataplug_amd.storage import MemoryStore


# ------------------------------------------------------------------------------------------------ ABI
def test_escape_entry_points_are_exported_and_refuse_a_null_context():
    lib = _quote.load()
    names = [n for n, _, _ in _quote.SIGNATURES]
    for n in ("dq_records_esc_async", "dq_records_esc_blocked_async", "dq_records_esc_result"):
        assert n in names
    assert lib.dq_records_esc_async(None, None, 0, 0, 0, 0, 34, 0, 92, 0, 0, None, 1, 0) == _quote.DQ_ERR_INVALID
    assert b"ctx" in lib.dq_last_error()
    assert lib.dq_records_esc_blocked_async(None, None, 0, 0, 0, 0, 34, 0, 92, 0, 0, None, 0, None, 0) == \
        _quote.DQ_ERR_INVALID
    assert lib.dq_records_esc_result(None, None, None, None, None) == _quote.DQ_ERR_INVALID
    assert lib.dq_abi_version() == _quote.ABI_VERSION == 1
    assert _quote.escape_flags("all") == 0 and _quote.escape_flags("quoted") == _quote.DQ_ESC_SCOPE_QUOTED
    with pytest.raises(ValueError):
        _quote.escape_flags("some")
    with pytest.raises(_quote.DPEscapeRunError):
        _quote.check(_quote.DQ_ERR_ESCAPE_RUN)


def test_stamp_lists_six_instantiations_without_scratch():
    import json
    from dataplug_amd import build as B
    with open(B.stamp_path(B.QUOTE_OUT)) as f:
        rep = json.load(f)
    assert len(rep["kernels"]) == 6 and rep["scratch"] == []
    assert {k.split("<")[0] for k in rep["kernels"]} == {"quote_kernel"}


# ------------------------------------------------------------------------------------------------ the fake device layer
def _note(c):
    """The fake device layer's launches as these tests read them: ("counts" | form, begin, end, carry) of a plain
    launch, (.. + "_esc", begin, end, carry, esc_carry, scope) of an escaped one."""
    if c.relaunch:
        return None
    name = "counts" if c.form == "count" else c.form
    return (name, c.begin, c.end, c.carry) if c.escape is None else \
        (name + "_esc", c.begin, c.end, c.carry, c.esc_carry, c.scope)


FakeDevices = functools.partial(_fake_scan.FakeDevices, note=_note)


def _co(data: bytes, key: str, name: str):
    MemoryStore._named.pop(name, None)
    cfg = {"endpoint_url": f"memory://{name}"}
    co = CloudObject.from_s3(fcsv.CSV, f"s3://data/{key}", fetch=False, s3_config=cfg)
    co.storage.create_bucket(Bucket="data")
    co.storage.put_object(Body=data, Bucket="data", Key=key)
    return CloudObject.from_s3(fcsv.CSV, f"s3://data/{key}", s3_config=cfg)


PART = 1000


def cut_object():
    """3 parts of 1000 bytes (line_parts cuts at 1000 and 2000): the first cut lies inside a run of 5 escape bytes
    (3 before it, so the byte at 1000 is escaped: an escape byte; the run's last byte escapes the quote behind it),
    the second right after a run of 1 inside a quoted field (the byte at 2000, a quote, is escaped)."""
    d = np.full(3000, ord("a"), np.uint8)
    d[99::100] = 10
    d[10], d[150] = 34, 34                               # a quoted field over a line break
    d[300:302] = (92, 34)                                # an escaped quote: the parity of quote BYTES is off from here
    d[997:1002] = 92
    d[1002] = 34                                         # escaped by the fifth escape byte
    d[1500] = 34                                         # opens a field ...
    d[1999], d[2000] = 92, 34                            # ... in which \" stands across the cut
    d[2450] = 34                                         # ... and which closes here
    return d


@pytest.mark.parametrize("devs", [[0], [0, 0, 0]])
@pytest.mark.parametrize("fmt", ["u64", "u16b"])
@pytest.mark.parametrize("scope", ["all", "quoted"])
def test_record_index_object_chains_escaped_parts(monkeypatch, devs, fmt, scope):
    d = cut_object()
    fake = FakeDevices(monkeypatch, devs)
    co = _co(d.tobytes(), "cut.csv", f"quote_escape_cut{len(devs)}{fmt}{scope}")
    parts = scan_objects.line_parts(0, len(d), len(devs), PART)
    assert parts == [(0, 1000), (1000, 2000), (2000, 3000)]
    want, toggles, _, _ = loop_record_ends(d, scope=scope)
    got = scan_objects.record_index_object(co, escape=92, escape_scope=scope, part_bytes=PART, fmt=fmt)
    got = got.to_u64() if isinstance(got, BlockedOffsets) else got
    assert np.array_equal(got, want)
    assert not np.array_equal(want, record_ends(d)[0])   # the parity of quote bytes gives another index
    # what each part was entered with: esc_carry read from the object, carry chained from the toggles
    emits = sorted(c[1:] for c in fake.calls if c[0] == f"{fmt}_esc")
    counts = sorted(c[1:] for c in fake.calls if c[0] == "counts_esc")
    t = [loop_record_ends(d, 0, hi, scope=scope)[1] for _, hi in parts]
    assert emits == [(0, 1000, 0, 0, scope), (1000, 2000, t[0] & 1, 1, scope), (2000, 3000, t[1] & 1, 1, scope)]
    assert counts == [(0, 1000, 0, 0, scope), (1000, 2000, 0, 1, scope), (2000, 3000, 0, 1, scope)]
    assert t[1] & 1 == 1                                 # the third part starts inside a quoted field
    nq = [int(np.count_nonzero(d[:hi] == 34)) & 1 for _, hi in parts]
    assert (nq[0], nq[1]) != (t[0] & 1, t[1] & 1)        # chaining quote bytes would have been wrong
    assert not [c for c in fake.calls if c[0] in ("counts", "u64", "u16b")]


def test_escape_carry_at_walks_back_only_as_far_as_the_run(monkeypatch):
    d = np.full(5000, ord("a"), np.uint8)
    d[1000:3000] = 92
    co = _co(d.tobytes(), "walk.csv", "quote_escape_walk")
    gets = []
    real = co.storage.get_object

    def get_object(**kw):
        gets.append(kw["Range"])
        return real(**kw)
    monkeypatch.setattr(co.storage, "get_object", get_object)
    assert scan_objects.escape_carry_at(co, 0, 500, 92) == 0 and gets == ["bytes=436-499"]
    assert scan_objects.escape_carry_at(co, 0, 1001, 92) == 1
    assert scan_objects.escape_carry_at(co, 0, 3000, 92) == 0          # 2000 escape bytes
    assert scan_objects.escape_carry_at(co, 1001, 3000, 92) == 1       # the scan starts inside the run: 1999
    assert scan_objects.escape_carry_at(co, 0, 2999, 92) == 1
    assert scan_objects.escape_carry_at(co, 7, 7, 92) == 0
    big = np.full(_quote.DQ_ESCAPE_RUN_MAX + 4096, 92, np.uint8)
    co2 = _co(big.tobytes(), "big.csv", "quote_escape_walk_big")
    with pytest.raises(_quote.DPEscapeRunError):
        scan_objects.escape_carry_at(co2, 0, len(big), 92)


@pytest.mark.parametrize("fmt", ["u64", "u16b"])
def test_without_an_escape_the_device_layer_sees_todays_calls(monkeypatch, fmt):
    d = synth.csv_quoted(3000, seed=2)
    fake = FakeDevices(monkeypatch, [0])
    co = _co(d.tobytes(), "plain.csv", f"quote_escape_plain{fmt}")
    got = scan_objects.record_index_object(co, part_bytes=PART, fmt=fmt)
    got = got.to_u64() if isinstance(got, BlockedOffsets) else got
    assert np.array_equal(got, record_ends(d)[0])
    assert sorted({c[0] for c in fake.calls}) == ["counts", fmt]
    assert [c[1:3] for c in fake.calls if c[0] == fmt] == [(0, 1000), (1000, 2000), (2000, 3000)]


def test_record_index_object_refuses_bad_escapes():
    co = _co(b"a\n", "bad.csv", "quote_escape_bad")
    for kw in (dict(escape=34), dict(escape=10), dict(escape=300), dict(escape=92, escape_scope="some")):
        with pytest.raises(ValueError):
            scan_objects.record_index_object(co, **kw)


# ------------------------------------------------------------------------------------------------ preprocess, partition
@pytest.fixture
def stub_scan(monkeypatch):
    """The GPU scans replaced by the byte loop over the object's bytes; records every call's keywords."""
    calls = []

    def _bytes(co, begin, end):
        return np.frombuffer(co.storage.get_object(Bucket=co.path.bucket, Key=co.path.key,
                                                   Range=f"bytes={begin}-{end - 1}")["Body"].read(), np.uint8)

    def line_index_object(co, begin=0, end=None, delim=10, max_devices=None, part_bytes=8 << 30, fmt="u64"):
        end = co.size if end is None else end
        return (begin + np.flatnonzero(_bytes(co, begin, end) == delim)).astype(np.uint64)

    def record_index_object(co, begin=0, end=None, quote=34, **kw):
        calls.append(dict(kw))
        end = co.size if end is None else end
        d = _bytes(co, begin, end)
        if "escape" in kw:
            ends = loop_record_ends(d, begin, end, quote, kw["escape"], scope=kw["escape_scope"], base=begin)[0]
        else:
            ends = record_ends(d, base=begin, quote=quote)[0]
        if kw.get("fmt") == "u16b":
            low, table = blocked(ends, begin, end)
            return BlockedOffsets(low, table, begin >> 16)
        return ends

    monkeypatch.setattr(scan_objects, "line_index_object", line_index_object)
    monkeypatch.setattr(scan_objects, "record_index_object", record_index_object)
    return calls


@pytest.mark.parametrize("fmt", ["u64", "u16b"])
@pytest.mark.parametrize("scope", ["all", "quoted"])
def test_preprocess_stores_the_dialect_and_slices_hold_whole_rows(stub_scan, fmt, scope):
    d = synth.csv_escaped(300_000, seed=5)
    raw = d.tobytes()
    whole = list(pycsv.reader(io.StringIO(raw.decode(), newline=""), escapechar="\\", doublequote=False))
    co = _co(raw, "esc.csv", f"quote_escape_pre{fmt}{scope}")
    co.preprocess(extra_args={"quotechar": '"', "escapechar": "\\", "escape_scope": scope,
                              "record_index_format": fmt})
    want_kw = {"escape": 92, "escape_scope": scope}
    if fmt == "u16b":
        want_kw["fmt"] = "u16b"
    assert stub_scan == [want_kw]
    at = co.attributes
    assert (at.escapechar, at.escape_scope, at.quotechar) == ("\\", scope, '"')
    assert at.num_records == len(whole) and at.columns[-1] == "Note" and len(at.columns) == 11
    for n in (1, 5, 33):
        slices = co.partition(fcsv.partition_records_num_chunks, num_chunks=n)
        assert b"".join(raw[s.body[0]:s.body[1]] for s in slices) == raw
        rows = []
        for s in slices:
            if s.body[1] == s.body[0]:
                continue
            df = s.get_as_pandas()
            assert list(df.columns) == at.columns        # whole rows of 11 fields, or pandas raises / shifts columns
            parsed = list(pycsv.reader(io.StringIO(s.get(), newline=""), escapechar="\\", doublequote=False))
            assert len(df) == len(parsed) - 1 and {len(r) for r in parsed} == {11}
            rows += parsed[1:]
        assert rows == whole[1:]


def test_preprocess_without_escapechar_is_unchanged(stub_scan):
    d = synth.csv_quoted(200_000, seed=6)
    co = _co(d.tobytes(), "q.csv", "quote_escape_pre_plain")
    co.preprocess(extra_args={"quotechar": '"'})
    assert stub_scan == [{}]
    at = co.attributes
    assert getattr(at, "escapechar", None) is None and getattr(at, "escape_scope", None) is None
    s = co.partition(fcsv.partition_records_num_chunks, num_chunks=3)[1]
    assert list(s.get_as_pandas().columns) == at.columns


def test_header_sample_counts_unescaped_quotes_only():
    assert fcsv._open_quotes(['a,"x \\" y'], '"', "\\") == 1       # the field is still open
    assert fcsv._open_quotes(['a,"x \\" y"'], '"', "\\") == 0
    assert fcsv._open_quotes(['a,"x \\\\"'], '"', "\\") == 0       # an escaped escape byte, then the closing quote
    assert fcsv._open_quotes(['a,"x \\" y'], '"', None) == 0       # today's rule: the parity of the quote characters


@pytest.mark.parametrize("args", [
    {"escapechar": "\\"},                                          # needs quotechar
    {"quotechar": '"', "escapechar": '"'},
    {"quotechar": '"', "escapechar": "\n"},
    {"quotechar": '"', "escapechar": "ab"},
    {"quotechar": '"', "escapechar": "é"},
    {"quotechar": '"', "escapechar": "\\", "escape_scope": "fields"},
    {"quotechar": '"', "escape_scope": "fields"},
])
def test_preprocess_refuses_bad_dialects(stub_scan, args):
    co = _co(synth.csv_escaped(5000, seed=1).tobytes(), "r.csv", "quote_escape_refuse")
    with pytest.raises(ValueError):
        co.preprocess(extra_args=args)
    assert stub_scan == []


def test_csv_escaped_is_exact_deterministic_and_ends_at_a_record_end():
    a, b = synth.csv_escaped(100_001, seed=4), synth.csv_escaped(100_001, seed=4)
    assert len(a) == 100_001 and np.array_equal(a, b) and a[-1] == 10
    assert not np.array_equal(a, synth.csv_escaped(100_001, seed=5))
    ends, _, esc, inside = loop_record_ends(a)
    assert (esc, inside) == (0, 0) and int(ends[-1]) == len(a) - 1
    assert b'\\"' in a.tobytes() and b'\\\\"\n' in a.tobytes()       # an escaped backslash right before a closing quote
    rows = list(pycsv.reader(io.StringIO(a.tobytes().decode(), newline=""), escapechar="\\", doublequote=False))
    assert len(rows) == len(ends) and {len(r) for r in rows} == {11}
    with pytest.raises(ValueError):
        synth.csv_escaped(100)
