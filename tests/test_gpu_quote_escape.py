"""The escape-aware instantiations of libdpquote.so's record-end kernel (quote_kernel<.., 1>) on the GPU, through the
C ABI and ScanContext: offsets, counts and toggles equal to the byte loop (tests/_escape_loop.py) and to the lane
model (tools/emulate_quote.py) in the uint32, uint64 and u16b forms -- every escape byte value at every chunk
position, escape runs across every chunk / row / wave / tile edge, an all-escape tile, esc_carry at every alignment,
8 MiB of random bytes and of synth.csv_escaped, the multi-part chain, bit-parity with the plain launch when the escape
byte does not occur, the argument checks and the over-bound run's status."""
import os
import sys
import time

import numpy as np
import pytest

import _escape_cases as C
from _escape_loop import blocked, loop_record_ends
from dataplug_amd import synth
from dataplug_amd.cloudobject import CloudObject
from dataplug_amd.formats.generic import csv as fcsv
from dataplug_amd.scan import DPScanError, _quote
from dataplug_amd.scan.objects import BlockedOffsets, record_index_object
from dataplug_amd.storage import MemoryStore

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import emulate_quote as emu  # noqa: E402

pytestmark = pytest.mark.gpu

T = emu.TILE_BYTES


def place(ctx, c, name="quote_esc_in"):
    d = ctx.workspace(name, len(c["buf"]) + 64)
    assert d.ptr % 16 == 0
    addr = d.ptr + c["base"] % 16
    ctx.h2d(addr, c["buf"])
    return addr


def launch(ctx, c, addr, form):
    """One escaped launch of a case: (out..., n_out, n_quotes, n_newlines, 0, toggles), shaped like C.model's."""
    a = (addr, len(c["buf"]), c["base"], c["begin"], c["end"])
    kw = dict(quote=c["quote"], carry=c["carry"], escape=c["escape"], esc_carry=c["esc_carry"], scope=c["scope"])
    out, table, nq, nn, tog, _ = ctx.records(*a, form=form, **kw)
    if form == "u16b":
        return out, table, len(out), nq, nn, 0, tog
    return out, len(out), nq, nn, 0, tog


def check(ctx, c, exp=None, forms=None, with_model=True):
    ends, nq, nn, tog = exp or C.expect(c)
    addr = place(ctx, c)
    for form in forms or c["forms"]:
        r = launch(ctx, c, addr, form)
        assert r[-5:] == (len(ends), nq, nn, 0, tog), (c["name"], form, r[-5:], (len(ends), nq, nn, tog))
        if form == "u16b":
            low, table = blocked(ends, c["begin"], c["end"])
            assert np.array_equal(r[0], low) and np.array_equal(r[1], table), (c["name"], form)
        else:
            assert np.array_equal(r[0].astype(np.uint64), ends), (c["name"], form)
        if with_model:
            m = C.model(emu, c, form)
            assert len(m) == len(r) and all(np.array_equal(x, y) for x, y in zip(m, r)), (c["name"], form)
    counts = ctx.records(addr, len(c["buf"]), c["base"], c["begin"], c["end"], quote=c["quote"], carry=c["carry"],
                         escape=c["escape"], esc_carry=c["esc_carry"], scope=c["scope"], form="count")
    assert (counts.n, counts.n_quotes, counts.n_newlines, counts.toggles) == (len(ends), nq, nn, tog)


def test_every_escape_byte_value_at_every_chunk_position(ctx):
    """4 KiB holding the escape byte at every chunk position, next to quotes and newlines."""
    for e in range(256):
        if e in (C.Q, C.NL):
            continue
        filler = ord("a") if e != ord("a") else ord("b")
        d = np.full(4096, filler, np.uint8)
        for pos in range(16):                            # chunk 4 * pos + 1: e at byte pos, then a quote; later a
            x = (4 * pos + 1) * 16 + pos                 # doubled escape before a quote, and an escaped newline
            d[x:x + 2] = (e, C.Q)
            d[x + 17:x + 20] = (e, e, C.Q)
            d[x + 33:x + 37] = (C.NL, e, C.NL, C.Q)
        d[15::16][200:] = e                              # escape bytes at chunk ends, newlines at chunk starts
        d[16::16][200:] = C.NL
        d[-1] = C.NL
        c = C.case(d, escape=e, scope="all" if e & 1 else "quoted", esc_carry=(e >> 1) & 1, name=f"byte{e}")
        check(ctx, c, with_model=e % 8 == 4)
        # the model on every eighth value: it shares the kernel's mask16, the loop above is the oracle of all


@pytest.mark.parametrize("edges", [C.EDGES_ODD, C.EDGES_EVEN], ids=["odd", "even"])
def test_runs_ending_at_every_edge(ctx, edges):
    for c in C.edge_cases(edges):
        check(ctx, c, with_model=len(c["name"]) % 2 == 0)


def test_exact_runs_all_escape_tile_and_deep_blocked_begin(ctx):
    for c in C.exact_run_cases() + C.all_escape_tile_cases() + C.blocked_large_begin_cases():
        check(ctx, c, with_model="@0" in c["name"] or "tile" in c["name"] or "blocked" in c["name"])


def test_begin_at_every_alignment_carry_esc_carry_scope(ctx):
    for c in C.alignment_cases():
        check(ctx, c)


def test_8mib_of_random_bytes(ctx):
    d = C.random_five(8 << 20, 11)
    c = C.case(d, begin=5, carry=1, esc_carry=1, scope="all", name="random8m")
    exp = C.expect(c)
    check(ctx, c, exp, with_model=False)
    m = C.model(emu, c, "u64", schedule="random:3")
    assert np.array_equal(m[0], exp[0]) and m[-1] == exp[3]


@pytest.fixture(scope="module")
def escaped_object():
    d = synth.csv_escaped(8 << 20, seed=3)
    assert len(d) == 8 << 20 and d[-1] == C.NL
    return d.tobytes(), d, loop_record_ends(d, scope="all")


def test_8mib_of_csv_escaped(ctx, escaped_object):
    data, d, (ends, tog, esc, inside) = escaped_object
    assert (esc, inside) == (0, 0) and int(ends[-1]) == len(d) - 1
    plain_ends = loop_record_ends(d, escape=1)[0]        # the parity rule alone cuts this object elsewhere
    assert not np.array_equal(plain_ends, ends)
    c = C.case(d, name="csv_escaped")
    for scope in ("all", "quoted"):
        c = dict(c, scope=scope)
        check(ctx, c, with_model=False)


def _co(data: bytes, key: str, name: str):
    MemoryStore._named.pop(name, None)
    cfg = {"endpoint_url": f"memory://{name}"}
    co = CloudObject.from_s3(fcsv.CSV, f"s3://data/{key}", fetch=False, s3_config=cfg)
    co.storage.create_bucket(Bucket="data")
    co.storage.put_object(Body=data, Bucket="data", Key=key)
    return CloudObject.from_s3(fcsv.CSV, f"s3://data/{key}", s3_config=cfg)


def test_record_index_object_chains_three_parts(ctx, escaped_object):
    data, d, (ends, _, _, _) = escaped_object
    co = _co(data, "e.csv", "gpu_quote_escape_parts")
    part = (3 << 20) - 4097
    got = record_index_object(co, escape=92, max_devices=1, part_bytes=part)
    assert np.array_equal(got, ends)
    got = record_index_object(co, 7, len(d) - 3, escape=92, escape_scope="quoted", max_devices=1, part_bytes=part,
                              fmt="u16b")
    want = loop_record_ends(d, 7, len(d) - 3, scope="quoted")[0]
    assert isinstance(got, BlockedOffsets) and np.array_equal(got.to_u64(), want)


def test_preprocess_and_partition_never_split_a_row(ctx):
    d = synth.csv_escaped((1 << 20) + 777, seed=31)
    raw = d.tobytes()
    co = _co(raw, "p.csv", "gpu_quote_escape_e2e")
    co.preprocess(extra_args={"quotechar": '"', "escapechar": "\\"})
    at = co.attributes
    ends = loop_record_ends(d)[0]
    assert (at.escapechar, at.escape_scope, at.quotechar, at.num_records) == ("\\", "all", '"', len(ends))
    for n in (1, 7, 40):
        slices = co.partition(fcsv.partition_records_num_chunks, num_chunks=n)
        assert b"".join(raw[s.body[0]:s.body[1]] for s in slices) == raw
        rows = 0
        for s in slices:
            if s.body[1] > s.body[0]:
                assert s.body[1] - 1 in ends                                     # cut at a record end only
                df = s.get_as_pandas()
                assert list(df.columns) == at.columns and df.shape[1] == 11      # whole rows
                rows += len(df)
        assert rows == at.num_records - 1


def test_an_absent_escape_byte_equals_the_plain_launch(ctx):
    d = C.random_five(3 * T + 77, 21)
    d[d == C.E] = ord("x")
    c = C.case(d, begin=9, carry=1, escape=C.E, name="absent")
    addr = place(ctx, c)
    a = (addr, len(d), 0, 9, len(d))
    for form in ("u32", "u64"):
        out, _, nq, nn, _, _ = ctx.records(*a, quote=C.Q, carry=1, form=form)
        for scope in ("all", "quoted"):
            eo, _, enq, enn, tog, _ = ctx.records(*a, quote=C.Q, carry=1, escape=C.E, scope=scope, form=form)
            assert eo.dtype == out.dtype and eo.tobytes() == out.tobytes() and (enq, enn, tog) == (nq, nn, nq)
    low, table, nq, nn, _, _ = ctx.records(*a, quote=C.Q, carry=1, form="u16b")
    elow, etable, enq, enn, tog, _ = ctx.records(*a, quote=C.Q, carry=1, escape=C.E, form="u16b")
    assert elow.tobytes() == low.tobytes() and etable.tobytes() == table.tobytes() and (enq, enn, tog) == (nq, nn, nq)


def test_entry_points_refuse_bad_escape_arguments(ctx):
    d = C.random_five(4096, 1)
    c = C.case(d)
    addr = place(ctx, c)
    a = (addr, len(d), 0, 0, len(d))
    for kw in (dict(escape=C.Q), dict(escape=10), dict(escape=256), dict(escape=92, esc_carry=2),
               dict(escape=92, quote=10), dict(escape=92, carry=2)):
        with pytest.raises(DPScanError) as ei:
            ctx.records(*a, **kw)
        assert ei.value.code == _quote.DQ_ERR_INVALID
        with pytest.raises(DPScanError) as ei:
            ctx.records(*a, form="u16b", **kw)
        assert ei.value.code == _quote.DQ_ERR_INVALID
    q, h = ctx._quote_ctx()
    import ctypes
    rc = q.dq_records_esc_async(h, ctypes.c_void_p(addr), len(d), 0, 0, len(d), 34, 0, 92, 0, 2, None, 1, 0)
    assert rc == _quote.DQ_ERR_INVALID                   # an unknown flags bit
    with pytest.raises(ValueError):
        ctx.records(*a, escape=92, scope="some")
    assert len(ctx.records(*a, escape=92).ends) == len(loop_record_ends(d)[0])   # the ctx is usable afterwards


def test_a_run_beyond_the_bound_is_reported_at_once(ctx):
    """A status path: the kernel walks back at most DQ_ESCAPE_RUN_MAX bytes, sets the error word and goes on."""
    n = _quote.DQ_ESCAPE_RUN_MAX + (64 << 10)
    d = C.plain(T + n + T, 2)
    d[T:T + n] = C.E
    c = C.case(d, name="overbound")
    addr = place(ctx, c)
    ctx.sync()
    t0 = time.perf_counter()
    with pytest.raises(_quote.DPEscapeRunError) as ei:
        ctx.records(addr, len(d), 0, 0, len(d), escape=92)
    dt = time.perf_counter() - t0
    assert ei.value.code == _quote.DQ_ERR_ESCAPE_RUN
    assert dt < 1.0, f"{dt:.3f} s"
    assert C.model(emu, c)[-2] == emu.ERR_ESCAPE_RUN
    d2 = d.copy()                                        # a run of exactly the bound on the same context: exact
    d2[T + _quote.DQ_ESCAPE_RUN_MAX:T + n] = ord("a")
    check(ctx, C.case(d2, name="atbound"), with_model=False)
