"""The blocked form u16b of libdpquote.so's record-end kernel (quote_kernel<2>) on the GPU, through
ScanContext.records(form="u16b"): the uint16 low words and the 64 KiB block table bit-equal to the lane-exact model
(tools/emulate_quote.py) and, decoded by BlockedOffsets, equal to the definition (tests/_quote_model.py).  With
T = 64 KiB and b0 = begin & 0xFFFF: lengths around the chunk and tile edges, first tiles entered up to 65535 bytes in,
both incoming states, more tiles than workgroups, tiles without a record end, object offsets above 2^32, canaries
behind both outputs, the alignment rule, both forms on one context, and preprocess + partition end to end."""
import csv as pycsv
import io
import os
import sys

import numpy as np
import pytest

from _quote_cases import ALPHABET, SPARSE, one_lane_16
from _quote_model import record_ends
from dataplug_amd import synth
from dataplug_amd.cloudobject import CloudObject
from dataplug_amd.formats.generic import csv as fcsv
from dataplug_amd.scan import DPCapacityError, DPScanError, ScanContext
from dataplug_amd.scan.objects import BlockedOffsets
from dataplug_amd.storage import MemoryStore

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import emulate_quote as emu  # noqa: E402

pytestmark = pytest.mark.gpu

T = emu.TILE_BYTES
PRE = 7
LOW_BLOCK, HIGH_BLOCK = 3, 70_001                        # begin >> 16; the second puts every offset above 2^32


@pytest.fixture(scope="module")
def geo(ctx):
    t, g = ctx.quote_geometry()
    assert t == T and g > 0
    return t, g


def tiles_of(begin, end):
    return ((end - 1) >> 16) - (begin >> 16) + 1 if end > begin else 0


def table_of(ends, begin, end):
    bounds = np.arange(begin >> 16, (begin >> 16) + tiles_of(begin, end), dtype=np.uint64) << np.uint64(16)
    return np.searchsorted(ends, bounds, side="left").astype(np.uint64)


def place(ctx, buf, lo, begin, name="quote_in"):
    """buf on the device with buf[lo] -- object byte ``begin`` -- at an address congruent to ``begin`` mod 16;
    returns (device address of buf[0], object offset of buf[0])."""
    buf_base = begin - lo
    d = ctx.workspace(name, len(buf) + 64)
    assert d.ptr % 16 == 0
    addr = d.ptr + buf_base % 16
    ctx.h2d(addr, buf)
    return addr, buf_base


def run_blocked(ctx, buf, lo, hi, begin, carry=0, cap=None, quote=34):
    """records(form="u16b") of buf[lo:hi] as object bytes [begin, begin + hi - lo), checked against the definition."""
    addr, buf_base = place(ctx, buf, lo, begin)
    end = begin + hi - lo
    low, table, nq, nn, _, _ = ctx.records(addr, len(buf), buf_base, begin, end, quote=quote, carry=carry, form="u16b",
                                           cap=cap)
    exp, eq, en = record_ends(buf[lo:hi], base=begin, quote=quote, carry=carry)
    assert low.dtype == np.uint16 and table.dtype == np.uint64 and (nq, nn) == (eq, en)
    assert len(table) == tiles_of(begin, end) and np.array_equal(table, table_of(exp, begin, end))
    assert len(low) == len(exp) and np.array_equal(BlockedOffsets(low, table, begin >> 16).to_u64(), exp)
    return low, table, addr, buf_base


def padded(content, n, seed):
    """PRE + n + 33 bytes: ``content`` inside [PRE, PRE + n), quotes and newlines alternating around it."""
    rng = np.random.default_rng(seed)
    buf = np.empty(n + 40, np.uint8)
    buf[PRE:PRE + n] = ALPHABET[rng.integers(0, 4, n)] if content == "alphabet" else one_lane_16(n, seed)
    pad = np.resize(np.frombuffer(b'\n"', np.uint8), n + 40)
    buf[:PRE], buf[PRE + n:] = pad[:PRE], pad[PRE + n:]
    return buf


@pytest.mark.parametrize("content", ["alphabet", "one_lane_16"])
def test_edges_kernel_equals_lane_model_and_definition(ctx, geo, content):
    k = 0
    for n in (1, 15, 16, 17, T - 1, T, T + 1, 2 * T + 5, 3 * T + 17):
        for b0 in (0, 5, 65520, 65535):
            k += 1
            buf = padded(content, n, k)
            begin = (HIGH_BLOCK if k % 2 else LOW_BLOCK) * T + b0
            P = None
            for carry in (0, 1):
                low, table, addr, buf_base = run_blocked(ctx, buf, PRE, PRE + n, begin, carry=carry)
                if P is None:                            # phase A of the model once: it depends on neither carry
                    P = emu.prepare(buf, dev_addr=addr, buf_base=buf_base, begin=begin, end=begin + n, blocked=True)
                mlow, mtable, n_out, _, _, err = emu.finish(P, carry=carry, fmt="u16b")
                assert err == 0 and n_out == len(low), (n, b0, carry)
                assert np.array_equal(mlow, low) and np.array_equal(mtable, table), (n, b0, carry)


def test_more_tiles_than_workgroups(ctx, geo):
    t, g = geo
    n = min(3 * g * t + 12345, 256 << 20)
    assert n > g * t, "the ticket must hand some workgroup a second tile"
    rng = np.random.default_rng(2)
    buf = SPARSE[rng.integers(0, 32, n + 16, dtype=np.uint8)]
    low, table, _, _ = run_blocked(ctx, buf, 3, 3 + n, HIGH_BLOCK * T + 65531, carry=1)
    assert len(table) == tiles_of(65531, 65531 + n) > g and len(low) > 1_000_000


def test_tiles_without_a_record_end(ctx, geo):
    n = 5 * T + 100
    rng = np.random.default_rng(3)
    buf = ALPHABET[rng.integers(0, 4, n)].copy()
    mid = buf[T + 50:4 * T + 50]                         # 3 T bytes without any newline
    mid[mid == 10] = 97
    for carry in (0, 1):
        low, table, _, _ = run_blocked(ctx, buf, 0, n, LOW_BLOCK * T + 40, carry=carry)
        assert len(table) == 6 and table[2] == table[3] == table[4] and 0 < table[1] <= table[2] < len(low)
    quiet = np.full(3 * T, 97, np.uint8)                 # no record end at all: the table is all zero
    low, table, _, _ = run_blocked(ctx, quiet, 0, 3 * T, 9 * T)
    assert len(low) == 0 and list(table) == [0, 0, 0]


def test_object_offsets_above_2_to_32(ctx, geo):
    buf = np.full(300, 10, np.uint8)
    begin = (1 << 32) - 100                              # the range crosses 2^32 and a block boundary
    low, table, _, _ = run_blocked(ctx, buf, 0, 300, begin)
    assert list(table) == [0, 100] and low[99] == 0xFFFF and low[100] == 0
    got = BlockedOffsets(low, table, begin >> 16).to_u64()
    assert int(got[0]) == begin and int(got[-1]) == begin + 299
    rng = np.random.default_rng(4)
    buf = ALPHABET[rng.integers(0, 4, 2 * T + 99)]
    run_blocked(ctx, buf, 11, len(buf), (1 << 40) + 65530, carry=1)


def test_canaries_and_the_capacity_error(ctx, geo):
    rng = np.random.default_rng(5)
    buf = ALPHABET[rng.integers(0, 4, 2 * T + 4096)]
    begin, n = LOW_BLOCK * T + 65520, len(buf) - 9
    end = begin + n
    addr, buf_base = place(ctx, buf, 9, begin)
    nt = tiles_of(begin, end)
    assert nt == 4
    for carry in (0, 1):
        exp, eq, en = record_ends(buf[9:], base=begin, carry=carry)
        assert len(exp) > 1000
        for cap in (777, len(exp)):
            low_canary = np.full(len(exp) + 64, 0xEEEE, np.uint16)
            tab_canary = np.full(nt + 8, 0xEEEEEEEEEEEEEEEE, np.uint64)
            d_low = ctx.workspace("quote_canary", low_canary.nbytes)
            d_tab = ctx.workspace("quote_table_canary", tab_canary.nbytes)
            ctx.h2d(d_low.ptr, low_canary)
            ctx.h2d(d_tab.ptr, tab_canary)
            ctx.records_async(addr, len(buf), buf_base, begin, end, quote=34, carry=carry, form="u16b", d_out=d_low.ptr,
                              cap=cap, d_table=d_tab.ptr, table_cap=nt)
            if cap < len(exp):
                with pytest.raises(DPCapacityError) as ei:
                    ctx.records_result()
                assert (ei.value.needed, ei.value.n_quotes, ei.value.n_newlines) == (len(exp), eq, en)
            else:
                assert ctx.records_result()[:3] == (len(exp), eq, en)
            low = ctx.d2h(np.empty_like(low_canary), d_low.ptr)
            tab = ctx.d2h(np.empty_like(tab_canary), d_tab.ptr)
            assert np.array_equal(low[:cap], (exp[:cap] & np.uint64(0xFFFF)).astype(np.uint16))
            assert np.array_equal(low[cap:], low_canary[cap:]), "written at or beyond low[cap]"
            assert np.array_equal(tab[:nt], table_of(exp, begin, end)), "the table is whole whatever cap is"
            assert np.array_equal(tab[nt:], tab_canary[nt:]), "written at or beyond table[ntiles]"
            mlow, mtab, n_out, _, _, err = emu.run(buf, dev_addr=addr, buf_base=buf_base, begin=begin, end=end,
                                                   carry=carry, cap=cap, fmt="u16b")
            assert err == (emu.ERR_CAPACITY if cap < len(exp) else 0) and n_out == len(exp)
            assert np.array_equal(mlow, low[:cap]) and np.array_equal(mtab, tab[:nt])
    low, table, _, _ = run_blocked(ctx, buf, 9, len(buf), begin, cap=1)          # the wrapper retries with the count
    assert len(low) == len(record_ends(buf[9:])[0])
    # the count-only call of this entry point: no low words, the table all the same
    ctx.h2d(d_tab.ptr, tab_canary)
    ctx.records_async(addr, len(buf), buf_base, begin, end, quote=34, carry=0, form="u16b", d_out=0, cap=0,
                      d_table=d_tab.ptr, table_cap=nt)
    assert ctx.records_result().n == len(low)
    assert np.array_equal(ctx.d2h(np.empty(nt, np.uint64), d_tab.ptr), table)


def test_misaligned_address_and_bad_tables_are_refused(ctx, geo):
    buf = np.full(4096, 10, np.uint8)
    begin = LOW_BLOCK * T + 16
    addr, buf_base = place(ctx, buf, 0, begin)
    out = ctx.workspace("out", 1 << 16)
    tab = ctx.workspace("record_blocks", 1 << 16)
    ok = (addr, 4000, buf_base, begin, begin + 4000, 34, 0, out.ptr, 4096, tab.ptr, 1)

    def launch(d_buf, buf_len, buf_base, begin, end, quote, carry, d_low, cap, d_table, table_cap):
        ctx.records_async(d_buf, buf_len, buf_base, begin, end, quote=quote, carry=carry, form="u16b", d_out=d_low,
                          cap=cap, d_table=d_table, table_cap=table_cap)

    def refused(**kw):
        args = dict(zip(("d_buf", "buf_len", "buf_base", "begin", "end", "quote", "carry", "d_low", "cap", "d_table",
                         "table_cap"), ok))
        args.update(kw)
        with pytest.raises(DPScanError):
            launch(*args.values())
    for off in (1, 8, 15):
        refused(d_buf=addr + off)                        # the device address of begin is not congruent to begin mod 16
    refused(buf_base=buf_base + 1, begin=begin + 1, end=begin + 4001)       # the same bytes, named one offset higher
    refused(table_cap=0)
    refused(d_table=0)
    refused(d_table=tab.ptr + 4)
    refused(d_low=out.ptr + 1)
    refused(d_low=0)
    refused(end=begin + T, buf_len=2 * T, table_cap=1)   # two tiles, room for one
    refused(quote=10)
    refused(carry=2)
    refused(end=begin + 5000)                            # past the buffer
    launch(*ok)                                          # nothing above left a launch in flight
    assert ctx.records_result()[:3] == (4000, 0, 4000)
    low, table, _, _, _, _ = ctx.records(addr + 5, 4000, buf_base, begin + 77, begin + 77, form="u16b")  # empty: no rule
    assert len(low) == 0 and len(table) == 0


def test_forms_agree_and_contexts_are_reusable(ctx, geo):
    rng = np.random.default_rng(6)
    big = ALPHABET[rng.integers(0, 4, 5 * T + 3)]
    small = ALPHABET[rng.integers(0, 4, T + 9)]

    def both(c, buf, lo, begin, carry):
        addr, buf_base = place(c, buf, lo, begin)
        end = begin + len(buf) - lo
        u64 = c.records(addr, len(buf), buf_base, begin, end, carry=carry).ends
        low, table, _, _, _, _ = c.records(addr, len(buf), buf_base, begin, end, carry=carry, form="u16b")
        again = c.records(addr, len(buf), buf_base, begin, end, carry=carry).ends
        dec = BlockedOffsets(low, table, begin >> 16).to_u64()
        assert np.array_equal(dec, u64) and np.array_equal(again, u64)
        assert np.array_equal(u64, record_ends(buf[lo:], base=begin, carry=carry)[0])
        return dec

    first = both(ctx, big, 0, LOW_BLOCK * T + 65000, 0)
    both(ctx, small, 2, HIGH_BLOCK * T + 17, 1)          # fewer tiles: the earlier descriptors and table are stale
    assert np.array_equal(both(ctx, big, 0, LOW_BLOCK * T + 65000, 0), first)
    other = ScanContext(0)
    try:
        assert np.array_equal(both(other, big, 0, LOW_BLOCK * T + 65000, 0), first)
        both(ctx, small, 2, HIGH_BLOCK * T + 17, 1)
        both(other, small, 0, 5, 1)
    finally:
        other.close()


def _co(data: bytes, key: str, name: str):
    MemoryStore._named.pop(name, None)
    cfg = {"endpoint_url": f"memory://{name}"}
    co = CloudObject.from_s3(fcsv.CSV, f"s3://data/{key}", fetch=False, s3_config=cfg)
    co.storage.create_bucket(Bucket="data")
    co.storage.put_object(Body=data, Bucket="data", Key=key)
    return CloudObject.from_s3(fcsv.CSV, f"s3://data/{key}", s3_config=cfg)


def test_preprocess_and_partition_end_to_end(geo):
    data = synth.csv_quoted((1 << 20) + 4321, seed=23)
    model = record_ends(data)[0]
    raw = data.tobytes()
    co16 = _co(raw, "q16.csv", "gpu_quote_blocked_u16b")
    co16.preprocess(extra_args={"quotechar": '"', "record_index_format": "u16b"})
    co64 = _co(raw, "q64.csv", "gpu_quote_blocked_u64")
    co64.preprocess(extra_args={"quotechar": '"'})
    at = co16.attributes
    assert at.record_index_dtype == "u16b" and at.num_records == len(model) == co64.attributes.num_records
    assert getattr(co64.attributes, "record_index_dtype", None) is None
    st, bucket = co16.storage, co16.meta_path.bucket
    low = np.frombuffer(st.get_object(Bucket=bucket, Key=at.record_index_key)["Body"].read(), "<u2")
    blocks = np.frombuffer(st.get_object(Bucket=bucket, Key=at.record_index_blocks_key)["Body"].read(), "<u8")
    assert len(low) == len(model) and len(blocks) == ((len(raw) - 1) >> 16) + 1 and at.record_index_block0 == 0
    assert np.array_equal(BlockedOffsets(low, blocks, 0).to_u64(), model)
    for n in (1, 3, 8, 50):
        s16 = co16.partition(fcsv.partition_records_num_chunks, num_chunks=n)
        s64 = co64.partition(fcsv.partition_records_num_chunks, num_chunks=n)
        assert [s.body for s in s16] == [s.body for s in s64] and len(s16) == n
        assert b"".join(raw[s.body[0]:s.body[1]] for s in s16) == raw
        rows = 0
        for s in s16:
            if s.body[1] == s.body[0]:
                continue
            parsed = list(pycsv.reader(io.StringIO(s.get(), newline="")))
            assert parsed[0] == at.columns and {len(r) for r in parsed} == {11}      # whole records only
            rows += len(parsed) - 1
        assert rows == at.num_records - 1
    # several parts per object, the parts' tables merged: the same index
    from dataplug_amd.scan import objects as so
    merged = so.record_index_object(co16, part_bytes=100_003, fmt="u16b")
    assert np.array_equal(merged.low, low) and np.array_equal(merged.table, blocks) and merged.j0 == 0
