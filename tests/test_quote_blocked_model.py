"""The blocked form u16b of the quote kernel (quote_kernel<2>, dq_records_blocked_async) in the lane-exact model
(tools/emulate_quote.py), without a GPU: tiles on the object's 64 KiB grid, a first tile entered up to 65535 bytes
in, the uint16 low words, the block table as each tile's exclusive look-back base, the cap and the alignment rule.
With T = 64 KiB and b0 = begin & 0xFFFF: the decode ``BlockedOffsets(low, table, begin >> 16).to_u64()`` must equal
the definition (tests/_quote_model.record_ends) and ``table[j]`` the definition's record ends below block
``(begin >> 16) + j``.  Every deliberate defect of ``emulate_quote.BLOCKED_MUTANTS`` must change a result here.
tests/test_gpu_quote_blocked.py pins this model to the hardware."""
import os
import sys

import numpy as np
import pytest

from _quote_cases import ALPHABET
from _quote_model import record_ends
from dataplug_amd.scan.objects import BlockedOffsets

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))
import emulate_quote as emu  # noqa: E402

T = emu.TILE_BYTES
B0S = (0, 1, 15, 16, 17, 65519, 65520, 65535)
LENGTHS = (1, 15, 16, 17, T - 1, T, T + 1, 2 * T + 5)
SCHEDULES = ("sequential", "all_agg", "random:0", "random:1")
PRE = 7                                                  # padding bytes in front of the range
LOW_BLOCK, HIGH_BLOCK = 3, 70_001                        # begin >> 16; the second puts begin above 2^32
assert HIGH_BLOCK << 16 > 1 << 32


def padded(n, seed, fill=None):
    """n + 40 bytes of ALPHABET (or ``fill``); outside [PRE, PRE + n) quotes and newlines alternate."""
    buf = ALPHABET[np.random.default_rng(seed).integers(0, 4, n + 40)].copy()
    if fill is not None:
        fill(buf[PRE:PRE + n])
    pad = np.resize(np.frombuffer(b'\n"', np.uint8), n + 40)
    buf[:PRE], buf[PRE + n:] = pad[:PRE], pad[PRE + n:]
    return buf


def placed(buf, n, b0, block):
    """(begin, end, prepare-arguments) of the range buf[PRE:PRE + n] as object bytes [begin, begin + n) with
    begin = block * T + b0, the buffer at a device address that keeps ``begin`` congruent mod 16."""
    begin = block * T + b0
    buf_base = begin - PRE
    return begin, begin + n, dict(dev_addr=(1 << 20) + buf_base % 16, buf_base=buf_base, begin=begin, end=begin + n)


def table_of(ends, begin, end):
    nt = ((end - 1) >> 16) - (begin >> 16) + 1
    bounds = (np.arange(begin >> 16, (begin >> 16) + nt, dtype=np.uint64)) << np.uint64(16)
    return np.searchsorted(ends, bounds, side="left").astype(np.uint64)


def check(P, buf, n, begin, end, carry, schedule, mutate=None, cap=None):
    """The launch's (low, table, counts, error) against the definition; a list of what differs."""
    st = {}
    low, table, n_out, nq, nn, err = emu.finish(P, carry=carry, schedule=schedule, mutate=mutate, cap=cap, stats=st,
                                                fmt="u16b")
    exp, eq, en = record_ends(buf[PRE:PRE + n], base=begin, carry=carry)
    keep = len(exp) if cap is None else min(cap, len(exp))
    bad = []
    if low.dtype != np.uint16 or table.dtype != np.uint64:
        bad.append("dtypes")
    if (n_out, nq, nn) != (len(exp), eq, en):
        bad.append("counts")
    if err != (emu.ERR_CAPACITY if cap is not None and 0 < cap < len(exp) else 0):
        bad.append(f"err {err}")
    if len(table) != ((end - 1) >> 16) - (begin >> 16) + 1 or not np.array_equal(table, table_of(exp, begin, end)):
        bad.append("table")
    if len(low) != keep or not np.array_equal(low, (exp[:keep] & np.uint64(0xFFFF)).astype(np.uint16)):
        bad.append("low")
    elif "table" not in bad and not np.array_equal(BlockedOffsets(low, table, begin >> 16).to_u64(), exp[:keep]):
        bad.append("decode")
    if not np.all(st["out_raw"][keep:] == 0xEEEE):
        bad.append("stored at or beyond cap")
    if not np.all(st["table_raw"][len(table):] == np.uint64(emu.CANARY)):
        bad.append("stored beyond the table")
    return bad


def grid_cases(mutate=None, b0s=B0S, lengths=LENGTHS):
    """(label, what differs) of every b0 x length x carry x schedule; phase A once per placement."""
    for bi, b0 in enumerate(b0s):
        for li, n in enumerate(lengths):
            buf = padded(n, 1000 * bi + li)
            block = HIGH_BLOCK if (bi + li) % 2 else LOW_BLOCK
            begin, end, kw = placed(buf, n, b0, block)
            P = emu.prepare(buf, blocked=True, **kw)
            assert P.blocked and P.args.lo == b0 and P.args.obj0 == block * T and P.args.base_addr % 16 == 0
            for carry in (0, 1):
                for schedule in SCHEDULES:
                    yield (b0, n, carry, schedule), check(P, buf, n, begin, end, carry, schedule, mutate)


def test_decode_and_table_equal_the_definition():
    bad = [(label, why) for label, why in grid_cases() if why]
    assert bad == []


def test_host_arguments_of_the_blocked_form():
    a = emu.host_args(dev_addr=0x7F0005, buf_len=3 * T, buf_base=5 * T + 5, begin=5 * T + 65535, end=7 * T + 1,
                      blocked=True)
    assert (a.lo, a.hi, a.obj0, a.ntiles) == (65535, 65535 + T + 2, 5 * T, 3)
    assert a.base_addr == 0x7F0005 + (65535 - 5) - 65535 and a.base_addr % 16 == 0     # below the buffer
    assert emu.host_args(0, 2 * T, 4 * T, 4 * T, 5 * T, blocked=True).ntiles == 1
    assert emu.host_args(0, 2 * T, 4 * T, 4 * T, 5 * T + 1, blocked=True).ntiles == 2
    assert emu.host_args(1, 100, 7 * T + 2, 7 * T + 40, 7 * T + 40, blocked=True).ntiles == 0     # empty: no rule
    # the same range in the other forms keeps its 16-byte shifted geometry
    b = emu.host_args(dev_addr=0x7F0005, buf_len=3 * T, buf_base=5 * T + 5, begin=5 * T + 65535, end=7 * T + 1)
    assert (b.lo, b.ntiles, b.obj0) == (15, 2, 5 * T + 65535 - 15)


def test_misaligned_device_address_is_refused():
    buf = padded(100, 1)
    begin, end, kw = placed(buf, 100, 16, LOW_BLOCK)
    for off in (1, 8, 15):
        with pytest.raises(ValueError, match="congruent"):
            emu.run(buf, fmt="u16b", **dict(kw, dev_addr=kw["dev_addr"] + off))
        with pytest.raises(ValueError, match="congruent"):
            emu.host_args(kw["dev_addr"] + off, len(buf), kw["buf_base"], begin, end, blocked=True)
    emu.run(buf, fmt="u16b", **dict(kw, dev_addr=kw["dev_addr"] + 16))


def test_middle_tile_without_a_newline_and_first_tile_of_one_byte():
    def hollow(d):                                       # no newline in the second 64 KiB block of the range's grid
        mid = d[T - 100:2 * T - 100]
        mid[mid == 10] = 97
    n, b0 = 3 * T - 200, 100                             # three blocks of the grid
    buf = padded(n, 5, hollow)
    begin, end, kw = placed(buf, n, b0, HIGH_BLOCK)
    P = emu.prepare(buf, blocked=True, **kw)
    for carry in (0, 1):
        for schedule in SCHEDULES:
            assert check(P, buf, n, begin, end, carry, schedule) == []
        table = emu.finish(P, carry=carry, fmt="u16b")[1]
        assert len(table) == 3 and table[1] == table[2] and table[1] > 0

    n, b0 = 2 * T + 5, 65535                             # tile 0 holds one byte of the range: a newline, kept
    buf = padded(n, 6)
    buf[PRE] = 10
    begin, end, kw = placed(buf, n, b0, LOW_BLOCK)
    P = emu.prepare(buf, blocked=True, **kw)
    assert P.args.ntiles == 4 and P.tiles[0] == emu.Sum(0, 1, 0)
    assert check(P, buf, n, begin, end, 0, "all_agg") == [] and check(P, buf, n, begin, end, 1, "all_agg") == []
    low, table = emu.finish(P, carry=0, fmt="u16b")[:2]
    assert low[0] == 65535 and list(table[:2]) == [0, 1]


def test_cap_clips_the_low_words_not_the_count_or_the_table():
    n, b0 = T + 4096, 65520
    buf = padded(n, 4)
    begin, end, kw = placed(buf, n, b0, LOW_BLOCK)
    P = emu.prepare(buf, blocked=True, **kw)
    for carry in (0, 1):
        count = len(record_ends(buf[PRE:PRE + n], carry=carry)[0])
        assert count > 1000
        for cap in (0, 1, 777, count - 1, count):
            assert check(P, buf, n, begin, end, carry, "sequential", cap=cap) == [], (carry, cap)


def test_every_blocked_mutant_is_killed():
    for mutate in emu.BLOCKED_MUTANTS:
        first = next((label for label, why in grid_cases(mutate, b0s=(0, 17), lengths=(17, T + 1)) if why), None)
        print(mutate, "killed by", first)
        assert first is not None, f"the defect {mutate!r} changes no result of this file"
    assert not set(emu.BLOCKED_MUTANTS) & set(emu.MUTANTS)
    for need in ("table_inclusive", "low_from_shifted", "table_skip_tile0"):
        assert need in emu.BLOCKED_MUTANTS


def test_uint64_model_is_untouched():
    n = T + 77
    buf = padded(n, 9)
    res = emu.run(buf, dev_addr=4096 + 5, buf_base=1_000_003, begin=1_000_003 + PRE, end=1_000_003 + PRE + n, carry=1,
                  schedule="all_agg")
    assert len(res) == 5
    got, n_out, nq, nn, err = res
    exp, eq, en = record_ends(buf[PRE:PRE + n], base=1_000_003 + PRE, carry=1)
    assert got.dtype == np.uint64 and err == 0 and (n_out, nq, nn) == (len(exp), eq, en) and np.array_equal(got, exp)
    assert emu.host_args(4096 + 5, len(buf), 1_000_003, 1_000_003 + PRE, 1_000_003 + PRE + n).lo == (5 + PRE) % 16
    for mutate in emu.BLOCKED_MUTANTS:                   # the blocked defects change nothing in the other forms
        assert np.array_equal(emu.run(buf, dev_addr=4096 + 5, buf_base=1_000_003, carry=1, mutate=mutate)[0],
                              emu.run(buf, dev_addr=4096 + 5, buf_base=1_000_003, carry=1)[0])
    with pytest.raises(ValueError):
        emu.run(buf, fmt="u8s")
    with pytest.raises(ValueError):                      # the form is decided when the launch is prepared
        emu.finish(emu.prepare(buf), fmt="u16b")
