"""The definition of a VCF record's end (include/dpvspan.h) without a GPU: the byte loop (tests/_vspan_loop.py) on the
hand-written lines of tests/_vspan_cases.py, one assertion per clause, the host's own form of the definition
(``scan.vspan.rec_end``) against the loop, the block maxima, and ``synth.gvcf``."""
import numpy as np
import pytest

import _vcfpos_loop as P
import _vspan_loop as L
from _vspan_cases import BIG_REF, CASES, FROM_END, MISSING_REF, TRUNCATED, line
from dataplug_amd import synth
from dataplug_amd.scan import vspan


@pytest.mark.parametrize("name,data,pos,end,flags", CASES, ids=[c[0] for c in CASES])
def test_loop_on_hand_written_lines(name, data, pos, end, flags):
    assert P.parse_line(data + b"\n", 0)[1] == pos                       # the case's POS is the line's own
    assert L.span_line(data, 0, pos) == (end, flags)
    assert flags & MISSING_REF or end >= pos
    # the same line behind another one, and with more lines behind it
    pre = b"chr1\t5\trs0\tAAAA\tC\t9\tPASS\tEND=77\n"
    more = data if data.endswith(b"\n") else data + b"\n"
    if data.endswith(b"\n"):
        assert L.span_line(pre + data + pre, len(pre), pos) == (end, flags)
    assert L.span_line(pre + more + pre, len(pre), pos) == L.span_line(more, 0, pos)
    # the host's form of the definition takes the line without its '\n'
    assert vspan.rec_end(data[:-1] if data.endswith(b"\n") else data, pos) == (end, flags)


def test_the_case_list_covers_every_clause():
    names = {c[0] for c in CASES}
    assert len(names) == len(CASES) >= 40
    by_flag = {f: sum(1 for c in CASES if c[4] == f) for f in (0, MISSING_REF, FROM_END)}
    assert by_flag[0] >= 15 and by_flag[MISSING_REF] >= 4 and by_flag[FROM_END] >= 15
    assert len(BIG_REF) == 70_000 and any(len(c[1]) > 70_000 for c in CASES)
    assert any(c[1].endswith(b"\r\n") for c in CASES) and any(not c[1].endswith(b"\n") for c in CASES)
    assert any(max(c[1]) >= 0x80 for c in CASES)


def test_saturating_add():
    assert L.sat_end(1, 1) == 1 and L.sat_end(100, 3) == 102
    assert L.sat_end(2**31 - 1, 2**31) == 2**32 - 2
    assert L.sat_end(2**31 - 1, 2**31 + 1) == 2**32 - 1                  # the largest sum that fits
    assert L.sat_end(2**31 - 1, 2**31 + 2) == 2**32 - 1                  # ... and the first that saturates
    assert L.sat_end(2**31 - 1, 2**40) == 2**32 - 1
    assert L.sat_end(0, 2**32 + 5) == 2**32 - 1 and L.sat_end(0, 1) == 0


def test_truncation_is_the_buffer_ending_below_the_size():
    d = line(100, b"ACG", info=b"NS=3;END=250")
    t4, t8 = d.index(b"ACG") + 1, d.index(b"END=") + 5
    for cut, want in ((t4, (0, TRUNCATED)), (t8, (0, TRUNCATED)), (len(d), (250, FROM_END)),
                      (d.index(b"\tGT") + 1, (250, FROM_END)), (d.index(b"\tGT"), (0, TRUNCATED))):
        assert L.span_line(d, 0, 100, limit=cut) == want, cut            # the buffer ends at ``cut``, the object goes on
    assert L.span_line(d[:t8], 0, 100) == (102, 0)                       # the object itself ends there: END=2 < POS
    assert L.span_line(d[:t4], 0, 100) == (100, 0)                       # ... inside REF: one base of it
    assert L.span_line(d, len(d), 100) == (0, TRUNCATED) and L.span_line(d, len(d) + 7, 100) == (0, TRUNCATED)
    short = b"chr1\t100\trs1\tACGTA\n"                                    # fewer than 8 fields: the '\n' must be seen
    assert L.span_line(short, 0, 100, limit=len(short)) == (104, 0)
    assert L.span_line(short + b"x", 0, 100, limit=len(short) - 1) == (0, TRUNCATED)
    empty = b"chr1\t100\trs1\t\tC\t9\n"                                   # an empty REF is seen before the buffer ends
    assert L.span_line(empty + b"x", 0, 100, limit=empty.index(b"\tC") + 1) == (0, MISSING_REF)


def test_launch_and_block_maxima_of_the_loop():
    rows = [line(10, b"AC"), line(12, info=b"END=900"), b"chr1\t13\trs\n", line(14, b"ACGT"), line(20, info=b"END=25")]
    d = b"".join(rows)
    st = P.line_starts(d, 0)
    pos = [10, 12, 13, 14, 20]
    ends, flags = L.loop_span(d, 0, len(d), st, pos)
    assert ends == [11, 900, 0, 17, 25] and flags == [0, FROM_END, MISSING_REF, 0, FROM_END]
    for ordinal0, every, want in ((0, 2, [900, 17, 25]), (1, 2, [11, 900, 25]), (3, 4, [11, 900]), (0, 8, [900]),
                                  (7, 1, ends)):
        slots, res = L.loop_blockmax(ends, flags, pos, ordinal0, every)
        assert slots == want and len(slots) == L.n_slots(ordinal0, 5, every)
        assert res == dict(n_missing=1, min_missing=2, n_truncated=0, min_truncated=L.NONE, n_from_end=2,
                           max_span=888)
    assert L.loop_blockmax([], [], [], 5, 2) == ([], dict(n_missing=0, min_missing=L.NONE, n_truncated=0,
                                                          min_truncated=L.NONE, n_from_end=0, max_span=0))
    with pytest.raises(L.LoopError) as e:
        L.loop_ends(d, 0, 2)
    assert (e.value.kind, e.value.ordinal, e.value.offset) == ("missing REF", 2, st[2])
    good = b"".join(rows[:2] + rows[3:])
    assert L.loop_ends(good, 0, 2) == ([900, 25], 888, 4)
    assert L.loop_overlap(good, 0, b"chr1", 18, 19) == rows[1] and L.loop_overlap(good, 0, b"chr1", 26, 30) == rows[1]
    assert L.loop_overlap(good, 0, b"chr1", 17, 20) == rows[1] + rows[3] + rows[4]


def test_gvcf_is_exact_sorted_seeded_and_has_every_kind_of_row():
    a = synth.gvcf(300_007, seed=9, contigs=3)
    head = synth.VCF_HEADER
    assert len(a) == 300_007 and a[-1] == 10 and a[:len(head)].tobytes() == head
    assert np.array_equal(a, synth.gvcf(300_007, seed=9, contigs=3))
    assert not np.array_equal(a, synth.gvcf(300_007, seed=10, contigs=3))
    d = a.tobytes()
    smp, contigs, n = P.loop_index(d, len(head), 1)                      # sorted, contiguous contigs
    assert [c[0] for c in contigs] == [b"chr1", b"chr2", b"chr3"] and n > 3000
    rows = L.line_ends(d, len(head))
    spans = np.array([e - p for _, p, e in rows])
    body = d[len(head):]
    assert body.count(b"<NON_REF>\t.\t.\tEND=") > n // 2 and body.count(b"<DEL>") >= 1
    assert ((spans >= 1) & (spans < 60)).sum() > n // 20                 # deletions and reference blocks
    assert 10**4 <= spans.max() <= 10**6 and (spans == 0).sum() > n // 10
    big = synth.gvcf(2_000_003, seed=1, contigs=2, block=100_003)        # several copies of the tile per contig
    rows = L.line_ends(big.tobytes(), len(head))
    assert max(p for _, p, _ in rows) > 5 * 10**7 and all(e >= p for _, p, e in rows)
    assert P.loop_index(big.tobytes(), len(head), 128)[2] == len(rows)
