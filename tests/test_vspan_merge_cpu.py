"""``scan.vspan``'s merge of the parts' slots without a GPU, at every part cut of a 40-line body (the manner of
tests/_part_cut_cases.py; the parts' launches are the definition's loop, tests/_vspan_model.py): the merged slots must
be the loop's slots of the whole body for cuts inside a K-block, on a block's edge and around parts of one line or
none, a line the look-ahead cuts is resolved on the host, and the first MISSING_REF line across the parts is the one
reported."""
import numpy as np
import pytest

import _vcfpos_loop as P
import _vspan_loop as L
import _vspan_model as M
from dataplug_amd.scan import vspan
from dataplug_amd.scan.vpos import KINDS, VcfFormatError

EVERY = (1, 2, 8)
BODY = M.body40()


def cut_sets(data: bytes):
    """Every single cut at a byte of the short rows and every seventh inside the long row, and the pairs (c, c + 1),
    (c, c + 2) around every line start and every fifth byte."""
    st = P.line_starts(data, 0)
    long_lo, long_hi = st[30], st[31]
    singles = [[c] for c in range(1, len(data)) if not long_lo + 40 < c < long_hi - 40 or c % 7 == 0]
    near = sorted({c for s in st for c in (s - 2, s - 1, s, s + 1)} | set(range(1, long_lo, 5)))
    pairs = [[c, c + d] for c in near for d in (1, 2) if 0 < c and c + d < len(data)]
    return singles, pairs


def merged(data, cuts, every):
    parts = M.spans_by_cuts(data, 0, cuts, every)
    slots, span, n = vspan.merge_parts(M.folded(data, parts, every), every)
    return slots.astype("<u4").tobytes(), span, n, parts


@pytest.mark.parametrize("every", EVERY)
def test_merged_slots_equal_the_loop_at_every_cut(every):
    want_slots, want_span, n = L.loop_ends(BODY, 0, every)
    assert n == 40 and len(want_slots) == -(-40 // every) and want_span == 300
    want = (L.slots_bytes(want_slots), want_span, n)
    assert merged(BODY, [], every)[:3] == want
    singles, pairs = cut_sets(BODY)
    seen = {"inside": 0, "edge": 0, "one_line": 0, "no_line": 0, "truncated": 0}
    for cuts in singles + pairs:
        got = merged(BODY, cuts, every)
        assert got[:3] == want, (cuts, every)
        for before, vs in got[3]:
            assert len(vs.blockmax) == L.n_slots(before, vs.n, every)
            seen["truncated"] += vs.n_truncated
            seen["one_line"] += vs.n == 1
            seen["no_line"] += vs.n == 0
            if before and vs.n:
                seen["inside" if before % every else "edge"] += 1
    # what the sweep covers: parts that begin inside a K-block and on its edge (K = 1: always the edge), parts of one
    # line and of none, and lines the 1024-byte look-ahead cuts
    assert seen["edge"] > 30 and (every == 1 or seen["inside"] > 30)
    assert seen["one_line"] > 10 and seen["no_line"] > 10 and seen["truncated"] > 10


def test_a_cut_line_is_resolved_on_the_host():
    st = P.line_starts(BODY, 0)
    cut = st[30] - 1                                                     # the '\n' in front of the long row
    parts = M.spans_by_cuts(BODY, 0, [cut, cut + 1], 8)
    assert [vs.n for _, vs in parts] == [30, 1, 9]
    vs = parts[1][1]                                                     # the long row alone, its INFO cut
    assert (vs.n_truncated, vs.first_truncated, vs.truncated_offset, vs.blockmax.tolist()) == (1, 0, st[30], [0])
    sp = M.folded(BODY, parts, 8)[1]
    pos = P.parse_line(BODY, st[30])[1]
    assert sp.blockmax.tolist() == [pos + 50] and sp.max_span == 50 and sp.first_missing is None
    with pytest.raises(RuntimeError):                                    # a cut line must be the part's last one
        vspan.fold_line(vs._replace(n=2, blockmax=np.array([0], np.uint32)), 30, 8, b"x")


def test_the_first_missing_ref_across_the_parts_is_reported():
    assert KINDS[-1] == "missing REF" and KINDS[:3] == ("malformed", "unsorted", "split contig")
    for missing in ((5,), (5, 33), (0, 39), (39,), (30,)):
        data = M.body40(missing=missing)
        st = P.line_starts(data, 0)
        with pytest.raises(L.LoopError) as le:
            L.loop_ends(data, 0, 2)
        assert (le.value.kind, le.value.ordinal, le.value.offset) == ("missing REF", missing[0], st[missing[0]])
        first = st[missing[0]]
        for cuts in ([], [first - 1], [first], [first + 1], [st[3], st[35]], [st[missing[-1]] - 1, st[missing[-1]] + 2],
                     [st[20] + 3]):
            cuts = [c for c in cuts if 0 < c < len(data)]
            parts = M.folded(data, M.spans_by_cuts(data, 0, cuts, 2), 2)
            with pytest.raises(VcfFormatError) as e:
                vspan.merge_parts(parts, 2)
            assert (e.value.kind, e.value.ordinal, e.value.offset) == ("missing REF", missing[0], first), cuts
            assert "missing REF" in str(e.value) and isinstance(e.value, ValueError)


def test_merge_of_nothing_and_block_filter():
    assert vspan.merge_parts([], 8)[1:] == (0, 0) and len(vspan.merge_parts([], 8)[0]) == 0
    ends = np.array([50, 10, 99, 10, 10], np.uint32)                     # slots 2 .. 6 of K = 4: lines 8 .. 27
    assert vspan.blocks_before(ends, 2, 4, 9, 26, 60) == [(16, 20), (24, 26)]     # the boundary's partial block stays
    assert vspan.blocks_before(ends, 2, 4, 9, 24, 60) == [(16, 20)]      # a boundary on a block's edge keeps none
    assert vspan.blocks_before(ends, 2, 4, 9, 26, 5) == [(9, 26)]        # adjacent blocks are joined
    assert vspan.blocks_before(ends, 2, 4, 9, 9, 5) == [] and vspan.blocks_before(ends, 2, 4, 9, 10, 500) == [(9, 10)]
