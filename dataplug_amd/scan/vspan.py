"""Host side of the VCF record-end index: the definition of a record's end (include/dpvspan.h) for single lines, the
per-part outputs of libdpvspan.so merged into the stored slots in vectorised numpy, and the block filter of an
overlap query.

    <key>.ends     the largest rec_end of every K-block of body lines, uint32 little-endian, aligned with <key>.pos
"""
from __future__ import annotations

from collections import namedtuple
from typing import List, Optional, Sequence, Tuple

import numpy as np

from .vpos import KINDS, VcfFormatError

END_MAX = 2**31 - 1
U32_MAX = 2**32 - 1
MISSING_REF, TRUNCATED, FROM_END = 1, 2, 4
MISSING_KIND = KINDS.index("missing REF")

# one part of a build, its truncated line (if any) already resolved on the host: ``n`` lines, ``blockmax`` its slots
# (the first and the last may be partial K-blocks), ``max_span`` its largest rec_end - POS, ``first_missing`` the lowest
# local index of a MISSING_REF line or None, and ``missing_offset`` that line's byte offset
SpanPart = namedtuple("SpanPart", "n blockmax max_span first_missing missing_offset")


def rec_end(line: bytes, pos: int) -> Tuple[int, int]:
    """(rec_end, flags) of one whole line (without its '\\n') whose POS is ``pos``: the definition of
    include/dpvspan.h on the host, for the lines a launch could not finish and for the lines a query fetches."""
    f = line.split(b"\t", 8)
    if len(f) < 4 or not f[3]:
        return 0, MISSING_REF
    if len(f) >= 8:
        for entry in f[7].split(b";"):
            if entry.startswith(b"END="):                    # the first such entry decides
                v = entry[4:]
                if 1 <= len(v) <= 10 and v.isdigit() and pos <= int(v) <= END_MAX:
                    return int(v), FROM_END
                break
    return min(pos + len(f[3]) - 1, U32_MAX), 0


def line_pos(line: bytes) -> int:
    """POS of a line as include/dpvpos.h defines it: field 2, 1 to 10 ASCII digits, at most 2^31 - 1, behind a
    non-empty CHROM and in front of a second tab inside the first 1024 bytes; ValueError for a line that is not well
    formed."""
    f = line.split(b"\t", 2)
    if len(f) < 3 or not f[0] or len(f[0]) + len(f[1]) + 1 >= 1024 or not 1 <= len(f[1]) <= 10 \
            or not f[1].isdigit() or int(f[1]) > END_MAX:
        raise ValueError("no well-formed POS")
    return int(f[1])


def fold_line(spans, ordinal0: int, every: int, line: Optional[bytes]) -> SpanPart:
    """A part's ``device.VcfSpans`` as a ``SpanPart``.  ``line``: the whole bytes of its TRUNCATED line, which can only
    be the part's last one -- the host applies the definition to it and folds the result into the last slot."""
    slots = np.array(spans.blockmax, np.uint32)
    span, fm, mo = int(spans.max_span), spans.first_missing, spans.missing_offset
    if spans.n_truncated:
        if spans.n_truncated != 1 or spans.first_truncated != spans.n - 1 or line is None:
            raise RuntimeError("record ends: a line other than the part's last was cut by the buffer")
        try:
            pos = line_pos(line)
        except (IndexError, ValueError):
            pos = 0                                          # (a malformed line: the position index reports it)
        end, fl = rec_end(line, pos)
        if fl & MISSING_REF:
            if fm is None:
                fm, mo = spans.first_truncated, spans.truncated_offset
        else:
            slots[-1] = max(int(slots[-1]), end)
            span = max(span, end - pos)
    return SpanPart(spans.n, slots, span, fm, mo)


def merge_parts(parts: Sequence[SpanPart], every: int) -> Tuple[np.ndarray, int, int]:
    """(slots uint32, max_span, number of lines) from the parts' ``SpanPart`` in object order, or ``VcfFormatError``
    ("missing REF") for the first such line in file order.  A part's slot j is the global slot ordinal0 // K + j;
    adjacent parts' boundary slots that belong to the same K-block are merged by maximum."""
    parts = [p for p in parts if p.n]
    n_lines = int(sum(p.n for p in parts))
    if not parts:
        return np.zeros(0, np.uint32), 0, 0
    k = int(every)
    ord0 = np.concatenate([[0], np.cumsum([p.n for p in parts])[:-1]]).astype(np.int64)
    for p, o in zip(parts, ord0):                            # in object order: the first is the lowest
        if p.first_missing is not None:
            raise VcfFormatError(KINDS[MISSING_KIND], int(o) + p.first_missing, p.missing_offset)
    idx = np.concatenate([o // k + np.arange(len(p.blockmax), dtype=np.int64) for p, o in zip(parts, ord0)])
    val = np.concatenate([p.blockmax for p in parts]).astype(np.uint32, copy=False)
    slots = np.zeros(-(-n_lines // k), np.uint32)
    assert len(idx) == len(val) and (not len(idx) or int(idx.max()) < len(slots))
    np.maximum.at(slots, idx, val)
    return slots, int(max(p.max_span for p in parts)), n_lines


def blocks_before(ends: np.ndarray, j_lo: int, every: int, l0: int, a: int, start: int) -> List[Tuple[int, int]]:
    """The line ranges [x, y) in front of line ``a`` that an overlap query has to look at: ``ends`` holds the slots
    j_lo, j_lo + 1, ... (j_lo = l0 // K) of the contig's lines [l0, a).  A block is kept when its slot is at least
    ``start``; the partial block that holds ``a`` is always kept.  Adjacent kept blocks are joined."""
    if a <= l0:
        return []
    k = int(every)
    j_hi = (a - 1) // k                                      # the block of the last line in front
    keep = np.asarray(ends[:j_hi - j_lo + 1], np.int64) >= int(start)
    if a % k:
        keep[-1] = True                                      # the block holding the boundary
    out = []
    for j in np.flatnonzero(keep).tolist():
        x, y = max(l0, (j_lo + j) * k), min(a, (j_lo + j + 1) * k)
        if out and out[-1][1] == x:
            out[-1] = (out[-1][0], y)
        else:
            out.append((x, y))
    return out
