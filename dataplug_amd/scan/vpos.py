"""Host side of the VCF position index: the per-part outputs of libdpvpos.so (include/dpvpos.h holds the
definition) merged into the stored samples and the contig table, in vectorised numpy, and the stored forms.

    <key>.pos      the POS of every K-th line, uint32 little-endian
    <key>.contigs  NAME FIRST_LINE NUM_LINES OFFSET END MIN_POS MAX_POS, tab-separated, one row per contig run
"""
from __future__ import annotations

from typing import List, Sequence, Tuple

import numpy as np

from .fai import first_duplicate

CONTIG_DTYPE = np.dtype([("first_line", "<u8"), ("num_lines", "<u8"), ("offset", "<u8"), ("end", "<u8"),
                         ("min_pos", "<u4"), ("max_pos", "<u4")])
KINDS = ("malformed", "unsorted", "split contig", "missing REF")


class VcfFormatError(ValueError):
    """The body cannot be indexed by position: ``kind`` is "malformed" (a line without CHROM and a POS of 1-10 digits
    <= 2**31 - 1 inside its first 1024 bytes), "unsorted" (POS decreases inside a contig) or "split contig" (the
    lines of a contig are not contiguous); with ``span_index`` also "missing REF" (a line with fewer than 4 fields or an
    empty field 4).  ``ordinal`` and ``offset`` are the first offending line's number in the
    body and its byte offset in the object."""

    def __init__(self, kind: str, ordinal: int, offset: int):
        super().__init__(f"VCF line {ordinal} at byte {offset}: {kind}")
        self.kind, self.ordinal, self.offset = kind, int(ordinal), int(offset)

    def __reduce__(self):
        return (VcfFormatError, (self.kind, self.ordinal, self.offset))


def merge_parts(parts: Sequence, size: int) -> Tuple[np.ndarray, List[bytes], np.ndarray, int]:
    """(samples uint32, names, rows ``CONTIG_DTYPE``, number of lines) from the parts' ``device.VcfPositions`` in
    object order, or ``VcfFormatError`` for the first offending line.

    Indices local to a part become global ordinals; adjacent parts' boundary runs with equal names are joined (a run
    may span any number of parts); the order check across a part boundary uses the parts' last and first POS; a name
    that occurs in two runs is the split-contig error."""
    parts = [p for p in parts if p.n]
    n_lines = int(sum(p.n for p in parts))
    if not parts:
        return np.zeros(0, np.uint32), [], np.zeros(0, CONTIG_DTYPE), 0
    ord0 = np.concatenate([[0], np.cumsum([p.n for p in parts])[:-1]]).astype(np.int64)
    samples = np.concatenate([p.samples for p in parts]).astype(np.uint32, copy=False)
    nruns = np.array([len(p.run_line) for p in parts], np.int64)
    head = np.concatenate([[0], np.cumsum(nruns)[:-1]])              # each part's first run among all runs
    line = np.concatenate([p.run_line + o for p, o in zip(parts, ord0)])
    last_line = np.concatenate([p.run_last_line + o for p, o in zip(parts, ord0)])
    first = np.concatenate([p.run_pos for p in parts])
    last = np.concatenate([p.run_last for p in parts])
    offset = np.concatenate([p.run_offset for p in parts]).astype(np.uint64)
    names = [nm for p in parts for nm in p.names]
    # the offending lines the launches saw, and those at the part boundaries
    found = []                                                       # (ordinal, rank of the kind, byte offset)
    for p, o in zip(parts, ord0):
        if p.first_malformed is not None:
            found.append((int(o) + p.first_malformed, 0, p.malformed_offset))
        if p.first_unsorted is not None:
            found.append((int(o) + p.first_unsorted, 1, p.unsorted_offset))
    join = np.zeros(len(line), bool)
    for k in range(1, len(parts)):
        a, b = parts[k - 1], parts[k]
        if a.names[-1] and a.names[-1] == b.names[0]:                # (a malformed line has the empty name)
            join[head[k]] = True
            if b.first_pos < a.last_pos:
                found.append((int(ord0[k]), 1, b.first_offset))
    grp = np.cumsum(~join) - 1
    g0 = np.flatnonzero(~join)                                       # each joined run's first piece
    g1 = np.append(g0[1:], len(line)) - 1                            # and its last one
    gnames = [names[i] for i in g0]
    dup = first_duplicate(gnames)
    if dup >= 0:
        found.append((int(line[g0[dup]]), 2, int(offset[g0[dup]])))
    if found:
        o, kind, off = min(found)
        raise VcfFormatError(KINDS[kind], o, off)
    rows = np.zeros(len(g0), CONTIG_DTYPE)
    rows["first_line"] = line[g0]
    rows["num_lines"] = last_line[g1] - line[g0] + 1
    rows["offset"] = offset[g0]
    rows["end"] = np.append(offset[g0][1:], np.uint64(size))
    rows["min_pos"] = first[g0]
    rows["max_pos"] = last[g1]
    assert int(grp[-1]) + 1 == len(g0) and int(rows["num_lines"].sum()) == n_lines
    return samples, gnames, rows, n_lines


def contigs_text(names: List[bytes], rows: np.ndarray) -> bytes:
    """NAME\\tFIRST_LINE\\tNUM_LINES\\tOFFSET\\tEND\\tMIN_POS\\tMAX_POS\\n per contig run."""
    if len(rows) == 0:
        return b""
    cols = [rows[k].astype("S20").tolist() for k in CONTIG_DTYPE.names]
    return b"\n".join(map(b"\t".join, zip(names, *cols))) + b"\n"


def parse_contigs(text: bytes) -> Tuple[List[bytes], np.ndarray]:
    """(names, rows) of a stored contig table (a name may hold any byte but tab and newline)."""
    lines = text.split(b"\n")[:-1] if text else []
    names = [ln.split(b"\t", 1)[0] for ln in lines]
    rows = np.zeros(len(lines), CONTIG_DTYPE)
    if lines:
        num = np.array([ln.split(b"\t")[1:7] for ln in lines], dtype="S20").astype(np.uint64)
        for k, col in zip(CONTIG_DTYPE.names, num.T):
            rows[k] = col
    return names, rows


def candidate_lines(s: np.ndarray, j0: int, every: int, l0: int, l1: int, start, end) -> Tuple[int, int]:
    """The candidate line range [a, b) of a query start <= POS <= end inside the contig's lines [l0, l1): from the
    last sample with POS < start (none: l0) to the first sample with POS > end (none: l1).  ``s`` holds the samples
    whose ordinals lie in [l0, l1): ``s[k]`` is the POS of line (j0 + k) * every, j0 = ceil(l0 / every); POS does not
    decrease inside a contig."""
    a, b = l0, l1
    s = np.asarray(s, np.int64)
    if start is not None:
        k = int(np.searchsorted(s, start, "left"))                   # samples [0, k) have POS < start
        if k > 0:
            a = (j0 + k - 1) * every
    if end is not None:
        k = int(np.searchsorted(s, end, "right"))                    # sample k is the first with POS > end
        if k < len(s):
            b = (j0 + k) * every
    return a, max(a, b)
