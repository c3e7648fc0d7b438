"""Host side of the FASTQ read index: the per-part outputs of libdpfq.so (include/dpfq.h holds the definition) merged
into the stored samples, in numpy, and the stored form.

    <key>.fqi   S + 1 pairs of little-endian uint64: (byte offset of read jK, bases before it) for j < S, then (size, B)
"""
from __future__ import annotations

from collections import namedtuple
from typing import Callable, Sequence

import numpy as np

SAMPLE_DTYPE = np.dtype([("offset", "<u8"), ("bases", "<u8")])
KINDS = ("well formed", "bad_header", "bad_separator", "length_mismatch", "truncated")
TRUNCATED = 4
# what ``merge_parts`` returns: ``samples`` a ``SAMPLE_DTYPE`` array of S + 1 entries
ReadsIndex = namedtuple("ReadsIndex", "samples num_reads num_bases min_read_len max_read_len")


class FastqFormatError(ValueError):
    """The object cannot be indexed as four-line FASTQ: ``kind`` is "bad_header" (the read's first line does not begin
    with '@'), "bad_separator" (its third line does not begin with '+'), "length_mismatch" (its sequence and quality
    lines differ in length, or are 4 GiB or longer) or "truncated" (the lines behind the last whole read are not a
    multiple of four).  ``read`` and ``offset`` are the first offending read's number and the byte offset of its
    first line.  Wrapped FASTQ, whose sequences span several lines, surfaces as one of these."""

    def __init__(self, kind: str, read: int, offset: int):
        super().__init__(f"FASTQ read {read} at byte {offset}: {kind}")
        self.kind, self.read, self.offset = kind, int(read), int(offset)

    def __reduce__(self):
        return (FastqFormatError, (self.kind, self.read, self.offset))


def part_plan(n_lines: int, skip: int, last: bool):
    """(device reads, the local numbers of the lines whose starts are read back) of a part that owns ``n_lines``
    lines, the first ``skip`` of a read begun earlier; ``last``: it reaches the object's end.  Every owned line is
    complete but a part's last one, unless the part is the last.  The device takes the reads whose four lines are
    complete; the lines in front of them, the first of them and the lines behind them are read back -- or all of
    them in a part with fewer than 8."""
    complete = n_lines if last else max(0, n_lines - 1)
    nr = (complete - skip) // 4 if n_lines >= 8 else 0
    if nr == 0:
        return 0, np.arange(n_lines, dtype=np.int64)
    return nr, np.concatenate([np.arange(0, skip + 1), np.arange(skip + 4 * nr, n_lines)]).astype(np.int64)


def empty_index() -> ReadsIndex:
    return ReadsIndex(np.zeros(1, SAMPLE_DTYPE), 0, 0, 0, 0)


def merge_parts(parts: Sequence, size: int, every: int, get_byte: Callable[[int], int], map_fn=map) -> ReadsIndex:
    """The index of an object of ``size`` bytes from its parts' ``device.FastqPart`` in object order, or
    ``FastqFormatError`` for the first offending read.  ``get_byte(offset)`` is one byte of the object; the offsets
    the edge reads need are collected first and fetched through one ``map_fn(get_byte, offsets)``, so a caller with
    many boundaries can run the single-byte requests side by side.

    The edge lines of all parts, in global line order, group into whole reads by construction (a device read never
    shares a line with them), but for the lines behind the last whole read.  Their lengths come from consecutive
    starts -- the line behind an edge line is another edge line, the first line of a part's device reads, or the
    object's end -- and the four bytes the definition looks at from the object itself.  The edge reads' samples go to
    their slots, and each part's samples get the bases of everything before the part's device reads."""
    size, k = int(size), int(every)
    if size == 0:
        return empty_index()
    n_lines = int(sum(p.n_lines for p in parts))
    before = np.concatenate([[0], np.cumsum([p.n_lines for p in parts])]).astype(np.int64)
    closed = bool(parts[-1].closed) if parts else False
    known = {n_lines: size if closed else size + 1}                  # where a line behind the last one would start
    for p, b in zip(parts, before):
        known.update(zip((p.edge_lines + b).tolist(), map(int, p.edge_starts)))
    device = np.zeros(n_lines + 1, bool)
    for p, b in zip(parts, before):
        assert (b + p.skip) % 4 == 0 or p.n_reads == 0
        assert p.n_reads == 0 or p.read0 == (b + p.skip) // 4
        device[b + p.skip:b + p.skip + 4 * p.n_reads] = True
    num_reads = n_lines // 4
    edge = np.flatnonzero(~device[:4 * num_reads:4])                     # the reads the host handles
    raw = lambda i: known[i + 1] - 1 - known[i]                          # line i up to its terminator
    need = set()                                                         # per edge read at most four offsets
    for r in edge.tolist():
        i = 4 * r
        need.update(q for ok, q in ((raw(i) >= 1, known[i]), (raw(i + 1) >= 1, known[i + 2] - 2),
                                    (raw(i + 2) >= 1, known[i + 2]), (raw(i + 3) >= 1, known[i + 4] - 2)) if ok)
    need = sorted(need)
    byte = dict(zip(need, (int(v) for v in map_fn(get_byte, need)))).__getitem__
    e_len = np.zeros(len(edge), np.uint64)
    found = []                                                           # (read, kind, offset)
    for j, r in enumerate(edge.tolist()):
        i = 4 * r
        c1 = raw(i + 1) - (raw(i + 1) >= 1 and byte(known[i + 2] - 2) == 13)
        c3 = raw(i + 3) - (raw(i + 3) >= 1 and byte(known[i + 4] - 2) == 13)
        e_len[j] = c1
        if not (raw(i) >= 1 and byte(known[i]) == 64):
            found.append((r, 1, known[i]))
        elif not (raw(i + 2) >= 1 and byte(known[i + 2]) == 43):
            found.append((r, 2, known[i]))
        elif c1 != c3 or c1 >= 1 << 32:
            found.append((r, 3, known[i]))
    for p in parts:
        if p.first_malformed is not None:
            found.append((p.read0 + p.first_malformed, p.malformed_kind, p.malformed_offset))
    if n_lines % 4:
        found.append((num_reads, TRUNCATED, known[4 * num_reads]))
    if found:
        r, kind, off = min(found)
        raise FastqFormatError(KINDS[kind], r, off)
    # bases before every edge read and before every part's device reads: a device block lies before read r iff its
    # first read does, an edge read before a block iff it lies before the block's first read
    dev = [p for p in parts if p.n_reads]
    d_first = np.array([p.read0 for p in dev], np.int64)
    d_cum = np.concatenate([[0], np.cumsum([p.bases for p in dev], dtype=np.uint64)]).astype(np.uint64)
    e_cum = np.concatenate([[0], np.cumsum(e_len, dtype=np.uint64)]).astype(np.uint64)
    e_before = e_cum[:-1] + d_cum[np.searchsorted(d_first, edge, "left")]
    d_before = d_cum[:-1] + e_cum[np.searchsorted(edge, d_first, "left")]
    n_samples = -(-num_reads // k)
    out = np.zeros(n_samples + 1, SAMPLE_DTYPE)
    filled = np.zeros(n_samples + 1, np.int64)
    for p, b in zip(dev, d_before):
        j0, j1 = -(-p.read0 // k), -(-(p.read0 + p.n_reads) // k)
        assert len(p.samples) == j1 - j0
        out["offset"][j0:j1] = p.samples[:, 0]
        out["bases"][j0:j1] = p.samples[:, 1] + b
        filled[j0:j1] += 1
    pick = np.flatnonzero(edge % k == 0)
    out["offset"][edge[pick] // k] = [known[4 * int(r)] for r in edge[pick]]
    out["bases"][edge[pick] // k] = e_before[pick]
    filled[edge[pick] // k] += 1
    total = int(d_cum[-1]) + int(e_cum[-1])
    out[n_samples] = (size, total)
    filled[n_samples] += 1
    assert (filled == 1).all(), "a sample slot was not written exactly once"
    lens_min = [p.min_len for p in dev] + ([int(e_len.min())] if len(edge) else [])
    lens_max = [p.max_len for p in dev] + ([int(e_len.max())] if len(edge) else [])
    return ReadsIndex(out, num_reads, total, min(lens_min, default=0), max(lens_max, default=0))


def samples_bytes(samples: np.ndarray) -> bytes:
    return np.ascontiguousarray(samples, SAMPLE_DTYPE).tobytes()


def parse_samples(raw: bytes) -> np.ndarray:
    return np.frombuffer(raw, SAMPLE_DTYPE)
