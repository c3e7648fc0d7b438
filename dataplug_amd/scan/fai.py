"""Host side of the faidx-compatible FASTA index: the columns derived from the GPU's per-body counts
(include/dpfai.h holds the definition), in vectorised numpy.

    NAME LENGTH OFFSET LINEBASES LINEWIDTH

Every body byte other than '\\n' and '\\r' counts as a base (spaces and tabs too; htslib counts graphic characters
only).  The header pairs are taken as stored.
"""
from __future__ import annotations

from typing import List, Tuple

import numpy as np

NONE = np.uint64(0xFFFFFFFFFFFFFFFF)
FAI_DTYPE = np.dtype([("length", "<u8"), ("offset", "<u8"), ("linebases", "<u4"), ("linewidth", "<u4")])
_NAME_MATRIX_MAX = 1 << 28               # bytes of the padded name matrix the duplicate check may build


class FaiFormatError(ValueError):
    """The object cannot be indexed as ``samtools faidx`` would refuse it: an irregular sequence (line widths or
    mixed line endings), a line width >= 2**32, or a duplicate name.  ``ordinal`` and ``name`` are the first
    offending sequence's."""

    def __init__(self, ordinal: int, name: bytes, reason: str):
        super().__init__(f"sequence {ordinal} ({name.decode('latin-1')!r}): {reason}")
        self.ordinal, self.name, self.reason = int(ordinal), bytes(name), reason


def bodies(pairs, size: int) -> Tuple[np.ndarray, np.ndarray]:
    """(b, e) uint64: the body of sequence i is [end_i, start_{i+1}) (``size`` for the last)."""
    p = np.asarray(pairs, np.uint64).reshape(-1, 2)
    b = np.ascontiguousarray(p[:, 1])
    e = np.append(p[1:, 0], np.uint64(size)).astype(np.uint64)
    return b, np.maximum(e, b)


def line_widths(b, e, nl, first) -> np.ndarray:
    """W_i (uint64): first_i - b_i + 1, or B_i for a body without any '\\n'."""
    has = nl > 0
    return np.where(has, np.where(has, first, b) - b + np.uint64(1), e - b)


def split_names(lens, packed) -> List[bytes]:
    """The names as a list of bytes, and nothing per sequence in Python where a padded matrix is affordable."""
    lens = np.asarray(lens, np.int64)
    h = len(lens)
    if h == 0:
        return []
    packed = np.asarray(packed, np.uint8)
    width = max(1, int(lens.max()))
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]])
    if h * width <= _NAME_MATRIX_MAX and not (packed == 0).any():
        mat = np.zeros((h, width), np.uint8)
        rows = np.repeat(np.arange(h), lens)
        mat[rows, np.arange(len(packed)) - np.repeat(offs, lens)] = packed
        return mat.view(f"S{width}").reshape(h).tolist()
    raw = packed.tobytes()
    return [raw[o:o + n] for o, n in zip(offs.tolist(), lens.tolist())]


def first_duplicate(names: List[bytes]) -> int:
    """The lowest ordinal whose name occurred before it, or -1."""
    if len(set(names)) == len(names):
        return -1
    arr = np.array(names, dtype=object)
    _, inv = np.unique(arr, return_inverse=True)
    order = np.argsort(inv, kind="stable")
    same = inv[order][1:] == inv[order][:-1]
    return int(order[1:][same].min())


def derive(b, e, nl, cr, first, off, lastoff, names: List[bytes]) -> np.ndarray:
    """The numeric columns (``FAI_DTYPE``) from the merged counts, or ``FaiFormatError`` for the first offending
    sequence."""
    b, e, nl, cr, off, lastoff = (np.asarray(a, np.uint64) for a in (b, e, nl, cr, off, lastoff))
    size = e - b
    w = line_widths(b, e, nl, np.asarray(first, np.uint64))
    has = nl > 0
    mixed = (cr != 0) & (cr != nl)
    t = np.where(cr == 0, 1, 2).astype(np.uint64)
    m = size // np.maximum(w, np.uint64(1))
    regular = ~has | ((nl - off == m) & ((off == 0) | ((off == 1) & (lastoff == e - np.uint64(1)))))
    wide = w >= np.uint64(1 << 32)
    bad = mixed | ~regular | wide
    dup = first_duplicate(names)
    if bad.any() or dup >= 0:
        i = int(np.argmax(bad)) if bad.any() else len(b)
        if 0 <= dup < i:
            raise FaiFormatError(dup, names[dup], "duplicate sequence name")
        reason = ("mixed line endings" if mixed[i] else "line width >= 2**32" if wide[i] else
                  "different line length in sequence")
        raise FaiFormatError(i, names[i], reason)
    rows = np.zeros(len(b), FAI_DTYPE)
    rows["length"] = size - nl - cr
    rows["offset"] = b
    rows["linewidth"] = w
    rows["linebases"] = np.where(has, w - np.minimum(t, w), size)
    return rows


def fai_text(names: List[bytes], rows: np.ndarray) -> bytes:
    """The samtools text: NAME\\tLENGTH\\tOFFSET\\tLINEBASES\\tLINEWIDTH\\n per sequence."""
    if len(rows) == 0:
        return b""
    cols = [rows[k].astype("S20").tolist() for k in ("length", "offset", "linebases", "linewidth")]
    return b"\n".join(map(b"\t".join, zip(names, *cols))) + b"\n"


def parse_fai(text: bytes) -> Tuple[List[bytes], np.ndarray]:
    """(names, rows) of a stored .fai text."""
    lines = text.split(b"\n")[:-1] if text else []
    names = [ln.split(b"\t", 1)[0] for ln in lines]
    rows = np.zeros(len(lines), FAI_DTYPE)
    if lines:
        num = np.array([ln.split(b"\t")[1:5] for ln in lines], dtype="S20").astype(np.uint64)
        rows["length"], rows["offset"], rows["linebases"], rows["linewidth"] = num.T
    return names, rows
