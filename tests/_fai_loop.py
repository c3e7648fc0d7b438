"""The definition of the faidx-compatible FASTA index (include/dpfai.h), as the plain byte loop it is stated as.

The oracle of every .fai test: it walks the lines of every body byte by byte, on purpose not the counts-and-formulas
form that the GPU path uses.  A line's width is its bytes with its '\\n'; a last line that lacks its '\\n' is
measured as if one followed.  Sequence i is regular iff every line but the last has the first line's width W and the
last one is no wider.  A body without any '\\n' is regular as it is (W = its bytes).
"""
from dataplug_amd.scan.fai import FaiFormatError

STOP = b" \t\r\n"


def loop_name(data, start, end):
    name = bytearray()
    for p in range(start + 1, end):
        if data[p] in STOP:
            break
        name.append(data[p])
    return bytes(name)


def loop_fai(data, pairs):
    """[(NAME, LENGTH, OFFSET, LINEBASES, LINEWIDTH), ...] of object ``data`` with the stored header ``pairs``
    [(start, end), ...], or ``FaiFormatError`` naming the first offending sequence."""
    data = bytes(data)
    pairs = [(int(s), int(e)) for s, e in pairs]
    rows, seen = [], set()
    for i, (start, end) in enumerate(pairs):
        name = loop_name(data, start, end)
        if name in seen:
            raise FaiFormatError(i, name, "duplicate sequence name")
        seen.add(name)
        b = end
        e = max(b, pairs[i + 1][0] if i + 1 < len(pairs) else len(data))
        widths, cur, nl, cr = [], 0, 0, 0
        for p in range(b, e):
            cur += 1
            if data[p] == 13:
                cr += 1
            elif data[p] == 10:
                nl += 1
                widths.append(cur)
                cur = 0
        if nl == 0:
            if cr:
                raise FaiFormatError(i, name, "mixed line endings")
            rows.append((name, e - b, b, e - b, e - b))
            continue
        if cur:
            widths.append(cur + 1)                       # the last line lacks its '\n': as if one followed
        w = widths[0]
        if any(x != w for x in widths[:-1]) or widths[-1] > w:
            raise FaiFormatError(i, name, "different line length in sequence")
        if cr not in (0, nl):
            raise FaiFormatError(i, name, "mixed line endings")
        if w >= 1 << 32:
            raise FaiFormatError(i, name, "line width >= 2**32")
        t = 2 if cr else 1
        rows.append((name, e - b - nl - cr, b, w - t, w))
    return rows


def loop_text(rows):
    return b"".join(b"%s\t%d\t%d\t%d\t%d\n" % r for r in rows)
