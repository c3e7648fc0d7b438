"""The definition of a VCF record's end (include/dpvspan.h) as a plain Python byte loop: the oracle of every vspan
test.  Nothing here is vectorised or shared with the package.  POS is the position loop's (tests/_vcfpos_loop.py)."""
import _vcfpos_loop as P

END_MAX = 2**31 - 1
U32_MAX = 2**32 - 1
MISSING_REF, TRUNCATED, FROM_END = 1, 2, 4
NONE = 0xFFFFFFFFFFFFFFFF


class LoopError(Exception):
    """What the definition refuses: ``kind`` "missing REF", at line ``ordinal`` which starts at byte ``offset``."""

    def __init__(self, kind, ordinal, offset):
        super().__init__(f"{kind} at line {ordinal} (byte {offset})")
        self.kind, self.ordinal, self.offset = kind, ordinal, offset


def sat_end(pos: int, reflen: int) -> int:
    """POS + reflen - 1, saturated at 2**32 - 1."""
    return min(pos + reflen - 1, U32_MAX)


def end_value(info: bytes, pos: int):
    """The END value of the INFO bytes if it counts, else None."""
    p = 0
    n = len(info)
    while p <= n:                                            # p is the first byte of an entry
        q = p
        while q < n and info[q] != 59:
            q += 1
        entry = info[p:q]
        if entry[:4] == b"END=":                             # the first such entry decides; later ones are ignored
            digits = entry[4:]
            if not 1 <= len(digits) <= 10:
                return None
            v = 0
            for b in digits:
                if not 48 <= b <= 57:
                    return None
                v = v * 10 + b - 48
            return v if pos <= v <= END_MAX else None
        p = q + 1
    return None


def span_line(data: bytes, s: int, pos: int, limit: int = None, size: int = None):
    """(rec_end, flags) of the line that starts at ``s`` with POS ``pos``.  ``size``: the object's size (default: all
    of ``data``); ``limit``: the bytes at and beyond it are not in the buffer."""
    size = len(data) if size is None else size
    limit = min(len(data), size) if limit is None else min(limit, size, len(data))
    if s < 0 or s >= limit:
        return 0, TRUNCATED
    tabs = []                                                # the tabs of the line, up to the eighth
    q = s
    ended = False
    while q < limit:
        b = data[q]
        if b == 10:
            ended = True
            break
        if b == 9:
            tabs.append(q)
            if len(tabs) == 4 and tabs[3] == tabs[2] + 1:    # an empty field 4: the walk stops here
                return 0, MISSING_REF
            if len(tabs) == 8:
                break
        q += 1
    e = q
    if len(tabs) < 8 and not ended and limit < size:         # the buffer ended first
        return 0, TRUNCATED
    if len(tabs) < 3:
        return 0, MISSING_REF
    reflen = (tabs[3] if len(tabs) >= 4 else e) - (tabs[2] + 1)
    if reflen == 0:
        return 0, MISSING_REF
    if len(tabs) >= 7:
        v = end_value(data[tabs[6] + 1:tabs[7] if len(tabs) == 8 else e], pos)
        if v is not None:
            return v, FROM_END
    return sat_end(pos, reflen), 0


def loop_span(buf: bytes, buf_base: int, size: int, starts, pos):
    """(end, flags) lists of one span launch over the buffer ``buf`` = object bytes from ``buf_base``."""
    top = min(len(buf), max(0, size - buf_base))
    ends, flags = [], []
    for s, p in zip(starts, pos):
        if s < buf_base:
            e, f = 0, TRUNCATED
        else:
            e, f = span_line(buf, s - buf_base, p, limit=top, size=max(0, size - buf_base))
        ends.append(e), flags.append(f)
    return ends, flags


def n_slots(ordinal0: int, n: int, every: int) -> int:
    return (ordinal0 + n - 1) // every - ordinal0 // every + 1 if n else 0


def loop_blockmax(ends, flags, pos, ordinal0: int, every: int):
    """The block-max launch's outputs: (slots, result dict)."""
    n = len(ends)
    slots = [0] * n_slots(ordinal0, n, every)
    for i in range(n):
        j = (ordinal0 + i) // every - ordinal0 // every
        slots[j] = max(slots[j], ends[i])
    mis = [i for i in range(n) if flags[i] & MISSING_REF]
    tru = [i for i in range(n) if flags[i] & TRUNCATED]
    spans = [ends[i] - pos[i] for i in range(n) if not flags[i] & (MISSING_REF | TRUNCATED)]
    res = dict(n_missing=len(mis), min_missing=mis[0] if mis else NONE, n_truncated=len(tru),
               min_truncated=tru[0] if tru else NONE, n_from_end=sum(1 for f in flags if f & FROM_END),
               max_span=max(spans + [0]))
    return slots, res


def line_ends(data: bytes, body_offset: int):
    """[(start, POS, rec_end)] of every body line, or ``LoopError`` for the first MISSING_REF line."""
    out = []
    for i, s in enumerate(P.line_starts(data, body_offset)):
        pos = P.parse_line(data, s)[1]
        e, f = span_line(data, s, pos)
        if f & MISSING_REF:
            raise LoopError("missing REF", i, s)
        out.append((s, pos, e))
    return out


def loop_ends(data: bytes, body_offset: int, every: int):
    """(slots, max_span, number of lines) of the whole object: slot j is the largest rec_end of lines
    [j * every, (j + 1) * every)."""
    rows = line_ends(data, body_offset)
    slots = [0] * (-(-len(rows) // every))
    for i, (_, _, e) in enumerate(rows):
        slots[i // every] = max(slots[i // every], e)
    return slots, max([e - p for _, p, e in rows] + [0]), len(rows)


def slots_bytes(slots) -> bytes:
    return b"".join(int(v).to_bytes(4, "little") for v in slots)


def loop_overlap(data: bytes, body_offset: int, chrom: bytes, start=None, end=None) -> bytes:
    """The lines of contig ``chrom`` whose [POS, rec_end] overlaps [start, end], each with its terminator."""
    out = []
    for s, e in P.lines_of(data, body_offset):
        c, p = P.parse_line(data, s)
        if c != chrom:
            continue
        r = span_line(data, s, p)[0]
        if (start is None or r >= start) and (end is None or p <= end):
            out.append(data[s:e])
    return b"".join(out)
