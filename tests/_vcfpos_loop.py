"""The definition of the VCF position index (include/dpvpos.h) as a plain Python byte loop: the oracle of every
vcfpos test.  Nothing here is vectorised or shared with the package."""
PREFIX_MAX = 1024
POS_MAX = 2**31 - 1
SAME, MALFORMED = 1, 2
NONE = 0xFFFFFFFFFFFFFFFF


class LoopError(Exception):
    """What the definition refuses: ``kind`` "malformed", "unsorted" or "split contig", at line ``ordinal`` which
    starts at byte ``offset``."""

    def __init__(self, kind, ordinal, offset):
        super().__init__(f"{kind} at line {ordinal} (byte {offset})")
        self.kind, self.ordinal, self.offset = kind, ordinal, offset


def line_starts(data: bytes, body_offset: int):
    size = len(data)
    if body_offset >= size:
        return []
    out = [body_offset]
    for p in range(body_offset, size):
        if data[p] == 10 and p + 1 < size:
            out.append(p + 1)
    return out


def parse_line(data: bytes, s: int, limit: int = None):
    """(CHROM, POS) of the line that starts at ``s``, or None when it is not well formed.  ``limit``: the bytes at and
    beyond it are not there (the object's size, or the end of a buffer)."""
    limit = len(data) if limit is None else min(limit, len(data))
    if s >= limit:
        return None
    t1 = t2 = None
    for q in range(s, min(s + PREFIX_MAX, limit)):
        b = data[q]
        if b == 10:
            return None
        if b == 9:
            if t1 is None:
                t1 = q
            else:
                t2 = q
                break
    if t2 is None:
        return None
    chrom, pos = data[s:t1], data[t1 + 1:t2]
    if len(chrom) == 0 or not 1 <= len(pos) <= 10:
        return None
    v = 0
    for b in pos:
        if not 48 <= b <= 57:
            return None
        v = v * 10 + b - 48
    if v > POS_MAX:
        return None
    return bytes(chrom), v


def first_field(data: bytes, s: int, limit: int):
    """The bytes of the line at ``s`` up to its first tab, or None when the line has none."""
    for q in range(s, limit):
        if data[q] == 10:
            return None
        if data[q] == 9:
            return bytes(data[s:q])
    return None


def loop_parse(buf: bytes, buf_base: int, size: int, starts):
    """(pos, clen, flags) lists of one parse launch over the buffer ``buf`` = object bytes from ``buf_base``."""
    top = min(len(buf), max(0, size - buf_base))
    pos, clen, flags = [], [], []
    for i, s in enumerate(starts):
        r = parse_line(buf, s - buf_base, top) if s >= buf_base else None
        if r is None:
            pos.append(0), clen.append(0), flags.append(MALFORMED)
            continue
        same = 0
        if i > 0 and starts[i - 1] >= buf_base and starts[i - 1] - buf_base < top:
            same = int(first_field(buf, starts[i - 1] - buf_base, top) == r[0])
        pos.append(r[1]), clen.append(len(r[0])), flags.append(same)
    return pos, clen, flags


def loop_reduce(pos, clen, flags, ordinal0: int, every: int):
    """The reduce launch's outputs: (samples, runs [(i, first pos, clen, last line, last pos)], result dict)."""
    n = len(pos)
    samples = [pos[i] for i in range(n) if (ordinal0 + i) % every == 0]
    starts = [i for i in range(n) if not flags[i] & SAME]
    ends = [i for i in range(n) if i + 1 == n or not flags[i + 1] & SAME]
    runs = [(a, pos[a], clen[a], b, pos[b]) for a, b in zip(starts, ends)]
    mal = [i for i in range(n) if flags[i] & MALFORMED]
    uns = [i for i in range(1, n) if flags[i] & SAME and pos[i] < pos[i - 1]]
    res = dict(n_runs=len(starts), n_malformed=len(mal), min_malformed=mal[0] if mal else NONE,
               n_unsorted=len(uns), min_unsorted=uns[0] if uns else NONE,
               first_pos=pos[0] if n else 0, last_pos=pos[-1] if n else 0)
    return samples, runs, res


def loop_index(data: bytes, body_offset: int, every: int = 128):
    """(samples [POS of every ``every``-th line], contigs [(name, first line, lines, offset, end, min, max)], number of
    lines) of the whole object, or ``LoopError`` for the first offending line."""
    size = len(data)
    starts = line_starts(data, body_offset)
    samples, contigs, seen = [], [], set()
    prev = None
    for i, s in enumerate(starts):
        r = parse_line(data, s)
        if r is None:
            raise LoopError("malformed", i, s)
        chrom, pos = r
        if prev is not None and prev[0] == chrom:
            if pos < prev[1]:
                raise LoopError("unsorted", i, s)
            c = contigs[-1]
            c[2] += 1
            c[6] = pos
        else:
            if chrom in seen:
                raise LoopError("split contig", i, s)
            seen.add(chrom)
            if contigs:
                contigs[-1][4] = s
            contigs.append([chrom, i, 1, s, size, pos, pos])
        if i % every == 0:
            samples.append(pos)
        prev = r
    return samples, [tuple(c) for c in contigs], len(starts)


def samples_bytes(samples) -> bytes:
    return b"".join(int(v).to_bytes(4, "little") for v in samples)


def contigs_text(contigs) -> bytes:
    return b"".join(b"%s\t%d\t%d\t%d\t%d\t%d\t%d\n" % c for c in contigs)


def lines_of(data: bytes, body_offset: int):
    """[(start, end with terminator)] of every line."""
    st = line_starts(data, body_offset)
    return [(s, st[k + 1] if k + 1 < len(st) else len(data)) for k, s in enumerate(st)]


def loop_region(data: bytes, body_offset: int, chrom: bytes, start=None, end=None) -> bytes:
    """The lines of contig ``chrom`` with start <= POS <= end, each with its terminator, in file order."""
    out = []
    for s, e in lines_of(data, body_offset):
        c, p = parse_line(data, s)
        if c == chrom and (start is None or p >= start) and (end is None or p <= end):
            out.append(data[s:e])
    return b"".join(out)
