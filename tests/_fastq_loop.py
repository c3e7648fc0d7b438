"""The definition of the FASTQ read index (include/dpfq.h) as a plain Python byte loop: the oracle of every fastq
test.  Nothing here is vectorised or shared with the package."""
import struct

KINDS = (None, "bad_header", "bad_separator", "length_mismatch")
NONE = 0xFFFFFFFFFFFFFFFF


class LoopError(Exception):
    """What the definition refuses: ``kind`` "bad_header", "bad_separator", "length_mismatch" or "truncated", at read
    ``read`` whose first line starts at byte ``offset``."""

    def __init__(self, kind, read, offset):
        super().__init__(f"{kind} at read {read} (byte {offset})")
        self.kind, self.read, self.offset = kind, read, offset


def lines_of(data: bytes):
    """[(s, e, c)] of every line: its start, the offset of its '\\n' (or size), its content length."""
    size = len(data)
    out = []
    s = 0
    while s < size:                                      # (bytes.find is the loop over the bytes up to the next '\n')
        p = data.find(b"\n", s)
        if p < 0:
            out.append((s, size))
            break
        out.append((s, p))
        s = p + 1
    return [(s, e, e - s - (1 if e > s and data[e - 1] == 13 else 0)) for s, e in out]


def read_kind(data: bytes, ln, r: int) -> int:
    """0 for a well-formed read r, else the index into KINDS of the first check that fails."""
    (s0, _, c0), (_, _, c1), (s2, _, c2), (_, _, c3) = ln[4 * r:4 * r + 4]
    if not (c0 >= 1 and data[s0] == 64):
        return 1
    if not (c2 >= 1 and data[s2] == 43):
        return 2
    if c1 != c3 or c1 >= 1 << 32:
        return 3
    return 0


def loop_index(data: bytes, every: int = 64):
    """(pairs, R, B, min_len, max_len): the stored (offset, bases) pairs with the closing one, or LoopError."""
    size = len(data)
    if size == 0:
        return [(0, 0)], 0, 0, 0, 0
    ln = lines_of(data)
    nreads = len(ln) // 4
    pairs, bases, lens = [], 0, []
    for r in range(nreads):
        k = read_kind(data, ln, r)
        if k:
            raise LoopError(KINDS[k], r, ln[4 * r][0])
        if r % every == 0:
            pairs.append((ln[4 * r][0], bases))
        bases += ln[4 * r + 1][2]
        lens.append(ln[4 * r + 1][2])
    if len(ln) % 4:
        raise LoopError("truncated", nreads, ln[4 * nreads][0])
    pairs.append((size, bases))
    return pairs, nreads, bases, min(lens, default=0), max(lens, default=0)


def index_bytes(pairs) -> bytes:
    return b"".join(struct.pack("<QQ", o, b) for o, b in pairs)


def read_ranges(data: bytes):
    """[(start, end)] of every whole read, terminators included."""
    ln = lines_of(data)
    return [(ln[4 * r][0], min(len(data), ln[4 * r + 3][1] + 1)) for r in range(len(ln) // 4)]


# ------------------------------------------------------------------------------------------------ one launch
def loop_launch(buf: bytes, base: int, size: int, starts, skip: int, n: int, last_end: int):
    """(len[], flags[]) of fq_read_kernel over ``buf`` = object bytes from ``base`` of an object of ``size`` bytes:
    read r is the entries skip + 4r .. skip + 4r + 3 of ``starts``, a line ends before the next entry and the last
    one at ``last_end``; a byte outside the buffer or at or beyond ``size`` reads as 0."""
    top = min(base + len(buf), size)

    def byte(q):
        return buf[q - base] if base <= q < top else 0

    lens, flags = [], []
    for r in range(n):
        s = list(starts[skip + 4 * r:skip + 4 * r + 4])
        s.append(starts[skip + 4 * r + 4] if r + 1 < n else last_end + 1)
        raw = [max(0, s[j + 1] - 1 - s[j]) for j in range(4)]
        c1 = raw[1] - (1 if raw[1] >= 1 and byte(s[2] - 2) == 13 else 0)
        c3 = raw[3] - (1 if raw[3] >= 1 and byte(s[4] - 2) == 13 else 0)
        if not (raw[0] >= 1 and byte(s[0]) == 64):
            f = 1
        elif not (raw[2] >= 1 and byte(s[2]) == 43):
            f = 2
        elif c1 != c3 or c1 >= 1 << 32:
            f = 3
        else:
            f = 0
        lens.append(c1 & 0xFFFFFFFF)
        flags.append(f)
    return lens, flags


def loop_result(lens, flags):
    """The result words of a launch: (malformed, max_len, bases, min_malformed, min_len)."""
    bad = [r for r, f in enumerate(flags) if f]
    return [len(bad), max(lens, default=0), sum(lens), bad[0] if bad else NONE, min(lens) if lens else NONE]


def loop_samples(starts, skip: int, lens, read0: int, every: int):
    """The (start, bases before it within the launch) pairs fq_sample_kernel writes, in slot order."""
    out, bases = [], 0
    for r, ln in enumerate(lens):
        if (read0 + r) % every == 0:
            out.append((starts[skip + 4 * r], bases))
        bases += ln
    return out
