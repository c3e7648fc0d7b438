"""The definition of the escape-aware record index (include/dpquote.h), as the byte loop it is stated as.

The oracle of every escape test: a plain loop over the bytes, on purpose not the masks-and-carries form that the
kernel and its lane model (tools/emulate_quote.py) use.
"""
import numpy as np

NL = 10


def loop_record_ends(d, begin=0, end=None, quote=34, escape=92, carry=0, esc_carry=0, scope="all", base=0):
    """(record ends as object offsets uint64, toggles, escape state after, quote state after) of ``d[begin - base,
    end - base)``: ``d`` holds object bytes [base, base + len(d))."""
    assert scope in ("all", "quoted") and escape != quote and escape != NL
    d = bytes(memoryview(np.ascontiguousarray(np.asarray(d, np.uint8))))
    end = base + len(d) if end is None else end
    esc, inside, toggles = esc_carry, carry, 0
    ends = []
    for p in range(begin, end):
        b = d[p - base]
        if esc:                                          # an escaped byte is literal, whatever it is
            esc = 0
            if b == NL and not inside and scope == "quoted":
                ends.append(p)
            continue
        if b == escape:
            esc = 1
        elif b == quote:
            inside ^= 1
            toggles += 1
        elif b == NL and not inside:
            ends.append(p)
    return np.asarray(ends, np.uint64), toggles, esc, inside


def loop_quote_bytes(d, begin=0, end=None, quote=34, base=0):
    """The bytes == quote of the range, escaped or not (what n_quotes reports)."""
    d = np.asarray(d, np.uint8)
    end = base + len(d) if end is None else end
    return int(np.count_nonzero(d[begin - base:end - base] == quote))


def loop_newlines(d, begin=0, end=None, quote=34, escape=92, esc_carry=0, scope="all", base=0):
    """What n_newlines reports: the '\\n' bytes that can end a record -- all of them under scope "quoted", the ones
    that are not escaped under scope "all" (the loop above with the quotes ignored)."""
    d = np.asarray(d, np.uint8)
    end = base + len(d) if end is None else end
    if scope == "quoted":
        return int(np.count_nonzero(d[begin - base:end - base] == NL))
    esc, cnt = esc_carry, 0
    for b in bytes(memoryview(np.ascontiguousarray(d[begin - base:end - base]))):
        if esc:
            esc = 0
        elif b == escape:
            esc = 1
        elif b == NL:
            cnt += 1
    return cnt


def blocked(ends, begin, end):
    """(low uint16, table uint64) of sorted object offsets ``ends`` in [begin, end): the u16b form."""
    ends = np.asarray(ends, np.uint64)
    if end <= begin:
        return ends.astype(np.uint16), np.zeros(0, np.uint64)
    j0, j1 = begin >> 16, (end - 1) >> 16
    edges = (np.arange(j0, j1 + 1, dtype=np.uint64) << np.uint64(16))
    return (ends & np.uint64(0xFFFF)).astype(np.uint16), np.searchsorted(ends, edges).astype(np.uint64)
