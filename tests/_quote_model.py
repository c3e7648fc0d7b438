"""The numpy model of the quote-aware record index (include/dpquote.h): the definition the kernel is checked against."""
import numpy as np


def record_ends(d, base=0, quote=34, carry=0):
    """(offsets uint64, n_quotes, n_newlines) of bytes ``d`` holding object bytes [base, base + len(d)): a '\\n' is a
    record end iff carry + the quote bytes before it is even.  (The inclusive sum equals the exclusive one at newline
    positions; uint8 wrap-around keeps the parity bit.)"""
    d = np.asarray(d, np.uint8)
    isq = d == quote
    par = (np.uint8(carry) + np.cumsum(isq, dtype=np.uint8)) & np.uint8(1)
    nl = d == 10
    ends = np.uint64(base) + np.flatnonzero(nl & (par == 0)).astype(np.uint64)
    return ends, int(np.count_nonzero(isq)), int(np.count_nonzero(nl))
