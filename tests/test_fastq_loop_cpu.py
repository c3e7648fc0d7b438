"""The definition of the FASTQ read index (include/dpfq.h) as restated by tests/_fastq_loop.py, on hand-written
vectors: every expected value below is written out by hand, none computed."""
import struct

import pytest

import _fastq_loop as L

A = b"@a\nACGT\n+\nIIII\n"                                 # 15 bytes, 4 bases
B = b"@b x\nAC\n+b x\n#!\n"                               # 16 bytes, 2 bases
Z = b"@\n\n+\n\n"                                          # 6 bytes, a read of zero bases


def err(data, every=64):
    with pytest.raises(L.LoopError) as e:
        L.loop_index(data, every)
    return e.value.kind, e.value.read, e.value.offset


def test_lines_and_terminators():
    assert L.lines_of(b"") == []
    assert L.lines_of(b"ab\ncd") == [(0, 2, 2), (3, 5, 2)]                 # an unterminated last line is a line
    assert L.lines_of(b"ab\ncd\n") == [(0, 2, 2), (3, 5, 2)]               # '\n' as the last byte: no line follows
    assert L.lines_of(b"ab\r\n\r\n\n\rc\n") == [(0, 3, 2), (4, 5, 0), (6, 6, 0), (7, 9, 2)]   # only a final '\r' goes
    assert L.lines_of(b"\n") == [(0, 0, 0)] and L.lines_of(b"x\r") == [(0, 2, 1)]


def test_well_formed_objects_and_the_final_newline():
    assert L.loop_index(A + B, 1) == ([(0, 0), (15, 4), (31, 6)], 2, 6, 2, 4)
    assert L.loop_index((A + B)[:-1], 1) == ([(0, 0), (15, 4), (30, 6)], 2, 6, 2, 4)     # without the final '\n'
    assert L.loop_index(b"", 64) == ([(0, 0)], 0, 0, 0, 0)                 # an empty object: the single pair
    assert L.index_bytes([(0, 0), (15, 4)]) == struct.pack("<4Q", 0, 0, 15, 4)


def test_crlf_and_mixed_endings():
    crlf = (A + B).replace(b"\n", b"\r\n")
    assert L.loop_index(crlf, 1) == ([(0, 0), (19, 4), (39, 6)], 2, 6, 2, 4)
    mixed = b"@a\r\nACGT\n+\r\nIIII\r\n"                                   # the sequence line alone ends in a bare '\n'
    assert L.loop_index(mixed, 1) == ([(0, 0), (18, 4)], 1, 4, 4, 4)
    assert L.loop_index(b"@a\nACGT\r\n+\nIIII", 1)[2] == 4                 # ... and the other way round, unterminated
    assert err(b"@a\nACG\r\n+\nIIII\n") == ("length_mismatch", 0, 0)        # the '\r' is not a base
    assert err(b"\r\nAC\n+\nII\n") == ("bad_header", 0, 0)                 # a line of '\r' alone is empty


def test_each_error_kind_and_their_order_within_a_read():
    assert err(A + b"a\nAC\n+\nII\n") == ("bad_header", 1, 15)
    assert err(A + b"\nAC\n+\nII\n") == ("bad_header", 1, 15)              # an empty header line
    assert err(A + b"@b\nAC\n-\nII\n") == ("bad_separator", 1, 15)
    assert err(A + b"@b\nAC\n\nII\n") == ("bad_separator", 1, 15)
    assert err(A + b"@b\nAC\n+\nIII\n") == ("length_mismatch", 1, 15)
    assert err(b"b\nAC\n-\nIII\n") == ("bad_header", 0, 0)                 # all three fail: the header is named
    assert err(b"@b\nAC\n-\nIII\n") == ("bad_separator", 0, 0)             # the separator before the lengths
    assert L.loop_index(b"@b\nAC\n+ anything @ here\n+@\n", 1)[1:3] == (1, 2)    # nothing behind the '+' is looked at


def test_truncation_and_what_comes_before_it():
    assert err(A + b"@b\nAC\n+\n") == ("truncated", 1, 15)
    assert err(A + b"@b") == ("truncated", 1, 15)
    assert err(b"@b\nAC\n") == ("truncated", 0, 0)
    assert err(A + B + b"\n") == ("truncated", 2, 31)                      # a trailing blank line
    assert err(b"@a\nACGT\n+\nIII\n" + b"@b\nAC\n") == ("length_mismatch", 0, 0)   # a malformed read comes first
    assert err(A + b"b\nAC\n+\nII\n" + b"@c\n") == ("bad_header", 1, 15)
    # wrapped FASTQ is not supported: its second sequence line is taken for the separator
    assert err(b"@w\nACGT\nACGT\n+\nIIII\nIIII\n") == ("bad_separator", 0, 0)


def test_a_quality_line_that_begins_with_at_is_harmless():
    data = b"@a\nACGT\n+\n@III\n" + b"@b\nAC\n+\n@+\n"
    assert L.loop_index(data, 1) == ([(0, 0), (15, 4), (26, 6)], 2, 6, 2, 4)   # 15 + 11 bytes


def test_zero_length_reads():
    assert L.loop_index(Z + Z + A, 1) == ([(0, 0), (6, 0), (12, 0), (27, 4)], 3, 4, 0, 4)
    assert L.loop_index(Z, 64) == ([(0, 0), (6, 0)], 1, 0, 0, 0)
    assert L.loop_index(b"@z\r\n\r\n+\r\n\r\n", 1) == ([(0, 0), (11, 0)], 1, 0, 0, 0)


@pytest.mark.parametrize("every, want", [
    (1, [(0, 0), (15, 4), (31, 6), (37, 6), (52, 10), (68, 12)]),
    (2, [(0, 0), (31, 6), (52, 10), (68, 12)]),
    (64, [(0, 0), (68, 12)]),                                              # K > R: read 0 and the closing pair
])
def test_stored_pairs(every, want):
    data = A + B + Z + A + B                                               # reads at 0, 15, 31, 37, 52; 68 bytes
    assert L.loop_index(data, every) == (want, 5, 12, 0, 4)
    assert L.index_bytes(want) == b"".join(struct.pack("<QQ", *p) for p in want)
    assert L.read_ranges(data) == [(0, 15), (15, 31), (31, 37), (37, 52), (52, 68)]


def test_the_launch_model_reads_zero_outside_the_buffer():
    data = A + B
    starts = [0, 3, 8, 10, 15, 20, 23, 28]
    assert L.loop_launch(data, 0, len(data), starts, 0, 2, 30) == ([4, 2], [0, 0])
    assert L.loop_launch(data[15:], 15, len(data), starts, 0, 2, 30) == ([4, 2], [1, 0])   # read 0 lies before it
    assert L.loop_launch(data, 0, 28, starts, 0, 2, 30) == ([4, 2], [0, 0])               # only '!' lies beyond size
    assert L.loop_launch(data, 0, len(data), starts, 0, 2, 29) == ([4, 2], [0, 3])         # a short last line
    assert L.loop_result([4, 2], [0, 3]) == [1, 4, 6, 1, 2] and L.loop_result([], []) == [0, 0, 0, L.NONE, L.NONE]
    assert L.loop_samples(starts, 0, [4, 2], 3, 2) == [(15, 4)] and L.loop_samples(starts, 0, [4, 2], 4, 1) == [(0, 0), (15, 4)]
