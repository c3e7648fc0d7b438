"""Hand-written VCF lines for the record-end definition (include/dpvspan.h), shared by the loop's CPU test and the
kernels' GPU test: ``CASES`` is a list of (name, line bytes, POS, expected rec_end, expected flags).  A line carries
its own terminator where it has one."""
MISSING_REF, TRUNCATED, FROM_END = 1, 2, 4


def line(pos, ref=b"A", info=b"NS=3", tail=b"\tGT\t0|1\n", chrom=b"chr1"):
    """A line of 8 fields plus ``tail`` (which starts with the tab that ends INFO, or is the terminator alone)."""
    return chrom + b"\t%d\trs1\t" % pos + ref + b"\tC\t9\tPASS\t" + info + tail


BIG_REF = b"ACGT" * 17_500                                   # 70,000 bytes

CASES = [
    # where the END entry may stand
    ("end first", line(100, info=b"END=250;NS=3"), 100, 250, FROM_END),
    ("end after semicolon", line(100, info=b"NS=3;END=250;DP=4"), 100, 250, FROM_END),
    ("end last, tab ends it", line(100, info=b"NS=3;END=250"), 100, 250, FROM_END),
    ("end last, newline ends it", line(100, info=b"NS=3;END=250", tail=b"\n"), 100, 250, FROM_END),
    ("end last, size ends it", line(100, info=b"NS=3;END=250", tail=b""), 100, 250, FROM_END),
    ("end alone", line(100, info=b"END=250", tail=b"\n"), 100, 250, FROM_END),
    # decoys
    ("CIEND before END", line(100, info=b"CIEND=1,2;END=300"), 100, 300, FROM_END),
    ("XEND before END", line(100, info=b"XEND=999;END=300"), 100, 300, FROM_END),
    ("only decoys", line(100, b"ACG", info=b"CIEND=900;XEND=999;ENDX=5;EN=7"), 100, 102, 0),
    ("END without equals", line(100, b"AC", info=b"END;END=400"), 100, 400, FROM_END),
    # values that do not count
    ("END=.", line(100, b"ACGT", info=b"END=."), 100, 103, 0),
    ("END= empty", line(100, b"ACGT", info=b"END=;NS=3"), 100, 103, 0),
    ("END= empty at the line's end", line(100, b"ACGT", info=b"END=", tail=b"\n"), 100, 103, 0),
    ("eleven digits", line(100, b"AC", info=b"END=00000000250"), 100, 101, 0),
    ("ten digits with zeros", line(100, b"AC", info=b"END=0000000250"), 100, 250, FROM_END),
    ("2^31 - 1 counts", line(100, info=b"END=2147483647"), 100, 2**31 - 1, FROM_END),
    ("2^31 does not", line(100, b"ACG", info=b"END=2147483648"), 100, 102, 0),
    ("9999999999 does not", line(100, b"ACG", info=b"END=9999999999"), 100, 102, 0),
    ("END = POS counts", line(100, b"ACG", info=b"END=100"), 100, 100, FROM_END),
    ("END = POS - 1 does not", line(100, b"ACG", info=b"END=99"), 100, 102, 0),
    ("a non-digit", line(100, b"ACG", info=b"END=25x"), 100, 102, 0),
    ("a sign", line(100, b"ACG", info=b"END=+250"), 100, 102, 0),
    ("two ENDs, the first counts", line(100, info=b"END=250;END=900"), 100, 250, FROM_END),
    ("two ENDs, the first does not", line(100, b"ACG", info=b"END=.;END=900"), 100, 102, 0),
    # the number of fields
    ("4 fields", b"chr1\t100\trs1\tACGTA\n", 100, 104, 0),
    ("4 fields, unterminated", b"chr1\t100\trs1\tACGTA", 100, 104, 0),
    ("5 fields", b"chr1\t100\trs1\tACGTA\tC\n", 100, 104, 0),
    ("7 fields: END= in FILTER is no INFO", b"chr1\t100\trs1\tAC\tC\t9\tEND=900\n", 100, 101, 0),
    ("8 fields", line(100, b"ACG", tail=b"\n"), 100, 102, 0),
    ("END= in FORMAT is not INFO", line(100, b"AC", info=b"NS=3", tail=b"\tEND=900\n"), 100, 101, 0),
    ("3 fields", b"chr1\t100\trs1\n", 100, 0, MISSING_REF),
    ("2 fields and a tab", b"chr1\t100\t\n", 100, 0, MISSING_REF),
    ("empty REF", line(100, b"", info=b"END=900"), 100, 0, MISSING_REF),
    ("empty REF as the last field", b"chr1\t100\trs1\t\n", 100, 0, MISSING_REF),
    # REF lengths
    ("REF of 1", line(2147483647, b"A"), 2147483647, 2147483647, 0),
    ("REF of 2", line(2147483647, b"AC"), 2147483647, 2147483648, 0),
    ("REF of 70,000", line(7, BIG_REF, info=b"NS=3;DP=9"), 7, 70_006, 0),
    ("REF of 70,000 and END", line(7, BIG_REF, info=b"NS=3;END=80000"), 7, 80_000, FROM_END),
    # any byte value in INFO
    ("high bytes in INFO", line(100, b"AC", info=b"N\xc3\xa9=\x80\xff;END=250;Z=\xfe"), 100, 250, FROM_END),
    ("high byte in the value", line(100, b"AC", info=b"END=25\xb0"), 100, 101, 0),
    # CRLF: the '\r' belongs to the last field
    ("CRLF behind INFO's END", line(100, b"ACG", info=b"END=250", tail=b"\r\n"), 100, 102, 0),
    ("CRLF behind a later field", line(100, b"ACG", info=b"END=250", tail=b"\tGT\t0|1\r\n"), 100, 250, FROM_END),
    ("CRLF behind REF as the last field", b"chr1\t100\trs1\tACG\r\n", 100, 103, 0),
]
