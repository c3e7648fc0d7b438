"""Seeded synthetic objects for tests and the benchmark (FASTA / CSV / VCF / FASTQ).

Every generator returns a ``numpy.uint8`` array of EXACTLY the requested size (or read count) and
is deterministic for a given ``seed`` on a given numpy version (tests pin the bytes with a sha256).
The shapes follow the reference's sample data and BASELINE.json configs:

* FASTA: ``>seq{i} synthetic record len={L}\\n`` headers, L uniform in [1000, 3000), 60-column
  ACGT lines.  The object never ends inside a header line, so the reference's
  uint32 index stays defined at exactly 4 GiB.
* CSV:   cities.csv row shape (10 columns, ``int,int,int,N,int,int,int,W,City,ST\\n``).
* VCF:   a VCFv4 header + 12 tab-separated columns per row.
* FASTQ: 4-line reads, ``@id / SEQ / + / QUAL``, fixed read length.

Large objects are built by :func:`tile_plan`: one seeded base block of a length that is NOT a power
of two, repeated, so that kernel tile boundaries fall at a different phase in every copy.
"""
from __future__ import annotations

import hashlib

import numpy as np

_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
_QUAL = np.frombuffer(b"!#$%&'()*+,-./0123456789:;<=>?@ABCDEFGHIJ", dtype=np.uint8)


def sha256(a) -> str:
    return hashlib.sha256(memoryview(np.ascontiguousarray(a)).cast("B")).hexdigest()


def _scatter_strings(out: np.ndarray, starts: np.ndarray, blob: np.ndarray, lens: np.ndarray) -> None:
    """out[starts[i] : starts[i]+lens[i]] = i-th string of the concatenated ``blob``."""
    if len(lens) == 0:
        return
    seg_start = np.repeat(starts - np.concatenate(([0], np.cumsum(lens)[:-1])), lens)
    idx = seg_start + np.arange(int(lens.sum()), dtype=np.int64)
    out[idx] = blob


def fasta(size: int, seed: int = 0, line_width: int = 60, seq_min: int = 1000, seq_max: int = 3000,
          first_id: int = 0) -> np.ndarray:
    """A FASTA object of exactly ``size`` bytes."""
    if size <= 0:
        return np.zeros(0, np.uint8)
    rng = np.random.default_rng(seed)
    avg = 40 + (seq_min + seq_max) / 2 * (1 + 1 / line_width)
    n = int(size / avg * 1.1) + 4
    L = rng.integers(seq_min, seq_max, n).astype(np.int64)
    headers = [f">seq{first_id + i} synthetic record len={int(l)}\n".encode() for i, l in enumerate(L)]
    hl = np.fromiter((len(h) for h in headers), dtype=np.int64, count=n)
    nlines = (L + line_width - 1) // line_width
    rec = hl + L + nlines
    ends = np.cumsum(rec)
    n = int(np.searchsorted(ends, size)) + 1            # records needed to cover ``size``
    L, hl, nlines, rec = L[:n], hl[:n], nlines[:n], rec[:n]
    total = int(rec.sum())
    starts = np.concatenate(([0], np.cumsum(rec)[:-1]))
    out = _ACGT[rng.integers(0, 4, total, dtype=np.uint8)]
    _scatter_strings(out, starts, np.frombuffer(b"".join(headers[:n]), np.uint8), hl)
    # newline after every ``line_width`` bases and after the last (partial) line of each record
    body = starts + hl
    k = np.arange(int(nlines.sum()), dtype=np.int64) - np.repeat(np.cumsum(nlines) - nlines, nlines)
    nl = np.repeat(body, nlines) + np.minimum((k + 1) * (line_width + 1) - 1,
                                              np.repeat(L + nlines - 1, nlines))
    out[nl] = 10
    out = out[:size].copy()
    _fix_fasta_tail(out)
    return out


def _fix_fasta_tail(a: np.ndarray) -> None:
    """Never end inside a header line (keeps every reference ``end`` < size, i.e. uint32-safe)."""
    nls = np.flatnonzero(a == 10)
    tail0 = int(nls[-1]) + 1 if len(nls) else 0
    if tail0 < len(a) and (a[tail0:] == ord(">")).any():
        a[tail0:] = ord("N")


_CITIES = [b"Youngstown,OH", b"Yankton,SD", b"Yakima,WA", b"Worcester,MA", b"Wisconsin Dells,WI",
           b"Winston-Salem,NC", b"Wilmington,DE", b"Williston,ND", b"Wichita Falls,TX", b"Wheeling,WV",
           b"Waterloo,IA", b"Salt Lake City,UT", b"San Antonio,TX", b"Sacramento,CA", b"Ravenna,OH"]
CSV_HEADER = b"LatD,LatM,LatS,NS,LonD,LonM,LonS,EW,City,State\n"


def csv(size: int, seed: int = 0) -> np.ndarray:
    """A cities.csv-shaped CSV object of exactly ``size`` bytes (ends with ``\\n``)."""
    rng = np.random.default_rng(seed)
    rows = [CSV_HEADER]
    total = len(CSV_HEADER)
    while total < size:
        m = 4096
        v = rng.integers(0, 60, (m, 6))
        ci = rng.integers(0, len(_CITIES), m)
        for j in range(m):
            r = b"%d,%d,%d,N,%d,%d,%d,W,%s\n" % (v[j, 0] % 50 + 25, v[j, 1], v[j, 2], v[j, 3] + 60,
                                                  v[j, 4], v[j, 5], _CITIES[ci[j]])
            rows.append(r)
            total += len(r)
    out = np.frombuffer(b"".join(rows), np.uint8)[:size].copy()
    if size:
        out[-1] = 10
    return out


def csv_wide(size: int, seed: int = 0, max_note: int = 1500) -> np.ndarray:
    """``csv`` rows with an 11th column ``Note`` of 0..max_note ASCII characters: rows longer than the
    reference's default slice padding (256 B), which reach CSVSlice.get's buffer expansion (csv.py:81-94)."""
    base = csv(size, seed).tobytes().split(b"\n")[1:-1]
    rng = np.random.default_rng(seed + 1)
    rows = [CSV_HEADER[:-1] + b",Note\n"]
    total = len(rows[0])
    i = 0
    while total < size:
        r = base[i % len(base)] + b"," + b"n" * int(rng.integers(0, max_note + 1)) + b"\n"
        rows.append(r)
        total += len(r)
        i += 1
    out = np.frombuffer(b"".join(rows), np.uint8)[:size].copy()
    if size:
        out[-1] = 10
    return out


_NOTES = [b"checked", b"two lines\nhere", b"a, b and c", b'called ""the falls""', b"\n", b'""', b",", b"moved\n\nsee above",
          b'""quoted"" start', b"ends with a break\n", b"plain text"]


def csv_quoted(size: int, seed: int = 0) -> np.ndarray:
    """``csv`` rows with an 11th column ``Note``: empty, plain, or RFC 4180 quoted text holding line breaks, commas
    and escaped quotes (``""``).  Exactly ``size`` bytes, valid RFC 4180, deterministic, ends with a record end (the
    last row's note is padded to fit)."""
    return _csv_noted(size, seed, _NOTES, "csv_quoted")


# the notes of csv_quoted in the dialect that escapes: \" for a quote, \\ for the escape byte itself
_NOTES_ESCAPED = [n.replace(b'""', b'\\"') for n in _NOTES] + [b"a back\\\\slash", b"C:\\\\dir\\\\", b"odd \\\\\\\"run"]


def csv_escaped(size: int, seed: int = 0) -> np.ndarray:
    """``csv_quoted`` in the dialect of Spark, Hive and ``csv.writer(escapechar='\\\\', doublequote=False)``: a quote
    inside a quoted note is written ``\\"`` and a backslash ``\\\\`` (some notes end in one, right before the closing
    quote).  Exactly ``size`` bytes, deterministic, ends with a record end."""
    return _csv_noted(size, seed, _NOTES_ESCAPED, "csv_escaped")


def _csv_noted(size: int, seed: int, notes, name: str) -> np.ndarray:
    head = CSV_HEADER[:-1] + b",Note\n"
    if size < len(head) + 128:
        raise ValueError(f"{name} needs at least {len(head) + 128} bytes")
    rng = np.random.default_rng(seed)
    rows = [head]
    total = len(head)
    while True:
        m = 4096
        v = rng.integers(0, 60, (m, 6))
        ci = rng.integers(0, len(_CITIES), m)
        kind = rng.integers(0, 4, m)                      # 0 empty, 1 plain, 2-3 quoted
        nfrag = rng.integers(1, 5, m)
        frag = rng.integers(0, len(notes), (m, 4))
        for j in range(m):
            base = b"%d,%d,%d,N,%d,%d,%d,W,%s," % (v[j, 0] % 50 + 25, v[j, 1], v[j, 2], v[j, 3] + 60, v[j, 4], v[j, 5],
                                                   _CITIES[ci[j]])
            if kind[j] == 0:
                note = b""
            elif kind[j] == 1:
                note = b"plain note"
            else:
                note = b'"' + b" ".join(notes[f] for f in frag[j, :nfrag[j]]) + b'"'
            r = base + note + b"\n"
            if size - total - len(r) < 128:               # the last row: a quoted note padded to the exact size
                rows.append(base + b'"' + b"x" * (size - total - len(base) - 3) + b'"\n')
                return np.frombuffer(b"".join(rows), np.uint8).copy()
            rows.append(r)
            total += len(r)


VCF_HEADER = (b"##fileformat=VCFv4.2\n"
              b"##source=dataplug_amd.synth\n"
              b"##INFO=<ID=NS,Number=1,Type=Integer,Description=\"Samples With Data\">\n"
              b"##INFO=<ID=DP,Number=1,Type=Integer,Description=\"Total Depth\">\n"
              b"##INFO=<ID=AF,Number=A,Type=Float,Description=\"Allele Frequency\">\n"
              b"##FILTER=<ID=q10,Description=\"Quality below 10\">\n"
              b"##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\">\n"
              b"##FORMAT=<ID=GQ,Number=1,Type=Integer,Description=\"Genotype Quality\">\n"
              b"#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS1\tS2\tS3\n")


def vcf(size: int, seed: int = 0) -> np.ndarray:
    """A VCF object of exactly ``size`` bytes: header + 12-column rows (ends with ``\\n``)."""
    rng = np.random.default_rng(seed)
    rows = [VCF_HEADER]
    total = len(VCF_HEADER)
    pos = 1000
    gts = [b"0|0", b"0|1", b"1|0", b"1/1", b"./."]
    while total < size:
        m = 4096
        v = rng.integers(0, 1 << 30, (m, 8))
        for j in range(m):
            pos += int(v[j, 0] % 500) + 1
            r = b"%d\t%d\trs%d\t%c\t%c\t%d\tPASS\tNS=3;DP=%d;AF=0.%d\tGT:GQ\t%s:%d\t%s:%d\t%s:%d\n" % (
                int(v[j, 1] % 22) + 1, pos, int(v[j, 2] % 10**7), b"ACGT"[v[j, 3] % 4], b"ACGT"[v[j, 4] % 4],
                int(v[j, 5] % 99), int(v[j, 6] % 40), int(v[j, 7] % 1000),
                gts[v[j, 1] % 5], int(v[j, 2] % 60), gts[v[j, 3] % 5], int(v[j, 4] % 60),
                gts[v[j, 5] % 5], int(v[j, 6] % 60))
            rows.append(r)
            total += len(r)
    out = np.frombuffer(b"".join(rows), np.uint8)[:size].copy()
    if size:
        out[-1] = 10
    return out


def vcf_wide(size: int, seed: int = 0, max_info: int = 1500) -> np.ndarray:
    """``vcf`` rows whose INFO field carries an extra ``NOTE=`` of 0..max_info characters: rows longer than
    the slice padding, which reach VCFSlice.get's range expansion (vcf.py:117-136)."""
    base = vcf(size, seed).tobytes()
    head_end = base.index(b"\n#CHROM") + 1
    head_end = base.index(b"\n", head_end) + 1
    body = base[head_end:].split(b"\n")[:-1]
    rng = np.random.default_rng(seed + 1)
    rows = [base[:head_end]]
    total = len(rows[0])
    i = 0
    while total < size:
        f = body[i % len(body)].split(b"\t")
        if len(f) >= 8:
            f[7] = f[7] + b";NOTE=" + b"v" * int(rng.integers(0, max_info + 1))
        r = b"\t".join(f) + b"\n"
        rows.append(r)
        total += len(r)
        i += 1
    out = np.frombuffer(b"".join(rows), np.uint8)[:size].copy()
    if size:
        out[-1] = 10
    return out


def vcf_sorted(size: int, seed: int = 0, contigs: int = 8, block: int = 4 * 2**20 - 333) -> np.ndarray:
    """A position-sorted VCF of exactly ``size`` bytes: ``vcf``'s header and row shape, but CHROM is constant within
    a block of rows (``chr1``, ``chr2``, ... in order, about ``(size - header) / contigs`` bytes each) and POS never
    decreases within a contig (about one row in eight repeats its neighbour's) and restarts at each contig.

    Each contig is one seeded tile of rows repeated: POS is written as nine digits, the copy's number in the first
    three (leading zeros) and the tile's own ascending six-digit position behind them, so a copy is the tile's bytes
    with three digits per row patched.  The last row's last field is padded to the exact size; ends with ``\\n``."""
    body = size - len(VCF_HEADER)
    share = body // max(1, contigs)
    if contigs < 1 or share < 256:
        raise ValueError(f"vcf_sorted needs at least {len(VCF_HEADER) + 256 * max(1, contigs)} bytes")
    tile_bytes = max(min(block, share), share // 900 + 1)
    if tile_bytes > 32 << 20:
        raise ValueError("vcf_sorted: a contig of this size needs more than 999 copies of a 32 MiB tile")
    rng = np.random.default_rng(seed)
    m = tile_bytes // 48 + 8                                  # more rows than the tile can hold (a row has >= 48 bytes)
    v = rng.integers(0, 1 << 30, (m, 8))
    top = max(2, min(37, 999_999 // m))
    rel = np.cumsum(np.where(v[:, 1] % 8 == 0, 0, v[:, 0] % top))
    gts = [b"0|0", b"0|1", b"1|0", b"1/1", b"./."]
    tails = [b"%06d\trs%d\t%c\t%c\t%d\tPASS\tNS=3;DP=%d;AF=0.%d\tGT:GQ\t%s:%d\t%s:%d\t%s:%d\n" % (
        int(rel[j]), int(v[j, 2] % 10**7), b"ACGT"[v[j, 3] % 4], b"ACGT"[v[j, 4] % 4], int(v[j, 5] % 99),
        int(v[j, 6] % 40), int(v[j, 7] % 1000), gts[v[j, 1] % 5], int(v[j, 2] % 60), gts[v[j, 3] % 5],
        int(v[j, 4] % 60), gts[v[j, 5] % 5], int(v[j, 6] % 60)) for j in range(m)]
    tlen = np.fromiter((len(t) for t in tails), np.int64, m)
    out = np.empty(size, np.uint8)
    out[:len(VCF_HEADER)] = np.frombuffer(VCF_HEADER, np.uint8)
    p = len(VCF_HEADER)
    for c in range(contigs):
        pre = b"chr%d\t000" % (c + 1)
        ends = np.cumsum(tlen + len(pre))
        nrows = max(1, int(np.searchsorted(ends, tile_bytes, "right")))
        tile = np.frombuffer(b"".join(pre + t for t in tails[:nrows]), np.uint8)
        digit0 = np.concatenate(([0], ends[:nrows - 1])) + len(pre) - 3          # each row's copy digits in the tile
        limit = size if c == contigs - 1 else len(VCF_HEADER) + share * (c + 1)
        k = 0
        while p < limit:
            nr = nrows if p + len(tile) <= limit else int(np.searchsorted(ends[:nrows], limit - p, "right"))
            if nr == 0:
                break
            n = int(ends[nr - 1])
            out[p:p + n] = tile[:n]
            for d, ch in enumerate(b"%03d" % k):
                out[p + digit0[:nr] + d] = ch
            p += n
            k += 1
    out[p - 1:size - 1] = ord("x")                            # the last row's last field padded to the exact size
    out[size - 1] = 10
    return out


def gvcf(size: int, seed: int = 0, contigs: int = 8, block: int = 4 * 2**20 - 333,
         del_every: int = 5000) -> np.ndarray:
    """A position-sorted gVCF of exactly ``size`` bytes: ``vcf``'s header, one sample column, CHROM constant within a
    block of rows (``chr1``, ``chr2``, ... in order) and POS never decreasing within a contig.  About seven rows in
    ten are reference blocks (``<NON_REF>``, ``END=`` one base in front of the next row's POS), two are SNVs, one is a
    deletion with a REF of 2 to 60 bases, and about one row in ``del_every`` (5,000) is a ``<DEL>`` whose ``END=``
    (behind ``SVTYPE=DEL;``) lies 10^4 to 10^6 beyond its POS.

    Each contig is one seeded tile of rows repeated, as in ``vcf_sorted``: POS and END are written as ten digits, the
    copy's number in the first three and the tile's own seven-digit position behind them, so a copy is the tile's
    bytes with three digits patched per number.  The last row's last field is padded to the exact size; ends with
    ``\\n``."""
    body = size - len(VCF_HEADER)
    share = body // max(1, contigs)
    if contigs < 1 or share < 512:
        raise ValueError(f"gvcf needs at least {len(VCF_HEADER) + 512 * max(1, contigs)} bytes")
    tile_bytes = max(min(block, share), share // 200 + 1)
    if tile_bytes > 32 << 20:
        raise ValueError("gvcf: a contig of this size needs more than 200 copies of a 32 MiB tile")
    rng = np.random.default_rng(seed)
    m = tile_bytes // 40 + 8                                  # more rows than the tile can hold (a row has >= 40 bytes)
    v = rng.integers(0, 1 << 30, (m, 6))
    top = max(2, min(200, 8_900_000 // m))
    step = 1 + v[:, 0] % top                                  # the distance to the next row's POS
    rel = np.concatenate(([1], 1 + np.cumsum(step)[:-1]))
    bases = b"ACGT"
    rows, patches = [], []                                    # per row: its bytes behind "chrN\t000", and the offsets
    for j in range(m):                                        # of the copy digits of its END (if it has one)
        kind, r = int(v[j, 1] % 10), int(rel[j])
        ref = bases[v[j, 2] % 4:v[j, 2] % 4 + 1]
        gq = int(v[j, 3] % 99)
        if v[j, 4] % del_every == 0:
            head = b"%07d\t.\t%s\t<DEL>\t%d\tPASS\tSVTYPE=DEL;END=" % (r, ref, gq)
            tail = b"000%07d;SVLEN=-1\tGT:GQ\t0/1:%d\n" % (r + 10**4 + int(v[j, 5] % (10**6 - 10**4 + 1)), gq)
        elif kind < 7:
            head = b"%07d\t.\t%s\t<NON_REF>\t.\t.\tEND=" % (r, ref)
            tail = b"000%07d\tGT:DP:GQ\t0/0:%d:%d\n" % (r + int(step[j]) - 1, int(v[j, 5] % 60), gq)
        elif kind < 9:
            head = b"%07d\trs%d\t%s\t%s,<NON_REF>\t%d\tPASS\tDP=%d;AF=0.%d\tGT:GQ\t0/1:%d\n" % (
                r, int(v[j, 5] % 10**7), ref, bases[(v[j, 2] + 1) % 4:(v[j, 2] + 1) % 4 + 1], gq, int(v[j, 3] % 40),
                int(v[j, 5] % 1000), gq)
            tail = None
        else:
            n = 2 + int(v[j, 5] % 59)
            head = b"%07d\t.\t%s\t%s\t%d\tPASS\tDP=%d\tGT:GQ\t1/1:%d\n" % (
                r, (bases * 16)[v[j, 2] % 4:v[j, 2] % 4 + n], ref, gq, int(v[j, 3] % 40), gq)
            tail = None
        patches.append(len(head) if tail is not None else -1)
        rows.append(head + (tail or b""))
    tlen = np.fromiter((len(t) for t in rows), np.int64, m)
    end_at = np.asarray(patches, np.int64)
    out = np.empty(size, np.uint8)
    out[:len(VCF_HEADER)] = np.frombuffer(VCF_HEADER, np.uint8)
    p = len(VCF_HEADER)
    for c in range(contigs):
        pre = b"chr%d\t000" % (c + 1)
        ends = np.cumsum(tlen + len(pre))
        nrows = max(1, int(np.searchsorted(ends, tile_bytes, "right")))
        tile = np.frombuffer(b"".join(pre + t for t in rows[:nrows]), np.uint8)
        row0 = np.concatenate(([0], ends[:nrows - 1]))
        digit0 = row0 + len(pre) - 3                          # each row's copy digits of POS in the tile
        has = end_at[:nrows] >= 0
        digit1 = (row0 + len(pre) + end_at[:nrows])[has]      # and of END, for the rows that have one
        rows_with = np.flatnonzero(has)
        limit = size if c == contigs - 1 else len(VCF_HEADER) + share * (c + 1)
        k = 0
        while p < limit:
            nr = nrows if p + len(tile) <= limit else int(np.searchsorted(ends[:nrows], limit - p, "right"))
            if nr == 0:
                break
            if k > 213:
                raise ValueError("gvcf: more than 214 copies of a tile in one contig")
            n = int(ends[nr - 1])
            out[p:p + n] = tile[:n]
            d1 = digit1[:int(np.searchsorted(rows_with, nr, "left"))]
            for d, ch in enumerate(b"%03d" % k):
                out[p + digit0[:nr] + d] = ch
                out[p + d1 + d] = ch
            p += n
            k += 1
    out[p - 1:size - 1] = ord("x")                            # the last row's last field padded to the exact size
    out[size - 1] = 10
    return out


def fastq(n_reads: int, seed: int = 0, read_len: int = 100) -> np.ndarray:
    """``n_reads`` 4-line FASTQ reads (inflated stream)."""
    rng = np.random.default_rng(seed)
    ids = [b"@read%d synthetic/1\n" % i for i in range(n_reads)]
    il = np.fromiter((len(h) for h in ids), np.int64, count=n_reads)
    rec = il + (read_len + 1) + 2 + (read_len + 1)
    starts = np.concatenate(([0], np.cumsum(rec)[:-1])).astype(np.int64)
    total = int(rec.sum())
    out = np.empty(total, np.uint8)
    _scatter_strings(out, starts, np.frombuffer(b"".join(ids), np.uint8), il)
    seq0 = starts + il
    j = np.arange(read_len, dtype=np.int64)
    out[(seq0[:, None] + j).ravel()] = _ACGT[rng.integers(0, 4, n_reads * read_len, dtype=np.uint8)]
    out[seq0 + read_len] = 10
    out[seq0 + read_len + 1] = ord("+")
    out[seq0 + read_len + 2] = 10
    q0 = seq0 + read_len + 3
    out[(q0[:, None] + j).ravel()] = _QUAL[rng.integers(0, len(_QUAL), n_reads * read_len, dtype=np.uint8)]
    out[q0 + read_len] = 10
    return out


def fastq_long(n_reads: int, seed: int = 0, len_min: int = 100, len_max: int = 100_000, crlf: bool = False) -> np.ndarray:
    """``n_reads`` 4-line FASTQ reads with long-read lengths: log-uniform in [len_min, len_max], as ONT and PacBio runs
    spread over orders of magnitude.  ``@read{i} long/1`` headers, a bare ``+``; ``crlf`` ends every line ``\\r\\n``."""
    rng = np.random.default_rng(seed)
    eol = 2 if crlf else 1
    L = np.exp(rng.uniform(np.log(len_min), np.log(len_max + 1), n_reads)).astype(np.int64)
    L = np.clip(L, len_min, len_max)
    ids = [b"@read%d long/1" % i for i in range(n_reads)]
    il = np.fromiter((len(h) for h in ids), np.int64, count=n_reads)
    rec = il + L + 1 + L + 4 * eol
    starts = np.concatenate(([0], np.cumsum(rec)[:-1])).astype(np.int64)
    total = int(rec.sum())
    out = np.empty(total, np.uint8)
    if total == 0:
        return out
    pick = rng.integers(0, 256, total, dtype=np.uint8)
    out[:] = _QUAL[pick % len(_QUAL)]                            # the quality bytes; the rest is written over them
    _scatter_strings(out, starts, np.frombuffer(b"".join(ids), np.uint8), il)
    seq0 = starts + il + eol
    seq = np.repeat(seq0 - np.concatenate(([0], np.cumsum(L)[:-1])), L) + np.arange(int(L.sum()), dtype=np.int64)
    out[seq] = _ACGT[pick[:len(seq)] & 3]
    plus = seq0 + L + eol
    out[plus] = ord("+")
    ends = np.stack([starts + il, seq0 + L, plus + 1, plus + 1 + eol + L])      # each line's first terminator byte
    if crlf:
        out[ends] = 13
        out[ends + 1] = 10
    else:
        out[ends] = 10
    return out


def tile_plan(block_len: int, size: int):
    """Copies of a base block that fill ``size`` bytes: list of (dst_offset, length)."""
    plan, off = [], 0
    while off < size:
        n = min(block_len, size - off)
        plan.append((off, n))
        off += n
    return plan


def tiled_fasta_host(size: int, seed: int = 0, block: int = 64 * 2**20 - 4099) -> np.ndarray:
    """Host-side FASTA of exactly ``size`` bytes made of repeated seeded blocks (tail-fixed)."""
    base = fasta(min(block, size), seed)
    out = np.empty(size, np.uint8)
    for off, n in tile_plan(len(base), size):
        out[off:off + n] = base[:n]
    _fix_fasta_tail(out)
    return out


class TiledFasta:
    """``tiled_fasta_host(size, seed)`` without materializing it: any byte range on demand.

    The multi-GPU benchmark indexes ONE object of N x 4 GiB whose chunk groups live on different GPUs; each
    worker builds only the bytes of its own group (plus the look-ahead halo).  ``bytes_range(0, size)``
    equals ``tiled_fasta_host(size, seed)`` byte for byte (tests/test_synth_tiled.py)."""

    def __init__(self, size: int, seed: int = 0, block: int = 64 * 2**20 - 4099):
        self.size = int(size)
        self.base = fasta(min(block, self.size), seed)
        # the object-level tail fix of _fix_fasta_tail: bytes after the object's last '\n'
        t0 = max(0, self.size - (1 << 20))
        tail = self._raw(t0, self.size)
        nls = np.flatnonzero(tail == 10)
        self.tail0 = t0 + int(nls[-1]) + 1 if len(nls) else 0
        self.tail_fix = self.tail0 < self.size and bool((tail[self.tail0 - t0:] == ord(">")).any())

    def _raw(self, start: int, end: int, out: np.ndarray | None = None) -> np.ndarray:
        out = np.empty(end - start, np.uint8) if out is None else out[: end - start]
        bl = len(self.base)
        p = start
        while p < end:
            q = p % bl
            n = min(bl - q, end - p)
            out[p - start:p - start + n] = self.base[q:q + n]
            p += n
        return out

    def bytes_range(self, start: int, end: int, out: np.ndarray | None = None) -> np.ndarray:
        out = self._raw(start, end, out)
        if self.tail_fix and end > self.tail0:
            out[max(self.tail0, start) - start:] = ord("N")
        return out


def tiled_host(base: np.ndarray, size: int) -> np.ndarray:
    """``size`` bytes made of repeated copies of ``base`` (the last copy truncated)."""
    out = np.empty(size, np.uint8)
    for off, n in tile_plan(len(base), size):
        out[off:off + n] = base[:n]
    return out


class TiledText:
    """A large line-oriented object: ``head`` once, then ``body`` repeated to exactly ``size`` bytes.

    Used for the BASELINE configs[2]/[3] shapes (32 GiB CSV, 64 GiB VCF): a rank materializes only the
    byte range it scans (:meth:`bytes_range`), and the expected newline offsets of any range follow from
    the body's own newlines (:meth:`delims_range`), so a multi-GiB index is checked without a second scan.
    """

    def __init__(self, head: np.ndarray, body: np.ndarray, size: int, delim: int = 10):
        self.head = np.ascontiguousarray(head, np.uint8)
        self.body = np.ascontiguousarray(body, np.uint8)
        self.size = int(size)
        self.delim = delim
        self.head_pos = np.flatnonzero(self.head == delim).astype(np.uint64)
        self.body_pos = np.flatnonzero(self.body == delim).astype(np.uint64)

    def _tiles(self, start: int, end: int):
        """(object offset, body offset, length) pieces of the body covering [start, end)."""
        h, bl = len(self.head), len(self.body)
        p = max(start, h)
        while p < end:
            q = (p - h) % bl
            n = min(bl - q, end - p)
            yield p, q, n
            p += n

    def bytes_range(self, start: int, end: int, out: np.ndarray | None = None) -> np.ndarray:
        out = np.empty(end - start, np.uint8) if out is None else out[: end - start]
        h = len(self.head)
        if start < h:
            out[: min(h, end) - start] = self.head[start:min(h, end)]
        for p, q, n in self._tiles(start, end):
            out[p - start:p - start + n] = self.body[q:q + n]
        return out

    def delims_range(self, start: int, end: int):
        """Yields sorted uint64 arrays: the delimiter offsets in [start, end), piece by piece."""
        h = len(self.head)
        if start < h:
            hp = self.head_pos
            yield hp[(hp >= start) & (hp < min(h, end))]
        bp = self.body_pos
        for p, q, n in self._tiles(start, end):
            lo, hi = np.searchsorted(bp, q), np.searchsorted(bp, q + n)
            yield bp[lo:hi] + np.uint64(p - q)

    def count_range(self, start: int, end: int) -> int:
        return int(sum(len(x) for x in self.delims_range(start, end)))


def tiled_csv(size: int, seed: int = 0, block: int = 64 * 2**20 - 333) -> TiledText:
    """cities.csv-shaped CSV of ``size`` bytes: one header line, then a seeded row block repeated."""
    base = csv(block, seed)
    h = len(CSV_HEADER)
    return TiledText(base[:h], base[h:], size)


def tiled_vcf(size: int, seed: int = 0, block: int = 64 * 2**20 - 333) -> TiledText:
    """VCF of ``size`` bytes: the header once, then a seeded row block repeated."""
    base = vcf(block, seed)
    h = len(VCF_HEADER)
    return TiledText(base[:h], base[h:], size)


def bgzf(raw: bytes, block: int = 65280, level: int = 6, eof: bool = True) -> bytes:
    """BGZF (blocked gzip, as samtools/htslib write FASTQ.gz): independent gzip members of at most ``block``
    inflated bytes, each carrying its compressed size in the "BC" extra subfield, plus the empty EOF member."""
    import struct
    import zlib
    out = []

    def member(data: bytes) -> bytes:
        c = zlib.compressobj(level, zlib.DEFLATED, -15)
        body = c.compress(data) + c.flush()
        bsize = 18 + len(body) + 8 - 1
        head = b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff" + struct.pack("<H", 6) + b"BC" + \
            struct.pack("<HH", 2, bsize)
        return head + body + struct.pack("<II", zlib.crc32(data) & 0xFFFFFFFF, len(data) & 0xFFFFFFFF)

    for i in range(0, len(raw), block):
        out.append(member(raw[i:i + block]))
    if eof:
        out.append(member(b""))
    return b"".join(out)
