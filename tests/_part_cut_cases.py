"""Named small objects (each at most 512 bytes, built here, no ``synth`` call) for the sweeps over every part cut:
tests/test_part_cuts_cpu.py runs them over the models and checks what the sweeps cover, tests/test_gpu_part_cuts.py
runs the same cuts through the device step.  Few bytes hold many lines, so that a cut at every byte meets every
position of a line and parts of every line count from none to dozens."""
import _fastq_loop as FQ
import _vcfpos_loop as VP

MAX_BYTES = 512
EVERY = (1, 2, 64)


def cut_sets(lo: int, size: int):
    """Every single cut c in lo + 1 .. size - 1, and every pair (c, c + 1), (c, c + 2) that lies inside."""
    singles = [[c] for c in range(lo + 1, size)]
    pairs = [[c, c + d] for c in range(lo + 1, size) for d in (1, 2) if c + d < size]
    return singles, pairs


def gpu_cut_sets(lo: int, size: int):
    """The device sweep: every single cut, and every twentieth pair."""
    singles, pairs = cut_sets(lo, size)
    return singles + pairs[::20]


# ------------------------------------------------------------------------------------------------ FASTQ
Z = b"@\n\n+\n\n"                                       # the empty read: four lines in six bytes


def fq_read(i: int, bases: int, eol: bytes = b"\n") -> bytes:
    seq = (b"ACGT" * (bases // 4 + 1))[:bases]
    return b"@r%d" % i + eol + seq + eol + b"+" + eol + b"I" * bases + eol


def fq_mixed(n: int, eol: bytes = b"\n") -> bytes:
    """``n`` reads, every fourth a real one of 0, 4 or 8 bases, the others empty."""
    return b"".join(fq_read(i, (0, 4, 8)[(i // 4) % 3], eol) if i % 4 == 3 else Z.replace(b"\n", eol)
                    for i in range(n))


def fq_broken(data: bytes, where: int, how: str) -> bytes:
    """``data`` with read ``where`` broken: its '@' or its '+' replaced, a base put in front of its sequence line, or
    the object cut off behind its sequence line ("truncated": two of its four lines stay)."""
    s, e = FQ.read_ranges(data)[where]
    ln = [x for x in FQ.lines_of(data) if s <= x[0] < e]
    if how == "truncated":
        return data[:ln[1][1] + 1]                       # the header line, the sequence line and its '\n': two lines
    if how == "length_mismatch":
        return data[:ln[1][0]] + b"A" + data[ln[1][0]:]
    p = {"bad_header": ln[0][0], "bad_separator": ln[2][0]}[how]
    return data[:p] + b"x" + data[p + 1:]


FQ_KINDS = ("bad_header", "bad_separator", "length_mismatch", "truncated")


def fastq_objects():
    """{name: bytes} of the well-formed objects, and {name: (bytes, kind, read)} of the broken twins of ``lf``."""
    lf = fq_mixed(30)
    good = {
        "lf": lf,
        "crlf": fq_mixed(24, b"\r\n"),
        "open": fq_mixed(20)[:-1],                                       # (read 19 is a real one: its last line stays)
        "closed_crlf": fq_mixed(10) + fq_read(10, 4, b"\r\n") + Z.replace(b"\n", b"\r\n"),
        "one_long": Z * 6 + fq_read(6, 200) + Z * 6,
    }
    n = len(FQ.read_ranges(lf))
    bad = {}
    for how in FQ_KINDS:
        for label, where in (("first", 0), ("middle", n // 2), ("last", n - 1)):
            bad[f"{how}_{label}"] = (fq_broken(lf, where, how), how, where)
    return good, bad


# ------------------------------------------------------------------------------------------------ VCF
VCF_HEAD = b"##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tX\n"      # 37 bytes


def vrow(chrom: bytes, pos, rest: bytes = b"x", eol: bytes = b"\n") -> bytes:
    return chrom + b"\t" + (pos if isinstance(pos, bytes) else b"%d" % pos) + b"\t" + rest + eol


def vcf_rows(eol: bytes = b"\n"):
    """40 rows over three contigs, the middle one of a single row; equal neighbours and POS of 1 to 3 digits."""
    rows = [(b"chr1", p) for p in (1, 1, 2, 5, 5, 9, 10, 11, 40, 40, 41, 99, 100, 101, 101, 150, 200, 201, 300, 301,
                                   302, 999)]
    rows += [(b"chr2", 7)]
    rows += [(b"chr3", p) for p in (3, 3, 4, 8, 15, 16, 23, 42, 42, 43, 50, 60, 70, 80, 90, 98, 99)]
    return [vrow(c, p, eol=eol) for c, p in rows]


def vcf_bodies():
    """{name: body bytes} of the well-formed bodies, and {name: (body, kind, ordinal)} of the broken twins."""
    rows = vcf_rows()
    short = [vrow(b"c1", p) for p in range(1, 9)]
    good = {
        "rows": b"".join(rows),
        "crlf": b"".join(vcf_rows(b"\r\n")),
        "open": b"".join(rows)[:-1],
        "prefix_at_end": b"".join(rows[:-1]) + b"chr3\t99\t",             # the prefix ends at the object's last byte
        "long_row": b"".join(short) + vrow(b"c1", 9, b"q" * 300) + b"".join(vrow(b"c2", p) for p in range(1, 9)),
        "prefix_names": b"".join(vrow(c, p) for c in (b"chr1", b"chr10", b"chr100", b"chr") for p in (2, 3, 3, 11)),
    }

    def swap(i, row):
        return b"".join(rows[:i] + [row] + rows[i + 1:])
    n = len(rows)
    bad = {
        "unsorted_first": (swap(1, vrow(b"chr1", 0)), "unsorted", 1),
        "unsorted_middle": (swap(12, vrow(b"chr1", 98)), "unsorted", 12),
        "unsorted_last": (swap(n - 1, vrow(b"chr3", 97)), "unsorted", n - 1),
        "split_first": (swap(1, vrow(b"chr3", 1)), "split contig", 2),    # chr1 comes back on row 2
        "split_middle": (swap(30, vrow(b"chr1", 1000)), "split contig", 30),
        "split_last": (swap(n - 1, vrow(b"chr2", 8)), "split contig", n - 1),
        "malformed_first": (swap(0, b"chr1 1 x\n"), "malformed", 0),
        "malformed_middle": (swap(22, b"chr2\t7x\tx\n"), "malformed", 22),
        "malformed_last": (b"".join(rows[:-1]) + b"chr3\t99", "malformed", n - 1),
        "unsorted_then_malformed": (b"".join(rows[:12] + [vrow(b"chr1", 98)] + rows[13:33] + [b"\t5\tx\n"] + rows[34:]),
                                    "unsorted", 12),
        "malformed_then_split": (b"".join(rows[:5] + [b"chr1\t\tx\n"] + rows[6:n - 1] + [vrow(b"chr2", 8)]),
                                 "malformed", 5),
    }
    return good, bad


# ------------------------------------------------------------------------------------------------ FASTA
FAI_HALO = 16
LONG_NAME = b"L" * 40


def fa_seq(name: bytes, bases: int, width: int, eol: bytes = b"\n", desc: bytes = b"", last_eol: bool = True) -> bytes:
    seq = (b"ACGTN" * (bases // 5 + 1))[:bases]
    body = b"".join(seq[k:k + width] + eol for k in range(0, bases, width))
    if body and not last_eol:
        body = body[:-len(eol)]
    return b">" + name + desc + eol + body


def fasta_objects():
    """{name: bytes} of the regular objects, and {name: (bytes, ordinal, sequence name)} of the irregular twins, one
    per class of ``test_fai_cpu.IRREGULAR``."""
    from test_fai_cpu import IRREGULAR
    wrapped = b"".join(fa_seq(b"s%d" % i, (2 * w + w // 2 + i % 2), w, b"\r\n" if i % 3 == 2 else b"\n")
                       for i, w in enumerate([1, 2, 3, 4, 5, 6, 7, 8, 9, 3, 1, 5]))
    good = {
        "wrapped": wrapped,
        "empty_and_short": fa_seq(b"e", 0, 4) + fa_seq(b"o", 3, 4) + fa_seq(b"e2", 0, 4) + fa_seq(b"p", 9, 4),
        "open": fa_seq(b"a", 10, 4) + fa_seq(b"b", 7, 3, b"\r\n") + fa_seq(b"c", 6, 4, last_eol=False),
        "described": fa_seq(b"d1", 9, 5, desc=b" a description") + fa_seq(b"d2", 6, 3, b"\r\n", desc=b"\ttabbed x") +
                     fa_seq(b"d3", 4, 4),
        "long_header": fa_seq(b"a", 6, 4) + fa_seq(LONG_NAME, 11, 4, desc=b" described at length") +
                       fa_seq(b"z", 5, 5),
    }
    bad = {f"irregular{k}": (data, ordinal, name) for k, (data, ordinal, name) in enumerate(IRREGULAR)}
    return good, bad


# ------------------------------------------------------------------------------------------------ the merged indexes
def with_header(body: bytes) -> bytes:
    return VCF_HEAD + body


def vcf_want(data: bytes, bo: int, every: int):
    smp, contigs, n = VP.loop_index(data, bo, every)
    return VP.samples_bytes(smp), VP.contigs_text(contigs), n


def vcf_got(parts, size: int):
    from dataplug_amd.scan import vpos
    smp, names, rows, n = vpos.merge_parts(parts, size)
    return smp.astype("<u4").tobytes(), vpos.contigs_text(names, rows), n


def fastq_got(parts, data: bytes, every: int):
    """``scan.fastq.merge_parts`` over the parts, in the form of ``_fastq_loop.loop_index``."""
    from dataplug_amd.scan import fastq
    return fastq_tuple(fastq.merge_parts(parts, len(data), every, lambda q: data[q]))


def fastq_tuple(idx):
    return ([tuple(map(int, p)) for p in idx.samples.tolist()], idx.num_reads, idx.num_bases, idx.min_read_len,
            idx.max_read_len)
