"""The corpus of tests/_part_cut_cases.py over the models, without a GPU: at every single cut and every pair
(c, c + 1), (c, c + 2) the merge over the model's parts equals the definition's byte loop (or raises what the loop
raises), and the sweeps cover what tests/test_gpu_part_cuts.py relies on -- device reads with every ``skip``, parts
without a line start, cuts on every kind of byte -- so that the device sweep over the same objects cannot be vacuous."""
import re

import pytest

import _fastq_loop as FQ
import _fastq_model as FM
import _part_cut_cases as C
import _vcfpos_loop as VP
import _vcfpos_model as VM
from _fai_loop import loop_fai, loop_text
from _fai_model import FakeDevices, header_pairs
from dataplug_amd.cloudobject import CloudObject
from dataplug_amd.formats.genomics import fasta as ffasta
from dataplug_amd.scan import fai as sfai
from dataplug_amd.scan import fastq
from dataplug_amd.scan import objects as scan_objects
from dataplug_amd.scan import vpos
from dataplug_amd.scan.fai import FaiFormatError
from dataplug_amd.scan.fastq import FastqFormatError
from dataplug_amd.scan.vpos import VcfFormatError
from dataplug_amd.storage import MemoryStore

FQ_GOOD, FQ_BAD = C.fastq_objects()
VCF_GOOD, VCF_BAD = C.vcf_bodies()
FA_GOOD, FA_BAD = C.fasta_objects()
VCF_CASES = [(name, bo) for name in list(VCF_GOOD) + list(VCF_BAD) for bo in (0, len(C.VCF_HEAD))]


def vcf_object(name, bo):
    body = VCF_GOOD[name] if name in VCF_GOOD else VCF_BAD[name][0]
    return (C.VCF_HEAD if bo else b"") + body


def test_the_corpus_is_small_and_the_loops_agree_with_its_labels():
    objs = list(FQ_GOOD.values()) + [v[0] for v in FQ_BAD.values()] + list(FA_GOOD.values()) + \
        [v[0] for v in FA_BAD.values()] + [vcf_object(n, bo) for n, bo in VCF_CASES]
    assert all(0 < len(d) <= C.MAX_BYTES for d in objs) and len(C.VCF_HEAD) == 37
    assert len(FQ.read_ranges(FQ_GOOD["lf"])) == 30 and len(FQ.read_ranges(FQ_GOOD["crlf"])) == 24
    assert FQ_GOOD["open"][-1] != 10 and FQ_GOOD["closed_crlf"].endswith(b"\r\n") and FQ_GOOD["crlf"].count(b"\r\n") == 96
    assert FQ.loop_index(FQ_GOOD["one_long"])[4] == 200
    for name, (data, kind, read) in FQ_BAD.items():
        with pytest.raises(FQ.LoopError) as e:
            FQ.loop_index(data, 2)
        assert (e.value.kind, e.value.read) == (kind, read), name
    assert VP.loop_index(VCF_GOOD["rows"], 0, 1)[2] == 40 and [c[2] for c in VP.loop_index(VCF_GOOD["rows"], 0)[1]][1] == 1
    assert VCF_GOOD["prefix_at_end"].endswith(b"chr3\t99\t") and VCF_GOOD["open"][-1] != 10
    assert max(e - s for s, e in VP.lines_of(VCF_GOOD["long_row"], 0)) > 300
    assert [c[0] for c in VP.loop_index(VCF_GOOD["prefix_names"], 0)[1]] == [b"chr1", b"chr10", b"chr100", b"chr"]
    for name, (body, kind, ordinal) in VCF_BAD.items():
        for bo in (0, 37):
            with pytest.raises(VP.LoopError) as e:
                VP.loop_index(vcf_object(name, bo), bo, 2)
            assert (e.value.kind, e.value.ordinal) == (kind, ordinal), name
    widths = {r[4] - (2 if b"\r" in FA_GOOD["wrapped"][r[2]:r[2] + r[4]] else 1)
              for r in loop_fai(FA_GOOD["wrapped"], header_pairs(FA_GOOD["wrapped"]))}
    assert widths == set(range(1, 10)) and len(header_pairs(FA_GOOD["wrapped"])) == 12
    s, e = header_pairs(FA_GOOD["long_header"])[1]
    assert e - s > C.FAI_HALO + 40 and FA_GOOD["long_header"][s + 1:s + 41] == C.LONG_NAME


# ------------------------------------------------------------------------------------------------ FASTQ
def fastq_sweep(data, check):
    """``check(parts, cuts, every)`` over every cut set and ``every``; the model's parts of every=2, by cut set."""
    singles, pairs = C.cut_sets(0, len(data))
    seen = {}
    for cuts in singles + pairs:
        for every in C.EVERY:
            parts = FM.parts_by_cuts(data, cuts, every)
            check(parts, cuts, every)
        seen[tuple(cuts)] = parts
    return singles, pairs, seen


@pytest.mark.parametrize("name", list(FQ_GOOD))
def test_fastq_merge_equals_the_loop_at_every_cut(name):
    data = FQ_GOOD[name]
    want = {k: FQ.loop_index(data, k) for k in C.EVERY}

    def check(parts, cuts, every):
        assert C.fastq_got(parts, data, every) == want[every], (name, cuts, every)
    singles, pairs, seen = fastq_sweep(data, check)
    assert len(singles) == len(data) - 1 and len(pairs) == 2 * len(data) - 5
    terminated = data[-1] == 10
    if name == "one_long":
        empty = [c for c, parts in seen.items() if any(p.n_lines == 0 for p in parts)]
        assert len(empty) >= 10
        gpu = {tuple(c) for c in C.gpu_cut_sets(0, len(data))}
        assert len(gpu & set(empty)) >= 3                                # the thinned device sweep meets some too
        assert sum(1 for parts in seen.values() if any(0 < p.n_lines < 8 for p in parts)) >= 100   # all host lines
        return
    both = sum(1 for c in singles if all(p.n_reads > 0 for p in seen[tuple(c)]))
    assert both >= len(singles) / 2, (name, both / len(singles))
    # device reads with every skip, in a first part and in a later one, closed and not; over the single cuts alone,
    # which the device sweep runs in full
    dev = [(k == 0, p.skip, bool(p.closed)) for c in singles for k, p in enumerate(seen[tuple(c)]) if p.n_reads]
    assert {s for first, s, _ in dev if not first} == {0, 1, 2, 3} and {s for first, s, _ in dev if first} == {0}
    assert {first for first, _, _ in dev} == {True, False}
    assert {closed for _, _, closed in dev} == ({True, False} if terminated else {False})


@pytest.mark.parametrize("name", list(FQ_BAD))
def test_fastq_broken_twin_raises_the_loops_error_at_every_cut(name):
    data, kind, read = FQ_BAD[name]
    with pytest.raises(FQ.LoopError) as le:
        FQ.loop_index(data, 2)
    want = (le.value.kind, le.value.read, le.value.offset)

    def check(parts, cuts, every):
        with pytest.raises(FastqFormatError) as e:
            fastq.merge_parts(parts, len(data), every, lambda q: data[q])
        assert (e.value.kind, e.value.read, e.value.offset) == want, (name, cuts, every)
    singles, pairs, seen = fastq_sweep(data, check)
    if kind != "truncated" and 0 < read < 29:        # at some cuts the device step finds it, at others the host does
        found = [any(p.first_malformed is not None for p in seen[tuple(c)]) for c in singles]
        assert any(found) and not all(found)


# ------------------------------------------------------------------------------------------------ VCF
@pytest.mark.parametrize("name,bo", VCF_CASES)
def test_vcf_merge_equals_the_loop_at_every_cut(name, bo):
    data = vcf_object(name, bo)
    size = len(data)
    singles, pairs = C.cut_sets(bo, size)
    assert len(singles) == size - bo - 1
    if name in VCF_GOOD:
        want = {k: C.vcf_want(data, bo, k) for k in C.EVERY}
    else:
        with pytest.raises(VP.LoopError) as le:
            VP.loop_index(data, bo, 2)
        want = (le.value.kind, le.value.ordinal, le.value.offset)
        assert want[:2] == VCF_BAD[name][1:]
    for cuts in singles + pairs:
        for every in C.EVERY:
            parts = VM.parts_by_cuts(data, bo, cuts, every)
            if name in VCF_GOOD:
                assert C.vcf_got(parts, size) == want[every], (name, bo, cuts, every)
            else:
                with pytest.raises(VcfFormatError) as e:
                    vpos.merge_parts(parts, size)
                assert (e.value.kind, e.value.ordinal, e.value.offset) == want, (name, bo, cuts, every)


def test_vcf_cuts_land_on_every_kind_of_byte():
    """Over the well-formed bodies some single cut lies on a '\\n', on the byte behind one, on a '\\r', on a tab,
    inside CHROM and inside POS, and some part's first owned line begins a contig."""
    seen = set()
    for name, body in VCF_GOOD.items():
        for bo in (0, 37):
            data = vcf_object(name, bo)
            lines = VP.lines_of(data, bo)
            chrom = [VP.parse_line(data, s)[0] for s, _ in lines]
            for (c,) in C.cut_sets(bo, len(data))[0]:
                i = max(k for k, (s, _) in enumerate(lines) if s <= c)   # the line the cut lies in
                s = lines[i][0]
                t1 = data.index(b"\t", s)
                t2 = data.index(b"\t", t1 + 1)
                seen |= {what for what, hit in (
                    ("newline", data[c] == 10), ("behind a newline", data[c - 1] == 10), ("cr", data[c] == 13),
                    ("tab", data[c] == 9), ("in chrom", s < c < t1), ("in pos", t1 + 1 < c < t2),
                    ("contig change on a part's first line", i + 1 < len(lines) and c > s and chrom[i + 1] != chrom[i]),
                    ("a cut on a line start whose line begins a contig", c == s and chrom[i] != chrom[i - 1]),
                ) if hit}
                if name == "rows" and c > s and i + 1 < len(lines):      # the model agrees on which line the part owns
                    parts = VM.parts_by_cuts(data, bo, [c], 1)
                    assert int(parts[1].run_offset[0]) == lines[i + 1][0] and parts[0].n == i + 1
    assert seen == {"newline", "behind a newline", "cr", "tab", "in chrom", "in pos",
                    "contig change on a part's first line", "a cut on a line start whose line begins a contig"}


# ------------------------------------------------------------------------------------------------ FASTA
def _co(data: bytes, name: str):
    MemoryStore._named.pop(name, None)
    cfg = {"endpoint_url": f"memory://{name}"}
    co = CloudObject.from_s3(ffasta.FASTA, "s3://data/c.fa", fetch=False, s3_config=cfg)
    co.storage.create_bucket(Bucket="data")
    co.storage.put_object(Body=data, Bucket="data", Key="c.fa")
    return CloudObject.from_s3(ffasta.FASTA, "s3://data/c.fa", s3_config=cfg)


def name_gets(co, monkeypatch):
    """The ranged GETs ``fai_index_object`` makes of the object besides its parts' fetches: the long-name fallback."""
    gets = []
    real = co.storage.get_object
    monkeypatch.setattr(co.storage, "get_object", lambda **kw: (gets.append(kw.get("Range")), real(**kw))[1])
    return gets


@pytest.mark.parametrize("name", list(FA_GOOD) + list(FA_BAD))
def test_fai_index_object_equals_the_loop_at_every_part_size(monkeypatch, name):
    data = FA_GOOD[name] if name in FA_GOOD else FA_BAD[name][0]
    pairs = header_pairs(data)
    FakeDevices(monkeypatch, [0])
    co = _co(data, f"part_cuts_cpu_{name}")
    gets = name_gets(co, monkeypatch)
    long_parts = []
    for p in range(1, len(data) + 1):
        del gets[:]
        if name in FA_GOOD:
            names, rows = scan_objects.fai_index_object(co, pairs, part_bytes=p, halo=C.FAI_HALO)
            assert sfai.fai_text(names, rows) == loop_text(loop_fai(data, pairs)), (name, p)
        else:
            with pytest.raises(FaiFormatError) as e:
                scan_objects.fai_index_object(co, pairs, part_bytes=p, halo=C.FAI_HALO)
            assert (e.value.ordinal, e.value.name) == FA_BAD[name][1:], (name, p)
        s, e = pairs[1] if len(pairs) > 1 else pairs[0]
        if f"bytes={s + 1}-{e - 1}" in gets:
            long_parts.append(p)
    if name == "long_header":                            # the name outruns the halo: the ranged-GET fallback ran
        assert len(long_parts) >= 10 and len(data) not in long_parts
    elif name in FA_GOOD:
        assert long_parts == []


def test_fasta_cuts_land_in_headers_names_and_on_line_ends():
    """Some ``part_bytes`` puts a part boundary inside a header line, inside a name, on a '>' and on the last '\\n'
    of a body."""
    seen = set()
    for name, data in FA_GOOD.items():
        pairs = header_pairs(data)
        b, e = sfai.bodies(pairs, len(data))
        for p in range(1, len(data) + 1):
            for c, _ in scan_objects.line_parts(0, len(data), 1, p)[1:]:
                for (s, he), bb, ee in zip(pairs, b.tolist(), e.tolist()):
                    nm = re.split(rb"[ \t\r\n]", data[s + 1:he], maxsplit=1)[0]
                    seen |= {what for what, hit in (
                        ("in a header line", s < c < he), ("in a name", s + 1 < c < s + 1 + len(nm)), ("on the '>'", c == s),
                        ("on a body's last newline", ee > bb and c == ee - 1 and data[c] == 10)) if hit}
    assert seen == {"in a header line", "in a name", "on the '>'", "on a body's last newline"}
