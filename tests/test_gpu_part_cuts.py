"""The per-part device step of the part-wise index builds (``ScanContext.fastq_lines`` / ``fastq_reads``,
``vcf_lines`` / ``vcf_positions``, ``fai_counts`` / ``fai_names``) against the models at every part cut of the small
objects of tests/_part_cut_cases.py: field by field per part, then the merge against the definition's byte loops, then
the object paths (``reads_index_object``, ``pos_index_object``, ``fai_index_object``) at every ``part_bytes`` on one
device entry and at a few on two.  tests/test_part_cuts_cpu.py shows what these sweeps cover."""
import numpy as np
import pytest

import _fastq_loop as FQ
import _fastq_model as FM
import _part_cut_cases as C
import _vcfpos_loop as VP
import _vcfpos_model as VM
from _fai_loop import loop_fai, loop_text
from _fai_model import header_pairs, np_names, np_pass1, np_pass2
from dataplug_amd.cloudobject import CloudObject
from dataplug_amd.formats.genomics import fasta as ffasta
from dataplug_amd.formats.genomics import fastq as ffq
from dataplug_amd.formats.genomics import vcf as fvcf
from dataplug_amd.scan import fai as sfai
from dataplug_amd.scan import fastq
from dataplug_amd.scan import objects as scan_objects
from dataplug_amd.scan import vpos
from dataplug_amd.scan.fai import FaiFormatError
from dataplug_amd.scan.fastq import FastqFormatError
from dataplug_amd.scan.vpos import VcfFormatError
from dataplug_amd.storage import MemoryStore

pytestmark = pytest.mark.gpu

FQ_GOOD, FQ_BAD = C.fastq_objects()
VCF_GOOD, VCF_BAD = C.vcf_bodies()
FA_GOOD, FA_BAD = C.fasta_objects()
VCF_CASES = [(name, bo) for name in list(VCF_GOOD) + list(VCF_BAD) for bo in (0, len(C.VCF_HEAD))]
# behind the object's last byte in the device buffer: bytes that would change a result if a launch read them
POISON = b"\n@\t7\t+\r" * 8


def vcf_object(name, bo):
    body = VCF_GOOD[name] if name in VCF_GOOD else VCF_BAD[name][0]
    return (C.VCF_HEAD if bo else b"") + body


def uploaded(ctx, data: bytes) -> int:
    """The object in workspace "input", uploaded once: byte ``lo`` lies at the returned address + ``lo``, which is
    congruent to ``lo`` mod 16 as ``scan.objects._resident`` gives it."""
    buf = ctx.workspace("input", len(data) + 64, placed=True)
    assert buf.ptr % 16 == 0 and len(POISON) <= 64
    ctx.h2d(buf.ptr, np.frombuffer(data + POISON, np.uint8))
    return buf.ptr


def real_part(ctx, d_obj: int):
    return lambda k, lo, hi, top: (ctx, d_obj + lo)


def plain(v):
    if isinstance(v, np.ndarray):
        return v.tolist()
    if isinstance(v, (list, tuple)):
        return [plain(x) for x in v]
    return v if v is None or isinstance(v, bytes) else int(v)


def assert_parts_equal(got, want, where):
    """Every field of every part, arrays through ``tolist`` and integers exactly; the message names the object, the
    cuts, the part and the first field that differs."""
    assert len(got) == len(want), where
    for k, (g, w) in enumerate(zip(got, want)):
        for f in type(w)._fields:
            a, b = plain(getattr(g, f)), plain(getattr(w, f))
            if a == b and type(a) is type(b):
                continue
            if isinstance(a, list) and isinstance(b, list):                  # the first entry that differs
                i = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
                a, b = f"{len(a)} entries, [{i}:] {a[i:i + 4]!r}", f"{len(b)} entries, [{i}:] {b[i:i + 4]!r}"
            pytest.fail(f"{where} part {k} field {f}: device {a!r}, model {b!r}")


# ------------------------------------------------------------------------------------------------ a. FASTQ
@pytest.mark.parametrize("name", list(FQ_GOOD) + list(FQ_BAD))
def test_fastq_device_step_equals_the_model_at_every_cut(ctx, name):
    data = FQ_GOOD[name] if name in FQ_GOOD else FQ_BAD[name][0]
    make = real_part(ctx, uploaded(ctx, data))
    if name in FQ_GOOD:
        want = {k: FQ.loop_index(data, k) for k in C.EVERY}
    else:
        with pytest.raises(FQ.LoopError) as le:
            FQ.loop_index(data, 2)
        want = (le.value.kind, le.value.read, le.value.offset)
    for cuts in C.gpu_cut_sets(0, len(data)):
        for every in C.EVERY:
            where = f"fastq {name} cuts {cuts} every {every}"
            parts = FM.parts_by_cuts(data, cuts, every, make)
            assert_parts_equal(parts, FM.parts_by_cuts(data, cuts, every), where)
            if name in FQ_GOOD:
                assert C.fastq_got(parts, data, every) == want[every], where
            else:
                with pytest.raises(FastqFormatError) as e:
                    fastq.merge_parts(parts, len(data), every, lambda q: data[q])
                assert (e.value.kind, e.value.read, e.value.offset) == want, where


# ------------------------------------------------------------------------------------------------ b. VCF
@pytest.mark.parametrize("name,bo", VCF_CASES)
def test_vcf_device_step_equals_the_model_at_every_cut(ctx, name, bo):
    data = vcf_object(name, bo)
    size = len(data)
    make = real_part(ctx, uploaded(ctx, data))
    if name in VCF_GOOD:
        want = {k: C.vcf_want(data, bo, k) for k in C.EVERY}
    else:
        with pytest.raises(VP.LoopError) as le:
            VP.loop_index(data, bo, 2)
        want = (le.value.kind, le.value.ordinal, le.value.offset)
    sweep = [(cuts, every, 1024) for cuts in C.gpu_cut_sets(bo, size) for every in C.EVERY]
    # the capacity retry on parts whose runs start at their first line: one run slot, the whole body and two halves
    sweep += [([], 2, 1), ([bo + (size - bo) // 2], 2, 1)]
    for cuts, every, run_cap in sweep:
        where = f"vcf {name} body_offset {bo} cuts {cuts} every {every} run_cap {run_cap}"
        parts = VM.parts_by_cuts(data, bo, cuts, every, make, run_cap=run_cap)
        assert_parts_equal(parts, VM.parts_by_cuts(data, bo, cuts, every), where)
        if name in VCF_GOOD:
            assert C.vcf_got(parts, size) == want[every], where
        else:
            with pytest.raises(VcfFormatError) as e:
                vpos.merge_parts(parts, size)
            assert (e.value.kind, e.value.ordinal, e.value.offset) == want, where


@pytest.mark.parametrize("bo", [0, len(C.VCF_HEAD)])
def test_vcf_runs_of_many_waves_come_back_in_line_order(ctx, bo):
    """The corpus' bodies fit one wave or two, whose run starts and run ends take their slots in line order anyway.
    Four workgroups of lines with a contig change on every third take them in any order: ``vcf_positions`` has to
    put the starts and the ends back in line order, each on its own.  (Built here, not part of the 512-byte corpus.)"""
    n = 4 * max(ctx.vpos_geometry()) + 5
    data = (C.VCF_HEAD if bo else b"") + b"".join(C.vrow(b"c%d" % (i // 3), 7 + i % 3) for i in range(n))
    size = len(data)
    make = real_part(ctx, uploaded(ctx, data))
    nl = [p for p in range(bo, size) if data[p] == 10]
    mid = nl[n // 2]
    for cuts in ([], [mid], [mid + 1], [nl[n // 3] - 2, mid + 3]):
        for every, run_cap in ((2, 1024), (64, 1)):
            where = f"vcf {n} rows body_offset {bo} cuts {cuts} every {every} run_cap {run_cap}"
            parts = VM.parts_by_cuts(data, bo, cuts, every, make, run_cap=run_cap)
            assert_parts_equal(parts, VM.parts_by_cuts(data, bo, cuts, every), where)
            assert C.vcf_got(parts, size) == C.vcf_want(data, bo, every), where
            assert sum(len(p.names) for p in parts) >= n // 3


# ------------------------------------------------------------------------------------------------ c. FASTA
def _co(fmt, data: bytes, name: str, key: str, devs):
    MemoryStore._named.pop(name, None)
    cfg = {"endpoint_url": f"memory://{name}"}
    co = CloudObject.from_s3(fmt, f"s3://data/{key}", fetch=False, s3_config=cfg)
    co.storage.create_bucket(Bucket="data")
    co.storage.put_object(Body=data, Bucket="data", Key=key)
    co = CloudObject.from_s3(fmt, f"s3://data/{key}", s3_config=cfg)
    setattr(co, scan_objects.DEVICES_ATTR, list(devs))
    return co


def assert_arrays_equal(got, want, fields, where):
    for f, g, w in zip(fields, got, want):
        assert g.tolist() == w.tolist(), f"{where} field {f}: device {g.tolist()}, model {w.tolist()}"


@pytest.mark.parametrize("name", list(FA_GOOD) + list(FA_BAD))
def test_fai_device_step_equals_the_model_at_every_part_size(ctx, name):
    data = FA_GOOD[name] if name in FA_GOOD else FA_BAD[name][0]
    size = len(data)
    d = np.frombuffer(data, np.uint8)
    pairs = np.asarray(header_pairs(data), np.uint64).reshape(-1, 2)
    starts, hends = np.ascontiguousarray(pairs[:, 0]), np.ascontiguousarray(pairs[:, 1])
    b, e = sfai.bodies(pairs, size)
    whole = np_pass1(d, 0, b, e)
    d_obj = uploaded(ctx, data)
    for p in range(1, size + 1):
        bounds = scan_objects.line_parts(0, size, 1, p)
        nl, first = np.zeros(len(b), np.uint64), np.full(len(b), sfai.NONE, np.uint64)
        clipped = []
        for k, (lo, hi) in enumerate(bounds):
            where = f"fasta {name} part_bytes {p} part {k}"
            top = min(size, hi + C.FAI_HALO)
            idx, plo, phi = scan_objects.clip_bodies(b, e, lo, hi)
            clipped.append((lo, top, idx, plo, phi))
            got = ctx.fai_counts(d_obj + lo, top - lo, lo, plo, phi, b[idx])
            assert_arrays_equal(got, np_pass1(d[lo:top], lo, plo, phi), ("nl", "cr", "first"), where + " pass 1")
            nl[idx] += got[0]
            first[idx] = np.minimum(first[idx], got[2])
            j0, j1 = int(np.searchsorted(starts, lo, "left")), int(np.searchsorted(starts, hi, "left"))
            cut = np.minimum(hends[j0:j1], np.uint64(top))
            got = ctx.fai_names(d_obj + lo, top - lo, lo, starts[j0:j1], cut)
            assert_arrays_equal(got, np_names(d[lo:top], lo, starts[j0:j1], cut), ("name lengths", "names"), where)
        assert nl.tolist() == whole[0].tolist() and first.tolist() == whole[2].tolist(), f"fasta {name} part_bytes {p}"
        w32 = np.minimum(sfai.line_widths(b, e, nl, first), np.uint64(0xFFFFFFFF)).astype(np.uint32)
        for k, (lo, top, idx, plo, phi) in enumerate(clipped):
            got = ctx.fai_counts(d_obj + lo, top - lo, lo, plo, phi, b[idx], width=w32[idx])
            assert_arrays_equal(got, np_pass2(d[lo:top], lo, plo, phi, b[idx], w32[idx]), ("off", "lastoff"),
                                f"fasta {name} part_bytes {p} part {k} pass 2")


def check_fai_object(co, data, pairs, name, where, **kw):
    if name in FA_GOOD:
        names, rows = scan_objects.fai_index_object(co, pairs, halo=C.FAI_HALO, **kw)
        assert sfai.fai_text(names, rows) == loop_text(loop_fai(data, pairs)), where
    else:
        with pytest.raises(FaiFormatError) as e:
            scan_objects.fai_index_object(co, pairs, halo=C.FAI_HALO, **kw)
        assert (e.value.ordinal, e.value.name) == FA_BAD[name][1:], where


@pytest.mark.parametrize("name", list(FA_GOOD) + list(FA_BAD))
def test_fai_index_object_at_every_part_size(name):
    data = FA_GOOD[name] if name in FA_GOOD else FA_BAD[name][0]
    pairs = header_pairs(data)
    co = _co(ffasta.FASTA, data, f"gpu_part_cuts_fa_{name}", "c.fa", [0])
    for p in range(1, len(data) + 1):
        check_fai_object(co, data, pairs, name, f"fasta {name} part_bytes {p}", part_bytes=p)


# ------------------------------------------------------------------------------------------------ d. the object paths
def check_reads_object(co, data, name, every, where, **kw):
    if name in FQ_GOOD:
        assert C.fastq_tuple(scan_objects.reads_index_object(co, every, **kw)) == FQ.loop_index(data, every), where
    else:
        with pytest.raises(FQ.LoopError) as le:
            FQ.loop_index(data, every)
        with pytest.raises(FastqFormatError) as e:
            scan_objects.reads_index_object(co, every, **kw)
        assert (e.value.kind, e.value.read, e.value.offset) == (le.value.kind, le.value.read, le.value.offset), where


def check_pos_object(co, data, bo, name, every, where, **kw):
    if name in VCF_GOOD:
        smp, names, rows, n = scan_objects.pos_index_object(co, bo, every, **kw)
        got = smp.astype("<u4").tobytes(), vpos.contigs_text(names, rows), n
        assert got == C.vcf_want(data, bo, every), where
    else:
        with pytest.raises(VP.LoopError) as le:
            VP.loop_index(data, bo, every)
        with pytest.raises(VcfFormatError) as e:
            scan_objects.pos_index_object(co, bo, every, **kw)
        assert (e.value.kind, e.value.ordinal, e.value.offset) == \
            (le.value.kind, le.value.ordinal, le.value.offset), where


@pytest.mark.parametrize("name", ["lf", "bad_separator_middle"])
def test_reads_index_object_at_every_part_size(name):
    data = FQ_GOOD[name] if name in FQ_GOOD else FQ_BAD[name][0]
    co = _co(ffq.FASTQ, data, f"gpu_part_cuts_fq_{name}", "c.fastq", [0])
    for p in range(1, len(data) + 1):
        every = C.EVERY[p % 3]
        check_reads_object(co, data, name, every, f"fastq {name} part_bytes {p} every {every}", part_bytes=p)


@pytest.mark.parametrize("name", ["rows", "unsorted_middle"])
def test_pos_index_object_at_every_part_size(name):
    bo = len(C.VCF_HEAD)
    data = vcf_object(name, bo)
    co = _co(fvcf.VCF, data, f"gpu_part_cuts_vcf_{name}", "c.vcf", [0])
    for p in range(1, len(data) - bo + 1):
        every = C.EVERY[p % 3]
        check_pos_object(co, data, bo, name, every, f"vcf {name} part_bytes {p} every {every}", part_bytes=p)


# ------------------------------------------------------------------------------------------------ e. two device entries
def part_sizes(begin, size):
    """``part_bytes`` that cut [begin, size) into 2 parts (one per entry of two), 3, 5 and 8."""
    out = {}
    for n in (2, 3, 5, 8):
        p = size - begin if n == 2 else -(-(size - begin) // n)
        assert len(scan_objects.line_parts(begin, size, 2, p)) == n
        out[n] = p
    return out


@pytest.mark.parametrize("name", ["lf", "crlf", "length_mismatch_middle"])
def test_reads_index_object_on_two_entries(name):
    data = FQ_GOOD[name] if name in FQ_GOOD else FQ_BAD[name][0]
    co = _co(ffq.FASTQ, data, f"gpu_part_cuts_fq2_{name}", "c.fastq", [0, 0])
    for n, p in part_sizes(0, len(data)).items():
        check_reads_object(co, data, name, 2, f"fastq {name} on two entries, {n} parts", part_bytes=p)


@pytest.mark.parametrize("name", ["rows", "crlf", "split_middle"])
def test_pos_index_object_on_two_entries(name):
    bo = len(C.VCF_HEAD)
    data = vcf_object(name, bo)
    co = _co(fvcf.VCF, data, f"gpu_part_cuts_vcf2_{name}", "c.vcf", [0, 0])
    for n, p in part_sizes(bo, len(data)).items():
        check_pos_object(co, data, bo, name, 2, f"vcf {name} on two entries, {n} parts", part_bytes=p)


@pytest.mark.parametrize("name", ["wrapped", "long_header", "irregular0"])
def test_fai_index_object_on_two_entries_refetches_only_with_several_parts(monkeypatch, name):
    data = FA_GOOD[name] if name in FA_GOOD else FA_BAD[name][0]
    pairs = header_pairs(data)
    co = _co(ffasta.FASTA, data, f"gpu_part_cuts_fa2_{name}", "c.fa", [0, 0])
    fetches = []
    real = scan_objects.fetch_to_device

    def counting(ctx, storage, bucket, key, lo, hi, d_ptr, **kw):
        fetches.append((lo, hi))                         # (list.append is atomic: the two workers share it)
        return real(ctx, storage, bucket, key, lo, hi, d_ptr, **kw)
    monkeypatch.setattr(scan_objects, "fetch_to_device", counting)
    d = np.frombuffer(data, np.uint8)
    b, e = sfai.bodies(pairs, len(data))
    has_lines = bool((np_pass1(d, 0, b, e)[0] > 0).any())
    for n, p in part_sizes(0, len(data)).items():
        del fetches[:]
        check_fai_object(co, data, pairs, name, f"fasta {name} on two entries, {n} parts", part_bytes=p)
        want = []
        for k, (lo, hi) in enumerate(scan_objects.line_parts(0, len(data), 2, p)):
            # an entry that holds one part runs pass 2 on the bytes still resident; one that holds several (entry
            # k mod 2 holds parts k, k + 2, ...) fetches each of its parts again
            again = has_lines and len(range(k % 2, n, 2)) > 1
            want += [(lo, min(len(data), hi + C.FAI_HALO))] * (2 if again else 1)
        assert sorted(fetches) == sorted(want), (name, n)
        assert n > 2 or len(fetches) == 2
