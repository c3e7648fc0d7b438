"""The per-part device step of the VCF record-end index over the model: tests/_vcfpos_model.py's numpy-backed context
with ``vcf_spans`` added, its launches computed by the definition's byte loop (tests/_vspan_loop.py), and the small
40-line body whose part cuts the CPU and the GPU sweeps share."""
import numpy as np

import _vcfpos_loop as P
import _vcfpos_model as VM
import _vspan_loop as L
from dataplug_amd.scan import vspan
from dataplug_amd.scan.device import VcfSpans


class FakeContext(VM.FakeContext):
    def vcf_spans(self, ordinal0, every):
        buf, buf_base, size, starts = self.vp
        pos = P.loop_parse(buf, buf_base, size, starts)[0]
        ends, flags = L.loop_span(buf, buf_base, size, starts, pos)
        slots, res = L.loop_blockmax(ends, flags, pos, ordinal0, every)
        self.layer.note("spans", starts[0] if starts else None, ordinal0, len(starts))
        none = lambda v: None if v == L.NONE else v
        at = lambda i: None if i is None else starts[i]
        fm, ft = none(res["min_missing"]), none(res["min_truncated"])
        return VcfSpans(len(starts), np.array(slots, np.uint32), res["n_missing"], fm, res["n_truncated"], ft,
                        res["n_from_end"], res["max_span"], at(fm), at(ft))


class FakeDevices(VM.FakeDevices):
    def get_context(self, device=0, slot=0):
        ctxs = self.tls.__dict__.setdefault("ctxs", {})
        if device not in ctxs:
            ctxs[device] = FakeContext(self)
        return ctxs[device]


def model_part(data: bytes):
    layer = type("Layer", (), {"note": lambda *a: None, "fail_at": ()})()

    def make_part(k, lo, hi, top):
        ctx = FakeContext(layer)
        ctx.mem = np.frombuffer(data[lo:top], np.uint8)
        return ctx, ctx.BASE
    return make_part


def spans_by_cuts(data: bytes, bo: int, cuts, every, make_part=None, halo: int = VM.HALO):
    """The parts' ``VcfSpans`` for parts cut at ``cuts``, as ``_vcfpos_model.parts_by_cuts`` gives their
    ``VcfPositions``: part k = [lo, hi) sees the buffer [lo, min(size, hi + halo))."""
    size = len(data)
    edges = [bo] + sorted(cuts) + [size]
    parts, before = [], 0
    make_part = make_part or model_part(data)
    for k, (lo, hi) in enumerate(zip(edges[:-1], edges[1:])):
        top = min(size, hi + halo)
        ctx, d_buf = make_part(k, lo, hi, top)
        n = ctx.vcf_lines(d_buf, top - lo, lo, lo, hi, size, first=k == 0)
        parts.append((before, ctx.vcf_spans(before, every)))
        before += n
    return parts


def folded(data: bytes, parts, every):
    """The parts as ``vspan.SpanPart``: a truncated last line is read from ``data`` up to its '\\n'."""
    out = []
    for before, vs in parts:
        ln = None
        if vs.n_truncated:
            e = data.find(b"\n", vs.truncated_offset)
            ln = data[vs.truncated_offset:len(data) if e < 0 else e]
        out.append(vspan.fold_line(vs, before, every, ln))
    return out


def row(chrom: bytes, pos: int, ref: bytes = b"A", info: bytes = b".", eol: bytes = b"\n") -> bytes:
    return chrom + b"\t%d\t.\t" % pos + ref + b"\tC\t.\t.\t" + info + eol


def body40(long_info: int = 1500, missing=()) -> bytes:
    """40 rows over three contigs: reference blocks, REF of several bases, an END far ahead, equal POS, and one row
    whose INFO of ``long_info`` bytes carries its END last, so that a part's look-ahead cuts it.  ``missing``: the
    ordinals whose REF is emptied."""
    rows = []
    for i in range(22):
        p = 10 * i + 1
        info = (b"END=%d" % (p + 9), b"DP=3", b"SVTYPE=DEL;END=%d" % (p + 300), b"END=.", b"CIEND=0,5")[i % 5]
        rows.append((b"chr1", p, (b"A", b"ACGT", b"AC")[i % 3], info))
    rows.append((b"chr2", 7, b"ACGTACGT", b"NS=1"))
    for i in range(17):
        p = 3 + 4 * (i // 2)
        rows.append((b"chr3", p, b"A" * (1 + i % 4), b"END=%d;X=1" % (p + i) if i % 3 else b"X=2"))
    rows[30] = (b"chr3", rows[30][1], b"AC", b"N=" + b"v" * long_info + b";END=%d" % (rows[30][1] + 50))
    return b"".join(row(c, p, b"" if i in missing else r, f) for i, (c, p, r, f) in enumerate(rows))
