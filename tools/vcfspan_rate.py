"""Device-resident rate of the VCF record-end index's launches (libdpvspan.so), for DESIGN.md §4.10 and the README row.

    python tools/vcfspan_rate.py [--gib G | --mib M] [--reps R] [--every K] [--e2e-gib E] [--shape gvcf|vcf_sorted|both]
                                 [--resources 0|1]

One process; per shape one buffer of the asked size resident on the device (``synth.gvcf``, and the ``synth.vcf_sorted``
that tools/vcfpos_rate.py uses).  After 2 warm-ups of each, R alternated launches of
* ``dp_stream_read`` and the uint64 newline launch (the line starts), timed by the library's own HIP events;
* parse (``dvp_parse_async``), span (``dvs_span_async``) and block-max (``dvs_blockmax_async``), HIP events on the
  context stream around the whole call (block-max: the initialisation of the slots and result words and the kernel).
The last outputs are verified on the host: the first 2^17 lines' ``end`` and ``flags`` and their slots against the
definition (``scan.vspan.rec_end``), no MISSING_REF and no TRUNCATED line, and for ``vcf_sorted`` every ``end`` equal to
its POS.  The kernels' VGPRs, waves per SIMD and scratch come from a verbose build's resource report.  ``--e2e-gib E``
(0: skip) then times ``co.preprocess()`` of an E GiB object in a memory store without an index, with ``pos_index`` and
with ``span_index`` added, best of three after a warm call.  Prints one JSON line per shape.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from dataplug_amd import synth  # noqa: E402
from dataplug_amd.scan import _vpos, _vspan, get_context, vspan  # noqa: E402
from vcfpos_rate import Events, GiB, host_lines  # noqa: E402


def resources() -> dict:
    """{kernel: [VGPRs, waves per SIMD, scratch bytes per lane]} from the compiler's resource report."""
    from dataplug_amd import build as B
    with tempfile.TemporaryDirectory(prefix="vcfspan_rate_") as tmp:     # compiled aside: nothing is installed
        code = (f"from dataplug_amd import build as B; B.build(verbose=True, out={os.path.join(tmp, 'x.so')!r}, "
                f"src=B.VSPAN_SRC, required=B.VSPAN_REQUIRED)")
        text = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True,
                              cwd=os.path.dirname(B.HERE)).stderr
    out = {}
    for m in re.finditer(r"Function Name: \S*?(vspan_\w+?_kernel)\S*.*?VGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+)"
                         r".*?Occupancy \[waves/SIMD\]: (\d+)", text, re.S):
        out[m.group(1)] = [int(m.group(2)), int(m.group(4)), int(m.group(3))]
    return out


def e2e(gib: float, shape: str) -> dict:
    from dataplug_amd.cloudobject import CloudObject
    from dataplug_amd.formats.genomics import vcf as fvcf
    from dataplug_amd.storage import MemoryStore
    data = getattr(synth, shape)(int(gib * GiB), seed=33)
    MemoryStore._named.pop("vcfspan_rate", None)
    cfg = {"endpoint_url": "memory://vcfspan_rate"}
    co = CloudObject.from_s3(fvcf.VCF, "s3://rate/e2e.vcf", fetch=False, s3_config=cfg)
    co.storage.create_bucket(Bucket="rate")
    co.storage.put_object(Body=data.tobytes(), Bucket="rate", Key="e2e.vcf")
    co = CloudObject.from_s3(fvcf.VCF, "s3://rate/e2e.vcf", s3_config=cfg)
    out = {"bytes": len(data)}
    for name, extra in (("without", {}), ("with_pos_index", {"pos_index": True}),
                        ("with_span_index", {"pos_index": True, "span_index": True})):
        ts = []
        for _ in range(4):                                # a warm call, then three
            t = time.perf_counter()
            co.preprocess(extra_args=dict(extra, dataplug_devices=[0]), force=True)
            ts.append(time.perf_counter() - t)
        out[name + "_s"] = [round(x, 4) for x in ts]
        out[name + "_best_s"] = round(min(ts[1:]), 4)
    out["lines"] = int(co.attributes.num_body_lines)
    out["max_span"] = int(co.attributes.max_span)
    return out


def run(shape: str, n: int, K: int, reps: int, e2e_gib: float, res: dict) -> bool:
    a = getattr(synth, shape)(n, seed=31)
    bo = len(synth.VCF_HEADER)
    starts = host_lines(a, bo)
    nl = len(starts)
    ctx = get_context(0)
    d = ctx.workspace("vcfspan_rate_in", n + 64, placed=True)
    for lo in range(0, n, 256 << 20):
        ctx.h2d(d.ptr + lo, a[lo:lo + (256 << 20)])
    cap = nl + 1024
    ws = ctx.workspace("vcfspan_rate_starts", 8 * (cap + 1) + 16)
    ctx.h2d(ws.ptr, np.array([bo], np.uint64))            # line 0's start in front of the newline launch's output
    lines = ctx.workspace("vcfspan_rate_lines", 12 * nl + 64)
    d_pos, d_end = lines.ptr, lines.ptr + 4 * nl
    d_clen, d_flags, d_sflags = d_end + 4 * nl, d_end + 6 * nl, d_end + 7 * nl
    ns = -(-nl // K)
    out = ctx.workspace("vcfspan_rate_out", 64 + 4 * ns + 64)
    d_res, d_max = out.ptr, out.ptr + 64
    v, h = ctx._vpos_ctx()
    s, hs = ctx._vspan_ctx()
    ev = Events(ctx.stream)
    p = ctypes.c_void_p
    rg = np.array([bo, n], np.uint64)
    n16 = n // 16 * 16

    def timed(fn):
        ctx.timing_read()
        fn()
        ms, k = ctx.timing_read()
        assert k >= 1
        return ms

    def read():
        return timed(lambda: ctx.stream_read(d.ptr, n16))

    def newline():
        def go():
            ctx.delim_ranges_async(d.ptr, n, 0, rg, 10, 1, 1, 0, ws.ptr + 8, 1, cap)
            return ctx.delim_ranges_result(1)
        return timed(go)

    def parse():
        ev.start()
        _vpos.check(v.dvp_parse_async(h, p(d.ptr), n, 0, n, p(ws.ptr), nl, p(d_pos), p(d_clen), p(d_flags)))
        return ev.stop_ms()

    def span():
        ev.start()
        _vspan.check(s.dvs_span_async(hs, p(d.ptr), n, 0, n, p(ws.ptr), nl, p(d_pos), p(d_end), p(d_sflags)))
        return ev.stop_ms()

    def blockmax():
        ev.start()
        _vspan.check(s.dvs_blockmax_async(hs, p(d_end), p(d_sflags), p(d_pos), nl, 0, K, p(d_max), p(d_res)))
        return ev.stop_ms()

    ctx.timing(True)
    for _ in range(2):
        read(), newline(), parse(), span(), blockmax()
    tr, tn, tp, ts, tb = [], [], [], [], []
    for _ in range(reps):
        tr.append(read())
        tn.append(newline())
        tp.append(parse())
        ts.append(span())
        tb.append(blockmax())
    ctx.timing(False)

    # ---- the last outputs against the definition on the host
    r = ctx.d2h(np.empty(_vspan.R_WORDS, np.uint64), d_res)
    slots = ctx.d2h(np.empty(ns, np.uint32), d_max)
    head = min(nl - 1, 1 << 17) // K * K
    end_head = ctx.d2h(np.empty(head, np.uint32), d_end)
    pos_head = ctx.d2h(np.empty(head, np.uint32), d_pos)
    fl_head = ctx.d2h(np.empty(head, np.uint8), d_sflags)
    raw = a[:int(starts[head])].tobytes()
    want = [vspan.rec_end(raw[int(x):int(y) - 1], int(q)) for x, y, q in zip(starts[:head], starts[1:head + 1], pos_head)]
    w_end = np.array([w[0] for w in want], np.uint32)
    ok = {
        "end": bool(np.array_equal(end_head, w_end)),
        "flags": bool(np.array_equal(fl_head, np.array([w[1] for w in want], np.uint8))),
        "slots": bool(np.array_equal(slots[:head // K], w_end.reshape(-1, K).max(axis=1))),
        "clean": bool(r[_vspan.R_MISSING] == 0 and r[_vspan.R_TRUNCATED] == 0),
    }
    if shape == "vcf_sorted":
        all_end = ctx.d2h(np.empty(nl, np.uint32), d_end)
        all_pos = ctx.d2h(np.empty(nl, np.uint32), d_pos)
        ok["end_is_pos"] = bool(np.array_equal(all_end, all_pos) and r[_vspan.R_MAX_SPAN] == 0)

    def stat(t):
        return [round(float(np.median(t)), 3), round(min(t), 3), round(max(t), 3)]

    med = lambda t: float(np.median(t))                                     # noqa: E731
    rate = lambda t, nb: round(nb / (med(t) / 1e3) / GiB, 1)                # noqa: E731
    line = {
        "shape": shape, "bytes": n, "lines": nl, "every": K, "reps": reps, "lines_per_workgroup": ctx.vspan_geometry(),
        "from_end": int(r[_vspan.R_FROM_END]), "max_span": int(r[_vspan.R_MAX_SPAN]),
        "stream_read_ms": stat(tr), "newline_u64_ms": stat(tn), "parse_ms": stat(tp), "span_ms": stat(ts),
        "blockmax_ms": stat(tb),
        "stream_read_GiB_per_s": rate(tr, n16), "newline_GiB_per_s": rate(tn, n), "parse_GiB_per_s": rate(tp, n),
        "span_GiB_per_s": rate(ts, n), "blockmax_GiB_per_s": rate(tb, n),
        "span_lines_per_us": round(nl / (med(ts) * 1e3), 1), "blockmax_lines_per_us": round(nl / (med(tb) * 1e3), 1),
        "span_rate_as_fraction_of_stream_read": round(med(tr) / med(ts), 3),
        "span_rate_as_fraction_of_parse": round(med(tp) / med(ts), 3),
        "span_rate_as_fraction_of_newline": round(med(tn) / med(ts), 3),
        "blockmax_rate_as_fraction_of_stream_read": round(med(tr) / med(tb), 3),
        "blockmax_rate_as_fraction_of_parse": round(med(tp) / med(tb), 3),
        "blockmax_rate_as_fraction_of_newline": round(med(tn) / med(tb), 3),
        "resources_vgprs_waves_scratch": res, "verified": ok}
    del a, starts, raw
    if e2e_gib > 0:
        line["e2e"] = e2e(e2e_gib, shape)
    print(json.dumps(line), flush=True)
    return all(ok.values()) and all(x[2] == 0 for x in res.values())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=4.0)
    ap.add_argument("--mib", type=float, default=None, help="buffer size in MiB instead of --gib")
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--every", type=int, default=128)
    ap.add_argument("--e2e-gib", type=float, default=1.0)
    ap.add_argument("--shape", default="both", choices=["gvcf", "vcf_sorted", "both"])
    ap.add_argument("--resources", type=int, default=1, help="0: skip the verbose compile behind the resource report")
    args = ap.parse_args()
    n = int((args.mib * (1 << 20)) if args.mib is not None else (args.gib * (1 << 30)))
    res = resources() if args.resources else {}
    shapes = ["gvcf", "vcf_sorted"] if args.shape == "both" else [args.shape]
    good = [run(sh, n, args.every, args.reps, args.e2e_gib, res) for sh in shapes]
    return 0 if all(good) else 1


if __name__ == "__main__":
    sys.exit(main())
