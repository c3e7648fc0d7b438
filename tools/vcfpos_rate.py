"""Device-resident rate of the VCF position index's launches (libdpvpos.so), for DESIGN.md §4.8 and the README row.

    python tools/vcfpos_rate.py [--gib G | --mib M] [--reps R] [--every K] [--e2e-gib E]

One process, one ``synth.vcf_sorted`` buffer of the asked size resident on the device.  After 2 warm-ups of each, R
alternated launches of
* ``dp_stream_read`` and the uint64 newline launch (``dp_delim_ranges`` out_mode 1, emit_add 1: the line starts), timed
  by the library's own HIP events;
* parse (``dvp_parse_async``) and reduce (``dvp_reduce_async``), HIP events on the context stream around the whole call
  (reduce: the initialisation of the result words and the kernel).
The last outputs are verified in numpy on the host: the number of lines, the samples against the POS digits of every
K-th line, the runs against the lines where CHROM changes, a stretch of the per-line ``pos`` array, no malformed and
no unsorted line.  ``--e2e-gib E`` (0: skip) then times ``co.preprocess()`` of an E GiB ``vcf_sorted`` in a memory
store with and without ``pos_index``, best of three after a warm call.  Prints one JSON line.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from dataplug_amd import synth  # noqa: E402
from dataplug_amd.scan import _vpos, get_context  # noqa: E402

GiB = float(1 << 30)


class Events:
    """A pair of HIP events on one stream (the runtime libdpscan already loaded)."""

    def __init__(self, stream: int):
        self.hip = ctypes.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))
        self.stream = ctypes.c_void_p(stream)
        self.a, self.b = ctypes.c_void_p(), ctypes.c_void_p()
        for e in (self.a, self.b):
            self._ok(self.hip.hipEventCreate(ctypes.byref(e)))

    @staticmethod
    def _ok(rc):
        if rc:
            raise RuntimeError(f"HIP event call failed: {rc}")

    def start(self):
        self._ok(self.hip.hipEventRecord(self.a, self.stream))

    def stop_ms(self) -> float:
        self._ok(self.hip.hipEventRecord(self.b, self.stream))
        self._ok(self.hip.hipEventSynchronize(self.b))
        ms = ctypes.c_float(0)
        self._ok(self.hip.hipEventElapsedTime(ctypes.byref(ms), self.a, self.b))
        return float(ms.value)


def host_lines(a: np.ndarray, bo: int) -> np.ndarray:
    """The line starts of the body, in pieces (no 4 GiB temporaries)."""
    out, step = [np.array([bo], np.int64)], 256 << 20
    for lo in range(bo, len(a), step):
        out.append(np.flatnonzero(a[lo:lo + step] == 10).astype(np.int64) + lo + 1)
    st = np.concatenate(out)
    return st[st < len(a)]


def host_fields(a: np.ndarray, starts: np.ndarray):
    """(CHROM length, POS) of the lines at ``starts`` of a vcf_sorted object: chrN / chrNN and nine digits."""
    cl = np.where(a[starts + 4] == 9, 4, 5)
    dig = a[(starts + cl + 1)[:, None] + np.arange(9)].astype(np.int64) - 48
    return cl, dig @ (10 ** np.arange(8, -1, -1))


def e2e(gib: float) -> dict:
    from dataplug_amd.cloudobject import CloudObject
    from dataplug_amd.formats.genomics import vcf as fvcf
    from dataplug_amd.storage import MemoryStore
    data = synth.vcf_sorted(int(gib * GiB), seed=33)
    MemoryStore._named.pop("vcfpos_rate", None)
    cfg = {"endpoint_url": "memory://vcfpos_rate"}
    co = CloudObject.from_s3(fvcf.VCF, "s3://rate/e2e.vcf", fetch=False, s3_config=cfg)
    co.storage.create_bucket(Bucket="rate")
    co.storage.put_object(Body=data.tobytes(), Bucket="rate", Key="e2e.vcf")
    co = CloudObject.from_s3(fvcf.VCF, "s3://rate/e2e.vcf", s3_config=cfg)
    out = {"bytes": len(data)}
    for name, extra in (("without", {}), ("with_pos_index", {"pos_index": True})):
        ts = []
        for _ in range(4):                                # a warm call, then three
            t = time.perf_counter()
            co.preprocess(extra_args=dict(extra, dataplug_devices=[0]), force=True)
            ts.append(time.perf_counter() - t)
        out[name + "_s"] = [round(x, 4) for x in ts]
        out[name + "_best_s"] = round(min(ts[1:]), 4)
    out["lines"] = int(co.attributes.num_body_lines)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=4.0)
    ap.add_argument("--mib", type=float, default=None, help="buffer size in MiB instead of --gib")
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--every", type=int, default=128)
    ap.add_argument("--e2e-gib", type=float, default=1.0)
    args = ap.parse_args()
    n = int((args.mib * (1 << 20)) if args.mib is not None else (args.gib * (1 << 30)))
    K = args.every
    a = synth.vcf_sorted(n, seed=31)
    bo = len(synth.VCF_HEADER)
    starts = host_lines(a, bo)
    nl = len(starts)

    ctx = get_context(0)
    d = ctx.workspace("vcfpos_rate_in", n + 64, placed=True)
    for lo in range(0, n, 256 << 20):
        ctx.h2d(d.ptr + lo, a[lo:lo + (256 << 20)])
    cap = nl + 1024
    ws = ctx.workspace("vcfpos_rate_starts", 8 * (cap + 1) + 16)
    ctx.h2d(ws.ptr, np.array([bo], np.uint64))            # line 0's start in front of the newline launch's output
    lines = ctx.workspace("vcfpos_rate_lines", 7 * nl + 64)
    d_pos, d_clen, d_flags = lines.ptr, lines.ptr + 4 * nl, lines.ptr + 6 * nl
    ns = -(-nl // K)
    rcap = 1024
    out = ctx.workspace("vcfpos_rate_out", 64 + 20 * rcap + 4 * ns + 64)
    d_res, d_runs = out.ptr, out.ptr + 64
    d_ends, d_rcl, d_smp = d_runs + 8 * rcap, d_runs + 16 * rcap, d_runs + 20 * rcap
    v, h = ctx._vpos_ctx()
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

    def reduce():
        ev.start()
        _vpos.check(v.dvp_reduce_async(h, p(d_pos), p(d_clen), p(d_flags), nl, 0, K, p(d_smp), p(d_runs), p(d_ends),
                                       p(d_rcl), rcap, p(d_res)))
        return ev.stop_ms()

    ctx.timing(True)
    for _ in range(2):
        read(), newline(), parse(), reduce()
    tr, tn, tp, td = [], [], [], []
    for _ in range(args.reps):
        tr.append(read())
        tn.append(newline())
        tp.append(parse())
        td.append(reduce())
    ctx.timing(False)

    # ---- the last outputs against numpy
    got_starts = ctx.d2h(np.empty(nl, np.uint64), ws.ptr)
    res = ctx.d2h(np.empty(_vpos.R_WORDS, np.uint64), d_res)
    smp = ctx.d2h(np.empty(ns, np.uint32), d_smp)
    m = int(res[_vpos.R_RUNS])
    runs = np.sort(ctx.d2h(np.empty(min(m, rcap), np.uint64), d_runs))
    ends = np.sort(ctx.d2h(np.empty(min(m, rcap), np.uint64), d_ends))
    head = min(nl, 1 << 20)
    pos_head = ctx.d2h(np.empty(head, np.uint32), d_pos)
    flags_head = ctx.d2h(np.empty(head, np.uint8), d_flags)
    cl, ps = host_fields(a, starts[::K])
    chrom = a[starts + 3].astype(np.int64) * 256 + a[starts + 4]          # chrN<tab> / chrNN: what tells contigs apart
    first = np.concatenate([[0], np.flatnonzero(chrom[1:] != chrom[:-1]) + 1])
    last = np.append(first[1:], nl) - 1
    _, pf = host_fields(a, starts[first])
    _, pl = host_fields(a, starts[last])
    clh, ph = host_fields(a, starts[:head])
    same = np.concatenate([[0], (chrom[1:head] == chrom[:head - 1]).astype(np.uint8)])
    ok = {
        "starts": bool(np.array_equal(got_starts, starts.astype(np.uint64))),
        "samples": bool(np.array_equal(smp, ps.astype(np.uint32))),
        "runs": bool(m == len(first) and np.array_equal(runs, (first.astype(np.uint64) << np.uint64(32)) | pf.astype(np.uint64))),
        "run_ends": bool(np.array_equal(ends, (last.astype(np.uint64) << np.uint64(32)) | pl.astype(np.uint64))),
        "pos": bool(np.array_equal(pos_head, ph.astype(np.uint32)) and np.array_equal(flags_head, same)),
        "clean": bool(res[_vpos.R_MALFORMED] == 0 and res[_vpos.R_UNSORTED] == 0),
    }

    def stat(ts):
        return [round(float(np.median(ts)), 3), round(min(ts), 3), round(max(ts), 3)]

    def rate(ts, nbytes):
        return round(nbytes / (float(np.median(ts)) / 1e3) / GiB, 1)

    med = lambda ts: float(np.median(ts))                                   # noqa: E731
    line = {
        "bytes": n, "lines": nl, "every": K, "runs": m, "reps": args.reps, "lines_per_workgroup": ctx.vpos_geometry(),
        "stream_read_ms": stat(tr), "newline_u64_ms": stat(tn), "parse_ms": stat(tp), "reduce_ms": stat(td),
        "stream_read_GiB_per_s": rate(tr, n16), "newline_GiB_per_s": rate(tn, n), "parse_GiB_per_s": rate(tp, n),
        "reduce_GiB_per_s": rate(td, n),
        "parse_lines_per_us": round(nl / (med(tp) * 1e3), 1), "reduce_lines_per_us": round(nl / (med(td) * 1e3), 1),
        "parse_rate_as_fraction_of_stream_read": round(med(tr) / med(tp), 3),
        "reduce_rate_as_fraction_of_stream_read": round(med(tr) / med(td), 3),
        "parse_rate_as_fraction_of_newline": round(med(tn) / med(tp), 3),
        "reduce_rate_as_fraction_of_newline": round(med(tn) / med(td), 3),
        "verified": ok}
    del a, starts, chrom
    if args.e2e_gib > 0:
        line["e2e"] = e2e(args.e2e_gib)
    print(json.dumps(line), flush=True)
    return 0 if all(ok.values()) else 1


if __name__ == "__main__":
    sys.exit(main())
