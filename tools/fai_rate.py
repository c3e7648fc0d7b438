"""Device-resident rate of the .fai counts (libdpfai.so: fai_count_kernel's two passes), for DESIGN.md §4.7 and the
README row.

    python tools/fai_rate.py [--gib G | --mib M] [--reps R] [--block-mib B] [--dense | --seq-min A --seq-max B]

A ``synth.fasta`` block (B MiB, its last byte made a line break) is copied end to end into one device buffer of the
asked size, so the expected counts are the block's, repeated.  ``--dense`` uses ``seq_min=50, seq_max=150``: several
sequences in every 16 KiB range, which takes the kernel's general (LDS slot) path instead of the one-segment fast
path; ``--seq-min 1000000 --seq-max 3000000`` is a genome's shape (bodies far longer than a range: the fast path).
On that one buffer, in one process, after 2 warm-ups of each, R alternated launches of
* ``dp_stream_read`` and ``dp_fasta_index`` (the header index), timed by the library's own HIP events;
* pass 1 (``dfai_count_async``) and pass 2 (``dfai_offgrid_async``), HIP events on the context stream around the whole
  call: the per-launch initialisation of the outputs and the kernel (the segments are resident).
Prints one JSON line: medians with min-max, each pass as a fraction of the same run's ``dp_stream_read`` rate, the
share of the 16 KiB ranges that took the fast path, and whether the last outputs equal numpy's.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from dataplug_amd import synth  # noqa: E402
from dataplug_amd.scan import _fai, get_context  # noqa: E402
from dataplug_amd.scan import fai as sfai  # noqa: E402

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


def block_counts(block: np.ndarray):
    """(pairs, b, e, nl, cr, first, width, off, lastoff) of one block by numpy (bodies between header lines)."""
    gt = np.flatnonzero(block == 62)
    starts = gt[(gt == 0) | (block[np.maximum(gt, 1) - 1] == 10)]
    nlpos = np.flatnonzero(block == 10)
    hend = nlpos[np.searchsorted(nlpos, starts)] + 1
    pairs = np.stack([starts, hend], 1).astype(np.uint64)
    b, e = sfai.bodies(pairs, len(block))
    cn = np.concatenate([[0], np.cumsum(block == 10)]).astype(np.uint64)
    cc = np.concatenate([[0], np.cumsum(block == 13)]).astype(np.uint64)
    bi, ei = b.astype(np.int64), e.astype(np.int64)
    nl, cr = cn[ei] - cn[bi], cc[ei] - cc[bi]
    k = np.searchsorted(nlpos, bi)
    first = np.where(nl > 0, nlpos[np.minimum(k, len(nlpos) - 1)], -1).astype(np.uint64)
    first[nl == 0] = sfai.NONE
    width = sfai.line_widths(b, e, nl, first)
    seg = np.searchsorted(bi, nlpos, "right") - 1
    inside = (seg >= 0) & (nlpos < ei[np.maximum(seg, 0)])
    p, s = nlpos[inside], seg[inside]
    bad = (p - bi[s] + 1) % width[s].astype(np.int64) != 0
    off = np.bincount(s[bad], minlength=len(b)).astype(np.uint64)
    last = np.zeros(len(b), np.int64)
    np.maximum.at(last, s[bad], p[bad])
    return pairs, b, e, nl, cr, first, width, off, last.astype(np.uint64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=4.0)
    ap.add_argument("--mib", type=float, default=None, help="buffer size in MiB instead of --gib")
    ap.add_argument("--block-mib", type=int, default=32)
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--dense", action="store_true", help="seq_min=50, seq_max=150: the LDS path")
    ap.add_argument("--seq-min", type=int, default=None)
    ap.add_argument("--seq-max", type=int, default=None)
    args = ap.parse_args()
    want = int((args.mib * (1 << 20)) if args.mib is not None else (args.gib * (1 << 30)))
    shape = {"seq_min": 50, "seq_max": 150} if args.dense else {}
    if args.seq_min is not None:
        shape = {"seq_min": args.seq_min, "seq_max": args.seq_max or 3 * args.seq_min}
    block = synth.fasta(min(args.block_mib << 20, want), seed=31, **shape).copy()
    block[-1] = 10
    copies = max(1, want // len(block))
    n = copies * len(block)
    pairs, b, e, nl, cr, first, width, off, last = block_counts(block)
    shift = (np.arange(copies, dtype=np.uint64) * np.uint64(len(block)))[:, None]
    tile = lambda a: (a[None, :] + shift).reshape(-1)                       # noqa: E731
    rep = lambda a: np.tile(a, copies)                                      # noqa: E731
    lo, hi = tile(b), tile(e)
    exp1 = (rep(nl), rep(cr), np.where(rep(nl) > 0, tile(first), sfai.NONE))
    exp2 = (rep(off), np.where(rep(off) > 0, tile(last), 0).astype(np.uint64))
    nseg = len(lo)

    ctx = get_context(0)
    d = ctx.workspace("fai_rate_in", n + 64, placed=True)
    for i in range(copies):
        ctx.h2d(d.ptr + i * len(block), block)
    seg = ctx.workspace("fai_rate_seg", 7 * 8 * nseg + 64)
    d_lo, d_hi, d_out, d_w = seg.ptr, seg.ptr + 8 * nseg, seg.ptr + 16 * nseg, seg.ptr + 40 * nseg
    ctx.h2d(d_lo, lo)
    ctx.h2d(d_hi, hi)
    ctx.h2d(d_w, rep(width).astype(np.uint32))
    f, h = ctx._fai_ctx()
    R, K, waves = ctx.fai_geometry()
    r0 = np.arange(0, n, R, dtype=np.uint64)
    k0 = np.searchsorted(hi, r0, "right")
    ok0 = k0 < nseg
    k0 = np.minimum(k0, nseg - 1)
    fast = ok0 & (lo[k0] <= r0) & (hi[k0] >= np.minimum(r0 + np.uint64(R), np.uint64(n)))
    ev = Events(ctx.stream)
    p = ctypes.c_void_p
    n16 = n // 16 * 16
    chunk = 64 << 20
    plan = np.array([[a, min(n, a + chunk)] for a in range(0, n, chunk)], np.uint64).reshape(-1)
    hcap = copies * len(pairs) + 1024
    hout = ctx.workspace("fai_rate_headers", 16 * hcap)

    def pass1():
        ev.start()
        _fai.check(f.dfai_count_async(h, p(d.ptr), n, 0, p(d_lo), p(d_hi), p(d_lo), nseg, p(d_out),
                                      p(d_out + 8 * nseg), p(d_out + 16 * nseg)))
        return ev.stop_ms()

    def pass2():
        ev.start()
        _fai.check(f.dfai_offgrid_async(h, p(d.ptr), n, 0, p(d_lo), p(d_hi), p(d_lo), p(d_w), nseg, p(d_out),
                                        p(d_out + 8 * nseg)))
        return ev.stop_ms()

    def timed(fn):
        ctx.timing_read()
        fn()
        ms, k = ctx.timing_read()
        assert k >= 1
        return ms

    def read():
        return timed(lambda: ctx.stream_read(d.ptr, n16))

    def headers():
        def go():
            ctx.fasta_index_async(d.ptr, n, 0, n, plan, hout.ptr, True, hcap)
            return ctx.fasta_result(len(plan) // 2)
        return timed(go)

    ctx.timing(True)
    for _ in range(2):
        read(), headers(), pass1(), pass2()
    tr, th, t1, t2 = [], [], [], []
    for i in range(args.reps):
        tr.append(read())
        th.append(headers())
        t2.append(pass2())
        if i == args.reps - 1:
            got2 = ctx.d2h(np.empty((2, nseg), np.uint64), d_out)
        t1.append(pass1())
    ctx.timing(False)
    got1 = ctx.d2h(np.empty((3, nseg), np.uint64), d_out)
    ok1 = all(np.array_equal(g, x) for g, x in zip(got1, exp1))
    ok2 = all(np.array_equal(g, x) for g, x in zip(got2, exp2))

    def stat(ts):
        return [round(float(np.median(ts)), 3), round(min(ts), 3), round(max(ts), 3)]

    def rate(ts, nbytes):
        return round(nbytes / (float(np.median(ts)) / 1e3) / GiB, 1)

    rr = rate(tr, n16)
    print(json.dumps({
        "bytes": n, "dense": bool(args.dense), "shape": shape, "segments": nseg, "reps": args.reps,
        "range_bytes_slots_waves": [R, K, waves], "fast_path_share_of_ranges": round(float(fast.mean()), 4),
        "stream_read_ms": stat(tr), "fasta_index_ms": stat(th), "pass1_ms": stat(t1), "pass2_ms": stat(t2),
        "stream_read_GiB_per_s": rr, "fasta_index_GiB_per_s": rate(th, n), "pass1_GiB_per_s": rate(t1, n),
        "pass2_GiB_per_s": rate(t2, n), "pass1_ratio_to_stream_read": round(rate(t1, n) / rr, 3),
        "pass2_ratio_to_stream_read": round(rate(t2, n) / rr, 3),
        "fasta_index_ratio_to_stream_read": round(rate(th, n) / rr, 3),
        "verified_pass1": bool(ok1), "verified_pass2": bool(ok2)}), flush=True)
    return 0 if ok1 and ok2 else 1


if __name__ == "__main__":
    sys.exit(main())
