"""Device-resident rate of the FASTQ read index's launches (libdpfq.so), for DESIGN.md §4.9 and the README row.

    python tools/fastq_index_rate.py [--gib G | --mib M] [--reps R] [--every K] [--e2e-gib E] [--no-resources]

One process.  Two buffers of about the asked size, one after the other resident on the device: whole copies of a
``synth.fastq`` block (100-base reads) and of a ``synth.fastq_long`` block (log-uniform 100 .. 100 000 bases).  Per
buffer, after 2 warm-ups of each, R alternated launches of
* ``dp_stream_read`` and the uint64 newline launch (``dp_delim_ranges`` out_mode 1, emit_add 1: the line starts), timed
  by the library's own HIP events;
* read (``dfq_reads_async``: the initialisation of the result words and fq_read_kernel), scan (``dfq_scan_async``) and
  sample (``dfq_sample_async``), HIP events on the context stream around each call.
The last outputs are verified on the host against the block's own lines: reads, bases, shortest and longest read, no
malformed read, and the samples.  The kernels' register counts and waves per SIMD come from a compile of dpfq.hip with
-Rpass-analysis=kernel-resource-usage.  ``--e2e-gib E`` (0: skip) then times ``co.preprocess()`` of an E GiB FASTQ in
a memory store, best of three after a warm call.  Prints one JSON line.
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

from dataplug_amd import build as B  # noqa: E402
from dataplug_amd import synth  # noqa: E402
from dataplug_amd.scan import _fq, get_context  # noqa: E402

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


def resources() -> dict:
    """Per kernel of dpfq.hip: VGPRs, SGPRs, LDS bytes, scratch bytes and waves per SIMD, as the compiler reports."""
    hipcc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    with tempfile.TemporaryDirectory(prefix="dpfq_res_") as d:
        r = subprocess.run([hipcc, f"--offload-arch={B.ARCH}", "-O3", "-std=c++17", "-fPIC", "-shared",
                            "-Rpass-analysis=kernel-resource-usage", "-o", os.path.join(d, "x.so"), B.FQ_SRC],
                           capture_output=True, text=True, cwd=d)
    out, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: \S*?(fq_\w+?_kernel)", line)
        if m:
            name = m.group(1)
            out[name] = {}
        for key, pat in (("vgprs", r" VGPRs: (\d+)"), ("sgprs", r"TotalSGPRs: (\d+)"), ("lds_bytes", r"LDS Size.*: (\d+)"),
                         ("scratch_bytes", r"ScratchSize.*: (\d+)"), ("waves_per_simd", r"Occupancy.*: (\d+)")):
            m = re.search(pat, line)
            if m and name:
                out[name][key] = int(m.group(1))
    return out


def tiled(block: np.ndarray, size: int) -> np.ndarray:
    """Whole copies of ``block`` (whole reads), about ``size`` bytes."""
    return np.tile(block, max(1, size // len(block)))


def block_lines(block: np.ndarray):
    """(line starts, sequence lengths) of a block of well-formed reads that ends in '\\n'."""
    nl = np.flatnonzero(block == 10).astype(np.int64)
    st = np.concatenate([[0], nl[:-1] + 1])
    cr = (block[nl - 1] == 13).astype(np.int64)
    return st, (nl - st - cr)[1::4]


def measure(ctx, name: str, block: np.ndarray, size: int, reps: int, K: int) -> dict:
    a = tiled(block, size)
    n, copies = len(a), len(a) // len(block)
    st, lens = block_lines(block)
    nr_block = len(lens)
    nl, nr = 4 * nr_block * copies, nr_block * copies
    d = ctx.workspace("fq_rate_in", n + 64, placed=True)
    for lo in range(0, n, 256 << 20):
        ctx.h2d(d.ptr + lo, a[lo:lo + (256 << 20)])
    del a
    cap = nl + 1024
    ws = ctx.workspace("fq_rate_starts", 8 * (cap + 1) + 16)
    ctx.h2d(ws.ptr, np.array([0], np.uint64))             # line 0's start in front of the newline launch's output
    g = ctx.fq_geometry()[0]
    nb, ns = -(-nr // g), -(-nr // K)
    out = ctx.workspace("fq_rate_out", 48 + 16 * ns + 8 * nb + 5 * nr + 64)
    d_res, d_smp = out.ptr, out.ptr + 48
    d_block = d_smp + 16 * ns
    d_len = d_block + 8 * nb
    d_flags = d_len + 4 * nr
    f, h = ctx._fq_ctx()
    ev = Events(ctx.stream)
    p = ctypes.c_void_p
    rg = np.array([0, n], np.uint64)
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

    def reads():
        ev.start()
        _fq.check(f.dfq_reads_async(h, p(d.ptr), n, 0, n, p(ws.ptr), 0, nr, n - 1, p(d_len), p(d_flags), p(d_block),
                                    p(d_res)))
        return ev.stop_ms()

    def scan():
        ev.start()
        _fq.check(f.dfq_scan_async(h, p(d_block), nb, p(d_res)))
        return ev.stop_ms()

    def sample():
        ev.start()
        _fq.check(f.dfq_sample_async(h, p(ws.ptr), 0, p(d_len), p(d_block), nr, 0, K, p(d_smp)))
        return ev.stop_ms()

    steps = (read, newline, reads, scan, sample)
    ctx.timing(True)
    for _ in range(2):
        for s in steps:
            s()
    ts = [[] for _ in steps]
    for _ in range(reps):
        for t, s in zip(ts, steps):
            t.append(s())
    ctx.timing(False)
    tr, tn, tq, tc, tp = ts

    # ---- the last outputs against the block's own lines
    res = ctx.d2h(np.empty(_fq.R_WORDS, np.uint64), d_res)
    smp = ctx.d2h(np.empty(2 * ns, np.uint64), d_smp).reshape(-1, 2)
    r = np.arange(0, nr, K, dtype=np.int64)
    cum = np.concatenate([[0], np.cumsum(lens)])
    want_off = (r // nr_block) * len(block) + st[4 * (r % nr_block)]
    want_bases = (r // nr_block) * int(cum[-1]) + cum[r % nr_block]
    ok = {
        "counts": bool(int(res[_fq.R_MALFORMED]) == 0 and int(res[_fq.R_BASES]) == int(cum[-1]) * copies),
        "min_max": bool(int(res[_fq.R_MIN_LEN]) == int(lens.min()) and int(res[_fq.R_MAX_LEN]) == int(lens.max())),
        "samples": bool(np.array_equal(smp[:, 0], want_off.astype(np.uint64))
                        and np.array_equal(smp[:, 1], want_bases.astype(np.uint64))),
    }

    def stat(t):
        return [round(float(np.median(t)), 3), round(min(t), 3), round(max(t), 3)]

    med = lambda t: float(np.median(t))                                     # noqa: E731
    three = med(tq) + med(tc) + med(tp)
    return {
        "input": name, "bytes": n, "reads": nr, "lines": nl, "bases": int(cum[-1]) * copies, "every": K, "reps": reps,
        "stream_read_ms": stat(tr), "newline_u64_ms": stat(tn), "read_ms": stat(tq), "scan_ms": stat(tc),
        "sample_ms": stat(tp),
        "stream_read_GiB_per_s": round(n16 / (med(tr) / 1e3) / GiB, 1),
        "newline_GiB_per_s": round(n / (med(tn) / 1e3) / GiB, 1),
        "read_kernel_reads_per_us": round(nr / (med(tq) * 1e3), 1),
        "read_kernel_time_over_stream_read": round(med(tq) / med(tr), 3),
        "read_kernel_time_over_newline": round(med(tq) / med(tn), 3),
        "three_launches_time_over_stream_read": round(three / med(tr), 3),
        "three_launches_time_over_newline": round(three / med(tn), 3),
        "verified": ok}


def e2e(gib: float) -> dict:
    from dataplug_amd.cloudobject import CloudObject
    from dataplug_amd.formats.genomics import fastq as ffq
    from dataplug_amd.storage import MemoryStore
    data = tiled(synth.fastq(200_000, seed=35), int(gib * GiB))
    MemoryStore._named.pop("fastq_rate", None)
    cfg = {"endpoint_url": "memory://fastq_rate"}
    co = CloudObject.from_s3(ffq.FASTQ, "s3://rate/e2e.fastq", fetch=False, s3_config=cfg)
    co.storage.create_bucket(Bucket="rate")
    co.storage.put_object(Body=data.tobytes(), Bucket="rate", Key="e2e.fastq")
    co = CloudObject.from_s3(ffq.FASTQ, "s3://rate/e2e.fastq", s3_config=cfg)
    ts = []
    for _ in range(4):                                    # a warm call, then three
        t = time.perf_counter()
        co.preprocess(extra_args={"dataplug_devices": [0]}, force=True)
        ts.append(time.perf_counter() - t)
    return {"bytes": len(data), "preprocess_s": [round(x, 4) for x in ts], "best_s": round(min(ts[1:]), 4),
            "GiB_per_s": round(len(data) / GiB / min(ts[1:]), 2), "reads": int(co.attributes.num_reads)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=4.0)
    ap.add_argument("--mib", type=float, default=None, help="buffer size in MiB instead of --gib")
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--every", type=int, default=64)
    ap.add_argument("--e2e-gib", type=float, default=1.0)
    ap.add_argument("--no-resources", action="store_true")
    args = ap.parse_args()
    n = int((args.mib * (1 << 20)) if args.mib is not None else (args.gib * (1 << 30)))
    ctx = get_context(0)
    runs = [measure(ctx, "synth.fastq", synth.fastq(min(200_000, max(8, n // 250)), seed=33), n, args.reps, args.every),
            measure(ctx, "synth.fastq_long", synth.fastq_long(min(2_000, max(8, n // 30_000)), seed=34), n, args.reps,
                    args.every)]
    line = {"reads_per_workgroup_scan_lanes": ctx.fq_geometry(), "runs": runs}
    if not args.no_resources:
        line["kernel_resources"] = resources()
    if args.e2e_gib > 0:
        line["e2e"] = e2e(args.e2e_gib)
    print(json.dumps(line), flush=True)
    return 0 if all(all(r["verified"].values()) for r in runs) else 1


if __name__ == "__main__":
    sys.exit(main())
