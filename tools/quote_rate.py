"""Device-resident rate of the quote-aware record index (libdpquote.so), for DESIGN.md and the README row.

    python tools/quote_rate.py [--gib G | --mib M] [--reps R] [--block-mib B]

A ``synth.csv_quoted`` block (B MiB, RFC 4180, ends at a record end) is copied end to end into one device buffer of
the asked size (whole blocks, so the expected record ends are the block's, shifted).  On that one buffer, in one
process, alternating launch by launch after a warm-up of each:
* ``dq_records_async`` (uint64 output), HIP events on the context stream around the whole call: the per-launch
  zeroing of the descriptors, the kernel and the 64-byte result copy;
* ``dq_records_blocked_async`` (u16b: uint16 low words + the 64 KiB block table), timed the same way;
* ``dq_records_esc_async`` (uint64 output, the escape-aware instantiation) on the same buffer with an escape byte that
  does not occur in it, so only the extra work is timed, and on a second buffer of ``synth.csv_escaped`` blocks;
* ``dp_stream_read``, the read-only calibration kernel, and ``dp_delim_index`` (uint64), the newline index, each timed
  by the library's own HIP events around its kernels (dp_timing_enable).
Prints one JSON line: the times and GiB/s (input bytes over time), the ratio of each record-index form's rate to the
read-only kernel's (and of the uint64 form's to the newline index's), the u16b form's time over the uint64 form's, and
whether the last output of each form, the u16b one decoded, equals the numpy model.
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
from dataplug_amd.scan import get_context  # noqa: E402
from dataplug_amd.scan.objects import BlockedOffsets  # noqa: E402

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


def model_ends(d: np.ndarray) -> np.ndarray:
    par = np.cumsum(d == 34, dtype=np.uint8) & np.uint8(1)
    return np.flatnonzero((d == 10) & (par == 0)).astype(np.uint64)


def escaped_ends(d: np.ndarray, q: int = 34, e: int = 92):
    """(record ends, toggles) by the definition's loop (scope "all"), visiting only the bytes that can matter."""
    pos = np.flatnonzero((d == q) | (d == e) | (d == 10))
    ends, esc_at, inside, tog = [], -1, 0, 0
    for p, b in zip(pos.tolist(), d[pos].tolist()):
        if p == esc_at:
            continue
        if b == e:
            esc_at = p + 1
        elif b == q:
            inside ^= 1
            tog += 1
        elif not inside:
            ends.append(p)
    return np.asarray(ends, np.uint64), tog


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=4.0)
    ap.add_argument("--mib", type=float, default=None, help="buffer size in MiB instead of --gib")
    ap.add_argument("--block-mib", type=int, default=32)
    ap.add_argument("--reps", type=int, default=12)
    args = ap.parse_args()
    assert args.reps >= 10, "at least 10 timed launches each"
    want = int((args.mib * (1 << 20)) if args.mib is not None else (args.gib * (1 << 30)))
    block = synth.csv_quoted(min(args.block_mib << 20, want), seed=21)
    copies = max(1, want // len(block))
    n = copies * len(block)
    ends = model_ends(block)
    assert int(np.count_nonzero(block == 34)) % 2 == 0 and int(ends[-1]) == len(block) - 1
    exp = np.concatenate([ends + np.uint64(i * len(block)) for i in range(copies)])
    absent = 1                                                      # an escape byte the quoted block does not hold
    assert not np.any(block == absent)
    eblock = synth.csv_escaped(len(block), seed=22)
    eends, etog = escaped_ends(eblock)
    assert int(eends[-1]) == len(eblock) - 1 and etog % 2 == 0
    eexp = np.concatenate([eends + np.uint64(i * len(eblock)) for i in range(copies)])

    ctx = get_context(0)
    d = ctx.workspace("quote_rate_in", n + 64, placed=True)
    for i in range(copies):
        ctx.h2d(d.ptr + i * len(block), block)
    d2 = ctx.workspace("quote_rate_in_escaped", n + 64, placed=True)
    for i in range(copies):
        ctx.h2d(d2.ptr + i * len(eblock), eblock)
    cap = max(len(exp), len(eexp)) + 1024
    nl_cap = copies * int(np.count_nonzero(block == 10)) + 1024
    out = ctx.workspace("quote_rate_out", 8 * max(cap, nl_cap))
    nt = ctx.record_block_tiles(0, n)
    low = ctx.workspace("quote_rate_low", 2 * cap)
    tab = ctx.workspace("quote_rate_blocks", 8 * nt)
    ev = Events(ctx.stream)
    n16 = n // 16 * 16

    def quote():
        ev.start()
        ctx.records_async(d.ptr, n, 0, 0, n, form="u64", d_out=out.ptr, cap=cap)
        ms = ev.stop_ms()
        return ms, ctx.records_result()

    def quote16():
        ev.start()
        ctx.records_async(d.ptr, n, 0, 0, n, form="u16b", d_out=low.ptr, cap=cap, d_table=tab.ptr, table_cap=nt)
        ms = ev.stop_ms()
        return ms, ctx.records_result()

    def quote_esc(buf, escape):
        ev.start()
        ctx.records_async(buf.ptr, n, 0, 0, n, escape=escape, form="u64", d_out=out.ptr, cap=cap)
        ms = ev.stop_ms()
        return ms, ctx.records_result()

    def timed(fn):
        ctx.timing_read()
        fn()
        ms, k = ctx.timing_read()
        assert k >= 1
        return ms

    def read():
        return timed(lambda: ctx.stream_read(d.ptr, n16))

    def delim():
        def go():
            ctx.delim_index_async(d.ptr, n, 0, 0, n, 10, 1, 0, out.ptr, True, nl_cap)
            ctx.delim_result()
        return timed(go)

    ctx.timing(True)
    for _ in range(2):                                              # warm-up of every kernel at this size
        quote(), quote16(), read(), delim(), quote_esc(d, absent), quote_esc(d2, 92)
    tq, tb, tr, td, te, te2 = [], [], [], [], [], []
    for _ in range(args.reps):
        tr.append(read())
        td.append(delim())
        ms, res16 = quote16()
        tb.append(ms)
        ms, rese2 = quote_esc(d2, 92)
        te2.append(ms)
        if _ == args.reps - 1:                                      # the escaped buffer's output, before it is reused
            gote2 = ctx.d2h(np.empty(min(rese2[0], cap), np.uint64), out.ptr)
        ms, rese = quote_esc(d, absent)
        te.append(ms)
        if _ == args.reps - 1:
            gote = ctx.d2h(np.empty(min(rese[0], cap), np.uint64), out.ptr)
        ms, (n_out, n_quotes, n_newlines, _) = quote()              # last: its output is the one verified
        tq.append(ms)
    ctx.timing(False)
    got = ctx.d2h(np.empty(n_out, np.uint64), out.ptr)
    ok = bool(n_out == len(exp) and np.array_equal(got, exp) and n_quotes == copies * int(np.count_nonzero(block == 34))
              and n_newlines == copies * int(np.count_nonzero(block == 10)))

    got16 = BlockedOffsets(ctx.d2h(np.empty(res16[0], np.uint16), low.ptr), ctx.d2h(np.empty(nt, np.uint64), tab.ptr),
                           0).to_u64()
    ok16 = bool(res16[:3] == (n_out, n_quotes, n_newlines) and np.array_equal(got16, exp))

    oke = bool(rese == (len(exp), n_quotes, n_newlines, n_quotes) and np.array_equal(gote, exp))
    oke2 = bool(rese2[0] == len(eexp) and rese2[3] == copies * etog and np.array_equal(gote2, eexp))

    def rate(ts, nbytes):
        return round(nbytes / (float(np.median(ts)) / 1e3) / GiB, 1)

    rq, rb, rr, rd = rate(tq, n), rate(tb, n), rate(tr, n16), rate(td, n)
    print(json.dumps({
        "bytes": n, "records": int(n_out), "newlines": int(n_newlines), "quotes": int(n_quotes), "reps": args.reps,
        "tile_bytes_grid": list(ctx.quote_geometry()),
        "record_index_ms": [round(float(np.median(tq)), 3), round(min(tq), 3), round(max(tq), 3)],
        "record_index_u16b_ms": [round(float(np.median(tb)), 3), round(min(tb), 3), round(max(tb), 3)],
        "stream_read_ms": [round(float(np.median(tr)), 3), round(min(tr), 3), round(max(tr), 3)],
        "newline_index_ms": [round(float(np.median(td)), 3), round(min(td), 3), round(max(td), 3)],
        "record_index_GiB_per_s": rq, "stream_read_GiB_per_s": rr, "newline_index_u64_GiB_per_s": rd,
        "ratio_to_stream_read": round(rq / rr, 3), "ratio_to_newline_index": round(rq / rd, 3),
        "record_index_u16b_GiB_per_s": rb, "u16b_ratio_to_stream_read": round(rb / rr, 3),
        "u16b_ms_over_u64_ms": round(float(np.median(tb)) / float(np.median(tq)), 3),
        "index_bytes": {"u64": 8 * int(n_out), "u16b": 2 * int(n_out) + 8 * nt},
        "escaped_absent_ms": [round(float(np.median(te)), 3), round(min(te), 3), round(max(te), 3)],
        "escaped_csv_escaped_ms": [round(float(np.median(te2)), 3), round(min(te2), 3), round(max(te2), 3)],
        "escaped_absent_ms_over_u64_ms": round(float(np.median(te)) / float(np.median(tq)), 3),
        "escaped_absent_ratio_to_stream_read": round(rate(te, n) / rr, 3),
        "escaped_csv_escaped_GiB_per_s": rate(te2, n),
        "escaped_csv_escaped_ratio_to_stream_read": round(rate(te2, n) / rr, 3),
        "newline_index_form": ctx.last_delim_form(), "verified": ok, "verified_u16b": ok16,
        "verified_escaped_absent": oke, "verified_escaped": oke2}), flush=True)
    return 0 if ok and ok16 and oke and oke2 else 1


if __name__ == "__main__":
    sys.exit(main())
