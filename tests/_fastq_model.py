"""A numpy stand-in for the per-part device step of the FASTQ read index: what ``reads_index_object`` uses of a
``ScanContext`` (``workspace``, ``fastq_lines``, ``fastq_reads``), over numpy memory, and the patches that put it in
the device layer's place.  The launches' outputs are computed with vectorised numpy from the part's own bytes, as
include/dpfq.h defines them; the CPU tests compare what comes out of the merge with the byte loop."""
import threading

import numpy as np

from dataplug_amd.scan import fastq
from dataplug_amd.scan import objects as scan_objects
from dataplug_amd.scan.device import FastqPart


class ModelBuffer:
    def __init__(self, ptr):
        self.ptr = ptr


class ModelContext:
    BASE = 1 << 20

    def __init__(self, layer=None):
        self.layer = layer
        self.mem = np.zeros(0, np.uint8)
        self.fq = None

    def workspace(self, name, nbytes, placed=False):
        assert name == "input"
        if len(self.mem) < nbytes:
            self.mem = np.zeros(nbytes, np.uint8)
        return ModelBuffer(self.BASE)

    def fastq_lines(self, d_buf, buf_len, buf_base, begin, end, size, first=False, cap=None):
        assert buf_base <= begin <= end <= buf_base + buf_len and d_buf + buf_len <= self.BASE + len(self.mem)
        buf = self.mem[d_buf - self.BASE:d_buf - self.BASE + buf_len]
        if self.layer is not None and begin in self.layer.fail_at:
            raise OSError("model: the part's launch failed")
        starts = np.flatnonzero(buf[begin - buf_base:end - buf_base] == 10).astype(np.int64) + begin + 1
        closed = bool(len(starts)) and end >= size and int(starts[-1]) >= size
        if closed:
            starts = starts[:-1]
        if first and begin < size:
            starts = np.concatenate([[begin], starts])
        self.fq = (buf, buf_base, size, starts, end >= size, closed)
        if self.layer is not None:
            self.layer.note("lines", begin, end, len(starts))
        return len(starts)

    def fastq_reads(self, skip, read0, every):
        buf, base, size, starts, last, closed = self.fq
        n = len(starts)
        nr, lines = fastq.part_plan(n, skip, last)
        if self.layer is not None:
            self.layer.note("reads", int(starts[0]) if n else None, skip, read0, nr)
        es = starts[lines].astype(np.uint64)
        if nr == 0:
            return FastqPart(n, skip, read0, 0, np.zeros((0, 2), np.uint64), 0, 0, None, 0, None, None, 0, lines, es,
                             closed)
        t0 = skip + 4 * nr
        nxt = int(starts[t0]) if t0 < n else (size if closed else size + 1)      # the start behind the last read
        s = np.concatenate([starts[skip:t0], [nxt]])
        top = min(base + len(buf), size)
        at = lambda q, ok: np.where(ok & (q >= base) & (q < top), buf[np.clip(q - base, 0, len(buf) - 1)], 0)
        raw = s[1:] - 1 - s[:-1]
        r0, r1, r2, r3 = (raw[j::4] for j in range(4))
        b0, b2 = at(s[0:-1:4], r0 >= 1), at(s[2::4], r2 >= 1)
        c1 = r1 - (at(s[2::4] - 2, r1 >= 1) == 13)
        c3 = r3 - (at(s[4::4] - 2, r3 >= 1) == 13)
        flags = np.where(b0 != 64, 1, np.where(b2 != 43, 2, np.where((c1 != c3) | (c1 >= 1 << 32), 3, 0)))
        lens = (c1 & 0xFFFFFFFF).astype(np.uint64)
        cum = np.concatenate([[0], np.cumsum(lens, dtype=np.uint64)]).astype(np.uint64)
        pick = np.flatnonzero((read0 + np.arange(nr)) % every == 0)
        smp = np.stack([s[0:-1:4][pick].astype(np.uint64), cum[pick]], axis=1)
        bad = np.flatnonzero(flags)
        fm = int(bad[0]) if len(bad) else None
        return FastqPart(n, skip, read0, nr, smp, int(cum[-1]), len(bad), fm, int(flags[fm]) if len(bad) else 0,
                         int(s[4 * fm]) if len(bad) else None, int(lens.min()), int(lens.max()), lines, es, closed)


class ModelDevices:
    """Puts ``ModelContext`` in the place of the device layer under ``scan.objects`` (one context per thread and
    device, as ``get_context`` gives) and records the launches and the fetched ranges."""

    def __init__(self, monkeypatch, devs, fail_at=()):
        self.tls = threading.local()
        self.lock = threading.Lock()
        self.calls, self.fetches, self.fail_at = [], [], set(fail_at)
        monkeypatch.setattr(scan_objects, "get_context", self.get_context)
        monkeypatch.setattr(scan_objects, "fetch_to_device", self.fetch_to_device)
        monkeypatch.setattr(scan_objects, "devices", lambda max_devices=None, co=None: list(devs))

    def note(self, *call):
        with self.lock:
            self.calls.append(call)

    def get_context(self, device=0, slot=0):
        ctxs = self.tls.__dict__.setdefault("ctxs", {})
        if device not in ctxs:
            ctxs[device] = ModelContext(self)
        return ctxs[device]

    def fetch_to_device(self, ctx, storage, bucket, key, lo, hi, d_ptr, **kw):
        raw = storage.get_object(Bucket=bucket, Key=key, Range=f"bytes={lo}-{hi - 1}")["Body"].read()
        assert len(raw) == hi - lo and d_ptr % 16 == lo % 16
        with self.lock:
            self.fetches.append((lo, hi))
        ctx.mem[d_ptr - ctx.BASE:d_ptr - ctx.BASE + hi - lo] = np.frombuffer(raw, np.uint8)


def model_part(data: bytes):
    """The ``make_part`` of ``parts_by_cuts`` over the model: a fresh context that holds the part's buffer only."""
    def make_part(k, lo, hi, top):
        ctx = ModelContext()
        ctx.mem = np.frombuffer(data[lo:top], np.uint8)
        return ctx, ctx.BASE
    return make_part


def parts_by_cuts(data: bytes, cuts, every: int, make_part=None):
    """The merge's input for parts cut at ``cuts``: each part sees its own bytes only (no halo: top = hi).
    ``make_part(k, lo, hi, top)`` gives ``(ctx, d_buf)``, the context that runs the part and the device address of
    object byte ``lo`` in it: the model's by default, or a real ``ScanContext`` with the bytes uploaded."""
    size = len(data)
    edges = [0] + sorted(cuts) + [size]
    parts, before = [], 0
    make_part = make_part or model_part(data)
    for k, (lo, hi) in enumerate(zip(edges[:-1], edges[1:])):
        ctx, d_buf = make_part(k, lo, hi, hi)
        n = ctx.fastq_lines(d_buf, hi - lo, lo, lo, hi, size, first=k == 0)
        parts.append(ctx.fastq_reads((-before) % 4, -(-before // 4), every))
        before += n
    return parts
