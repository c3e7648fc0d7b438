"""A numpy-backed stand-in for the per-part device step of the VCF position index: what ``pos_index_object`` uses of a
``ScanContext`` (``workspace``, ``vcf_lines``, ``vcf_positions``), over numpy memory, a launch's outputs computed by
the definition's byte loop (tests/_vcfpos_loop.py), and the patches that put it in the device layer's place."""
import threading

import numpy as np

import _vcfpos_loop as L
from dataplug_amd.scan import objects as scan_objects
from dataplug_amd.scan.device import VcfPositions


class FakeBuffer:
    def __init__(self, ptr):
        self.ptr = ptr


class FakeContext:
    """What pos_index_object uses of a ScanContext, over numpy memory; a launch's outputs come from the loop."""
    BASE = 1 << 20

    def __init__(self, layer):
        self.layer = layer
        self.mem = np.zeros(0, np.uint8)
        self.vp = None

    def workspace(self, name, nbytes, placed=False):
        assert name == "input"
        if len(self.mem) < nbytes:
            self.mem = np.zeros(nbytes, np.uint8)
        return FakeBuffer(self.BASE)

    def vcf_lines(self, d_buf, buf_len, buf_base, begin, end, size, first=False, cap=None):
        assert buf_base <= begin <= end <= buf_base + buf_len and d_buf + buf_len <= self.BASE + len(self.mem)
        buf = self.mem[d_buf - self.BASE:d_buf - self.BASE + buf_len].tobytes()
        if begin in self.layer.fail_at:                                  # the parts (by their first byte) that fail
            raise OSError("fake: the part's launch failed")
        starts = [begin] if first and begin < size else []
        starts += [p + 1 for p in range(begin, end) if buf[p - buf_base] == 10 and p + 1 < size]
        self.vp = (buf, buf_base, size, starts)
        self.layer.note("lines", begin, end, len(starts))
        return len(starts)

    def vcf_positions(self, ordinal0, every, run_cap=1024):
        buf, buf_base, size, starts = self.vp
        pos, clen, flags = L.loop_parse(buf, buf_base, size, starts)
        smp, runs, res = L.loop_reduce(pos, clen, flags, ordinal0, every)
        self.layer.note("reduce", starts[0] if starts else None, ordinal0, len(starts))
        none = lambda v: None if v == L.NONE else v
        at = lambda i: None if i is None else starts[i]
        i64 = lambda k: np.array([r[k] for r in runs], np.int64)
        names = [buf[starts[r[0]] - buf_base:starts[r[0]] - buf_base + r[2]] for r in runs]
        fm, fu = none(res["min_malformed"]), none(res["min_unsorted"])
        return VcfPositions(len(starts), np.array(smp, np.uint32), i64(0), i64(1), i64(3), i64(4), names,
                            np.array([starts[r[0]] for r in runs], np.uint64), res["n_malformed"], fm,
                            res["n_unsorted"], fu, res["first_pos"], res["last_pos"], at(0 if starts else None),
                            at(fm), at(fu))


class FakeDevices:
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
            ctxs[device] = FakeContext(self)
        return ctxs[device]

    def fetch_to_device(self, ctx, storage, bucket, key, lo, hi, d_ptr, **kw):
        raw = storage.get_object(Bucket=bucket, Key=key, Range=f"bytes={lo}-{hi - 1}")["Body"].read()
        assert len(raw) == hi - lo and d_ptr % 16 == lo % 16
        with self.lock:
            self.fetches.append((lo, hi))
        ctx.mem[d_ptr - ctx.BASE:d_ptr - ctx.BASE + hi - lo] = np.frombuffer(raw, np.uint8)


HALO = 1024                                              # pos_index_object's smallest: a line's prefix (VPOS_PREFIX_MAX)


def model_part(data: bytes):
    """The ``make_part`` of ``parts_by_cuts`` over the model: a fresh context that holds the part's buffer only."""
    layer = type("Layer", (), {"note": lambda *a: None, "fail_at": ()})()

    def make_part(k, lo, hi, top):
        ctx = FakeContext(layer)
        ctx.mem = np.frombuffer(data[lo:top], np.uint8)
        return ctx, ctx.BASE
    return make_part


def parts_by_cuts(data: bytes, bo: int, cuts, every, make_part=None, run_cap: int = 1024):
    """The merge's input for parts cut at ``cuts`` (a part owns the lines that start behind a '\\n' of its bytes).
    Part k = [lo, hi) sees the buffer [lo, top), top = min(size, hi + 1024) as in ``pos_index_object``.
    ``make_part(k, lo, hi, top)`` gives ``(ctx, d_buf)``, the context that runs the part and the device address of
    object byte ``lo`` in it: the model's by default, or a real ``ScanContext`` with the bytes uploaded."""
    size = len(data)
    edges = [bo] + sorted(cuts) + [size]
    parts, before = [], 0
    make_part = make_part or model_part(data)
    for k, (lo, hi) in enumerate(zip(edges[:-1], edges[1:])):
        top = min(size, hi + HALO)
        ctx, d_buf = make_part(k, lo, hi, top)
        n = ctx.vcf_lines(d_buf, top - lo, lo, lo, hi, size, first=k == 0)
        parts.append(ctx.vcf_positions(before, every, run_cap=run_cap))
        before += n
    return parts
