"""A numpy stand-in for the per-part device step of the faidx-compatible FASTA index: the counts of include/dpfai.h
in numpy (``np_pass1`` / ``np_pass2`` / ``np_names``), what ``fai_index_object`` uses of a ``ScanContext`` over numpy
memory (``FakeContext``), and the patches that put it in the device layer's place (``FakeDevices``)."""
import re
import threading

import numpy as np

from dataplug_amd.scan import objects as scan_objects

NONE = 0xFFFFFFFFFFFFFFFF


def header_pairs(data: bytes):
    """Header lines as (start, end): a '>' at the object's start or after a '\\n', up to and including its '\\n'."""
    pairs, p = [], 0
    while p < len(data):
        q = data.find(b"\n", p)
        q = len(data) if q < 0 else q + 1
        if data[p:p + 1] == b">":
            pairs.append((p, q))
        p = q
    return pairs


# ------------------------------------------------------------------------------------------------ counts in numpy
def np_pass1(data, base, lo, hi):
    nl, cr, first = [], [], []
    for a, b in zip(lo, hi):
        s = data[int(a) - base:int(b) - base]
        w = np.flatnonzero(s == 10)
        nl.append(len(w))
        cr.append(int(np.count_nonzero(s == 13)))
        first.append(int(a) + int(w[0]) if len(w) else NONE)
    return np.array(nl, np.uint64), np.array(cr, np.uint64), np.array(first, np.uint64)


def np_pass2(data, base, lo, hi, origin, width):
    off, last = [], []
    for a, b, o, w in zip(lo, hi, origin, width):
        p = int(a) + np.flatnonzero(data[int(a) - base:int(b) - base] == 10).astype(np.int64)
        bad = p[(p - int(o) + 1) % int(w) != 0] if int(w) else p
        off.append(len(bad))
        last.append(int(bad[-1]) if len(bad) else 0)
    return np.array(off, np.uint64), np.array(last, np.uint64)


def np_names(data, base, starts, ends):
    names = []
    for s, e in zip(starts, ends):
        raw = data[int(s) + 1 - base:int(e) - base].tobytes()
        names.append(re.split(rb"[ \t\r\n]", raw, maxsplit=1)[0])
    return np.array([len(n) for n in names], np.uint32), np.frombuffer(b"".join(names), np.uint8)


# ------------------------------------------------------------------------------------------------ the fake device layer
class FakeBuffer:
    def __init__(self, ptr):
        self.ptr = ptr


class FakeContext:
    """What fai_index_object uses of a ScanContext, over numpy memory."""
    BASE = 1 << 20

    def __init__(self, layer):
        self.layer = layer
        self.mem = np.zeros(0, np.uint8)

    def workspace(self, name, nbytes, placed=False):
        assert name == "input"
        if len(self.mem) < nbytes:
            self.mem = np.zeros(nbytes, np.uint8)
        return FakeBuffer(self.BASE)

    def _buf(self, d_buf, buf_len, buf_base, lo, hi):
        assert d_buf + buf_len <= self.BASE + len(self.mem)
        lo, hi = np.asarray(lo, np.uint64), np.asarray(hi, np.uint64)
        assert (lo <= hi).all() and (lo[1:] >= hi[:-1]).all(), "segments must ascend and be disjoint"
        assert len(lo) == 0 or (int(lo[0]) >= buf_base and int(hi[-1]) <= buf_base + buf_len), "clipped to the buffer"
        return self.mem[d_buf - self.BASE:d_buf - self.BASE + buf_len]

    def fai_counts(self, d_buf, buf_len, buf_base, lo, hi, origin, width=None):
        data = self._buf(d_buf, buf_len, buf_base, lo, hi)
        self.layer.note("pass2" if width is not None else "pass1", buf_base, buf_len, len(lo))
        if width is None:
            return np_pass1(data, buf_base, lo, hi)
        return np_pass2(data, buf_base, lo, hi, origin, width)

    def fai_names(self, d_buf, buf_len, buf_base, starts, ends):
        assert all(buf_base <= int(s) < int(e) <= buf_base + buf_len for s, e in zip(starts, ends))
        return np_names(self.mem[d_buf - self.BASE:d_buf - self.BASE + buf_len], buf_base, starts, ends)


class FakeDevices:
    def __init__(self, monkeypatch, devs):
        self.tls = threading.local()
        self.lock = threading.Lock()
        self.calls, self.fetches = [], []
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
