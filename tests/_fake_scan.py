"""A numpy-backed fake of the device layer under scan.objects.record_index_object, shared by the CPU tests of the
record index: ``workspace`` and ``records`` of a ScanContext over numpy memory, the plain scans from the definition
(tests/_quote_model.py), the escaped ones from the byte loop (tests/_escape_loop.py), honouring carry, esc_carry, scope
and cap (a too small cap costs a second launch, as on the GPU)."""
import threading
from collections import namedtuple

import numpy as np

from _escape_loop import blocked, loop_quote_bytes, loop_record_ends
from _quote_model import record_ends
from dataplug_amd.scan import objects as scan_objects
from dataplug_amd.scan.device import Records

# one launch as the fake saw it; ``relaunch``: the second launch after a capacity error, ``cap`` the count
Launch = namedtuple("Launch", "form escape begin end carry esc_carry scope cap relaunch")


class FakeBuffer:
    def __init__(self, ptr):
        self.ptr = ptr


class FakeContext:
    """What record_index_object uses of a ScanContext, over numpy memory."""
    BASE = 1 << 20                                       # device address of the context's memory, 16-byte aligned

    def __init__(self, layer):
        self.layer = layer
        self.mem = np.zeros(0, np.uint8)

    def workspace(self, name, nbytes, placed=False):
        assert name == "input"
        if len(self.mem) < nbytes:
            self.mem = np.zeros(nbytes, np.uint8)
        return FakeBuffer(self.BASE)

    def _bytes(self, d_buf, buf_len, buf_base, begin, end):
        assert buf_base <= begin <= end <= buf_base + buf_len and d_buf + buf_len <= self.BASE + len(self.mem)
        a = d_buf - self.BASE + (begin - buf_base)
        return self.mem[a:a + end - begin]

    def records(self, d_buf, buf_len, buf_base, begin, end, *, quote=34, carry=0, escape=None, esc_carry=0,
                scope="all", form="u64", cap=None):
        assert form in ("count", "u64", "u16b")
        if form == "u16b":                               # the alignment rule of the blocked entry points
            assert (d_buf + (begin - buf_base)) % 16 == begin % 16, "device address not congruent to begin mod 16"
        launch = Launch(form, escape, begin, end, carry, esc_carry, scope, 0, False)
        if form == "count":
            self.layer.note(launch)
            if self.layer.fail_counts_at == begin:
                raise RuntimeError("fake: record_counts failed")
        d = self._bytes(d_buf, buf_len, buf_base, begin, end)
        if escape is None:
            ends, nq, nn = record_ends(d, begin, quote, carry)
            tog = nq
        else:
            ends, tog, _, _ = loop_record_ends(d, begin, end, quote, escape, carry, esc_carry, scope, base=begin)
            nq, nn = loop_quote_bytes(d, quote=quote), int(np.count_nonzero(d == 10))
        if form == "count":
            return Records(None, None, nq, nn, tog, len(ends))
        if cap is None:
            cap = (end - begin) // 16 + 1024
        self.layer.note(launch._replace(cap=cap))
        if len(ends) > cap:                              # DPCapacityError, then the launch sized by the count
            self.layer.note(launch._replace(cap=len(ends), relaunch=True))
        low, table = blocked(ends, begin, end) if form == "u16b" else (ends, None)
        return Records(low, table, nq, nn, tog, len(ends))


class FakeDevices:
    """scan.objects' device layer replaced: get_context (one context per thread and device, like the real one),
    fetch_to_device (the object's bytes into the context's numpy memory) and devices.  ``calls`` collects what
    ``note`` makes of every ``Launch`` (None: not recorded); ``fail_counts_at``: the count launch of the part that
    begins there raises."""

    def __init__(self, monkeypatch, devs, note=lambda launch: launch):
        self.tls = threading.local()
        self.lock = threading.Lock()
        self.calls = []
        self.fail_counts_at = None
        self._note = note
        monkeypatch.setattr(scan_objects, "get_context", self.get_context)
        monkeypatch.setattr(scan_objects, "fetch_to_device", self.fetch_to_device)
        monkeypatch.setattr(scan_objects, "devices", lambda max_devices=None, co=None: list(devs))

    def note(self, launch):
        call = self._note(launch)
        if call is not None:
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
        a = d_ptr - ctx.BASE
        ctx.mem[a:a + hi - lo] = np.frombuffer(raw, np.uint8)
