"""Device-side scan contexts: one ``dp_ctx`` (device + HIP stream + workspace) per host thread per GPU.

This is the only Python module that talks to libdpscan.so.  Buffers handed to the kernels are device
pointers (ints): either the context's own grow-only staging buffers (``*_host`` helpers upload Python
bytes / numpy arrays), or caller-owned device memory (e.g. a torch tensor's ``data_ptr()``).
"""
from __future__ import annotations

import ctypes
import importlib
import threading
from collections import namedtuple
from typing import Iterable, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from ._lib import DPCapacityError, check

_U64P = ctypes.POINTER(ctypes.c_uint64)
_I64P = ctypes.POINTER(ctypes.c_int64)


def _host_ptr(data) -> Tuple[int, int, object]:
    """(address, nbytes, keepalive) of a bytes-like / numpy object without copying."""
    if isinstance(data, np.ndarray):
        a = np.ascontiguousarray(data).view(np.uint8).reshape(-1)
    else:
        a = np.frombuffer(memoryview(data).cast("B"), dtype=np.uint8)
    return a.ctypes.data, a.nbytes, a


def _check_capacity(rc: int, needed: int) -> None:
    """``check`` for a libdpscan status that may be DP_ERR_CAPACITY: that one raised with the entries ``needed``."""
    if rc == _lib.DP_ERR_CAPACITY:
        e = DPCapacityError(rc, f"output capacity below {needed} entries")
        e.needed = needed
        raise e
    check(rc)


def _retry_capacity(cap: int, launch):
    """The result of ``launch(cap)``: launched again, with the capacity the DPCapacityError says is ``needed``, until
    the output fits (the synchronous forms of every index share this loop)."""
    while True:
        try:
            return launch(cap)
        except DPCapacityError as e:
            cap = e.needed


# the record index (libdpquote.so): what a launch counts, and what the synchronous ``ScanContext.records`` returns
RecordCounts = namedtuple("RecordCounts", "n n_quotes n_newlines toggles")
Records = namedtuple("Records", "ends table n_quotes n_newlines toggles n")
# what ``ScanContext.vcf_positions`` reads back of one part (libdpvpos.so).  Per run, in line order, with line indices
# local to the launch: ``run_line`` / ``run_pos`` (the run's first line and its POS), ``run_last_line`` / ``run_last``
# (its last line and that POS), ``names`` and ``run_offset`` (the byte offset of the run's first line).
# ``first_malformed`` / ``first_unsorted``: the lowest such local index, or None; ``malformed_offset`` /
# ``unsorted_offset`` those lines' byte offsets and ``first_offset`` that of the launch's line 0.
VcfPositions = namedtuple("VcfPositions", "n samples run_line run_pos run_last_line run_last names run_offset "
                                          "n_malformed first_malformed n_unsorted first_unsorted first_pos last_pos "
                                          "first_offset malformed_offset unsorted_offset")
# what ``ScanContext.vcf_spans`` reads back of one part (libdpvspan.so): ``blockmax`` the part's slots (its first and
# last may be partial K-blocks), the result words, and the byte offsets of the flagged lines: ``first_missing`` /
# ``first_truncated`` are the lowest such local index or None, ``missing_offset`` / ``truncated_offset`` their lines'.
VcfSpans = namedtuple("VcfSpans", "n blockmax n_missing first_missing n_truncated first_truncated n_from_end max_span "
                                  "missing_offset truncated_offset")
# what ``ScanContext.fastq_reads`` reads back of one part (libdpfq.so).  The part's owned lines are numbered from 0;
# ``skip`` of them in front belong to a read begun earlier, the device handled the ``n_reads`` reads behind those
# (global index ``read0`` on) and ``samples`` holds their (offset, bases before it within the launch) pairs.
# ``edge_lines`` / ``edge_starts``: the local numbers and byte offsets of the lines the device did not handle, and of
# the first one it did (the terminator of the edge line before it).  ``first_malformed``: the lowest malformed local
# read or None, with its ``malformed_kind`` (include/dpfq.h) and ``malformed_offset``.  ``closed``: the part reaches
# the object's end and the object's last byte is a '\n'.
FastqPart = namedtuple("FastqPart", "n_lines skip read0 n_reads samples bases n_malformed first_malformed "
                                    "malformed_kind malformed_offset min_len max_len edge_lines edge_starts closed")
# the libraries that keep a context of their own on a ScanContext's stream, by binding module: the attribute that holds
# the handle and the prefix of the symbols that create and destroy it (``ScanContext._sub_ctx`` / ``close``)
_SUB_CTXS = {"_quote": ("_dq", "dq"), "_fai": ("_dfai", "dfai"), "_vpos": ("_dvp", "dvp"), "_fq": ("_dfq", "dfq"),
             "_vspan": ("_dvs", "dvs")}
_RECORD_FORMS = {"count": None, "u32": np.uint32, "u64": np.uint64, "u16b": np.uint16}


def _record_form(form: str, escape: Optional[int], scope: str):
    """(output dtype, escape flags) of a record launch; ValueError for an unknown form or, with an escape, scope."""
    from ._quote import escape_flags
    if form not in _RECORD_FORMS:
        raise ValueError(f"record form must be one of {tuple(_RECORD_FORMS)}, not {form!r}")
    return _RECORD_FORMS[form], 0 if escape is None else escape_flags(scope)


class DeviceBuffer:
    """Device memory owned through the C ABI (freed with the context)."""

    def __init__(self, ctx: "ScanContext", nbytes: int):
        self.ctx = ctx
        self.nbytes = int(nbytes)
        p = ctypes.c_void_p()
        check(_lib.load().dp_malloc(ctx.handle, max(16, self.nbytes), ctypes.byref(p)))
        self.ptr = int(p.value)

    def free(self):
        if self.ptr and self.ctx.handle:
            check(_lib.load().dp_free(self.ctx.handle, ctypes.c_void_p(self.ptr)))
        self.ptr = 0


class PinnedBuffer:
    """Page-locked host memory (dp_host_alloc) with a uint8 numpy view; H2D from it is a true async DMA."""

    def __init__(self, nbytes: int):
        self.nbytes = int(nbytes)
        p = ctypes.c_void_p()
        check(_lib.load().dp_host_alloc(max(16, self.nbytes), ctypes.byref(p)))
        self.ptr = int(p.value)
        self.array = np.ctypeslib.as_array((ctypes.c_uint8 * max(16, self.nbytes)).from_address(self.ptr))

    def view(self, n: Optional[int] = None) -> memoryview:
        return memoryview(self.array)[: self.nbytes if n is None else n]

    def free(self):
        if self.ptr:
            self.array = None
            check(_lib.load().dp_host_free(ctypes.c_void_p(self.ptr)))
        self.ptr = 0


# Placement-aware input buffers (round 6, profiles/r06/placement/): about half of the large device buffers a process
# allocates sit in a "slow mode" where a kernel reading the buffer while writing a few % of its size elsewhere runs
# 10-16 % slower than on the other half (reads alone are not affected; the input buffer alone decides, whatever the
# output buffer).  An input buffer of at least PLACEMENT_MIN bytes is therefore probed when it is allocated: the
# calibration kernels read it alone and read it while writing 1/32 of it; a time ratio above PLACEMENT_SLOW marks the
# slow mode, and another buffer is allocated (the slow one held meanwhile, so it is not handed back) -- at most
# PLACEMENT_TRIES, the best kept (or the best of those that fit in HBM).  Eight 4 GiB buffers of one process
# (tools/placement_probe.py, profiles/r06/placement/probe8.log): ratios 1.088-1.106 where line_kernel's u8s scan of a
# 4 GiB CSV takes 688-700 us, 1.167-1.193 where it takes 787-792 us (8 GiB: 1.080-1.094 / 1,352-1,356 us against
# 1.184-1.199 / 1,567-1,569 us, probe8g.log).  Larger buffers are mixtures (four 32 GiB
# ones: ratios 1.055-1.108 against scans of 6,006-6,302 us, no separation; profiles/r06/placement/probe32.log), so
# buffers above PLACEMENT_MAX are allocated once, unprobed.
PLACEMENT_MIN = 256 << 20
PLACEMENT_MAX = 8 << 30
PLACEMENT_TRIES = 5
PLACEMENT_SLOW = 1.125
_PROBE_WPR = 1.0 / 32


class ScanContext:
    """A ``dp_ctx``: device, stream and scan workspace.  Not shared between threads."""

    def __init__(self, device: int = 0):
        self.lib = _lib.load()
        h = ctypes.c_void_p()
        check(self.lib.dp_ctx_create(int(device), ctypes.byref(h)))
        self.handle = h
        self.device = int(device)
        self._bufs = {}
        self._pinned = {}
        self._get_pool = None
        self._timing_on = False
        self.placements = []                          # per placed buffer: the probe ratios of its candidates
        self._dq = None                               # libdpquote's dq_ctx on this context's stream (records)
        self._dfai = None                             # libdpfai's dfai_ctx on this context's stream (fai_counts)
        self._dvp = None                              # libdpvpos's dvp_ctx on this context's stream (vcf_positions)
        self._vp = None                               # the resident lines of the last vcf_lines
        self._dfq = None                              # libdpfq's dfq_ctx on this context's stream (fastq_reads)
        self._dvs = None                              # libdpvspan's dvs_ctx on this context's stream (vcf_spans)
        self._fq = None                               # the resident lines of the last fastq_lines

    # ---------------------------------------------------------------- memory
    def workspace(self, name: str, nbytes: int, placed: bool = False) -> DeviceBuffer:
        """Grow-only named device buffer; ``placed``: an input buffer, probed for the slow placement mode when it is
        allocated (``PLACEMENT_MIN`` .. ``PLACEMENT_MAX`` bytes)."""
        b = self._bufs.get(name)
        if b is None or b.nbytes < nbytes:
            if b is not None:
                b.free()
                del self._bufs[name]
            size = max(int(nbytes), 1 << 16)
            b = (self._placed_buffer(size) if placed and PLACEMENT_MIN <= size <= PLACEMENT_MAX
                 else DeviceBuffer(self, size))
            self._bufs[name] = b
        return b

    def placement_ratio(self, buf: DeviceBuffer, nbytes: Optional[int] = None) -> float:
        """Time of the read-while-writing calibration kernel over ``buf`` / time of the read-only one (each the
        mean of two launches): ~1.0-1.03 on a fast buffer, ~1.08-1.16 in the slow mode."""
        n = (buf.nbytes if nbytes is None else nbytes) // 16 * 16
        out = DeviceBuffer(self, int(n * _PROBE_WPR) + (1 << 16))
        was_on = self._timing_on
        try:
            self.stream_read(buf.ptr, n)
            self.sync()
            t = []
            for rw in (False, True):
                self.timing(True)
                self.timing_read()
                for _ in range(2):
                    if rw:
                        self.stream_rw(buf.ptr, n, out.ptr, _PROBE_WPR)
                    else:
                        self.stream_read(buf.ptr, n)
                ms, k = self.timing_read()
                t.append(ms / max(1, k))
            return t[1] / t[0]
        finally:
            self.timing(was_on)
            out.free()

    def _placed_buffer(self, size: int) -> DeviceBuffer:
        cands = []
        try:
            for _ in range(PLACEMENT_TRIES):
                try:
                    c = DeviceBuffer(self, size)
                except _lib.DPScanError:
                    if cands:                         # no room for another candidate: the best so far
                        break
                    raise
                cands.append((self.placement_ratio(c), c))
                if cands[-1][0] <= PLACEMENT_SLOW:
                    break
        except BaseException:
            for _, c in cands:
                c.free()
            raise
        best = min(cands, key=lambda rc: rc[0])
        for rc in cands:
            if rc is not best:
                rc[1].free()
        self.placements.append([round(r, 4) for r, _ in cands])
        return best[1]

    def pinned(self, name: str, nbytes: int) -> PinnedBuffer:
        """Grow-only named pinned host buffer."""
        b = self._pinned.get(name)
        if b is None or b.nbytes < nbytes:
            if b is not None:
                b.free()
            b = PinnedBuffer(max(int(nbytes), 1 << 16))
            self._pinned[name] = b
        return b

    def get_pool(self, threads: int):
        """The context's persistent pool of ranged-GET threads (``fetch_to_device``): created once per context,
        i.e. once per (host thread, device) — a persistent per-GPU worker reuses it for every object."""
        import concurrent.futures as cf
        if self._get_pool is None or self._get_pool._max_workers < threads:
            if self._get_pool is not None:
                self._get_pool.shutdown(wait=True)
            self._get_pool = cf.ThreadPoolExecutor(threads, thread_name_prefix=f"dpscan-get{self.device}")
        return self._get_pool

    def h2d_async(self, dst: int, src_ptr: int, nbytes: int) -> None:
        """Async copy from pinned host memory on the context stream (caller keeps the source alive)."""
        check(self.lib.dp_h2d(self.handle, ctypes.c_void_p(dst), ctypes.c_void_p(src_ptr), int(nbytes)))

    def h2d(self, dst: int, data, nbytes: Optional[int] = None) -> None:
        ptr, n, keep = _host_ptr(data)
        n = n if nbytes is None else nbytes
        check(self.lib.dp_h2d(self.handle, ctypes.c_void_p(dst), ctypes.c_void_p(ptr), n))
        check(self.lib.dp_sync(self.handle))   # pageable source: keep it alive until the copy is done
        del keep

    def d2h_async(self, dst_ptr: int, src: int, nbytes: int) -> None:
        """Async copy to pinned host memory on the context stream (ordered after the work enqueued before it)."""
        if nbytes:
            check(self.lib.dp_d2h(self.handle, ctypes.c_void_p(dst_ptr), ctypes.c_void_p(src), int(nbytes)))

    def d2h(self, out: np.ndarray, src: int) -> np.ndarray:
        if out.nbytes:
            check(self.lib.dp_d2h(self.handle, ctypes.c_void_p(out.ctypes.data), ctypes.c_void_p(src), out.nbytes))
            check(self.lib.dp_sync(self.handle))
        return out

    def upload(self, data, name: str = "input") -> Tuple[int, int]:
        """Copy host bytes into the named staging buffer; returns (device pointer, nbytes)."""
        _, n, _ = _host_ptr(data)
        buf = self.workspace(name, n + 16)
        self.h2d(buf.ptr, data)
        return buf.ptr, n

    def sync(self) -> None:
        check(self.lib.dp_sync(self.handle))

    @property
    def stream(self) -> int:
        s = ctypes.c_void_p()
        check(self.lib.dp_ctx_get_stream(self.handle, ctypes.byref(s)))
        return int(s.value or 0)

    def set_stream(self, stream: Optional[int]) -> None:
        check(self.lib.dp_ctx_set_stream(self.handle, ctypes.c_void_p(stream or 0)))

    def wait_for(self, other: "ScanContext") -> None:
        """This context's stream waits (on the device) for everything enqueued on ``other``'s so far."""
        check(self.lib.dp_ctx_wait(self.handle, other.handle))

    # ---------------------------------------------------------------- FASTA
    def fasta_index(self, d_buf: int, buf_len: int, buf_base: int, obj_size: int,
                    chunks: Sequence[Tuple[int, int]], u64: bool = False, cap: Optional[int] = None):
        """FASTA (start, end) pairs of a chunk plan over device bytes (dp_fasta_index).

        Returns (pairs (n, 2) uint32|uint64, pending (nchunks,) int64, chunk_end (nchunks,) uint64).
        """
        ch = np.ascontiguousarray(np.asarray(chunks, dtype=np.uint64).reshape(-1))
        nch = len(ch) // 2
        dtype = np.uint64 if u64 else np.uint32
        if cap is None:
            cap = buf_len // 512 + 1024
        pending = np.full(nch, -1, np.int64)
        cend = np.zeros(nch, np.uint64)
        n = ctypes.c_uint64(0)

        def launch(cap):
            out = self.workspace("out", 2 * cap * np.dtype(dtype).itemsize + 16)
            rc = self.lib.dp_fasta_index(self.handle, ctypes.c_void_p(d_buf), buf_len, buf_base, obj_size,
                                         ch.ctypes.data_as(_U64P), nch, ctypes.c_void_p(out.ptr), int(u64), cap,
                                         ctypes.byref(n), pending.ctypes.data_as(_I64P), cend.ctypes.data_as(_U64P))
            _check_capacity(rc, int(n.value))
            return self.d2h(np.empty((int(n.value), 2), dtype), out.ptr)
        return _retry_capacity(cap, launch), pending, cend

    def fasta_index_async(self, d_buf, buf_len, buf_base, obj_size, chunks_u64: np.ndarray, d_out: int,
                          u64: bool, cap: int) -> None:
        check(self.lib.dp_fasta_index_async(self.handle, ctypes.c_void_p(d_buf), buf_len, buf_base, obj_size,
                                            chunks_u64.ctypes.data_as(_U64P), len(chunks_u64) // 2,
                                            ctypes.c_void_p(d_out), int(u64), cap))

    def fasta_result(self, nchunks: int):
        n = ctypes.c_uint64(0)
        pending = np.full(nchunks, -1, np.int64)
        cend = np.zeros(nchunks, np.uint64)
        check(self.lib.dp_fasta_result(self.handle, ctypes.byref(n), pending.ctypes.data_as(_I64P),
                                       cend.ctypes.data_as(_U64P)))
        return int(n.value), pending, cend

    # ---------------------------------------------------------------- delimiters
    def delim_index(self, d_buf: int, buf_len: int, buf_base: int, begin: int, end: int, delim: int = 10,
                    every_k: int = 1, emit_add: int = 0, u64: bool = True, cap: Optional[int] = None):
        """Sorted offsets of every ``every_k``-th ``delim`` in object bytes [begin, end) (dp_delim_index).

        Returns (offsets uint64|uint32, number of delimiters seen)."""
        dtype = np.uint64 if u64 else np.uint32
        if cap is None:
            cap = (end - begin) // (16 * every_k) + 1024
        n = ctypes.c_uint64(0)
        nd = ctypes.c_uint64(0)

        def launch(cap):
            out = self.workspace("out", cap * np.dtype(dtype).itemsize + 16)
            rc = self.lib.dp_delim_index(self.handle, ctypes.c_void_p(d_buf), buf_len, buf_base, begin, end,
                                         int(delim), int(every_k), int(emit_add), ctypes.c_void_p(out.ptr),
                                         int(u64), cap, ctypes.byref(n), ctypes.byref(nd))
            _check_capacity(rc, int(n.value))
            return self.d2h(np.empty(int(n.value), dtype), out.ptr), int(nd.value)
        return _retry_capacity(cap, launch)

    def delim_index_async(self, d_buf, buf_len, buf_base, begin, end, delim, every_k, emit_add, d_out, u64, cap):
        check(self.lib.dp_delim_index_async(self.handle, ctypes.c_void_p(d_buf), buf_len, buf_base, begin, end,
                                            int(delim), int(every_k), int(emit_add), ctypes.c_void_p(d_out),
                                            int(u64), cap))

    def delim_result(self):
        n = ctypes.c_uint64(0)
        nd = ctypes.c_uint64(0)
        check(self.lib.dp_delim_result(self.handle, ctypes.byref(n), ctypes.byref(nd)))
        return int(n.value), int(nd.value)

    def delim_ranges_async(self, d_buf: int, buf_len: int, buf_base: int, ranges: np.ndarray, delim: int,
                           every_k: int, emit_add: int, carry: int, d_out: int, out_mode: int, cap: int) -> None:
        """dp_delim_ranges_async; ``ranges`` a contiguous uint64 array [lo0, hi0, lo1, hi1, ...] kept alive by
        the caller until the result is collected."""
        check(self.lib.dp_delim_ranges_async(self.handle, ctypes.c_void_p(d_buf), buf_len, buf_base,
                                             ranges.ctypes.data_as(_U64P), len(ranges) // 2, int(delim),
                                             int(every_k), int(emit_add), int(carry), ctypes.c_void_p(d_out),
                                             int(out_mode), int(cap)))

    def delim_ranges_result(self, nranges: int):
        """(entries, delimiters seen, per-range cumulative delimiter counts)."""
        n = ctypes.c_uint64(0)
        nd = ctypes.c_uint64(0)
        ends = np.zeros(nranges, np.uint64)
        rc = self.lib.dp_delim_ranges_result(self.handle, ctypes.byref(n), ctypes.byref(nd), ends.ctypes.data_as(_U64P))
        _check_capacity(rc, int(n.value))
        return int(n.value), int(nd.value), ends

    @staticmethod
    def block_table_size(ranges: np.ndarray) -> Tuple[int, int]:
        """(j0, entries) of the 64 KiB block table out_mode 3 writes for these ranges."""
        first, last = int(ranges[0]), int(ranges[-1])
        j0 = first >> 16
        return j0, (((last - 1) >> 16) - j0 + 1) if last > first else 1

    @staticmethod
    def sub_table_size(ranges: np.ndarray) -> Tuple[int, int]:
        """(s0, entries) of the 256-byte table out_mode 4 writes for these ranges."""
        first, last = int(ranges[0]), int(ranges[-1])
        s0 = first >> 8
        return s0, (((last - 1) >> 8) - s0 + 1) if last > first else 1

    @staticmethod
    def _tab_off(cap: int, out_mode: int) -> int:
        return ((2 if out_mode == 3 else 1) * cap + 15) & ~15

    @staticmethod
    def _sub_off(cap: int, ranges: np.ndarray) -> int:
        return (ScanContext._tab_off(cap, 4) + 8 * ScanContext.block_table_size(ranges)[1] + 15) & ~15

    @staticmethod
    def out_bytes(cap: int, out_mode: int, ranges: np.ndarray) -> int:
        """Bytes of a dp_delim_ranges output buffer for ``cap`` entries (out_mode 3: + the block table; 4: + the
        block table and the 256-byte table)."""
        if out_mode == 3:
            return ScanContext._tab_off(cap, 3) + 8 * ScanContext.block_table_size(ranges)[1] + 16
        if out_mode == 4:
            return ScanContext._sub_off(cap, ranges) + 2 * ScanContext.sub_table_size(ranges)[1] + 16
        return cap * (8 if out_mode == 1 else 4) + 16

    def block_table(self, d_out: int, cap: int, ranges: np.ndarray, out_mode: int = 3) -> np.ndarray:
        """The 64 KiB block table of an out_mode 3 / 4 result: entries before (j0 + j) * 64 KiB (this launch)."""
        j0, nt = self.block_table_size(ranges)
        tab = self.d2h(np.empty(nt, np.uint64), d_out + self._tab_off(cap, out_mode))
        if int(ranges[0]) & 0xFFFF:
            tab[0] = 0                                   # the boundary below the first byte: not a range start
        return tab

    def sub_table(self, d_out: int, cap: int, ranges: np.ndarray) -> np.ndarray:
        """The 256-byte table of an out_mode 4 result: low 16 bits of the entries before (s0 + s) * 256."""
        s0, ns = self.sub_table_size(ranges)
        sub = self.d2h(np.empty(ns, np.uint16), d_out + self._sub_off(cap, ranges))
        if int(ranges[0]) & 0xFF:
            sub[0] = 0                                   # the boundary below the first byte
        return sub

    def delim_ranges(self, d_buf: int, buf_len: int, buf_base: int, ranges, delim: int = 10, every_k: int = 1,
                     emit_add: int = 0, carry: int = 0, out_mode: int = 1, cap: Optional[int] = None):
        """Synchronous dp_delim_ranges: (offsets, delimiters seen, per-range cumulative counts); out_mode 1
        uint64, 0 uint32, 2 uint32 low words, 3 uint16 low words (+ ``block_table``, returned as a 4th item), 4 uint8
        low bytes (+ ``block_table`` and ``sub_table``, a 4th and 5th item)."""
        rg = np.ascontiguousarray(np.asarray(ranges, dtype=np.uint64).reshape(-1))
        span = int(sum(int(rg[2 * i + 1]) - int(rg[2 * i]) for i in range(len(rg) // 2)))
        dtype = {0: np.uint32, 1: np.uint64, 2: np.uint32, 3: np.uint16, 4: np.uint8}[out_mode]
        if cap is None:
            cap = span // (16 * every_k) + 1024

        def launch(cap):
            out = self.workspace("out", self.out_bytes(cap, out_mode, rg))
            self.delim_ranges_async(d_buf, buf_len, buf_base, rg, delim, every_k, emit_add, carry, out.ptr,
                                    out_mode, cap)
            n, nd, ends = self.delim_ranges_result(len(rg) // 2)
            vals = self.d2h(np.empty(n, dtype), out.ptr)
            if out_mode == 3:
                return vals, nd, ends, self.block_table(out.ptr, cap, rg)
            if out_mode == 4:
                return vals, nd, ends, self.block_table(out.ptr, cap, rg, 4), self.sub_table(out.ptr, cap, rg)
            return vals, nd, ends
        return _retry_capacity(cap, launch)

    def _line_starts(self, name: str, d_buf: int, buf_len: int, buf_base: int, begin: int, end: int, size: int,
                     first: bool, cap: Optional[int]) -> Tuple[int, int, bool]:
        """The newline launch of one part (``vcf_lines`` / ``fastq_lines``), the uint64 starts left in workspace
        ``name``: (their device address, their number, whether a start equal to ``size`` was dropped)."""
        rg = np.asarray([begin, end], np.uint64)
        if cap is None:
            cap = (end - begin) // 32 + 1024

        def launch(cap):
            ws = self.workspace(name, 8 * (cap + 1) + 16)
            if end > begin:
                self.delim_ranges_async(d_buf, buf_len, buf_base, rg, 10, 1, 1, 0, ws.ptr + 8, 1, cap)
                return ws, self.delim_ranges_result(1)[0]
            return ws, 0
        ws, n = _retry_capacity(cap, launch)
        # only a part that reaches the object's end can hold a start equal to ``size`` (the '\n' is the object's last
        # byte: no line follows it); the others skip the read-back and its synchronisation
        dropped = bool(n and end >= size and int(self.d2h(np.empty(1, np.uint64), ws.ptr + 8 * n)[0]) >= size)
        n -= dropped
        if first and begin < size:
            self.h2d(ws.ptr, np.asarray([begin], np.uint64))
            return ws.ptr, n + 1, dropped
        return ws.ptr + 8, n, dropped

    # ---------------------------------------------------------------- the other libraries' contexts
    def _sub_ctx(self, name: str):
        """(library, handle) of binding module ``name`` (``_SUB_CTXS``): its context on this one's device, created on
        first use on this context's current stream."""
        attr, prefix = _SUB_CTXS[name]
        mod = importlib.import_module("." + name, __package__)
        if getattr(self, attr) is None:
            h = ctypes.c_void_p()
            create = getattr(mod.load(), prefix + "_ctx_create")
            mod.check(create(self.device, ctypes.c_void_p(self.stream), ctypes.byref(h)))
            setattr(self, attr, h)
        return mod.load(), getattr(self, attr)

    # ---------------------------------------------------------------- quote-aware record ends (libdpquote.so)
    def _quote_ctx(self):
        return self._sub_ctx("_quote")

    def quote_geometry(self) -> Tuple[int, int]:
        """(tile bytes, workgroups of the persistent grid) of the record-end kernel (dq_geometry)."""
        from . import _quote
        q, h = self._quote_ctx()
        g = ctypes.c_int(0)
        t = ctypes.c_int(0)
        _quote.check(q.dq_geometry(h, ctypes.byref(g), ctypes.byref(t)))
        return int(t.value), int(g.value)

    @staticmethod
    def record_block_tiles(begin: int, end: int) -> int:
        """Entries of the block table of object bytes [begin, end): the 64 KiB blocks that hold one of them."""
        return ((end - 1) >> 16) - (begin >> 16) + 1 if end > begin else 0

    def records_async(self, d_buf: int, buf_len: int, buf_base: int, begin: int, end: int, *, quote: int = 34,
                      carry: int = 0, escape: Optional[int] = None, esc_carry: int = 0, scope: str = "all", form: str,
                      d_out: int = 0, cap: int = 0, d_table: int = 0, table_cap: int = 0) -> None:
        """One launch of the record-end kernel over object bytes [begin, end) (include/dpquote.h), collected by
        ``records_result``: the only place that picks among the dq_records_*_async entry points.  ``form`` "u32" /
        "u64": offsets at ``d_out``; "u16b": uint16 low words at ``d_out`` and the 64 KiB block table at ``d_table``
        (the device address of ``begin`` must be congruent to ``begin`` mod 16); "count": no output.  ``escape``: the
        byte after an unescaped escape byte is literal (``esc_carry``: the byte at ``begin`` is escaped; ``scope``
        "all" or "quoted"), None: the plain launch."""
        from . import _quote
        _, flags = _record_form(form, escape, scope)
        esc = () if escape is None else (int(escape), int(esc_carry), flags)
        q, h = self._quote_ctx()
        if form == "u16b":
            fn = q.dq_records_blocked_async if escape is None else q.dq_records_esc_blocked_async
            out = (ctypes.c_void_p(d_out or 0), int(cap), ctypes.c_void_p(d_table or 0), int(table_cap))
        else:
            fn = q.dq_records_async if escape is None else q.dq_records_esc_async
            if form == "count":
                d_out = cap = 0
            out = (ctypes.c_void_p(d_out or 0), int(form != "u32"), int(cap))
        _quote.check(fn(h, ctypes.c_void_p(d_buf), buf_len, buf_base, begin, end, int(quote), int(carry), *esc, *out))

    def records_result(self) -> RecordCounts:
        """(record ends, quote bytes, newlines, toggles) of the launch in flight: ``toggles`` are the quote bytes that
        are not escaped (all of them after a plain launch).  DPCapacityError carries ``needed``, ``n_quotes``,
        ``n_newlines`` and ``n_toggles``; a run of escape bytes beyond DQ_ESCAPE_RUN_MAX raises
        ``_quote.DPEscapeRunError``."""
        from . import _quote
        q, h = self._quote_ctx()
        v = [ctypes.c_uint64(0) for _ in range(4)]
        rc = q.dq_records_esc_result(h, *(ctypes.byref(x) for x in v))
        res = RecordCounts(*(int(x.value) for x in v))
        if rc == _quote.DQ_ERR_CAPACITY:
            e = DPCapacityError(rc, _quote.last_error())
            e.needed, e.n_quotes, e.n_newlines, e.n_toggles = res
            raise e
        _quote.check(rc)
        return res

    def records(self, d_buf: int, buf_len: int, buf_base: int, begin: int, end: int, *, quote: int = 34,
                carry: int = 0, escape: Optional[int] = None, esc_carry: int = 0, scope: str = "all",
                form: str = "u64", cap: Optional[int] = None) -> Records:
        """Sorted object offsets of the '\\n' that end a CSV record in object bytes [begin, end): those with an even
        number of ``quote`` bytes (plus ``carry``) before them, escaped quotes not counted (``records_async``).

        ``ends``: uint64 | uint32 offsets; for "u16b" the low 16 bits of each, with ``table[j]`` = the record ends
        before object offset ``((begin >> 16) + j) << 16`` (``scan.objects.BlockedOffsets(ends, table, begin >> 16)``
        decodes them); for "count" None, one launch without output.  ``n``: the record ends."""
        dtype, _ = _record_form(form, escape, scope)
        kw = dict(quote=quote, carry=carry, escape=escape, esc_carry=esc_carry, scope=scope, form=form)
        if form == "count":
            self.records_async(d_buf, buf_len, buf_base, begin, end, **kw)
            r = self.records_result()
            return Records(None, None, *r[1:], r.n)
        if cap is None:
            cap = (end - begin) // 16 + 1024
        nt = self.record_block_tiles(begin, end)

        def launch(cap):
            out = self.workspace("out", cap * np.dtype(dtype).itemsize + 16)
            tab = self.workspace("record_blocks", nt * 8 + 16) if form == "u16b" else None
            self.records_async(d_buf, buf_len, buf_base, begin, end, d_out=out.ptr, cap=cap,
                               d_table=tab.ptr if tab else 0, table_cap=nt if tab else 0, **kw)
            r = self.records_result()
            return Records(self.d2h(np.empty(r.n, dtype), out.ptr),
                           self.d2h(np.empty(nt, np.uint64), tab.ptr) if tab else None, *r[1:], r.n)
        return _retry_capacity(cap, launch)

    # ---------------------------------------------------------------- FASTA .fai counts (libdpfai.so)
    def _fai_ctx(self):
        return self._sub_ctx("_fai")

    def fai_geometry(self) -> Tuple[int, int, int]:
        """(R, the bytes of the range a wave takes at a time; K, the per-wave segment slots; the waves of the grid)
        of fai_count_kernel (dfai_geometry)."""
        from . import _fai
        f, h = self._fai_ctx()
        r, k, g = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
        _fai.check(f.dfai_geometry(h, ctypes.byref(r), ctypes.byref(k), ctypes.byref(g)))
        return int(r.value), int(k.value), int(g.value)

    def fai_counts(self, d_buf: int, buf_len: int, buf_base: int, lo, hi, origin, width=None):
        """Per-segment counts over device bytes (include/dpfai.h): ``lo``, ``hi``, ``origin`` are uint64 object
        offsets of n ascending, disjoint segments clipped to the buffer (``origin``: the unclipped body start).
        Without ``width`` pass 1: (nl, cr, first) uint64 arrays, ``first`` all-ones where the segment holds no
        '\\n'.  With ``width`` (uint32 per segment) pass 2: (off, lastoff)."""
        from . import _fai
        f, h = self._fai_ctx()
        seg = np.ascontiguousarray(np.stack([np.asarray(a, np.uint64).reshape(-1) for a in (lo, hi, origin)]))
        n = seg.shape[1]
        nout = 3 if width is None else 2
        if n == 0:
            return tuple(np.zeros(0, np.uint64) for _ in range(nout))
        ws = self.workspace("fai_seg", 7 * 8 * n + 16)
        d_seg, d_out, d_w = ws.ptr, ws.ptr + 24 * n, ws.ptr + 48 * n
        self.h2d(d_seg, seg)
        p = ctypes.c_void_p
        if width is None:
            _fai.check(f.dfai_count_async(h, p(d_buf), buf_len, buf_base, p(d_seg), p(d_seg + 8 * n),
                                          p(d_seg + 16 * n), n, p(d_out), p(d_out + 8 * n), p(d_out + 16 * n)))
        else:
            w = np.ascontiguousarray(np.asarray(width, np.uint32).reshape(-1))
            if len(w) != n:
                raise ValueError("width must hold one entry per segment")
            self.h2d(d_w, w)
            _fai.check(f.dfai_offgrid_async(h, p(d_buf), buf_len, buf_base, p(d_seg), p(d_seg + 8 * n),
                                            p(d_seg + 16 * n), p(d_w), n, p(d_out), p(d_out + 8 * n)))
        out = self.d2h(np.empty((nout, n), np.uint64), d_out)
        return tuple(out[i] for i in range(nout))

    def fai_names(self, d_buf: int, buf_len: int, buf_base: int, starts, ends):
        """The names of the headers whose '>' lie at object offsets ``starts`` and which end before ``ends`` (both
        clipped to the buffer): (lengths uint32, the names packed back to back as uint8) -- the bytes after the '>'
        up to the first space, tab, '\\r' or '\\n', or up to ``ends``.  Two launches of fai_name_kernel; the
        exclusive sums between them are made on the host."""
        from . import _fai
        f, h = self._fai_ctx()
        se = np.ascontiguousarray(np.stack([np.asarray(a, np.uint64).reshape(-1) for a in (starts, ends)]))
        n = se.shape[1]
        if n == 0:
            return np.zeros(0, np.uint32), np.zeros(0, np.uint8)
        ws = self.workspace("fai_hdr", 28 * n + 16)
        d_se, d_off, d_len = ws.ptr, ws.ptr + 16 * n, ws.ptr + 24 * n
        self.h2d(d_se, se)
        p = ctypes.c_void_p
        _fai.check(f.dfai_name_len_async(h, p(d_buf), buf_len, buf_base, p(d_se), p(d_se + 8 * n), n, p(d_len)))
        lens = self.d2h(np.empty(n, np.uint32), d_len)
        offs = np.zeros(n, np.uint64)
        np.cumsum(lens[:-1], dtype=np.uint64, out=offs[1:])
        total = int(offs[-1]) + int(lens[-1])
        if total == 0:
            return lens, np.zeros(0, np.uint8)
        out = self.workspace("fai_names", total + 16)
        self.h2d(d_off, offs)
        _fai.check(f.dfai_name_copy_async(h, p(d_buf), buf_len, buf_base, p(d_se), p(d_len), p(d_off), n,
                                          p(out.ptr), total))
        return lens, self.d2h(np.empty(total, np.uint8), out.ptr)

    # ---------------------------------------------------------------- VCF CHROM / POS (libdpvpos.so)
    def _vpos_ctx(self):
        return self._sub_ctx("_vpos")

    def vpos_geometry(self) -> Tuple[int, int]:
        """(lines per workgroup of vpos_parse_kernel, of vpos_reduce_kernel) (dvp_geometry)."""
        from . import _vpos
        v, h = self._vpos_ctx()
        a, b = ctypes.c_int(0), ctypes.c_int(0)
        _vpos.check(v.dvp_geometry(h, ctypes.byref(a), ctypes.byref(b)))
        return int(a.value), int(b.value)

    def vcf_parse(self, d_buf: int, buf_len: int, buf_base: int, size: int, d_starts: int, n: int) -> None:
        """The parse launch (vpos_parse_kernel) over ``n`` uint64 line starts at device address ``d_starts``; pos,
        clen and flags stay in the context's workspace for ``vcf_positions``."""
        from . import _vpos
        v, h = self._vpos_ctx()
        n = int(n)
        ws = self.workspace("vpos_lines", 7 * n + 64)
        d_pos, d_clen = ws.ptr, ws.ptr + 4 * n
        d_clen += d_clen & 1
        d_flags = d_clen + 2 * n
        p = ctypes.c_void_p
        _vpos.check(v.dvp_parse_async(h, p(d_buf), int(buf_len), int(buf_base), int(size), p(d_starts), n, p(d_pos),
                                      p(d_clen), p(d_flags)))
        self._vp = dict(d_buf=d_buf, buf_len=int(buf_len), buf_base=int(buf_base), size=int(size),
                        d_starts=d_starts, n=n, d_pos=d_pos, d_clen=d_clen, d_flags=d_flags)

    def vcf_lines(self, d_buf: int, buf_len: int, buf_base: int, begin: int, end: int, size: int,
                  first: bool = False, cap: Optional[int] = None) -> int:
        """The newline launch and the parse launch of one part: the lines that start at p + 1 for a '\\n' at p in
        object bytes [begin, end), with ``first`` also the line at ``begin`` itself, in front; a start equal to
        ``size`` is dropped.  Returns the number of lines.  The uint64 starts come from the newline kernel
        (``delim_ranges_async`` out_mode 1, emit_add 1) and never leave the device."""
        d_starts, n, _ = self._line_starts("vpos_starts", d_buf, buf_len, buf_base, begin, end, size, first, cap)
        self.vcf_parse(d_buf, buf_len, buf_base, size, d_starts, n)
        return n

    def vcf_positions(self, ordinal0: int, every: int, run_cap: int = 1024) -> VcfPositions:
        """The reduce launch (vpos_reduce_kernel) over the lines of the last ``vcf_lines`` / ``vcf_parse``, line 0 of
        which has the global ordinal ``ordinal0``, and the names launch over its run starts (include/dpvpos.h).  Only
        the samples, the runs, the names and the result words are read back."""
        from . import _vpos
        v, h = self._vpos_ctx()
        s = self._vp
        n = s["n"]
        k = int(every)
        ns = -(-(ordinal0 + n) // k) - -(-ordinal0 // k) if k > 0 else 0
        p = ctypes.c_void_p

        def launch(cap):
            ws = self.workspace("vpos_out", 4 * ns + 20 * cap + 8 * _vpos.R_WORDS + 64)
            d_res = ws.ptr
            d_runs = d_res + 8 * _vpos.R_WORDS
            d_ends = d_runs + 8 * cap
            d_rcl = d_ends + 8 * cap
            d_smp = d_rcl + 4 * cap
            _vpos.check(v.dvp_reduce_async(h, p(s["d_pos"]), p(s["d_clen"]), p(s["d_flags"]), n, int(ordinal0), k,
                                           p(d_smp), p(d_runs), p(d_ends), p(d_rcl), cap, p(d_res)))
            res = self.d2h(np.empty(_vpos.R_WORDS, np.uint64), d_res)
            if int(res[_vpos.R_RUNS]) > cap:
                e = DPCapacityError(_lib.DP_ERR_CAPACITY, f"run capacity below {int(res[_vpos.R_RUNS])} entries")
                e.needed = int(res[_vpos.R_RUNS])
                raise e
            m = int(res[_vpos.R_RUNS])
            out = self.d2h(np.empty(20 * cap + 4 * ns, np.uint8), d_runs)
            return res, m, out[:8 * m].view(np.uint64), out[8 * cap:8 * cap + 8 * m].view(np.uint64), \
                out[16 * cap:16 * cap + 4 * m].view(np.uint32), out[20 * cap:].view(np.uint32).copy()
        res, m, runs, ends, rcl, samples = _retry_capacity(max(1, int(run_cap)), launch)
        order = np.argsort(runs, kind="stable")
        runs, rcl, ends = runs[order], rcl[order], np.sort(ends)
        run_line = (runs >> np.uint64(32)).astype(np.int64)
        lens = rcl.astype(np.int64)
        total = int(lens.sum())
        names, run_offset = [], np.zeros(0, np.uint64)
        if m:
            offs = np.zeros(m, np.uint64)
            np.cumsum(lens[:-1], out=offs[1:], dtype=np.uint64)
            ws = self.workspace("vpos_names", 20 * m + total + 64)
            d_off, d_ls, d_lines = ws.ptr, ws.ptr + 8 * m, ws.ptr + 16 * m
            d_out = d_lines + 4 * m
            self.h2d(d_off, offs)
            self.h2d(d_lines, run_line.astype(np.uint32))
            _vpos.check(v.dvp_names_async(h, p(s["d_buf"]), s["buf_len"], s["buf_base"], p(s["d_starts"]),
                                          p(s["d_clen"]), n, p(d_lines), p(d_off), m, p(d_out), total, p(d_ls)))
            run_offset = self.d2h(np.empty(m, np.uint64), d_ls)
            raw = self.d2h(np.empty(total, np.uint8), d_out).tobytes()
            names = [raw[int(o):int(o) + int(ln)] for o, ln in zip(offs, lens)]
        none = np.uint64(_vpos.DVP_NONE)
        low = lambda w: None if res[w] == none else int(res[w])
        at = lambda i: None if i is None else int(self.d2h(np.empty(1, np.uint64), s["d_starts"] + 8 * i)[0])
        fm, fu = low(_vpos.R_MIN_MALFORMED), low(_vpos.R_MIN_UNSORTED)
        return VcfPositions(n, samples, run_line, (runs & np.uint64(0xFFFFFFFF)).astype(np.int64),
                            (ends >> np.uint64(32)).astype(np.int64), (ends & np.uint64(0xFFFFFFFF)).astype(np.int64),
                            names, run_offset, int(res[_vpos.R_MALFORMED]), fm, int(res[_vpos.R_UNSORTED]), fu,
                            int(res[_vpos.R_FIRST_POS]), int(res[_vpos.R_LAST_POS]), at(0 if n else None), at(fm),
                            at(fu))

    # ---------------------------------------------------------------- VCF record ends (libdpvspan.so)
    def _vspan_ctx(self):
        return self._sub_ctx("_vspan")

    def vspan_geometry(self) -> Tuple[int, int]:
        """(lines per workgroup of vspan_span_kernel, of vspan_blockmax_kernel) (dvs_geometry)."""
        from . import _vspan
        v, h = self._vspan_ctx()
        a, b = ctypes.c_int(0), ctypes.c_int(0)
        _vspan.check(v.dvs_geometry(h, ctypes.byref(a), ctypes.byref(b)))
        return int(a.value), int(b.value)

    def vcf_spans(self, ordinal0: int, every: int) -> VcfSpans:
        """The span launch (vspan_span_kernel) and the block-max launch (vspan_blockmax_kernel) over the lines the last
        ``vcf_lines`` / ``vcf_parse`` left resident -- their starts and their parsed POS -- line 0 of which has the
        global ordinal ``ordinal0`` (include/dpvspan.h).  Only the slots, the result words and the offsets of the
        flagged lines are read back."""
        from . import _vspan
        v, h = self._vspan_ctx()
        s = self._vp
        n, k = s["n"], int(every)
        ns = (ordinal0 + n - 1) // k - ordinal0 // k + 1 if n else 0
        ws = self.workspace("vspan_lines", 5 * n + 64)
        d_end, d_flags = ws.ptr, ws.ptr + 4 * n
        wo = self.workspace("vspan_out", 8 * _vspan.R_WORDS + 4 * ns + 64)
        d_res, d_max = wo.ptr, wo.ptr + 8 * _vspan.R_WORDS
        p = ctypes.c_void_p
        _vspan.check(v.dvs_span_async(h, p(s["d_buf"]), s["buf_len"], s["buf_base"], int(s["size"]), p(s["d_starts"]),
                                      n, p(s["d_pos"]), p(d_end), p(d_flags)))
        _vspan.check(v.dvs_blockmax_async(h, p(d_end), p(d_flags), p(s["d_pos"]), n, int(ordinal0), k, p(d_max),
                                          p(d_res)))
        out = self.d2h(np.empty(8 * _vspan.R_WORDS + 4 * ns, np.uint8), d_res)
        res, slots = out[:8 * _vspan.R_WORDS].view(np.uint64), out[8 * _vspan.R_WORDS:].view(np.uint32).copy()
        none = np.uint64(_vspan.DVS_NONE)
        low = lambda w: None if res[w] == none else int(res[w])
        at = lambda i: None if i is None else int(self.d2h(np.empty(1, np.uint64), s["d_starts"] + 8 * i)[0])
        fm, ft = low(_vspan.R_MIN_MISSING), low(_vspan.R_MIN_TRUNCATED)
        return VcfSpans(n, slots, int(res[_vspan.R_MISSING]), fm, int(res[_vspan.R_TRUNCATED]), ft,
                        int(res[_vspan.R_FROM_END]), int(res[_vspan.R_MAX_SPAN]), at(fm), at(ft))

    # ---------------------------------------------------------------- FASTQ reads (libdpfq.so)
    def _fq_ctx(self):
        return self._sub_ctx("_fq")

    def fq_geometry(self) -> Tuple[int, int]:
        """(reads per workgroup of fq_read_kernel and fq_sample_kernel, lanes of fq_scan_kernel) (dfq_geometry)."""
        from . import _fq
        f, h = self._fq_ctx()
        a, b = ctypes.c_int(0), ctypes.c_int(0)
        _fq.check(f.dfq_geometry(h, ctypes.byref(a), ctypes.byref(b)))
        return int(a.value), int(b.value)

    def fastq_lines(self, d_buf: int, buf_len: int, buf_base: int, begin: int, end: int, size: int,
                    first: bool = False, cap: Optional[int] = None) -> int:
        """The newline launch of one part, with ``vcf_lines``' ownership: the lines that start at p + 1 for a '\n' at
        p in object bytes [begin, end), with ``first`` also the line at ``begin`` itself, in front; a start equal to
        ``size`` is dropped.  Returns the number of lines.  The uint64 starts come from the newline kernel
        (``delim_ranges_async`` out_mode 1, emit_add 1) and stay on the device for ``fastq_reads``."""
        d_starts, n, closed = self._line_starts("fq_starts", d_buf, buf_len, buf_base, begin, end, size, first, cap)
        self._fq = dict(d_buf=d_buf, buf_len=int(buf_len), buf_base=int(buf_base), size=int(size), d_starts=d_starts,
                        n=n, last=end >= size, closed=closed)
        return n

    def fastq_reads(self, skip: int, read0: int, every: int) -> FastqPart:
        """The three launches (fq_read_kernel, fq_scan_kernel, fq_sample_kernel; include/dpfq.h) over the lines of the
        last ``fastq_lines``: the first ``skip`` lines belong to a read begun before the part, and the reads whose four
        lines are all complete in the part -- every owned line but the last, whose terminator lies beyond the part's
        bytes, or every line where the part reaches the object's end -- are the device's, read ``read0`` on.  A part
        with fewer than 8 lines leaves them all to the host.  Only the samples, the result words and the starts of
        the edge lines are read back."""
        from . import _fq
        s = self._fq
        n, skip, read0, k = s["n"], int(skip), int(read0), int(every)
        if k < 1 or k & (k - 1):
            raise ValueError(f"every must be a power of two >= 1, not {every}")
        from .fastq import part_plan
        nr, lines = part_plan(n, skip, s["last"])
        d_starts = s["d_starts"]
        u64 = lambda i0, i1: self.d2h(np.empty(max(0, i1 - i0), np.uint64), d_starts + 8 * i0)
        if nr == 0:
            return FastqPart(n, skip, read0, 0, np.zeros((0, 2), np.uint64), 0, 0, None, 0, None, None, 0, lines,
                             u64(0, n), s["closed"])
        tail = u64(skip + 4 * nr, n)
        starts = np.concatenate([u64(0, skip + 1), tail])
        last_end = int(tail[0]) - 1 if len(tail) else s["size"] - (1 if s["closed"] else 0)
        f, h = self._fq_ctx()
        g = self.fq_geometry()[0]
        nb = -(-nr // g)
        ns = -(-(read0 + nr) // k) - -(-read0 // k)
        ws = self.workspace("fq_reads", 48 + 16 * ns + 8 * nb + 5 * nr + 64)
        d_res, d_smp = ws.ptr, ws.ptr + 48
        d_block = d_smp + 16 * ns
        d_len = d_block + 8 * nb
        d_flags = d_len + 4 * nr
        p = ctypes.c_void_p
        _fq.check(f.dfq_reads_async(h, p(s["d_buf"]), s["buf_len"], s["buf_base"], s["size"], p(d_starts), skip, nr,
                                    last_end, p(d_len), p(d_flags), p(d_block), p(d_res)))
        _fq.check(f.dfq_scan_async(h, p(d_block), nb, p(d_res)))
        _fq.check(f.dfq_sample_async(h, p(d_starts), skip, p(d_len), p(d_block), nr, read0, k, p(d_smp)))
        out = self.d2h(np.empty(48 + 16 * ns, np.uint8), d_res)
        res = out[:8 * _fq.R_WORDS].view(np.uint64)
        fm = None if int(res[_fq.R_MIN_MALFORMED]) == _fq.DFQ_NONE else int(res[_fq.R_MIN_MALFORMED])
        kind, off = 0, None
        if fm is not None:
            kind = int(self.d2h(np.empty(1, np.uint8), d_flags + fm)[0])
            off = int(u64(skip + 4 * fm, skip + 4 * fm + 1)[0])
        return FastqPart(n, skip, read0, nr, out[48:].view(np.uint64).reshape(-1, 2).copy(), int(res[_fq.R_BASES]),
                         int(res[_fq.R_MALFORMED]), fm, kind, off, int(res[_fq.R_MIN_LEN]), int(res[_fq.R_MAX_LEN]),
                         lines, starts, s["closed"])

    def find_delim(self, d_buf: int, buf_len: int, buf_base: int, start: int, delim: int = 10) -> int:
        """First object offset >= start holding ``delim`` in the buffer, or -1."""
        pos = ctypes.c_int64(-1)
        check(self.lib.dp_find_delim(self.handle, ctypes.c_void_p(d_buf), buf_len, buf_base, start, int(delim),
                                     ctypes.byref(pos)))
        return int(pos.value)

    # ---------------------------------------------------------------- host-buffer conveniences
    def fasta_index_host(self, data, buf_base: int, obj_size: int, chunks, u64: bool = False):
        ptr, n = self.upload(data)
        return self.fasta_index(ptr, n, buf_base, obj_size, chunks, u64=u64)

    def delim_index_host(self, data, buf_base: int, begin: int, end: int, **kw):
        ptr, n = self.upload(data)
        return self.delim_index(ptr, n, buf_base, begin, end, **kw)

    def find_delim_host(self, data, buf_base: int, start: int, delim: int = 10) -> int:
        ptr, n = self.upload(data, name="halo")
        return self.find_delim(ptr, n, buf_base, start, delim)

    def stream_read(self, d_buf: int, nbytes: int, blocks_per_cu: int = 0) -> None:
        """Calibration read of ``nbytes`` device bytes (async; time it with timing())."""
        check(self.lib.dp_stream_read(self.handle, ctypes.c_void_p(d_buf), nbytes, blocks_per_cu))

    def stream_rw(self, d_in: int, nbytes: int, d_out: int, write_per_read: float, blocks_per_cu: int = 0) -> None:
        """Calibration read of ``nbytes`` plus ``write_per_read * nbytes`` contiguous output bytes (async)."""
        q = int(round(write_per_read * 65536))
        check(self.lib.dp_stream_rw(self.handle, ctypes.c_void_p(d_in), nbytes, ctypes.c_void_p(d_out if q else 0),
                                    q, blocks_per_cu))

    # ---------------------------------------------------------------- timing / geometry
    def timing(self, enable: bool) -> None:
        check(self.lib.dp_timing_enable(self.handle, int(bool(enable))))
        self._timing_on = bool(enable)

    def timing_read(self) -> Tuple[float, int]:
        ms = ctypes.c_double(0.0)
        n = ctypes.c_uint64(0)
        check(self.lib.dp_timing_read(self.handle, ctypes.byref(ms), ctypes.byref(n)))
        return float(ms.value), int(n.value)

    _FORM_KEYS = {"fasta": _lib.DP_FORM_FASTA, "delim": _lib.DP_FORM_DELIM,
                  "delim_line_max": _lib.DP_FORM_DELIM_LINE_MAX, "delim_dense": _lib.DP_FORM_DELIM_DENSE}

    def set_form(self, **kw) -> None:
        """dp_ctx_set_form: fasta=0 (map + placement, default) | 1 (one-pass); delim=0 (auto, default) | 1 (line) |
        3 (one-pass); delim_line_max=bytes; delim_dense=delimiters per KiB x 1000.  The shipped
        defaults need no call; tests and A/B runs pin a form with it."""
        for k, v in kw.items():
            check(self.lib.dp_ctx_set_form(self.handle, self._FORM_KEYS[k], int(v)))

    def get_form(self, key: str) -> int:
        v = ctypes.c_uint64(0)
        check(self.lib.dp_ctx_get_form(self.handle, self._FORM_KEYS[key], ctypes.byref(v)))
        return int(v.value)

    DELIM_FORMS = {0: "auto: the density probe picks per launch",
                   1: "line_kernel<DELIM> (lockstep one pass)",
                   3: "scan_kernel<DELIM> (one-pass look-back)"}

    def delim_form(self, span: int, out_mode: int = 3) -> int:
        """The kernels a newline launch of ``span`` bytes into ``out_mode`` takes (dp_scan_delim_form: 1 line,
        3 one-pass; 0: the launch's own bytes decide on the device)."""
        f = ctypes.c_int(0)
        check(self.lib.dp_scan_delim_form(self.handle, int(span), int(out_mode), ctypes.byref(f)))
        return int(f.value)

    def last_delim_form(self) -> int:
        """The kernels the last collected newline launch ran (dp_last_delim_form: 1 or 3; 0 before any)."""
        f = ctypes.c_int(0)
        check(self.lib.dp_last_delim_form(self.handle, ctypes.byref(f)))
        return int(f.value)

    def geometry(self) -> Tuple[int, int]:
        g = ctypes.c_int(0)
        u = ctypes.c_int(0)
        check(self.lib.dp_scan_geometry(self.handle, ctypes.byref(g), ctypes.byref(u)))
        return int(g.value), int(u.value)

    def close(self) -> None:
        if self._get_pool is not None:
            self._get_pool.shutdown(wait=True)
            self._get_pool = None
        for name, (attr, prefix) in _SUB_CTXS.items():
            h = getattr(self, attr, None)                 # (a context built without some of them closes too)
            if h is not None:
                mod = importlib.import_module("." + name, __package__)
                setattr(self, attr, None)
                mod.check(getattr(mod.load(), prefix + "_ctx_destroy")(h))
        if self.handle:
            for b in list(self._bufs.values()) + list(self._pinned.values()):
                b.free()
            self._bufs.clear()
            self._pinned.clear()
            check(self.lib.dp_ctx_destroy(self.handle))
            self.handle = None

    def __del__(self):  # pragma: no cover - interpreter shutdown order
        try:
            self.close()
        except Exception:
            pass


_tls = threading.local()


def device_count() -> int:
    return _lib.device_count()


def get_context(device: int = 0, slot: int = 0) -> ScanContext:
    """The calling thread's context for ``device`` (created on first use); ``slot`` > 0 names further contexts of
    the thread on the same device (their own stream and buffers: a thread alternating two overlaps one's copies with
    the other's scan)."""
    ctxs = getattr(_tls, "ctxs", None)
    if ctxs is None:
        ctxs = _tls.ctxs = {}
    key = device if slot == 0 else (device, slot)
    c = ctxs.get(key)
    if c is None:
        c = ctxs[key] = ScanContext(device)
    return c


def close_context(device: int = 0) -> None:
    """Close the calling thread's contexts for ``device``, if any (their streams, pinned staging and HBM workspaces
    are freed; the next ``get_context`` makes new ones)."""
    ctxs = getattr(_tls, "ctxs", {})
    for key in [k for k in ctxs if k == device or (isinstance(k, tuple) and k[0] == device)]:
        ctxs.pop(key).close()


def pick_device(i: int, devices: Optional[Iterable[int]] = None) -> int:
    """Round-robin device for job ``i`` over ``devices`` (default: every visible GPU)."""
    devs = list(devices) if devices is not None else list(range(max(1, device_count())))
    return devs[i % len(devs)]
