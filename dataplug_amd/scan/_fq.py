"""ctypes binding of libdpfq.so (the C ABI declared in include/dpfq.h): the read lengths and cumulative bases of an
uncompressed FASTQ.

Built in-tree by ``dataplug_amd.build.build_fq()`` into ``dataplug_amd/lib/libdpfq.so``.  The refusal rules are those
of ``_lib.py``, ``_quote.py``, ``_fai.py`` and ``_vpos.py``: there is NO fallback -- a missing or unloadable library
raises ``DPScanUnavailable``, and so does one whose ISA-guard stamp (``<lib>.isa.json``) is missing, failed or belongs
to another file.
"""
from __future__ import annotations

import ctypes
import os

from ._lib import load_guarded, raise_for

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DPFQ_LIB", os.path.join(os.path.dirname(_HERE), "lib", "libdpfq.so"))

DFQ_OK = 0
DFQ_ERR_INVALID = 1
DFQ_ERR_HIP = 2
DFQ_NONE = 0xFFFFFFFFFFFFFFFF            # a lowest index, or a minimum, of which there is none
WELL_FORMED, BAD_HEADER, BAD_SEPARATOR, LENGTH_MISMATCH = range(4)
# the result words
R_MALFORMED, R_MAX_LEN, R_BASES, R_MIN_MALFORMED, R_MIN_LEN, R_WORDS = range(6)

# (name, restype, argtypes) for every symbol include/dpfq.h declares
_c = ctypes
_p = _c.c_void_p
_u64 = _c.c_uint64
_u32 = _c.c_uint32
_ip = _c.POINTER(_c.c_int)
SIGNATURES = [
    ("dfq_abi_version", _c.c_int, []),
    ("dfq_last_error", _c.c_char_p, []),
    ("dfq_ctx_create", _c.c_int, [_c.c_int, _p, _c.POINTER(_p)]),
    ("dfq_ctx_destroy", _c.c_int, [_p]),
    ("dfq_reads_async", _c.c_int, [_p, _p, _u64, _u64, _u64, _p, _u32, _u64, _u64, _p, _p, _p, _p]),
    ("dfq_scan_async", _c.c_int, [_p, _p, _u64, _p]),
    ("dfq_sample_async", _c.c_int, [_p, _p, _u32, _p, _p, _u64, _u64, _u32, _p]),
    ("dfq_geometry", _c.c_int, [_p, _ip, _ip]),
]

_lib = None
ABI_VERSION = 1                          # include/dpfq.h DFQ_ABI_VERSION


def load(path: str = None):
    """Load libdpfq.so once (raises DPScanUnavailable); ``path`` loads another file, uncached (tests)."""
    global _lib
    if path is None and _lib is not None:
        return _lib
    lib = load_guarded(path or LIB_PATH, SIGNATURES, "dfq_abi_version", ABI_VERSION, exact=True)
    if path is None:
        _lib = lib
    return lib


def last_error() -> str:
    return (load().dfq_last_error() or b"").decode(errors="replace")


def check(rc: int) -> None:
    if rc != DFQ_OK:
        raise_for(rc, last_error())
