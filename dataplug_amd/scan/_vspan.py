"""ctypes binding of libdpvspan.so (the C ABI declared in include/dpvspan.h): the record ends of a VCF body.

Built in-tree by ``dataplug_amd.build.build_vspan()`` into ``dataplug_amd/lib/libdpvspan.so``.  The refusal rules are
those of ``_lib.py``, ``_quote.py``, ``_fai.py`` and ``_vpos.py``: there is NO fallback -- a missing or unloadable
library raises ``DPScanUnavailable``, and so does one whose ISA-guard stamp (``<lib>.isa.json``) is missing, failed or
belongs to another file.
"""
from __future__ import annotations

import ctypes
import os

from ._lib import load_guarded, raise_for

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DPVSPAN_LIB", os.path.join(os.path.dirname(_HERE), "lib", "libdpvspan.so"))

DVS_OK = 0
DVS_ERR_INVALID = 1
DVS_ERR_HIP = 2
DVS_NONE = 0xFFFFFFFFFFFFFFFF            # a lowest index of which there is none
VSPAN_END_MAX = 2**31 - 1
VSPAN_MISSING_REF, VSPAN_TRUNCATED, VSPAN_FROM_END = 1, 2, 4
# the result words of dvs_blockmax_async
R_MISSING, R_TRUNCATED, R_FROM_END, R_MAX_SPAN, R_MIN_MISSING, R_MIN_TRUNCATED, R_WORDS = range(7)

# (name, restype, argtypes) for every symbol include/dpvspan.h declares
_c = ctypes
_p = _c.c_void_p
_u64 = _c.c_uint64
_ip = _c.POINTER(_c.c_int)
SIGNATURES = [
    ("dvs_abi_version", _c.c_int, []),
    ("dvs_last_error", _c.c_char_p, []),
    ("dvs_ctx_create", _c.c_int, [_c.c_int, _p, _c.POINTER(_p)]),
    ("dvs_ctx_destroy", _c.c_int, [_p]),
    ("dvs_span_async", _c.c_int, [_p, _p, _u64, _u64, _u64, _p, _u64, _p, _p, _p]),
    ("dvs_blockmax_async", _c.c_int, [_p, _p, _p, _p, _u64, _u64, _c.c_uint32, _p, _p]),
    ("dvs_geometry", _c.c_int, [_p, _ip, _ip]),
]

_lib = None
ABI_VERSION = 1                          # include/dpvspan.h DVS_ABI_VERSION


def load(path: str = None):
    """Load libdpvspan.so once (raises DPScanUnavailable); ``path`` loads another file, uncached (tests)."""
    global _lib
    if path is None and _lib is not None:
        return _lib
    lib = load_guarded(path or LIB_PATH, SIGNATURES, "dvs_abi_version", ABI_VERSION, exact=True)
    if path is None:
        _lib = lib
    return lib


def last_error() -> str:
    return (load().dvs_last_error() or b"").decode(errors="replace")


def check(rc: int) -> None:
    if rc != DVS_OK:
        raise_for(rc, last_error())
