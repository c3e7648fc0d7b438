"""ctypes binding of libdpvpos.so (the C ABI declared in include/dpvpos.h): the CHROM / POS parse of a VCF body.

Built in-tree by ``dataplug_amd.build.build_vpos()`` into ``dataplug_amd/lib/libdpvpos.so``.  The refusal rules are
those of ``_lib.py``, ``_quote.py`` and ``_fai.py``: there is NO fallback -- a missing or unloadable library raises
``DPScanUnavailable``, and so does one whose ISA-guard stamp (``<lib>.isa.json``) is missing, failed or belongs to
another file.
"""
from __future__ import annotations

import ctypes
import os

from ._lib import load_guarded, raise_for

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DPVPOS_LIB", os.path.join(os.path.dirname(_HERE), "lib", "libdpvpos.so"))

DVP_OK = 0
DVP_ERR_INVALID = 1
DVP_ERR_HIP = 2
DVP_NONE = 0xFFFFFFFFFFFFFFFF            # a lowest index of which there is none
VPOS_PREFIX_MAX = 1024
VPOS_SAME, VPOS_MALFORMED = 1, 2
# the result words of dvp_reduce_async
R_RUNS, R_MALFORMED, R_UNSORTED, R_FIRST_POS, R_LAST_POS, R_RUN_ENDS, R_MIN_MALFORMED, R_MIN_UNSORTED, R_WORDS = range(9)

# (name, restype, argtypes) for every symbol include/dpvpos.h declares
_c = ctypes
_p = _c.c_void_p
_u64 = _c.c_uint64
_ip = _c.POINTER(_c.c_int)
SIGNATURES = [
    ("dvp_abi_version", _c.c_int, []),
    ("dvp_last_error", _c.c_char_p, []),
    ("dvp_ctx_create", _c.c_int, [_c.c_int, _p, _c.POINTER(_p)]),
    ("dvp_ctx_destroy", _c.c_int, [_p]),
    ("dvp_parse_async", _c.c_int, [_p, _p, _u64, _u64, _u64, _p, _u64, _p, _p, _p]),
    ("dvp_reduce_async", _c.c_int, [_p, _p, _p, _p, _u64, _u64, _c.c_uint32, _p, _p, _p, _p, _u64, _p]),
    ("dvp_names_async", _c.c_int, [_p, _p, _u64, _u64, _p, _p, _u64, _p, _p, _u64, _p, _u64, _p]),
    ("dvp_geometry", _c.c_int, [_p, _ip, _ip]),
]

_lib = None
ABI_VERSION = 1                          # include/dpvpos.h DVP_ABI_VERSION


def load(path: str = None):
    """Load libdpvpos.so once (raises DPScanUnavailable); ``path`` loads another file, uncached (tests)."""
    global _lib
    if path is None and _lib is not None:
        return _lib
    lib = load_guarded(path or LIB_PATH, SIGNATURES, "dvp_abi_version", ABI_VERSION, exact=True)
    if path is None:
        _lib = lib
    return lib


def last_error() -> str:
    return (load().dvp_last_error() or b"").decode(errors="replace")


def check(rc: int) -> None:
    if rc != DVP_OK:
        raise_for(rc, last_error())
