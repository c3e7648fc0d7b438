"""ctypes binding of libdpfai.so (the C ABI declared in include/dpfai.h): the per-sequence counts of a FASTA .fai.

Built in-tree by ``dataplug_amd.build.build_fai()`` into ``dataplug_amd/lib/libdpfai.so``.  The refusal rules are
those of ``_lib.py`` and ``_quote.py``: there is NO fallback -- a missing or unloadable library raises
``DPScanUnavailable``, and so does one whose ISA-guard stamp (``<lib>.isa.json``) is missing, failed or belongs to
another file.
"""
from __future__ import annotations

import ctypes
import os

from ._lib import load_guarded, raise_for

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DPFAI_LIB", os.path.join(os.path.dirname(_HERE), "lib", "libdpfai.so"))

DFAI_OK = 0
DFAI_ERR_INVALID = 1
DFAI_ERR_HIP = 2
DFAI_NONE = 0xFFFFFFFFFFFFFFFF           # first[i] of a segment without any '\n'

# (name, restype, argtypes) for every symbol include/dpfai.h declares
_c = ctypes
_p = _c.c_void_p
_u64 = _c.c_uint64
_ip = _c.POINTER(_c.c_int)
SIGNATURES = [
    ("dfai_abi_version", _c.c_int, []),
    ("dfai_last_error", _c.c_char_p, []),
    ("dfai_ctx_create", _c.c_int, [_c.c_int, _p, _c.POINTER(_p)]),
    ("dfai_ctx_destroy", _c.c_int, [_p]),
    ("dfai_count_async", _c.c_int, [_p, _p, _u64, _u64, _p, _p, _p, _u64, _p, _p, _p]),
    ("dfai_offgrid_async", _c.c_int, [_p, _p, _u64, _u64, _p, _p, _p, _p, _u64, _p, _p]),
    ("dfai_name_len_async", _c.c_int, [_p, _p, _u64, _u64, _p, _p, _u64, _p]),
    ("dfai_name_copy_async", _c.c_int, [_p, _p, _u64, _u64, _p, _p, _p, _u64, _p, _u64]),
    ("dfai_geometry", _c.c_int, [_p, _ip, _ip, _ip]),
]

_lib = None
ABI_VERSION = 1                          # include/dpfai.h DFAI_ABI_VERSION


def load(path: str = None):
    """Load libdpfai.so once (raises DPScanUnavailable); ``path`` loads another file, uncached (tests)."""
    global _lib
    if path is None and _lib is not None:
        return _lib
    lib = load_guarded(path or LIB_PATH, SIGNATURES, "dfai_abi_version", ABI_VERSION, exact=True)
    if path is None:
        _lib = lib
    return lib


def last_error() -> str:
    return (load().dfai_last_error() or b"").decode(errors="replace")


def check(rc: int) -> None:
    if rc != DFAI_OK:
        raise_for(rc, last_error())
