"""ctypes binding of libdpquote.so (the C ABI declared in include/dpquote.h): the quote-aware CSV record index.

Built in-tree by ``dataplug_amd.build.build_quote()`` into ``dataplug_amd/lib/libdpquote.so``.  The refusal rules
are those of ``_lib.py``: there is NO fallback -- a missing or unloadable library raises ``DPScanUnavailable``, and
so does one whose ISA-guard stamp (``<lib>.isa.json``) is missing, failed or belongs to another file.
"""
from __future__ import annotations

import ctypes
import os

from ._lib import DPScanError, load_guarded, raise_for

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DPQUOTE_LIB", os.path.join(os.path.dirname(_HERE), "lib", "libdpquote.so"))

DQ_OK = 0
DQ_ERR_INVALID = 1
DQ_ERR_HIP = 2
DQ_ERR_CAPACITY = 3
DQ_ERR_OVERFLOW = 4
DQ_ERR_TIMEOUT = 5
DQ_ERR_ESCAPE_RUN = 6

DQ_ESCAPE_RUN_MAX = 1 << 20              # include/dpquote.h: runs of escape bytes up to this many bytes are exact
DQ_ESC_SCOPE_QUOTED = 1                  # flags bit of the escape-aware launches
ESCAPE_SCOPES = {"all": 0, "quoted": DQ_ESC_SCOPE_QUOTED}

# (name, restype, argtypes) for every symbol include/dpquote.h declares
_c = ctypes
_p = _c.c_void_p
_u64 = _c.c_uint64
_u64p = _c.POINTER(_c.c_uint64)
SIGNATURES = [
    ("dq_abi_version", _c.c_int, []),
    ("dq_last_error", _c.c_char_p, []),
    ("dq_ctx_create", _c.c_int, [_c.c_int, _p, _c.POINTER(_p)]),
    ("dq_ctx_destroy", _c.c_int, [_p]),
    ("dq_records_async", _c.c_int, [_p, _p, _u64, _u64, _u64, _u64, _c.c_uint32, _c.c_uint32, _p, _c.c_int, _u64]),
    ("dq_records_blocked_async", _c.c_int, [_p, _p, _u64, _u64, _u64, _u64, _c.c_uint32, _c.c_uint32, _p, _u64, _p,
                                            _u64]),
    ("dq_records_result",_c.c_int, [_p, _u64p, _u64p, _u64p]),
    ("dq_records_esc_async", _c.c_int, [_p, _p, _u64, _u64, _u64, _u64, _c.c_uint32, _c.c_uint32, _c.c_uint32,
                                        _c.c_uint32, _c.c_uint32, _p, _c.c_int, _u64]),
    ("dq_records_esc_blocked_async", _c.c_int, [_p, _p, _u64, _u64, _u64, _u64, _c.c_uint32, _c.c_uint32,
                                                _c.c_uint32, _c.c_uint32, _c.c_uint32, _p, _u64, _p, _u64]),
    ("dq_records_esc_result", _c.c_int, [_p, _u64p, _u64p, _u64p, _u64p]),
    ("dq_geometry", _c.c_int, [_p, _c.POINTER(_c.c_int), _c.POINTER(_c.c_int)]),
]

_lib = None
ABI_VERSION = 1                          # include/dpquote.h DQ_ABI_VERSION


def load(path: str = None):
    """Load libdpquote.so once (raises DPScanUnavailable); ``path`` loads another file, uncached (tests)."""
    global _lib
    if path is None and _lib is not None:
        return _lib
    lib = load_guarded(path or LIB_PATH, SIGNATURES, "dq_abi_version", ABI_VERSION, exact=True)
    if path is None:
        _lib = lib
    return lib


class DPEscapeRunError(DPScanError):
    """A run of escape bytes longer than DQ_ESCAPE_RUN_MAX: no index is returned (DQ_ERR_ESCAPE_RUN)."""


def escape_flags(scope: str) -> int:
    if scope not in ESCAPE_SCOPES:
        raise ValueError(f"escape_scope must be 'all' or 'quoted', not {scope!r}")
    return ESCAPE_SCOPES[scope]


def last_error() -> str:
    return (load().dq_last_error() or b"").decode(errors="replace")


def check(rc: int) -> None:
    if rc != DQ_OK:
        raise_for(rc, last_error(), ((DQ_ERR_ESCAPE_RUN, DPEscapeRunError),))
