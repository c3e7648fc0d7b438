"""The host layer above the C ABI without a GPU and without loading a library: ScanContext.records_async /
records_result / records over a stub that stands in for libdpquote.so and records the calls -- which entry point each
(form, escape) picks and with which positional arguments, the refusals made before any call, the one capacity-retry
loop and the status mapping -- and ``_lib.load_guarded``, the one loader behind the three libraries, over a fake of
``ctypes.CDLL``: every refusal, both ABI-version rules and DPSCAN_LIB's leniency."""
import ctypes
import hashlib
import json

import numpy as np
import pytest

from dataplug_amd.scan import DPCapacityError, _fai, _lib, _quote
from dataplug_amd.scan.device import RecordCounts, Records, ScanContext

HANDLE = 7
BUF = (0x1000, 500, 100, 110, 600)                       # d_buf, buf_len, buf_base, begin, end
HEAD = (HANDLE,) + BUF + (39, 1)                         # ... quote, carry
OUT = dict(d_out=0x2000, cap=55, d_table=0x3000, table_cap=3)


class StubQuote:
    """Stands in for the ctypes library: every dq_* call is recorded as (name, plain argument values...) and returns
    DQ_OK, but dq_records_esc_result, which hands out ``results`` in turn: (status, n, n_quotes, n_newlines,
    toggles)."""

    def __init__(self, results=()):
        self.calls = []
        self.results = list(results)

    def __getattr__(self, name):
        if not name.startswith("dq_"):
            raise AttributeError(name)

        def call(*args):
            self.calls.append((name,) + tuple(getattr(a, "value", a) for a in args))
            return _quote.DQ_OK
        return call

    def dq_last_error(self):
        return b"stub: the last error"

    def dq_records_esc_result(self, h, *refs):
        self.calls.append(("dq_records_esc_result", h.value))
        rc, *values = self.results.pop(0)
        for ref, v in zip(refs, values):
            ref._obj.value = v
        return rc


class Buffer:
    def __init__(self, ptr):
        self.ptr = ptr


@pytest.fixture
def stub_ctx(monkeypatch):
    """(a ScanContext that was never created on a device, the stub behind it): workspace and d2h recorded too."""
    stub = StubQuote()
    monkeypatch.setattr(_quote, "_lib", stub)            # _quote.load(), for the last error's text
    ctx = ScanContext.__new__(ScanContext)
    ctx.handle = ctx._get_pool = ctx._dq = ctx._dfai = None
    ctx._quote_ctx = lambda: (stub, ctypes.c_void_p(HANDLE))
    ptrs = {"out": 0x2000, "record_blocks": 0x3000}

    def workspace(name, nbytes, placed=False):
        stub.calls.append(("workspace", name, nbytes))
        return Buffer(ptrs[name])

    def d2h(out, src):
        stub.calls.append(("d2h", src, out.dtype, len(out)))
        launches = sum(1 for c in stub.calls if c[0].endswith("_async"))
        out[:] = np.arange(len(out)) + 100 * launches   # the data of the launch before it
        return out

    ctx.workspace, ctx.d2h = workspace, d2h
    return ctx, stub


@pytest.mark.parametrize("escape", [None, 92])
@pytest.mark.parametrize("form,symbol,tail", [
    ("count", "dq_records{}_async", (None, 1, 0)),                   # no output through the flat uint64 entry point
    ("u32", "dq_records{}_async", (0x2000, 0, 55)),
    ("u64", "dq_records{}_async", (0x2000, 1, 55)),
    ("u16b", "dq_records{}_blocked_async", (0x2000, 55, 0x3000, 3)),  # d_table / table_cap for the blocked form only
])
def test_records_async_picks_the_entry_point_and_its_arguments(stub_ctx, form, symbol, tail, escape):
    ctx, stub = stub_ctx
    for scope, flags in (("all", 0), ("quoted", _quote.DQ_ESC_SCOPE_QUOTED)):
        stub.calls.clear()
        ctx.records_async(*BUF, quote=39, carry=1, escape=escape, esc_carry=1, scope=scope, form=form, **OUT)
        esc = () if escape is None else (92, 1, flags)
        assert stub.calls == [(symbol.format("" if escape is None else "_esc"),) + HEAD + esc + tail]
    stub.calls.clear()
    ctx.records_async(*BUF, escape=escape, form=form)    # the defaults: quote '"', states 0, no output
    esc = () if escape is None else (92, 0, 0)
    rest = (None, 0, None, 0) if form == "u16b" else (None, int(form != "u32"), 0)
    assert len(stub.calls) == 1 and stub.calls[0][2 + len(BUF):] == (34, 0) + esc + rest


def test_bad_form_or_scope_is_refused_before_any_call(stub_ctx):
    ctx, stub = stub_ctx
    for call in (ctx.records_async, ctx.records):
        for kw in (dict(form="u8s"), dict(form="U64"), dict(form=None), dict(form="u64", escape=92, scope="some"),
                   dict(form="count", escape=92, scope="")):
            with pytest.raises(ValueError):
                call(*BUF, **kw)
    with pytest.raises(TypeError):
        ctx.records_async(*BUF)                          # the launch has no default form
    assert stub.calls == []


def test_records_result_always_asks_for_the_toggles(stub_ctx):
    ctx, stub = stub_ctx
    stub.results = [(_quote.DQ_OK, 5, 8, 9, 8), (_quote.DQ_OK, 5, 8, 9, 6)]
    assert ctx.records_result() == RecordCounts(n=5, n_quotes=8, n_newlines=9, toggles=8) == (5, 8, 9, 8)
    assert ctx.records_result().toggles == 6
    assert stub.calls == [("dq_records_esc_result", HANDLE)] * 2


def test_records_result_maps_the_statuses(stub_ctx):
    ctx, stub = stub_ctx
    stub.results = [(_quote.DQ_ERR_ESCAPE_RUN, 0, 0, 0, 0), (_quote.DQ_ERR_CAPACITY, 9, 4, 12, 3),
                    (_quote.DQ_ERR_OVERFLOW, 1, 0, 1, 0), (_quote.DQ_ERR_TIMEOUT, 0, 0, 0, 0)]
    with pytest.raises(_quote.DPEscapeRunError) as ei:
        ctx.records_result()
    assert ei.value.code == _quote.DQ_ERR_ESCAPE_RUN and "stub: the last error" in str(ei.value)
    with pytest.raises(DPCapacityError) as ei:
        ctx.records_result()
    e = ei.value
    assert (e.code, e.needed, e.n_quotes, e.n_newlines, e.n_toggles) == (_quote.DQ_ERR_CAPACITY, 9, 4, 12, 3)
    with pytest.raises(OverflowError):
        ctx.records_result()
    with pytest.raises(_lib.DPScanError) as ei:
        ctx.records_result()
    assert type(ei.value) is _lib.DPScanError and ei.value.code == _quote.DQ_ERR_TIMEOUT


@pytest.mark.parametrize("form,dtype,item", [("u32", np.uint32, 4), ("u64", np.uint64, 8), ("u16b", np.uint16, 2)])
def test_records_relaunches_once_with_the_needed_capacity(stub_ctx, form, dtype, item):
    ctx, stub = stub_ctx
    stub.results = [(_quote.DQ_ERR_CAPACITY, 9, 4, 12, 3), (_quote.DQ_OK, 9, 4, 12, 3)]
    begin, end = 110, 600 + (1 << 16)                    # two 64 KiB blocks
    r = ctx.records(0x1000, 1 << 17, 100, begin, end, escape=92, form=form, cap=2)
    blocked = form == "u16b"
    sym = "dq_records_esc_blocked_async" if blocked else "dq_records_esc_async"
    head = (HANDLE, 0x1000, 1 << 17, 100, begin, end, 34, 0, 92, 0, 0)
    tab = [("workspace", "record_blocks", 2 * 8 + 16)] if blocked else []

    def tail(cap):
        return (0x2000, cap, 0x3000, 2) if blocked else (0x2000, int(form == "u64"), cap)
    assert stub.calls == (
        [("workspace", "out", 2 * item + 16)] + tab + [(sym,) + head + tail(2), ("dq_records_esc_result", HANDLE)] +
        [("workspace", "out", 9 * item + 16)] + tab + [(sym,) + head + tail(9), ("dq_records_esc_result", HANDLE)] +
        [("d2h", 0x2000, np.dtype(dtype), 9)] + ([("d2h", 0x3000, np.dtype(np.uint64), 2)] if blocked else []))
    assert isinstance(r, Records) and r[2:] == (4, 12, 3, 9)
    assert r.ends.dtype == dtype and np.array_equal(r.ends, np.arange(9) + 200)      # the second launch's data
    assert (np.array_equal(r.table, np.arange(2) + 200) and r.table.dtype == np.uint64) if blocked else r.table is None


def test_records_default_capacity_and_the_count_form(stub_ctx):
    ctx, stub = stub_ctx
    stub.results = [(_quote.DQ_OK, 3, 2, 5, 2), (_quote.DQ_OK, 3, 2, 5, 2)]
    r = ctx.records(*BUF)                                # plain uint64, cap (end - begin) // 16 + 1024
    cap = (600 - 110) // 16 + 1024
    assert stub.calls[:2] == [("workspace", "out", 8 * cap + 16),
                              ("dq_records_async", HANDLE) + BUF + (34, 0, 0x2000, 1, cap)]
    assert (r.n, r.n_quotes, r.n_newlines, r.toggles) == (3, 2, 5, 2) and len(r.ends) == 3 and r.table is None
    stub.calls.clear()
    r = ctx.records(*BUF, form="count", cap=99)          # one launch, no workspace, nothing read back
    assert stub.calls == [("dq_records_async", HANDLE) + BUF + (34, 0, None, 1, 0), ("dq_records_esc_result", HANDLE)]
    assert r == Records(None, None, 2, 5, 2, 3)


# ------------------------------------------------------------------------------------------------ load_guarded
SIGS = [("x_abi_version", ctypes.c_int, []), ("x_run", ctypes.c_int, [ctypes.c_void_p]),
        ("x_new", ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint64])]


class FakeLib:
    def __init__(self, version, names):
        for n in names:
            setattr(self, n, (lambda v=version: v) if n.endswith("_abi_version") else (lambda *a: 0))


@pytest.fixture
def fake_file(tmp_path, monkeypatch):
    """(path of a stamped file, set(version, names): what the fake ctypes.CDLL makes of it)."""
    path = tmp_path / "libx.so"
    path.write_bytes(b"not a library")
    (tmp_path / "libx.so.isa.json").write_text(json.dumps(
        {"result": "ok", "so_sha256": hashlib.sha256(b"not a library").hexdigest()}))
    made = {}

    def cdll(p):
        assert p == str(path)
        return FakeLib(made["version"], made["names"])

    def set_lib(version, names=tuple(n for n, _, _ in SIGS)):
        made.update(version=version, names=names)
    monkeypatch.setattr(_lib.ctypes, "CDLL", cdll)
    set_lib(2)
    return str(path), set_lib


def load_x(path, **kw):
    return _lib.load_guarded(path, SIGS, "x_abi_version", 2, **kw)


def test_load_guarded_refuses_what_it_cannot_vouch_for(fake_file, tmp_path):
    path, set_lib = fake_file
    with pytest.raises(_lib.DPScanUnavailable, match="not found"):
        load_x(str(tmp_path / "missing.so"), exact=True)
    bare = tmp_path / "bare.so"
    bare.write_bytes(b"not a library")
    with pytest.raises(_lib.DPScanUnavailable, match="no ISA-guard stamp"):
        load_x(str(bare), exact=True)
    (tmp_path / "bare.so.isa.json").write_text(json.dumps({"result": "ok", "so_sha256": "0" * 64}))
    with pytest.raises(_lib.DPScanUnavailable, match="not loaded"):
        load_x(str(bare), exact=True)
    set_lib(2, ("x_abi_version", "x_run"))
    with pytest.raises(_lib.DPScanUnavailable, match="does not export x_new: rebuild it"):
        load_x(path, exact=True)
    set_lib(2, ("x_run", "x_new"))
    for kw in (dict(exact=True), dict(exact=False, tolerate_missing=True)):
        with pytest.raises(_lib.DPScanUnavailable, match="does not export x_abi_version"):
            load_x(path, **kw)
    set_lib(2)
    lib = load_x(path, exact=True)
    assert lib.x_run.restype is ctypes.c_int and lib.x_run.argtypes == [ctypes.c_void_p]
    assert lib.x_new.argtypes == [ctypes.c_void_p, ctypes.c_uint64] and lib.x_abi_version() == 2


@pytest.mark.parametrize("version", [1, 2, 3])
def test_load_guarded_keeps_both_version_rules(fake_file, version):
    path, set_lib = fake_file
    set_lib(version)
    for exact, accepted in ((True, version == 2), (False, version >= 2)):
        if accepted:
            assert load_x(path, exact=exact).x_abi_version() == version
        else:
            with pytest.raises(_lib.DPScanUnavailable,
                               match=f"has ABI version {version}, this binding needs 2: rebuild it"):
                load_x(path, exact=exact)
    if version < 2:                                      # a library's note on what changed stands in the refusal
        with pytest.raises(_lib.DPScanUnavailable, match=r"needs 2 \(since x_new\): rebuild it"):
            load_x(path, exact=False, abi_note=" (since x_new)")
    # the leniency of an A/B against an older build: neither the version nor a missing entry point refuses
    set_lib(version, ("x_abi_version", "x_run"))
    lib = load_x(path, exact=False, tolerate_missing=True)
    assert lib.x_run.restype is ctypes.c_int and not hasattr(lib, "x_new")


def test_the_three_loaders_keep_their_own_rule(fake_file, monkeypatch):
    """dpscan: at least its version, and lenient under DPSCAN_LIB; dpquote and dpfai: exactly theirs."""
    path, set_lib = fake_file
    monkeypatch.delenv("DPSCAN_LIB", raising=False)
    monkeypatch.setattr(_lib, "LIB_PATH", path)
    scan_names = tuple(n for n, _, _ in _lib.SIGNATURES)
    for version, ok in ((_lib.ABI_VERSION - 1, False), (_lib.ABI_VERSION, True), (_lib.ABI_VERSION + 1, True)):
        monkeypatch.setattr(_lib, "_lib", None)
        set_lib(version, scan_names)
        if ok:
            assert _lib.load().dp_abi_version() == version and _lib.load() is _lib._lib       # cached
        else:
            with pytest.raises(_lib.DPScanUnavailable, match="dp_scan_delim_form's argument list changed in 2"):
                _lib.load()
    monkeypatch.setattr(_lib, "_lib", None)
    set_lib(_lib.ABI_VERSION, scan_names[:-1])
    with pytest.raises(_lib.DPScanUnavailable, match=f"does not export {scan_names[-1]}"):
        _lib.load()
    monkeypatch.setenv("DPSCAN_LIB", path)
    set_lib(_lib.ABI_VERSION - 1, scan_names[:-1])
    assert _lib.load().dp_abi_version() == _lib.ABI_VERSION - 1 and _lib._lib is not None
    for mod, prefix in ((_quote, "dq"), (_fai, "dfai")):
        names = tuple(n for n, _, _ in mod.SIGNATURES)
        monkeypatch.setattr(mod, "_lib", None)
        for version in (mod.ABI_VERSION - 1, mod.ABI_VERSION + 1):
            set_lib(version, names)
            with pytest.raises(_lib.DPScanUnavailable, match=f"this binding needs {mod.ABI_VERSION}: rebuild it"):
                mod.load(path)
        set_lib(mod.ABI_VERSION, names[:-1])
        with pytest.raises(_lib.DPScanUnavailable, match=f"does not export {names[-1]}"):
            mod.load(path)                               # no leniency here, DPSCAN_LIB or not
        set_lib(mod.ABI_VERSION, names)
        assert getattr(mod.load(path), prefix + "_abi_version")() == mod.ABI_VERSION
        assert mod._lib is None                          # a given path is not cached ...
        monkeypatch.setattr(mod, "LIB_PATH", path)
        assert mod.load() is mod.load() is mod._lib      # ... the library's own is
