"""The integer-point Shamir calls without a GPU: the header declares them, the built library exports them, hbmpc.py binds them,
rust/hbmpc_sys.rs lists them with the right argument counts, and a null context is refused by every new call before any device is
touched."""
import ctypes as C
import os
import re

from __graft_entry__ import ROOT, load_package

# name without the field prefix -> number of arguments (the context first)
CALLS = {"shamir_compute_shares": 7, "dev_shamir_compute_shares": 8, "shamir_recover_secret": 8, "shamir_batch_interpolate": 7,
         "dev_shamir_batch_interpolate": 9, "dev_shamir_batch_interpolate_c0": 10}
SYMBOLS = {pfx + name: n for name, n in CALLS.items() for pfx in ("hbmpc_", "hbmpc_gl_")}
SYMBOLS.update({"hbmpc_set_shamir_route": 2, "hbmpc_shamir_route": 6})


def test_header_declares_and_library_exports():
    pkg = load_package()
    header = open(os.path.join(ROOT, "include", "hbmpc_hip.h")).read()
    for sym, nargs in SYMBOLS.items():
        m = re.search(rf"^ShareErrorCode {sym}\((.*?)\);", header, re.M | re.S)
        assert m, sym
        assert len(m.group(1).split(",")) == nargs, sym
        assert hasattr(pkg.lib(), sym), sym                   # dlsym resolves it in the built library
    # the contract notes the issue asks for
    assert "There is no seeded entry" in header and "hbmpc_[gl_]dev_fill_coeffs followed by" in header
    assert "result_poly[0]" in header[header.index("==== Shamirshare"):header.index("ShareErrorCode hbmpc_shamir_recover_secret(")]
    for sym in SYMBOLS:
        if "compute_shares" in sym or "interpolate" in sym:
            assert re.search(rf"{sym}\(hbmpc_ctx\* ctx, [^;]*const uint64_t\* points", header), sym   # points are u64 ids, not size_t domain indices


def test_python_binds_them():
    E = load_package().hbmpc.Engine
    for name in list(CALLS) + ["set_shamir_route", "shamir_route"]:
        assert callable(getattr(E, name)), name


def test_rust_binding_lists_them():
    sys_rs = open(os.path.join(ROOT, "rust", "hbmpc_sys.rs")).read()
    for sym, nargs in SYMBOLS.items():
        m = re.search(rf"pub fn {sym}\((.*?)\) -> ShareErrorCode;", sys_rs, re.S)
        assert m, sym
        assert len(m.group(1).split(",")) == nargs, sym


def test_null_context_is_invalid_input():
    """no context, so no device: InvalidInput (4) from every new call -- with non-null buffers and valid points, so no other check is
    the one that answers"""
    L = load_package().lib()
    p, z = C.c_void_p(64), C.c_size_t
    pts = (C.c_uint64 * 3)(1, 2, 3)
    degs = (C.c_size_t * 3)(2, 2, 2)
    n = C.c_size_t(0)
    k = C.c_int(0)
    for pfx in ("hbmpc_", "hbmpc_gl_"):
        f = lambda name: getattr(L, pfx + name)
        assert f("shamir_compute_shares")(None, p, z(4), pts, z(3), z(2), p) == 4
        assert f("dev_shamir_compute_shares")(None, p, z(4), pts, z(3), z(2), p, None) == 4
        assert f("shamir_recover_secret")(None, pts, degs, p, z(3), p, C.byref(n), p) == 4
        assert f("shamir_batch_interpolate")(None, pts, z(3), p, z(4), p, p) == 4
        assert f("dev_shamir_batch_interpolate")(None, pts, z(3), p, z(4), z(4), p, p, None) == 4
        assert f("dev_shamir_batch_interpolate_c0")(None, pts, z(3), p, z(4), z(4), p, p, p, None) == 4
    assert L.hbmpc_set_shamir_route(None, C.c_int(1)) == 4
    assert L.hbmpc_shamir_route(None, pts, z(3), z(2), z(4), C.byref(k)) == 4


def test_entry_points_check_before_touching_the_device():
    """every entry of capi_shamir.inc refuses a null context in its first statement, and validates the points before hipSetDevice"""
    src = open(os.path.join(ROOT, "mpc-protocols_amd", "csrc", "capi_shamir.inc")).read()
    for fn, check in (("shamir_encode_dev", "shamir_check_encode("), ("shamir_encode_host", "shamir_check_encode("),
                      ("shamir_interpolate_host", "shamir_check_points("), ("shamir_recover_any", "shamir_has_duplicates(")):
        body = src[src.index("ShareErrorCode " + fn + "("):]
        body = body[:body.index("\n}\n")]
        first = body[body.index("{") + 1:].strip().splitlines()[0].strip()
        assert first == "if (!ctx) return InvalidInput;", fn
        assert body.index(check) < body.index("hipSetDevice"), fn
    body = src[src.index("ShareErrorCode shamir_interpolate_dev("):]
    body = body[:body.index("\n}\n")]
    assert body.index("if (!ctx) return InvalidInput;") < body.index("shamir_check_points(") < body.index("batch_interpolate_dev(")
