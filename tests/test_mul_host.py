"""The Mul entry points without a GPU: the built library exports them, the header declares them, the Python wrapper exists, a null
context is refused before any device is touched, and the Python default of the one-launch threshold is the library's."""
import ctypes as C
import os
import re

from __graft_entry__ import PKG_DIR, ROOT, load_package

SYMBOLS = ("hbmpc_dev_mul_parties", "hbmpc_gl_dev_mul_parties", "hbmpc_set_fused_mul", "hbmpc_pipe_mul_create")


def test_library_exports_and_header_declares():
    pkg = load_package()
    header = open(os.path.join(ROOT, "include", "hbmpc_hip.h")).read()
    for sym in SYMBOLS:
        assert re.search(rf"^ShareErrorCode {sym}\(", header, re.M), sym
        assert hasattr(pkg.lib(), sym), sym                                      # dlsym resolves it in the built library


def test_pipeline_wrapper_exists():
    pl = load_package().pipelines
    assert issubclass(pl.Mul, pl._Pipe)
    for name in ("upload", "download"):
        assert callable(getattr(pl.Mul, name))


def test_null_context_is_invalid_input():
    """no context, so no device: InvalidInput (4) from both device calls, the setter and the pipeline's create"""
    L = load_package().lib()
    z = C.c_size_t(0)
    args = [None, None, z] + [None] * 5 + [C.c_size_t(5), C.c_size_t(4), C.c_size_t(1)] + [None] * 6
    assert L.hbmpc_dev_mul_parties(*args) == 4
    assert L.hbmpc_gl_dev_mul_parties(*args) == 4
    assert L.hbmpc_set_fused_mul(None, C.c_size_t(16)) == 4
    h = C.c_void_p()
    assert L.hbmpc_pipe_mul_create(None, C.c_size_t(4), C.c_size_t(1), C.c_size_t(5), z, None, C.byref(h)) == 4 and not h.value


def test_python_default_matches_the_library():
    """FUSED_MUL_DEFAULT (what tests put back after hbmpc_set_fused_mul) is the context's initial value"""
    H = load_package().hbmpc
    src = open(os.path.join(PKG_DIR, "csrc", "hbmpc_capi.hip")).read()
    assert int(re.search(r"\bfused_mul_max\s*=\s*(\d+)\s*;", src).group(1)) == H.FUSED_MUL_DEFAULT
