"""The Input / Output entry points without a GPU: the built library exports them, the header declares them, the Python wrappers
exist, a null context is refused before any device is touched, and the Python default of the one-launch threshold is the library's."""
import ctypes as C
import os
import re

from __graft_entry__ import PKG_DIR, ROOT, load_package

SYMBOLS = ("hbmpc_dev_input_parties", "hbmpc_gl_dev_input_parties", "hbmpc_dev_output_parties", "hbmpc_gl_dev_output_parties",
           "hbmpc_set_fused_input", "hbmpc_pipe_input_create", "hbmpc_pipe_output_create")


def test_library_exports_and_header_declares():
    pkg = load_package()
    header = open(os.path.join(ROOT, "include", "hbmpc_hip.h")).read()
    for sym in SYMBOLS:
        assert re.search(rf"^ShareErrorCode {sym}\(", header, re.M), sym
        assert hasattr(pkg.lib(), sym), sym                                      # dlsym resolves it in the built library


def test_wrappers_exist():
    pkg = load_package()
    pl = pkg.pipelines
    for cls in (pl.Input, pl.Output):
        assert issubclass(cls, pl._Pipe)
        for name in ("upload", "download"):
            assert callable(getattr(cls, name))
    for name in ("input_parties", "output_parties", "set_fused_input"):
        assert callable(getattr(pkg.Engine, name))
    cpp = open(os.path.join(ROOT, "include", "hbmpc_pipelines.hpp")).read()
    assert "class Input : public Pipeline" in cpp and "class Output : public Pipeline" in cpp
    rust = open(os.path.join(ROOT, "rust", "gpu_shares.rs")).read()
    assert "pub fn pipe_input(" in rust and "pub fn pipe_output(" in rust


def test_null_context_is_invalid_input():
    """no context, so no device: InvalidInput (4) from the four device calls, the setter and the two handles' create -- with non-null
    buffers, so the null-buffer check is not the one that answers"""
    L = load_package().lib()
    p, z = C.c_void_p(64), C.c_size_t
    inp = [None, p, z(3), p, p, z(5), z(4), z(1), p, p, p, p, None, None]
    assert L.hbmpc_dev_input_parties(*inp) == 4
    assert L.hbmpc_gl_dev_input_parties(*inp) == 4
    out = [None, p, z(3), p, z(5), z(4), z(1), p, p, None, None]
    assert L.hbmpc_dev_output_parties(*out) == 4
    assert L.hbmpc_gl_dev_output_parties(*out) == 4
    assert L.hbmpc_set_fused_input(None, z(16)) == 4
    for fn in (L.hbmpc_pipe_input_create, L.hbmpc_pipe_output_create):
        h = C.c_void_p()
        assert fn(None, z(4), z(1), z(5), z(0), None, C.byref(h)) == 4 and not h.value


def test_python_default_matches_the_library():
    """FUSED_INPUT_DEFAULT (what tests put back after hbmpc_set_fused_input) is the context's initial value"""
    H = load_package().hbmpc
    src = open(os.path.join(PKG_DIR, "csrc", "hbmpc_capi.hip")).read()
    assert int(re.search(r"\bfused_input_max\s*=\s*(\d+)\s*;", src).group(1)) == H.FUSED_INPUT_DEFAULT
