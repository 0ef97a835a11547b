"""The producers' device calls without a GPU: the header declares the five new symbols, the built library exports them, hbmpc.py binds
them, rust/hbmpc_sys.rs lists them, a null context is refused before any device is touched, and the Python defaults of the
one-launch threshold are the library's."""
import ctypes as C
import os
import re

from __graft_entry__ import PKG_DIR, ROOT, load_package

SYMBOLS = ("hbmpc_dev_ransha_parties", "hbmpc_gl_dev_ransha_parties", "hbmpc_dev_randousha_parties", "hbmpc_gl_dev_randousha_parties",
           "hbmpc_set_fused_producers")


def test_header_declares_and_library_exports():
    pkg = load_package()
    header = open(os.path.join(ROOT, "include", "hbmpc_hip.h")).read()
    for sym in SYMBOLS:
        assert re.search(rf"^ShareErrorCode {sym}\(", header, re.M), sym
        assert hasattr(pkg.lib(), sym), sym                                      # dlsym resolves it in the built library


def test_python_binds_them():
    H = load_package().hbmpc
    assert callable(H.Engine.ransha_parties) and callable(H.Engine.randousha_parties) and callable(H.Engine.set_fused_producers)
    assert set(H.FUSED_PRODUCERS_DEFAULT) == {"fr", "goldilocks"}


def test_rust_binding_lists_them():
    sys_rs = open(os.path.join(ROOT, "rust", "hbmpc_sys.rs")).read()
    for sym in SYMBOLS:
        assert re.search(rf"\bpub fn {sym}\(", sys_rs), sym
    # 14 arguments: the context, 2 inputs, 4 sizes, 3 element buffers, the status bytes, the summary, the verdict and the stream
    args = re.search(r"pub fn hbmpc_dev_ransha_parties\((.*?)\) -> ShareErrorCode;", sys_rs).group(1)
    assert len(args.split(",")) == 14
    # 19: the context, 4 inputs, 3 sizes, 5 element buffers, 2 + 2 verifier results, the verdict and the stream
    args = re.search(r"pub fn hbmpc_gl_dev_randousha_parties\((.*?)\) -> ShareErrorCode;", sys_rs).group(1)
    assert len(args.split(",")) == 19


def test_null_context_is_invalid_input():
    """no context, so no device: InvalidInput (4) from the four device calls and the setter"""
    L = load_package().lib()
    ransha = [None] * 3 + [C.c_size_t(2), C.c_size_t(4), C.c_size_t(1), C.c_size_t(3)] + [None] * 7
    randousha = [None] * 5 + [C.c_size_t(2), C.c_size_t(4), C.c_size_t(1)] + [None] * 11
    assert L.hbmpc_dev_ransha_parties(*ransha) == 4
    assert L.hbmpc_gl_dev_ransha_parties(*ransha) == 4
    assert L.hbmpc_dev_randousha_parties(*randousha) == 4
    assert L.hbmpc_gl_dev_randousha_parties(*randousha) == 4
    assert L.hbmpc_set_fused_producers(None, C.c_size_t(16)) == 4


def test_python_defaults_match_the_library():
    """FUSED_PRODUCERS_DEFAULT (what tests put back after hbmpc_set_fused_producers) holds the contexts' initial values"""
    H = load_package().hbmpc
    src = open(os.path.join(PKG_DIR, "csrc", "hbmpc_capi.hip")).read()
    m = re.search(r"\bFUSED_PRODUCERS_FR\s*=\s*(\d+)\s*,\s*FUSED_PRODUCERS_GL\s*=\s*(\d+)\s*;", src)
    assert (int(m.group(1)), int(m.group(2))) == (H.FUSED_PRODUCERS_DEFAULT["fr"], H.FUSED_PRODUCERS_DEFAULT["goldilocks"])
