"""The RandBit device call without a GPU: the header declares the three new symbols, the built library exports them, hbmpc.py binds
them, rust/hbmpc_sys.rs lists them, a null context is refused before any device is touched, and the Python defaults of the
one-launch threshold are the library's."""
import ctypes as C
import os
import re

from __graft_entry__ import PKG_DIR, ROOT, load_package

SYMBOLS = ("hbmpc_dev_randbit_parties", "hbmpc_gl_dev_randbit_parties", "hbmpc_set_fused_randbit")


def test_header_declares_and_library_exports():
    pkg = load_package()
    header = open(os.path.join(ROOT, "include", "hbmpc_hip.h")).read()
    for sym in SYMBOLS:
        assert re.search(rf"^ShareErrorCode {sym}\(", header, re.M), sym
        assert hasattr(pkg.lib(), sym), sym                                      # dlsym resolves it in the built library


def test_python_binds_them():
    H = load_package().hbmpc
    assert callable(H.Engine.randbit_parties) and callable(H.Engine.set_fused_randbit)
    assert set(H.FUSED_RANDBIT_DEFAULT) == {"fr", "goldilocks"}


def test_rust_binding_lists_them():
    sys_rs = open(os.path.join(ROOT, "rust", "hbmpc_sys.rs")).read()
    for sym in SYMBOLS:
        assert re.search(rf"\bpub fn {sym}\(", sys_rs), sym
    # 24 arguments: 4 inputs, 3 sizes, 7 element buffers, 3 status buffers, 5 summaries, the context and the stream
    args = re.search(r"pub fn hbmpc_dev_randbit_parties\((.*?)\) -> ShareErrorCode;", sys_rs).group(1)
    assert len(args.split(",")) == 24


def test_null_context_is_invalid_input():
    """no context, so no device: InvalidInput (4) from both device calls and the setter"""
    L = load_package().lib()
    args = [None] * 5 + [C.c_size_t(4), C.c_size_t(4), C.c_size_t(1)] + [None] * 16
    assert L.hbmpc_dev_randbit_parties(*args) == 4
    assert L.hbmpc_gl_dev_randbit_parties(*args) == 4
    assert L.hbmpc_set_fused_randbit(None, C.c_size_t(16)) == 4


def test_python_defaults_match_the_library():
    """FUSED_RANDBIT_DEFAULT (what tests put back after hbmpc_set_fused_randbit) holds the contexts' initial values"""
    H = load_package().hbmpc
    src = open(os.path.join(PKG_DIR, "csrc", "hbmpc_capi.hip")).read()
    m = re.search(r"\bFUSED_RANDBIT_FR\s*=\s*(\d+)\s*,\s*FUSED_RANDBIT_GL\s*=\s*(\d+)\s*;", src)
    assert (int(m.group(1)), int(m.group(2))) == (H.FUSED_RANDBIT_DEFAULT["fr"], H.FUSED_RANDBIT_DEFAULT["goldilocks"])
