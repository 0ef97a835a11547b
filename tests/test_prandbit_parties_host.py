"""The PRandBit / PRandInt device calls and handles without a GPU: the header declares the five new symbols, the built library exports
them, hbmpc.py binds the calls, rust/hbmpc_sys.rs lists them, a null context is refused before any device is touched, and the Python
default of the one-launch threshold is the library's."""
import ctypes as C
import os
import re

from __graft_entry__ import PKG_DIR, ROOT, load_package

SYMBOLS = ("hbmpc_dev_prandbit_parties", "hbmpc_dev_prandint_parties", "hbmpc_set_fused_prandbit", "hbmpc_pipe_prandbit_create",
           "hbmpc_pipe_prandint_create")
# arguments of each: 2 contexts, 2 inputs, 5 sizes, 12 buffers, 2 summaries, the stream | the context, the input, 4 sizes, 3 buffers, the
# stream | context, value | 2 contexts, 5 sizes, the stream, the handle | the context, 4 sizes, the stream, the handle
ARGS = dict(zip(SYMBOLS, (24, 10, 2, 9, 7)))


def test_header_declares_and_library_exports():
    pkg = load_package()
    header = open(os.path.join(ROOT, "include", "hbmpc_hip.h")).read()
    for sym in SYMBOLS:
        assert re.search(rf"^ShareErrorCode {sym}\(", header, re.M), sym
        assert hasattr(pkg.lib(), sym), sym                                      # dlsym resolves it in the built library


def test_python_binds_them():
    pkg = load_package()
    H = pkg.hbmpc
    assert callable(H.Engine.prandbit_parties) and callable(H.Engine.prandint_parties) and callable(H.Engine.set_fused_prandbit)
    assert callable(pkg.pipelines.PRandBitPipe) and callable(pkg.pipelines.PRandIntPipe)


def test_rust_binding_lists_them():
    sys_rs = open(os.path.join(ROOT, "rust", "hbmpc_sys.rs")).read()
    for sym in SYMBOLS:
        assert re.search(rf"\bpub fn {sym}\(", sys_rs), sym
        args = re.search(rf"pub fn {sym}\((.*?)\) -> ShareErrorCode;", sys_rs, re.S).group(1)
        assert len(args.split(",")) == ARGS[sym], sym


def test_null_context_is_invalid_input():
    """no context, so no device: InvalidInput (4) from both device calls, the setter and both handle constructors -- non-null buffers,
    so the null-buffer check is not the one that answers; a refused constructor leaves the handle NULL"""
    L = load_package().lib()
    p, z = C.c_void_p(64), C.c_size_t
    bit = [None, None, p, p, z(4), z(1), z(2), z(40), z(0)] + [p] * 14 + [None]
    assert L.hbmpc_dev_prandbit_parties(*bit) == 4
    assert L.hbmpc_dev_prandint_parties(None, p, z(4), z(1), z(2), z(40), p, p, p, None) == 4
    assert L.hbmpc_set_fused_prandbit(None, z(16)) == 4
    for fr, gl in ((None, None), (None, p), (p, None)):  # a non-null context is not read before the null one is refused
        h = C.c_void_p(1234)
        assert L.hbmpc_pipe_prandbit_create(fr, gl, z(4), z(1), z(2), z(40), z(0), None, C.byref(h)) == 4 and h.value is None, (fr, gl)
    h = C.c_void_p(1234)
    assert L.hbmpc_pipe_prandint_create(None, z(4), z(1), z(2), z(40), None, C.byref(h)) == 4 and h.value is None
    assert L.hbmpc_pipe_prandbit_create(None, None, z(4), z(1), z(2), z(40), z(0), None, None) == 4


def test_the_gpu_tests_model_is_the_restatement():
    """tests/test_gpu_prandbit_parties.py compares the device's bytes with its own model (which also covers tampered shares); on honest
    inputs that model must be tests/prandbit_ref.py's PR.prandbit -- checked here without a GPU, at the shapes and chunk counts whose
    restatement is quick"""
    import tests.test_gpu_prandbit_parties as G
    for n, t, chunks in ((4, 1, 1), (5, 1, 3), (7, 2, 3), (10, 3, 1), (12, 3, 1)):
        contrib, bits, b_q, lk, m = G.honest(n, t, chunks)
        G.equals_restatement(n, t, contrib, b_q, lk, m)
        assert G.PR.recovered_bits(n, t, m) == (bits, bits)


def test_python_default_matches_the_library():
    """FUSED_PRANDBIT_DEFAULT (what tests put back after hbmpc_set_fused_prandbit) holds the contexts' initial value"""
    H = load_package().hbmpc
    src = open(os.path.join(PKG_DIR, "csrc", "hbmpc_capi.hip")).read()
    m = re.search(r"\bFUSED_PRANDBIT\s*=\s*(\d+)\s*;", src)
    assert int(m.group(1)) == H.FUSED_PRANDBIT_DEFAULT
