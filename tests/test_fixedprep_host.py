"""hbmpc_dev_take_rows and the FixedPrep handle without a GPU: the header declares the new symbols, the built library exports them,
hbmpc.py and pipelines.py bind them, rust/hbmpc_sys.rs lists them with the right argument counts, a null context is refused by every new
call and a refused create leaves the handle NULL, the take's argument checks (csrc/take_plan.hpp, the functions hbmpc_dev_take_rows
calls before it touches a device) refuse each invalid slice the header names, and the take model equals plain numpy indexing."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from __graft_entry__ import ROOT, load_package
from tests import fixedprep_ref as FR

SYMBOLS = ("hbmpc_dev_take_rows", "hbmpc_pipe_fixedprep_create", "hbmpc_pipe_fixedprep_take", "hbmpc_pipe_fixedprep_available")
# arguments of each: the context, the slices, 2 sizes, the stream | 2 contexts, 5 sizes, the stream, the handle | the handle, 2 sizes, 2
# destinations | the handle, the result
ARGS = dict(zip(SYMBOLS, (5, 9, 5, 2)))


def test_header_declares_and_library_exports():
    pkg = load_package()
    header = open(os.path.join(ROOT, "include", "hbmpc_hip.h")).read()
    for sym in SYMBOLS:
        assert re.search(rf"^ShareErrorCode {sym}\(", header, re.M), sym
        assert hasattr(pkg.lib(), sym), sym                                      # dlsym resolves it in the built library
    assert re.search(r"\}\s*hbmpc_take_slice;", header)


def test_python_binds_them():
    pkg = load_package()
    assert callable(pkg.hbmpc.Engine.take_rows)
    F = pkg.pipelines.FixedPrep
    assert all(callable(getattr(F, name)) for name in ("take", "take_raw", "available", "deal", "finish", "verdict", "sizes"))
    fields = [name for name, _ in pkg.hbmpc.TakeSlice._fields_]
    assert fields == ["src", "src_row_stride", "dst", "dst_row_stride", "elements", "group"] and C.sizeof(pkg.hbmpc.TakeSlice) == 48


def test_python_sizes_are_the_restatements():
    F = load_package().pipelines.FixedPrep
    for n, t in ((4, 1), (7, 2), (10, 3), (13, 4), (16, 5)):
        for nb in (1, 2, 5, 16, 20, 33, 1 << 16):
            assert F.sizes(n, t, nb) == FR.sizes(n, t, nb), (n, t, nb)


def test_rust_binding_lists_them():
    sys_rs = open(os.path.join(ROOT, "rust", "hbmpc_sys.rs")).read()
    for sym in SYMBOLS:
        args = re.search(rf"pub fn {sym}\((.*?)\) -> ShareErrorCode;", sys_rs, re.S).group(1)
        assert len(args.split(",")) == ARGS[sym], sym
    body = re.search(r"pub struct TakeSlice \{(.*?)\}", sys_rs, re.S).group(1)
    assert [f.split(":")[0].replace("pub", "").strip() for f in body.strip().rstrip(",").split(",")] == \
        ["src", "src_row_stride", "dst", "dst_row_stride", "elements", "group"]


def test_null_context_is_invalid_input():
    """no context, so no device: InvalidInput (4) from every new call -- non-null buffers, so the null-buffer check is not the one that
    answers; a refused create leaves the handle NULL"""
    pkg = load_package()
    L = pkg.lib()
    p, z = C.c_void_p(64), C.c_size_t
    sl = (pkg.hbmpc.TakeSlice * 1)(pkg.hbmpc.TakeSlice(64, 8, 1024, 8, 8, 2))
    assert L.hbmpc_dev_take_rows(None, sl, z(1), z(4), None) == 4
    for fr, gl in ((None, None), (None, p), (p, None)):  # a non-null context is not read before the null one is refused
        h = C.c_void_p(1234)
        assert L.hbmpc_pipe_fixedprep_create(fr, gl, z(4), z(1), z(4), z(3), z(40), None, C.byref(h)) == 4 and h.value is None, (fr, gl)
    assert L.hbmpc_pipe_fixedprep_create(None, None, z(4), z(1), z(4), z(3), z(40), None, None) == 4
    out = (C.c_size_t * 2)(7, 7)
    assert L.hbmpc_pipe_fixedprep_take(None, z(4), z(1), p, p) == 4
    assert L.hbmpc_pipe_fixedprep_available(None, out) == 4 and list(out) == [7, 7]


def test_take_refuses_each_invalid_slice_before_a_device():
    """the checks hbmpc_dev_take_rows applies (csrc/take_plan.hpp), compiled for the CPU: the call's, then the slice's, in the header's
    order -- query: has_slices count rows src src_stride dst dst_stride elements group"""
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "cpp"), "-f", "take.mk"], stdout=subprocess.DEVNULL)
    good = (1, 2, 4, 64, 24, 1024, 24, 24, 4)
    cases = [(good, "ok"), ((1, 8, 65535, 8, 24, 16, 1 << 40, 24, 24), "ok"),
             ((0,) + good[1:], "1 to 8 slices"), ((1, 0) + good[2:], "1 to 8 slices"), ((1, 9) + good[2:], "1 to 8 slices"),
             ((1, 2, 0) + good[3:], "1 to 65535 rows"), ((1, 2, 65536) + good[3:], "1 to 65535 rows"),
             (good[:3] + (0,) + good[4:], "null or misaligned"), (good[:5] + (0,) + good[6:], "null or misaligned"),
             (good[:3] + (68,) + good[4:], "null or misaligned"), (good[:5] + (1028,) + good[6:], "null or misaligned"),
             (good[:7] + (0, 4), "positive multiple"), (good[:7] + (24, 0), "positive multiple"), (good[:7] + (24, 5), "positive multiple"),
             (good[:4] + (23,) + good[5:], "row stride below"), (good[:6] + (23,) + good[7:], "row stride below"),
             ((1, 1, 1, 64, 1 << 32, 1024, 1 << 32, (1 << 31) + 2, 2), "beyond"), ((1, 1, 1, 64, (1 << 40) + 1, 1024, 24, 24, 4), "beyond"),
             # the order: the call before the slice, the pointers before the sizes, the sizes before the strides
             ((1, 9, 0, 0, 1, 0, 1, 0, 0), "1 to 8 slices"), ((1, 1, 0, 0, 1, 0, 1, 0, 0), "1 to 65535 rows"),
             ((1, 1, 1, 0, 1, 64, 1, 5, 0), "null or misaligned"), ((1, 1, 1, 64, 1, 64, 1, 5, 2), "positive multiple")]
    text = "".join(" ".join(map(str, q)) + "\n" for q, _ in cases)
    p = subprocess.run([os.path.join(ROOT, "tests", "cpp", "take_routes_dump"), "check"], input=text, capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = p.stdout.splitlines()
    assert len(lines) == len(cases)
    for (q, want), line in zip(cases, lines):
        assert (line == "ok") if want == "ok" else (line.startswith("refused: ") and want in line), (q, line)
    src = open(os.path.join(ROOT, "mpc-protocols_amd", "csrc", "hbmpc_capi.hip")).read()
    body = src[src.index('ShareErrorCode hbmpc_dev_take_rows('):]
    body = body[:body.index("\n}\n")]
    # the entry point applies exactly these, and before the first call that touches the device
    assert body.index("check_take_call(") < body.index("check_take_slice(") < body.index("hipSetDevice") < body.index("launch_take_rows(")


def test_the_take_model_equals_plain_numpy_indexing():
    rng = np.random.default_rng(5)
    for tail in ((), (4,)):
        for rows, elements, group, spad, dpad in ((1, 1, 1, 0, 0), (3, 24, 4, 5, 2), (2, 35, 5, 0, 3), (4, 16, 16, 1, 0), (2, 12, 1, 2, 2)):
            srs, drs, Cn = elements + spad, elements + dpad, elements // group
            src = rng.integers(0, 1 << 64, size=(rows * srs,) + tail, dtype=np.uint64)
            a = FR.take_rows(src, rows, srs, np.zeros((rows * drs,) + tail, dtype=np.uint64), drs, elements, group)
            b = FR.take_rows_np(src, rows, srs, np.zeros((rows * drs,) + tail, dtype=np.uint64), drs, elements, group)
            want = np.zeros((rows, drs) + tail, dtype=np.uint64)
            want[:, :elements] = src.reshape((rows, srs) + tail)[:, :elements].reshape((rows, Cn, group) + tail).swapaxes(1, 2).reshape(
                (rows, elements) + tail)
            assert np.array_equal(a, want.reshape(a.shape)) and np.array_equal(b, a), (tail, rows, elements, group)
