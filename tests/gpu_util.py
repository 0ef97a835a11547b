"""Helpers of the GPU edge tests that need nothing but an engine: the planners' knob strings applied to a context, and device buffers
filled from and read back into numpy arrays.  (tests/test_gpu_mfma_edges.py keeps its own, older copies.)"""
import numpy as np


def configure(eng, knobs):
    """the knob strings of the planners' dump tools (tests/cpp/encode_routes_dump.cpp) applied to a context"""
    mode, mn = 1, 0
    eng.set_small_batch_chunks(8192)
    eng.set_matrix_core_workgroups(0)
    for tok in knobs.split(","):
        if tok.startswith("mc"):
            mode = int(tok[2:])
        elif tok.startswith("min"):
            mn = int(tok[3:])
        elif tok == "small0":
            eng.set_small_batch_chunks(0)
        elif tok == "wgs8":
            eng.set_matrix_core_workgroups(8)
        else:
            assert tok == "default", tok
    eng.set_matrix_cores(mode, mn if mn else 65536)      # 65 536: every threshold back at its default (each is capped there)


def dev_buf(eng, arr):
    p = eng.dev_alloc(max(arr.nbytes, 16))
    eng.h2d(p, np.ascontiguousarray(arr))
    return p


def fetch(eng, ptr, shape, dtype=np.uint64):
    out = np.zeros(shape, dtype=dtype)
    eng.d2h(out, ptr)
    return out
