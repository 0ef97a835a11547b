"""hbmpc_fixed_point_reciprocal_scaled (host arithmetic, no GPU) against a big-int restatement of the reference's
fixed_point_reciprocal_scaled (fpdiv/mod.rs:8-60): the low 16 bytes of the canonical denominator as a u128 b,
w = (2^(2f) + (b >> 1)) / b in u128, written into the two low limbs of an Fr element."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from __graft_entry__ import PKG_DIR, load_package
from oracle import cref as O
from oracle import spec as S

R = S.R_MOD
M128 = (1 << 128) - 1


def ref_reciprocal(values, f):
    """fpdiv/mod.rs:8-60 on canonical integers: (w per value, or the index of the first InvalidDivisor)"""
    assert 2 * f < 128, "1u128 << (2 f) overflows"
    out = []
    for i, v in enumerate(values):
        b = v & M128                       # :23-30 the lowest 16 bytes of into_bigint().to_bytes_le()
        if v == 0 or b == 0:               # :18-20, :32-34
            return None, i
        w = ((1 << (2 * f)) + (b >> 1)) // b
        assert w <= M128                   # u128 arithmetic never wrapped
        out.append(w)
    return out, None


@pytest.fixture(scope="module")
def H():
    return load_package().hbmpc


@pytest.mark.parametrize("f", [0, 4, 16, 63])
def test_reciprocal_matches_the_reference_formula(H, f):
    rng = np.random.default_rng(0xD1 + f)
    vals = [i << f for i in range(1, 6)]                                                # the bench's divisors i << f
    vals += [1, 2, 3, (1 << f) + 1, M128, (1 << 127), (1 << 127) + 1, 1 << 64, (1 << 64) - 1]
    vals += [int.from_bytes(rng.bytes(16), "little") | 1 for _ in range(40)]           # random 128-bit values
    vals += [v for v in O.u256_to_ints(O.fill_random(77 + f, 40)) if v & M128]          # full-width canonical values: the low two limbs count
    vals += [R - b for b in (1, 2, 5, 1 << f, (3 << f) + 1, 1 << 100)]                  # negative encodings r - b
    vals += [(5 << 128) + 7, (1 << 200) + (1 << 127)]                                   # high limbs are ignored
    assert all(0 < v < R for v in vals)
    want, bad = ref_reciprocal(vals, f)
    assert bad is None
    rc, w, first_bad = H.fixed_point_reciprocal_scaled(O.ints_to_u256(vals), f)
    assert rc == 0 and first_bad is None
    assert O.u256_to_ints(w) == want
    assert not w[:, 2:].any()                                                           # only the two low limbs are written


def test_bench_divisors_f4(H):
    """benches/hmpc_fpdiv_const_bench.rs: denominators i << f, f = 4 -> round(2^f / i) as a fixed-point value"""
    rc, w, _ = H.fixed_point_reciprocal_scaled(O.ints_to_u256([i << 4 for i in range(1, 6)]), 4)
    assert rc == 0 and O.u256_to_ints(w) == [16, 8, 5, 4, 3]


def test_reciprocal_rejections(H):
    L = load_package().lib()
    good = O.ints_to_u256([3, 5, 7, 9])
    marker = O.fill_random(5, 4)

    def call(denom, f, n=4):
        w, bad = marker.copy(), C.c_size_t(12345)
        rc = L.hbmpc_fixed_point_reciprocal_scaled(None if denom is None else denom.ctypes.data_as(C.c_void_p), C.c_size_t(n), C.c_size_t(f),
                                                   w.ctypes.data_as(C.c_void_p), C.byref(bad))
        assert rc == 0 or np.array_equal(w, marker), "nothing is written on error"
        return rc, bad.value

    none = C.c_size_t(-1).value
    assert call(good, 4) == (0, none)
    assert call(good, 64) == (4, none) and call(good, 100) == (4, none)               # 2f >= 128
    assert call(good, 63)[0] == 0
    assert call(O.ints_to_u256([3, 5, 0, 0]), 4) == (4, 2)                             # zero: the first one's index
    assert call(O.ints_to_u256([3, 1 << 128, 7, 0]), 4) == (4, 1)                      # nonzero, low 128 bits zero
    assert call(O.ints_to_u256([R - 1, 3 << 192, 7, 9]), 4) == (4, 1)
    assert call(None, 4) == (4, none)                                                  # null input
    assert L.hbmpc_fixed_point_reciprocal_scaled(good.ctypes.data_as(C.c_void_p), C.c_size_t(4), C.c_size_t(4), None, None) == 4  # null output
    assert L.hbmpc_fixed_point_reciprocal_scaled(good.ctypes.data_as(C.c_void_p), C.c_size_t(4), C.c_size_t(4),
                                                 marker.copy().ctypes.data_as(C.c_void_p), None) == 0          # first_bad_out may be null
    assert L.hbmpc_fixed_point_reciprocal_scaled(None, C.c_size_t(0), C.c_size_t(4), None, None) == 0            # nothing to do


def test_python_default_matches_the_library(H):
    """FUSED_TRUNCPR_DEFAULT (what tests put back after hbmpc_set_fused_truncpr) is the context's initial value"""
    src = open(os.path.join(PKG_DIR, "csrc", "hbmpc_capi.hip")).read()
    assert int(re.search(r"\bfused_truncpr_max\s*=\s*(\d+)\s*;", src).group(1)) == H.FUSED_TRUNCPR_DEFAULT
