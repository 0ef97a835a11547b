"""RandBit restated (fpmul/rand_bit.rs:242-293, 197-220) for the tests: ark-ff 0.5's Field::sqrt and Field::inverse, phase 2 with its
error precedence, and the whole pipeline (Beaver square -> BatchRecon -> phase 2) over both fields.

The ark-ff crate is not part of this repository; sqrt is restated line by line from its fields/sqrt.rs (TonelliShanks arm), so which
of the two roots it picks is as unpinned as the rest of the oracle.  closed_sqrt is the branch-free form the
device kernels compute (csrc/kernels_sqrt.hpp); test_randbit_ref.py checks the two against each other."""
from __future__ import annotations

import numpy as np

from oracle import cref as O
from oracle import cref_gl as OG
from oracle import spec as S

P_FR = S.R_MOD
P_GL = 2**64 - 2**32 + 1
PRIME = {"fr": P_FR, "goldilocks": P_GL}
TWO_ADICITY = 32
ZERO_SQUARE, NO_SQUARE_ROOT = 102, 103  # HBMPC_ZERO_SQUARE, HBMPC_NO_SQUARE_ROOT
ST_OK, ST_ZERO, ST_NO_ROOT = 0, 1, 2


def trace(p):
    return (p - 1) >> TWO_ADICITY


def omega(p):
    """TWO_ADIC_ROOT_OF_UNITY = 7^T (spec.TWO_ADIC_ROOT for Fr)"""
    return pow(7, trace(p), p)


def ark_sqrt(a, p):
    """ark-ff 0.5 Field::sqrt, SqrtPrecomputation::TonelliShanks: None when a is not a square"""
    if a == 0:
        return 0
    z = omega(p)                               # quadratic_nonresidue_to_trace
    w = pow(a, (trace(p) - 1) // 2, p)         # trace_of_modulus_minus_one_div_two
    x = w * a % p
    b = x * w % p
    v = TWO_ADICITY
    while b != 1:
        k, b2k = 0, b
        while b2k != 1:
            b2k = b2k * b2k % p
            k += 1
        if k == TWO_ADICITY:
            return None
        j = v - k
        w = z
        for _ in range(1, j):
            w = w * w % p
        z = w * w % p
        b = b * z % p
        x = x * w % p
        v = k
    return x if x * x % p == a else None


def dlog_omega(g, p):
    """L in [0, 2^32) with omega^L = g (g in the 2^32-element subgroup), bit by bit"""
    om = omega(p)
    om_inv = pow(om, p - 2, p)
    L = 0
    for i in range(TWO_ADICITY):
        h = g * pow(om_inv, L, p) % p
        if pow(h, 1 << (TWO_ADICITY - 1 - i), p) != 1:
            L |= 1 << i
    return L


def closed_sqrt(a, p):
    """u = a^((T-1)/2), a^T = u^2 a = omega^L: a square iff L is even, and then ark's root is a u omega^E, E = (-L/2) mod 2^31"""
    if a == 0:
        return 0
    u = pow(a, (trace(p) - 1) // 2, p)
    L = dlog_omega(u * u * a % p, p)
    if L & 1:
        return None
    E = (-(L >> 1)) % (1 << 31)
    return a * u * pow(omega(p), E, p) % p


def ark_inverse(a, p):
    return None if a == 0 else pow(a, p - 2, p)


def phase2(sq, a_shares, p):
    """rand_bit.rs:197-220.  sq: the opened squares [N]; a_shares: [parties][N].  -> (error, first index, status [N], out [parties][N]):
    ZeroSquare if any square is zero (whatever comes before it), else SquareRoot at the first square without a root; a failed
    element's shares are 0 (what the device writes)."""
    inv2 = pow(2, p - 2, p)
    status, binv = [], []
    for A in sq:
        if A == 0:
            status.append(ST_ZERO)
            binv.append(None)
            continue
        b = ark_sqrt(A, p)
        status.append(ST_OK if b is not None else ST_NO_ROOT)
        binv.append(None if b is None else ark_inverse(b, p))
    err, first = 0, None
    if ST_ZERO in status:
        err, first = ZERO_SQUARE, status.index(ST_ZERO)
    elif ST_NO_ROOT in status:
        err, first = NO_SQUARE_ROOT, status.index(ST_NO_ROOT)
    out = [[0 if bi is None else (a * bi % p + 1) * inv2 % p for a, bi in zip(row, binv)] for row in a_shares]
    return err, first, status, out


# ---- element arrays <-> python ints -------------------------------------------------------------------------------------
def to_ints(arr, field):
    arr = np.asarray(arr, dtype=np.uint64)
    if field == "goldilocks":
        return [int(x) for x in arr.reshape(-1)]
    f = arr.reshape(-1, 4)
    return [int(r[0]) | (int(r[1]) << 64) | (int(r[2]) << 128) | (int(r[3]) << 192) for r in f]


def from_ints(vals, field):
    if field == "goldilocks":
        return np.array([int(v) for v in vals], dtype=np.uint64)
    out = np.zeros((len(vals), 4), dtype=np.uint64)
    for i, v in enumerate(vals):
        for k in range(4):
            out[i, k] = (v >> (64 * k)) & 0xFFFFFFFFFFFFFFFF
    return out


def fill_random(field, seed, count):
    return O.fill_random(seed, count) if field == "fr" else OG.fill_random(seed, count)


def share_all(field, secrets, n, d, seed):
    """[n][N] degree-d sharings of N secrets (random higher coefficients), by the C oracle"""
    N = secrets.shape[0]
    if field == "fr":
        co = O.fill_random(seed, N * (d + 1)).reshape(N, d + 1, 4)
        co[:, 0] = secrets
        rc, sh = O.compute_shares(co, n, d)
    else:
        co = OG.fill_random(seed, N * (d + 1)).reshape(N, d + 1)
        co[:, 0] = secrets
        rc, sh = OG.compute_shares(co, n, d)
    assert rc == 0
    return sh


def product(field, x, y):
    if field == "fr":
        return O.fr_binop("mul", x, y)
    return np.array([(int(a) * int(b)) % P_GL for a, b in zip(x, y)], dtype=np.uint64)


def pipeline_inputs(field, n, t, N, seed):
    """secrets a, ta, tb (random) and tc = ta tb, shared with degree t: dict of [n][N] arrays plus the secrets"""
    a, ta, tb = (fill_random(field, seed + k, N) for k in range(3))
    tc = product(field, ta, tb)
    sec = {"a": a, "ta": ta, "tb": tb, "tc": tc}
    sh = {k: share_all(field, v, n, t, seed + 10 + i) for i, (k, v) in enumerate(sec.items())}
    return sec, sh


def pipeline_columns(field, sec, sh, cols):
    """the restated pipeline at columns `cols` (honest shares): Multiply's opened d = ta - a, e = tb - a (multiplication.rs:417-426),
    finalize_mul's [a^2] (:57-100), the opened squares, phase 2 -> (sq [n][len(cols)], sqop [len(cols)], phase-2 result)"""
    p = PRIME[field]
    n = sh["a"].shape[0]
    col = lambda arr: to_ints(arr[cols], field)  # noqa: E731
    A, TA, TB = col(sec["a"]), col(sec["ta"]), col(sec["tb"])
    d = [(x - y) % p for x, y in zip(TA, A)]
    e = [(x - y) % p for x, y in zip(TB, A)]
    a_p = [col(sh["a"][q]) for q in range(n)]
    tc_p = [col(sh["tc"][q]) for q in range(n)]
    sq = [[(c - di * ei - di * ai - ei * ai) % p for c, di, ei, ai in zip(tc_p[q], d, e, a_p[q])] for q in range(n)]
    sqop = [x * x % p for x in A]
    return sq, sqop, phase2(sqop, a_p, p)
