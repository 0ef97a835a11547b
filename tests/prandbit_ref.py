"""PRandBit / PRandInt restated in plain Python integers (fpmul/prandbitd.rs, fpmul/mod.rs:258-279, fpmul/f256.rs) for the tests.

  tsets            combinations(0..n, t)                                   prandbitd.rs:479
  f_T              the polynomial with f(0) = 1, f(alpha_m) = 0, m in T     fpmul/mod.rs:258-279, f256.rs:236-256
  GF(2^8)          AES polynomial 0x11B, generator 3, domain 3^i            f256.rs:58-110, 266-292
  fold             bound test and sum of the senders' contributions        prandbitd.rs:638-647, 667-684
  convert          RISS -> Shamir in Goldilocks, Fr and GF(2^8)             prandbitd.rs:311-356
  finalize         b_p = G(v) - r_p, b_2 = r_2 + lsb(v)                     prandbitd.rs:189-211
  prandbit/prandint  the whole of both protocols for all parties in one process (open: BatchRecon's result, the interpolation at 0)

convert() is the line-by-line form; convert_fast() computes the same sums as exact float64 matrix products of 16-bit limbs (every
partial sum stays below 2^53) so that the GPU tests can afford n = 16, t = 5; test_prandbit_ref.py checks the two against each other."""
from __future__ import annotations

import functools
import itertools
import math
import random

import numpy as np

from oracle import spec as S

P_FR = S.R_MOD
P_GL = 2**64 - 2**32 + 1
PRIME = {"fr": P_FR, "goldilocks": P_GL}
FIELD_CAPACITY = 104  # HBMPC_FIELD_CAPACITY
MAX_TSETS = 8192


def tsets(n, t):
    return list(itertools.combinations(range(n), t))


def own_tsets(n, t, j):
    """the sets party j holds a value for (prandbitd.rs:483-487)"""
    return [T for T in tsets(n, t) if j not in T]


@functools.lru_cache(maxsize=None)
def domain_element(p, n, j):
    """GeneralEvaluationDomain::new(n).element(j): omega of the next power of two, generator 7, two-adicity 32 in both fields"""
    size = 1
    while size < n:
        size *= 2
    w = pow(pow(7, (p - 1) >> 32, p), 2**32 // size, p)
    return pow(w, j, p)


# ---- GF(2^8) (f256.rs:58-110) ----
def gf_mul(a, b):
    r = 0
    while b:
        if b & 1:
            r ^= a
        a <<= 1
        if a & 0x100:
            a ^= 0x11B
        b >>= 1
    return r


def gf_pow(a, e):
    r = 1
    while e:
        if e & 1:
            r = gf_mul(r, a)
        a = gf_mul(a, a)
        e >>= 1
    return r


@functools.lru_cache(maxsize=None)
def gf_inv(a):
    assert a != 0
    return gf_pow(a, 254)


@functools.lru_cache(maxsize=None)
def gf_domain_element(j):
    """Gf256Domain: element(i) = 3^i (f256.rs:266-292); at most 255 elements"""
    return gf_pow(3, j)


# ---- f_T ----
@functools.lru_cache(maxsize=None)
def _domain_inverse(p, n, m):
    return pow(domain_element(p, n, m), p - 2, p)


def f_prime(p, n, T, j):
    """f_T(alpha_j) from the closed product prod (1 - x / alpha_m)"""
    x, r = domain_element(p, n, j), 1
    for m in T:
        r = r * (1 - x * _domain_inverse(p, n, m)) % p
    return r


def f_gf(T, j):
    x, r = gf_domain_element(j), 1
    for m in T:
        r = gf_mul(r, 1 ^ gf_mul(x, gf_inv(gf_domain_element(m))))
    return r


def lagrange_interpolate(p, xs, ys):
    """coefficients (lowest first) of the polynomial through the points, over the prime field p (what build_all_f_polys calls)"""
    m = len(xs)
    out = [0] * m
    for i in range(m):
        num, den = [1], 1
        for k in range(m):
            if k == i:
                continue
            num = [(a - xs[k] * b) % p for a, b in zip([0] + num, num + [0])]
            den = den * (xs[i] - xs[k]) % p
        s = ys[i] * pow(den, p - 2, p) % p
        out = [(o + s * c) % p for o, c in zip(out, num)]
    return out


def gf_lagrange_interpolate(xs, ys):
    """lagrange_interpolate_f2_8 (f256.rs:200-234)"""
    m = len(xs)
    out = [0] * m
    for i in range(m):
        num, den = [1], 1
        for k in range(m):
            if k == i:
                continue
            num = [a ^ gf_mul(xs[k], b) for a, b in zip([0] + num, num + [0])]
            den = gf_mul(den, xs[i] ^ xs[k])
        s = gf_mul(ys[i], gf_inv(den))
        out = [o ^ gf_mul(s, c) for o, c in zip(out, num)]
    return out


def poly_eval(p, coeffs, x):
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * x + c) % p
    return acc


def gf_poly_eval(coeffs, x):
    acc = 0
    for c in reversed(coeffs):
        acc = gf_mul(acc, x) ^ c
    return acc


def f_prime_interpolated(p, n, T, j):
    """as the reference builds it: interpolate (0, 1), (alpha_m, 0), evaluate at alpha_j (fpmul/mod.rs:258-279, prandbitd.rs:328-334)"""
    xs = [0] + [domain_element(p, n, m) for m in T]
    return poly_eval(p, lagrange_interpolate(p, xs, [1] + [0] * len(T)), domain_element(p, n, j))


def f_gf_interpolated(T, j):
    xs = [0] + [gf_domain_element(m) for m in T]
    return gf_poly_eval(gf_lagrange_interpolate(xs, [1] + [0] * len(T)), gf_domain_element(j))


# ---- the protocol steps ----
def capacity_ok(n, lk):
    """prandbitd.rs:506-517 with both moduli: the smaller has 64 bits"""
    return lk + 2 + math.ceil(math.log2(n)) < 64


def fold(contrib, lk):
    """contrib[s][T][i] -> (sums[T][i] of all n senders, modulo 2^64 as the device holds them; bad[s][T] = any value > 2^lk)"""
    n, Tn = len(contrib), len(contrib[0])
    bound = 1 << lk
    sums = [[sum(contrib[s][T][i] for s in range(n)) % 2**64 for i in range(len(contrib[0][T]))] for T in range(Tn)]
    bad = [[int(any(v > bound for v in contrib[s][T])) for T in range(Tn)] for s in range(n)]
    return sums, bad


def convert(p, n, t, r, parties=None, own=None):
    """r[T][i] over tsets(n, t) (own = j: over own_tsets(n, t, j)) -> (shares[party][i] mod p, shares2[party][i] in GF(2^8))"""
    sets = tsets(n, t) if own is None else own_tsets(n, t, own)
    parties = list(range(n)) if parties is None else list(parties)
    B = len(r[0]) if r else 0
    out, out2 = [], []
    for j in parties:
        sp, s2 = [0] * B, [0] * B
        for k, T in enumerate(sets):
            if j in T:
                continue  # the reference never holds r_T for these; f_T(alpha_j) = 0 anyway
            cp, c2 = f_prime(p, n, T, j), (f_gf(T, j) if n <= 255 else 0)
            for i in range(B):
                sp[i] = (sp[i] + r[k][i] * cp) % p
                if r[k][i] & 1:
                    s2[i] ^= c2
        out.append(sp)
        out2.append(s2)
    return out, out2


_COLUMNS = {}


def _tables(p, n, t, parties):
    """({party: its column of f_T(alpha_j) over tsets(n, t)}, the same in GF(2^8)): a column is computed once, and only the parties asked for"""
    sets = None
    for j in set(parties):
        if (p, n, t, j) not in _COLUMNS:
            sets = sets or tsets(n, t)
            _COLUMNS[(p, n, t, j)] = ([0 if j in T else f_prime(p, n, T, j) for T in sets],
                                      [0 if j in T or n > 255 else f_gf(T, j) for T in sets])
    return {j: _COLUMNS[(p, n, t, j)][0] for j in parties}, {j: _COLUMNS[(p, n, t, j)][1] for j in parties}


def convert_fast(p, n, t, r, parties=None):
    """convert() for r as a numpy uint64 array [C(n,t)][B]: exact float64 products of 16-bit limbs"""
    r = np.asarray(r, dtype=np.uint64)
    Tn, B = r.shape
    parties = list(range(n)) if parties is None else list(parties)
    cp, c2 = _tables(p, n, t, parties)
    nl = (p.bit_length() + 15) // 16
    C = np.zeros((Tn, len(parties) * nl), dtype=np.float64)
    for k in range(Tn):
        for q, j in enumerate(parties):
            v = cp[j][k]
            for b in range(nl):
                C[k, q * nl + b] = (v >> (16 * b)) & 0xFFFF
    assert Tn * 65535 * 65535 < 2**53
    acc = [[0] * B for _ in parties]
    for a in range(4):
        limb = ((r >> np.uint64(16 * a)) & np.uint64(0xFFFF)).astype(np.float64)  # [Tn][B]
        M = limb.T @ C  # [B][parties nl], every entry an exact integer below 2^53
        Mi = M.astype(np.int64)
        for q in range(len(parties)):
            for b in range(nl):
                col = Mi[:, q * nl + b]
                sh = 16 * (a + b)
                row = acc[q]
                for i in range(B):
                    row[i] += int(col[i]) << sh
    out = [[v % p for v in row] for row in acc]
    par = (r & np.uint64(1)).astype(np.float64)  # [Tn][B]
    out2 = []
    for j in parties:
        planes = np.array([[(c2[j][k] >> b) & 1 for b in range(8)] for k in range(Tn)], dtype=np.float64)  # [Tn][8]
        bits = (par.T @ planes).astype(np.int64) & 1  # [B][8]
        out2.append([int(sum(int(bits[i, b]) << b for b in range(8))) for i in range(B)])
    return out, out2


def finalize(v, r_p, r_2):
    """try_finalize_bit's arithmetic (prandbitd.rs:189-211): v the opened r + b as Goldilocks integers"""
    bp = [[(x - rp) % P_FR for x, rp in zip(v, row)] for row in r_p]
    b2 = [[r2 ^ (x & 1) for x, r2 in zip(v, row)] for row in r_2]
    return bp, b2


def lagrange_at_zero(p, xs, ys):
    s = 0
    for i, xi in enumerate(xs):
        num = den = 1
        for k, xk in enumerate(xs):
            if k != i:
                num = num * (-xk) % p
                den = den * (xi - xk) % p
        s = (s + ys[i] * num * pow(den, p - 2, p)) % p
    return s


def gf_lagrange_at_zero(xs, ys):
    s = 0
    for i, xi in enumerate(xs):
        num = den = 1
        for k, xk in enumerate(xs):
            if k != i:
                num = gf_mul(num, xk)
                den = gf_mul(den, xi ^ xk)
        s ^= gf_mul(ys[i], gf_mul(num, gf_inv(den)))
    return s


def share_secret(p, n, t, secret, rng):
    """a degree-t Shamir sharing of `secret` over the field's domain -> shares[party]"""
    c = [secret] + [rng.randrange(p) for _ in range(t)]
    return [poly_eval(p, c, domain_element(p, n, j)) for j in range(n)]


def make_inputs(n, t, B, lk, seed, with_bits=True):
    """contrib[s][T][i] uniform in [0, 2^lk], bits[i], b_q[party][i] (Goldilocks shares of the bits)"""
    rng = random.Random(seed)
    Tn = len(tsets(n, t))
    contrib = [[[rng.randrange(0, (1 << lk) + 1) for _ in range(B)] for _ in range(Tn)] for _ in range(n)]
    bits = [rng.randrange(2) for _ in range(B)] if with_bits else []
    cols = [share_secret(P_GL, n, t, b, rng) for b in bits]
    b_q = [[cols[i][j] for i in range(len(bits))] for j in range(n)]
    return contrib, bits, b_q


def prandint(n, t, contrib, lk, fast=False):
    """-> dict: sums, bad, r_p[party][i] (the Fr shares of the random integers: PRandInt's output)"""
    sums, bad = fold(contrib, lk)
    conv = (lambda p: convert_fast(p, n, t, np.array(sums, dtype=np.uint64))) if fast else (lambda p: convert(p, n, t, sums))
    r_p, r_2 = conv(P_FR)
    return {"sums": sums, "bad": bad, "r_p": r_p, "r_2": r_2}


def prandbit(n, t, contrib, lk, b_q, fast=False):
    """-> dict with every intermediate: sums, bad, r_q, r_p, r_2, rb (r_q + b_q), opened, b_p, b_2"""
    d = prandint(n, t, contrib, lk, fast)
    sums = d["sums"]
    r_q = (convert_fast(P_GL, n, t, np.array(sums, dtype=np.uint64)) if fast else convert(P_GL, n, t, sums))[0]
    B = len(b_q[0])
    rb = [[(r_q[j][i] + b_q[j][i]) % P_GL for i in range(B)] for j in range(n)]
    xs = [domain_element(P_GL, n, j) for j in range(t + 1)]
    opened = [lagrange_at_zero(P_GL, xs, [rb[j][i] for j in range(t + 1)]) for i in range(B)]
    b_p, b_2 = finalize(opened, d["r_p"], d["r_2"])
    d.update({"r_q": r_q, "rb": rb, "opened": opened, "b_p": b_p, "b_2": b_2})
    return d


def recovered_bits(n, t, d):
    """the Fr and GF(2^8) values the output shares hold (from the last t + 1 parties, then from the first)"""
    B = len(d["opened"])
    ids = list(range(n - t - 1, n))
    xs = [domain_element(P_FR, n, j) for j in ids]
    vp = [lagrange_at_zero(P_FR, xs, [d["b_p"][j][i] for j in ids]) for i in range(B)]
    x2 = [gf_domain_element(j) for j in range(t + 1)]
    v2 = [gf_lagrange_at_zero(x2, [d["b_2"][j][i] for j in range(t + 1)]) for i in range(B)]
    return vp, v2


# ---- numpy forms of field elements (U256 = [..., 4] uint64 limbs, Goldilocks = uint64) ----
def from_ints(vals, field):
    if field == "goldilocks":
        return np.array(vals, dtype=np.uint64)
    out = np.zeros((len(vals), 4), dtype=np.uint64)
    for i, v in enumerate(vals):
        for k in range(4):
            out[i, k] = (v >> (64 * k)) & 0xFFFFFFFFFFFFFFFF
    return out


def to_ints(arr, field):
    if field == "goldilocks":
        return [int(v) for v in arr]
    return [sum(int(row[k]) << (64 * k) for k in range(4)) for row in arr]


def rows_from_ints(rows, field):
    return np.stack([from_ints(r, field) for r in rows])
