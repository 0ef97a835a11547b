"""tests/verdict_model.py (the contract of the verdict calls, which the GPU edge tests compare the kernels with) against
oracle/spec.py: the model's degree is DensePolynomial::degree(), and its verdict over one verifier's columns is "no failure"
exactly when the verifier loops of S.ransha / S.randousha say good.  No GPU."""
import random

import pytest

from oracle import spec as SFR
from oracle.spec_gl import S as SGL
from tests import verdict_model as M

FIELDS = {"fr": SFR, "goldilocks": SGL}


def test_the_worked_example_of_the_contract():
    """columns = 100, two verifiers, failing entries 70 (verifier 0, column 70) and 105 (verifier 1, column 5): both sit in the same
    wave of 64 entries (64..127) with the HIGHER column first, and the contract says lowest failing column"""
    top = [1] * 200
    top[70] = top[105] = 0
    assert M.check_top_coeff(top, None, 2, columns=100) == [2, 5]
    assert M.check_top_coeff(top, None, 2) == [2, 70]                      # one verifier of 200 columns: the entry itself
    assert M.check_top_coeff(top, None, 2, bad=(3, 4), columns=100) == [5, 4]  # accumulated: the count adds, the lower first stays
    # verifier by verifier (the loop the fused form must agree with)
    bad = M.FRESH
    for q in range(2):
        bad = M.check_top_coeff(top[100 * q: 100 * (q + 1)], None, 2, bad=bad)
    assert bad == [2, 5]
    assert M.check_top_coeff([1] * 200, None, 2, columns=100) == list(M.FRESH)


@pytest.mark.parametrize("field", ["fr", "goldilocks"])
def test_degree_is_dense_polynomial_degree(field):
    S = FIELDS[field]
    r = S.R_MOD
    for c in ([], [0], [5], [0, 0, 0], [0, 1], [3, 0], [1, 2, 3], [1, 2, 0], [1, 0, 0, 0], [0, 0, r - 1, 0, 0], [0, 0, 0, 1], [r - 1] * 6):
        assert M.degree(c) == S.p_degree(S.p_norm(c)), c


def _tops_zero_at(S, n, i):
    """top coefficients a_p of the n dealers such that sum_p x_i^p a_p = 0 at verifier i alone: a_0 = -x_i, a_1 = 1, the others 0
    (sum_p x_j^p a_p = x_j - x_i, zero only at j = i: the domain elements are distinct)"""
    return [(-S.domain_element(n, i)) % S.R_MOD, 1] + [0] * (n - 2)


def _dealers(S, rng, n, K, deg):
    return [[[rng.randrange(1, S.R_MOD) for _ in range(deg + 1)] for _ in range(K)] for _ in range(n)]


@pytest.mark.parametrize("field", ["fr", "goldilocks"])
def test_model_verdict_is_the_ransha_verifiers(field):
    S = FIELDS[field]
    n, t, K = 4, 1, 3
    rng = random.Random(41)
    honest = _dealers(S, rng, n, K, t)
    one = [[list(c) for c in d] for d in honest]          # column 1 has degree t - 1 at verifier 1 alone
    for p, a in enumerate(_tops_zero_at(S, n, 1)):
        one[p][1][t] = a
    every = [[list(c) for c in d] for d in honest]        # column 2 has degree t - 1 at every verifier
    for p in range(n):
        every[p][2][t] = 0
    seen = set()
    for coeffs in (honest, one, every):
        _, ok = S.ransha(coeffs, n, t)
        r = S._deal_and_mix(coeffs, n, t)
        for i in range(2 * t):
            polys, status = [], []
            for k in range(K):
                try:
                    poly, _ = S.recover_secret([S.Share(r[j][k][i].v, j, t) for j in range(2 * t + 1)], n, t)
                    polys.append(list(poly) + [0] * (t + 1 - len(poly)))
                    status.append(0)
                except S.ShareErr:
                    polys.append([0] * (t + 1))
                    status.append(8)
            full = M.check_degree(polys, status, t)
            top = M.check_top_coeff([c[t] for c in polys], status, t)
            assert full == top and (full[0] == 0) == ok[i], (i, full, top, ok)
            seen.add(tuple(full))
    assert seen == {M.FRESH, (1, 1), (1, 2)}


@pytest.mark.parametrize("field", ["fr", "goldilocks"])
def test_model_verdict_is_the_randousha_verifiers(field):
    S = FIELDS[field]
    n, t, K = 4, 1, 3
    rng = random.Random(43)
    ct = _dealers(S, rng, n, K, t)
    c2t = _dealers(S, rng, n, K, 2 * t)
    for p in range(n):
        for k in range(K):
            c2t[p][k][0] = ct[p][k][0]
    low_t = [[list(c) for c in d] for d in ct]            # column 0: degree t - 1 at verifier 3 alone
    for p, a in enumerate(_tops_zero_at(S, n, 3)):
        low_t[p][0][t] = a
    low_2t = [[list(c) for c in d] for d in c2t]          # column 2: degree 2t - 1 at verifier 2 alone
    for p, a in enumerate(_tops_zero_at(S, n, 2)):
        low_2t[p][2][2 * t] = a
    other = [[list(c) for c in d] for d in c2t]           # column 1: dealer 1's two secrets differ (every verifier sees it)
    other[1][1][0] = (other[1][1][0] + 1) % S.R_MOD
    seen = set()
    for a, b in ((ct, c2t), (low_t, c2t), (ct, low_2t), (ct, other)):
        _, _, ok = S.randousha(a, b, n, t)
        rt, r2t = S._deal_and_mix(a, n, t), S._deal_and_mix(b, n, 2 * t)
        xs = [S.domain_element(n, j) for j in range(n)]
        for v, i in enumerate(range(t + 1, n)):
            pt = [S.lagrange_interpolate(xs, [rt[j][k][i].v for j in range(n)]) for k in range(K)]
            p2t = [S.lagrange_interpolate(xs, [r2t[j][k][i].v for j in range(n)]) for k in range(K)]
            pt = [list(p) + [0] * (n - len(p)) for p in pt]
            p2t = [list(p) + [0] * (n - len(p)) for p in p2t]
            full = M.check_double_share(pt, p2t, t)
            c0 = M.check_double_share_c0([p[0] for p in pt], [M.degree(p) for p in pt], [p[0] for p in p2t], [M.degree(p) for p in p2t], t)
            # the selective form: status 8 and zeros when the points lie on no polynomial of degree <= d, (c0, coefficient d) otherwise
            sel = []
            for polys, d in ((pt, t), (p2t, 2 * t)):
                high = [M.degree(p) > d for p in polys]
                sel.append(([(0, 0) if h else (p[0], p[d]) for p, h in zip(polys, high)], [8 if h else 0 for h in high]))
            picked = M.check_double_share_sel(sel[0][0], sel[0][1], sel[1][0], sel[1][1], t)
            assert full == c0 == picked and (full[0] == 0) == ok[v], (i, full, c0, picked, ok)
            seen.add(tuple(full))
    assert seen == {M.FRESH, (1, 0), (1, 1), (1, 2)}
