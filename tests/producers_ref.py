"""RanSha and DouSha + RanDouSha for all parties restated from the DEALT SHARES on (share_gen/share_gen.rs:401-454, 516-530, 199-203;
ran_dou_sha/mod.rs:371-449, 569-602, 314-331) for the tests, in Python big integers over both fields, on oracle/spec.py -- never on the
library.  From dealt shares, because that is what lets a test play a dealer whose shares lie on no polynomial.

The calls (hbmpc_[gl_]dev_ransha_parties / _randousha_parties): dealt [dealer][recipient][K] ->
  mix      y[i][j][k] = sum_p alpha_i^p dealt[p][j][k]                  (apply_vandermonde(make_vandermonde(n, n - 1), .))
  RanSha   out [party][K][n - 2t] = rows 2t .. n - 1; yv [party][2t][K] = rows 0 .. 2t - 1; verifier i < 2t: recover_secret of every
           column from the shares of parties 0 .. S - 1, degree exactly t
  RanDouSha  out [party][K][t + 1] = rows 0 .. t; yv [party][n - t - 1][K] = rows t + 1 .. n - 1; verifier i > t:
           NonRobustShare::recover_secret of both sharings through all n shares, degrees exactly t and 2t, equal constant terms
bad = (failing (verifier, column) pairs, the lowest failing column or 0xffffffff).

RanSha's status byte (verifier i, column k) at i K + k: 0 when the lowest 2t + 1 senders' shares lie on a polynomial of degree <= t,
1 when recover_secret's OEC over all S senders recovers, else the error code; the summary as in tests/batchrecon_ref.py.
RanDouSha's verifier results, entry (i - t - 1) K + k, as the field's calls leave them: over Fr sel = (constant term, coefficient d) and
a status byte (8 and zeros when the n points lie on no polynomial of degree <= d); over Goldilocks the constant term and the degree
of the interpolant through all n points."""
from __future__ import annotations

import functools
import random

from tests.batchrecon_ref import NONE, PRIME, SPEC, summary

DECODING_ERROR = 8


def mix(field, dealt, n):
    """dealt [dealer][recipient][K] -> y [row][party][K]"""
    Sp = SPEC[field]
    K = len(dealt[0][0])
    vdm = Sp.make_vandermonde(n, n - 1)
    y = [[[0] * K for _ in range(n)] for _ in range(n)]
    for j in range(n):
        for k in range(K):
            col = Sp.apply_vandermonde(vdm, [Sp.Share(dealt[p][j][k], j, 0) for p in range(n)])
            for i in range(n):
                y[i][j][k] = col[i].v
    return y


def deal(field, coeffs, n, deg):
    """coeffs [dealer][K][deg + 1] -> dealt [dealer][recipient][K] (compute_shares)"""
    Sp = SPEC[field]
    return [[[Sp.compute_shares(list(poly), n, deg)[j].v for poly in coeffs[p]] for j in range(n)] for p in range(n)]


def _lists(y, rows, n, K):
    return [[y[i][j][k] for k in range(K) for i in rows] for j in range(n)]


def _on_degree(field, n, vals, d):
    """the points (party s, vals[s]), s < len(vals): the polynomial through the first d + 1 of them, and whether the others lie on it"""
    Sp = SPEC[field]
    xs = [Sp.domain_element(n, s) for s in range(len(vals))]
    poly = list(Sp.lagrange_interpolate(xs[: d + 1], vals[: d + 1]))
    on = all(Sp.p_eval(poly, xs[s]) == vals[s] for s in range(d + 1, len(vals)))
    return poly + [0] * (d + 1 - len(poly)), on  # lagrange_interpolate trims: all d + 1 coefficients


def ransha_model(field, n, t, dealt, S=None):
    """-> {"out", "yv": [party][..] flat, "status": [2t K], "summary", "bad"}"""
    Sp = SPEC[field]
    S = 2 * t + 1 if S is None else S
    K = len(dealt[0][0])
    y = mix(field, dealt, n)
    status, wrong = [], []
    for i in range(2 * t):
        for k in range(K):
            vals = [y[i][j][k] for j in range(S)]
            good = True
            try:
                poly, _ = Sp.recover_secret([Sp.Share(v, j, t) for j, v in enumerate(vals)], n, t)
                st = 0 if _on_degree(field, n, vals[: 2 * t + 1], t)[1] else 1
                good = Sp.p_degree(poly) == t
            except Sp.ShareErr as e:
                st, good = e.code, False
            status.append(st)
            if not good:
                wrong.append(k)
    return {"out": _lists(y, range(2 * t, n), n, K), "yv": _lists_rows(y, range(2 * t), n, K), "status": status, "summary": summary(status),
            "bad": (len(wrong), min(wrong) if wrong else NONE)}


def _lists_rows(y, rows, n, K):
    """[party][verifier][K]"""
    return [[y[i][j][k] for i in rows for k in range(K)] for j in range(n)]


def randousha_model(field, n, t, dealt_t, dealt_2t):
    """-> {"out_t", "out_2t", "yv_t", "yv_2t", "bad"} and the verifiers' results: over Fr "sel_t", "sel_2t" ([G][2] flat) and "st_t",
    "st_2t" (status bytes); over Goldilocks "sel_*" = the constant terms [G], "st_*" = the degrees [G]"""
    Sp = SPEC[field]
    K = len(dealt_t[0][0])
    ys = (mix(field, dealt_t, n), mix(field, dealt_2t, n))
    out = {}
    res = {0: {"sel": [], "st": []}, 1: {"sel": [], "st": []}}
    wrong = []
    for i in range(t + 1, n):
        for k in range(K):
            good = True
            secrets = []
            for s, d in ((0, t), (1, 2 * t)):
                vals = [ys[s][i][j][k] for j in range(n)]
                try:
                    poly, sec = Sp.nonrobust_recover_secret([Sp.Share(v, j, d) for j, v in enumerate(vals)], n)
                    good = good and Sp.p_degree(poly) == d
                    secrets.append(sec)
                except Sp.ShareErr:
                    good = False
                if field == "fr":
                    low, on = _on_degree(field, n, vals, d)
                    res[s]["sel"] += [low[0], low[d]] if on else [0, 0]
                    res[s]["st"].append(0 if on else DECODING_ERROR)
                else:
                    full, _ = _on_degree(field, n, vals, n - 1)
                    while full and full[-1] == 0:
                        full.pop()
                    res[s]["sel"].append(full[0] if full else 0)
                    res[s]["st"].append(Sp.p_degree(full))
            if not good or len(secrets) != 2 or secrets[0] != secrets[1]:
                wrong.append(k)
    for s, nm in ((0, "t"), (1, "2t")):
        out["out_" + nm] = _lists(ys[s], range(t + 1), n, K)
        out["yv_" + nm] = _lists_rows(ys[s], range(t + 1, n), n, K)
        out["sel_" + nm], out["st_" + nm] = res[s]["sel"], res[s]["st"]
    out["bad"] = (len(wrong), min(wrong) if wrong else NONE)
    return out


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def honest_coeffs(field, n, deg, K, seed=0):
    """[dealer][K][deg + 1] with a top coefficient that is never zero, computed once per shape; treat as read-only"""
    q = PRIME[field]
    rnd = random.Random(6007 * n + 101 * deg + 13 * K + seed + (1 if field == "fr" else 2))
    return tuple(tuple(tuple([rnd.randrange(q) for _ in range(deg)] + [rnd.randrange(1, q)]) for _ in range(K)) for _ in range(n))


def double_coeffs(field, n, t, K, seed=0):
    """(coeffs_t, coeffs_2t) with equal secrets, as lists"""
    ct = [[list(p) for p in row] for row in honest_coeffs(field, n, t, K, seed)]
    c2 = [[list(p) for p in row] for row in honest_coeffs(field, n, 2 * t, K, seed + 1)]
    for p in range(n):
        for k in range(K):
            c2[p][k][0] = ct[p][k][0]
            if t == 0:
                c2[p][k] = list(ct[p][k])
    return ct, c2
