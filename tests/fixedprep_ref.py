"""Restatement of FixedPrep (hbmpc_pipe_fixedprep_create): the second half of run_preprocessing (honeybadger/mod.rs:1396-1410,
ensure_prandbit_shares :1951-2086, ensure_prandint_shares :2088-2150) for all n parties, composed from the restatements this directory
already has -- producers_ref (RanSha, RanDouSha), oracle/spec.py (TripleGen), randbit_ref, prandbit_ref -- plus the reference's sizing
arithmetic, the order in which it takes from its pools (preprocessing.rs:126-163) and a numpy model of hbmpc_dev_take_rows.
Plain Python integers and numpy; no GPU, no library."""
import functools
import math
import random

import numpy as np

from tests import prandbit_ref as PR
from tests import producers_ref as PD
from tests import randbit_ref as RB
from tests.batchrecon_ref import NONE, SPEC


# ---- the take -------------------------------------------------------------------------------------------------------
def take_rows(src, rows, src_row_stride, dst, dst_row_stride, elements, group):
    """hbmpc_dev_take_rows for one slice, on flat arrays of elements ([len] uint64 or [len][4]): for every row r
    dst[r * dst_row_stride + j * C + i] = src[r * src_row_stride + i * group + j], C = elements / group.  Written as the loop the
    header states; dst is changed in place."""
    assert elements % group == 0
    C = elements // group
    for r in range(rows):
        for i in range(C):
            for j in range(group):
                dst[r * dst_row_stride + j * C + i] = src[r * src_row_stride + i * group + j]
    return dst


def take_rows_np(src, rows, src_row_stride, dst, dst_row_stride, elements, group):
    """the same by numpy indexing (what the GPU tests compare against: the loop above is too slow for their shapes)"""
    C = elements // group
    tail = src.shape[1:]
    for r in range(rows):
        block = src[r * src_row_stride: r * src_row_stride + elements].reshape((C, group) + tail)
        dst[r * dst_row_stride: r * dst_row_stride + elements] = np.swapaxes(block, 0, 1).reshape((elements,) + tail)
    return dst


# ---- sizes (the reference's arithmetic, bit for bit) ---------------------------------------------------------------------------
def sizes(n, t, n_prandbit):
    """(R, T, K1, K2): mod.rs:1973-1974 (bits rounded up to whole RandBit batches of t + 1), :1998-2001 (triples up to whole TripleGen
    batches of 2t + 1), :2004-2008 with :1618-1619 (RanSha runs of n - 2t outputs for R + 2 T random shares), :1816-1817 (RanDouSha runs
    of t + 1 outputs for T double shares)"""
    R = (n_prandbit + t) // (t + 1) * (t + 1)
    T = (R + 2 * t) // (2 * t + 1) * (2 * t + 1)
    K1 = (R + 2 * T + (n - 2 * t) - 1) // (n - 2 * t)
    K2 = (T + t) // (t + 1)
    return R, T, K1, K2


def pool_take(bits_row, ints_row, cursor_bits, cursor_ints, m, N):
    """mul_fixed's drain of one party's pools (mod.rs:1031-1045) for N multiplications with f = m fractional bits: element i takes
    r_bits.drain(0..f) and one r_int, from the front.  -> (rbits [m][N] in fpmul.rs's order: bit j of element i at [j][i], rint [N])"""
    per_element = [[bits_row[cursor_bits + i * m + j] for j in range(m)] for i in range(N)]   # the i-th drain(0..f)
    rbits = [[per_element[i][j] for i in range(N)] for j in range(m)]
    return rbits, [ints_row[cursor_ints + i] for i in range(N)]


# ---- the chain --------------------------------------------------------------------------------------------------------------------
GL = "goldilocks"
Q = PR.P_GL


def lk_for(n, t):
    """l + k with C(n,t) n 2^(l+k) + 1 < q, so that r + b never wraps in Goldilocks (as tests/test_gpu_prandbit_parties.py chooses it)"""
    lk = 55
    while math.comb(n, t) * n * 2**lk + 1 >= Q:
        lk -= 1
    return lk


def open_honest(x, n, d):
    """the secrets of consistent degree-d sharings x [party][N], from parties 0 .. d"""
    xs = [PR.domain_element(Q, n, j) for j in range(d + 1)]
    return [PR.lagrange_at_zero(Q, xs, [x[j][i] for j in range(d + 1)]) for i in range(len(x[0]))]


@functools.lru_cache(maxsize=None)
def inputs(n, t, n_prandbit, n_prandint, seed=0):
    """what a caller uploads: the dealers' Goldilocks polynomials of both producers ([dealer][K][deg + 1], equal secrets in the double
    sharing) and the RISS contributions of both RISS parts ([sender][C(n,t)][B] in [0, 2^lk]); computed once per shape, read-only"""
    lk = lk_for(n, t)
    rnd = random.Random(40503 * n + 977 * n_prandbit + 31 * n_prandint + seed)
    Tn = math.comb(n, t)
    out = {"lk": lk}
    if n_prandbit:
        R, T, K1, K2 = sizes(n, t, n_prandbit)
        out["coeffs"] = [[list(p) for p in row] for row in PD.honest_coeffs(GL, n, t, K1, seed + 5)]
        out["coeffs_t"], out["coeffs_2t"] = PD.double_coeffs(GL, n, t, K2, seed + 7)
        out["contrib_bit"] = [[[rnd.randrange(0, (1 << lk) + 1) for _ in range(R)] for _ in range(Tn)] for _ in range(n)]
    if n_prandint:
        out["contrib_int"] = [[[rnd.randrange(0, (1 << lk) + 1) for _ in range(n_prandint)] for _ in range(Tn)] for _ in range(n)]
    return out


def triplegen(n, t, a, b, r2t, rt):
    """TripleGenNode for all parties on honest inputs [party][N] (triple_generation.rs:333-340, 196-208 through oracle/spec.py over
    Goldilocks): -> (opened [N] = a b - r, c [party][N])"""
    Sp = SPEC[GL]
    N = len(a[0])
    local = [[Sp.triple_local(Sp.Share(a[p][i], p, t), Sp.Share(b[p][i], p, t), Sp.Share(r2t[p][i], p, 2 * t)).v for i in range(N)] for p in range(n)]
    opened = open_honest(local, n, 2 * t)
    c = [[Sp.triple_finalize(Sp.Share(rt[p][i], p, t), opened[i]).v for i in range(N)] for p in range(n)]
    return opened, c


def randbit(n, t, a, ta, tb, tc):
    """RandBit for all parties on honest inputs [party][N] over Goldilocks (rand_bit.rs:242-293, 197-220): Multiply(a, a) with the
    triples (multiplication.rs:417-426, 57-100 through oracle/spec.py), the opened squares, phase 2 (tests/randbit_ref.py)"""
    Sp = SPEC[GL]
    N = len(a[0])
    sh = lambda rows, p, i: Sp.Share(rows[p][i], p, t)  # noqa: E731
    de = [[Sp.beaver_open_shares(sh(ta, p, i), sh(tb, p, i), sh(a, p, i), sh(a, p, i)) for i in range(N)] for p in range(n)]
    d = open_honest([[de[p][i][0].v for i in range(N)] for p in range(n)], n, t)
    e = open_honest([[de[p][i][1].v for i in range(N)] for p in range(n)], n, t)
    sq = [[Sp.beaver_finalize(sh(tc, p, i), sh(a, p, i), sh(a, p, i), d[i], e[i]).v for i in range(N)] for p in range(n)]
    sqop = open_honest(sq, n, t)
    err, first, status, out = RB.phase2(sqop, a, Q)
    return {"deop": d + e, "sq": sq, "sqop": sqop, "status": status, "out": out, "error": err}


def fixedprep(n, t, n_prandbit, n_prandint, inp):
    """one refill for all n parties from inputs(): every part's defined buffers as Python integers, and the pools
    r_bits [party][R] (Fr), r_bits2 [party][R] (GF(2^8) bytes), r_int [party][n_prandint] (Fr)"""
    out = {"lk": inp["lk"]}
    if n_prandbit:
        R, T, K1, K2 = sizes(n, t, n_prandbit)
        dealt = PD.deal(GL, inp["coeffs"], n, t)
        rs = PD.ransha_model(GL, n, t, dealt)
        dealt_t, dealt_2t = PD.deal(GL, inp["coeffs_t"], n, t), PD.deal(GL, inp["coeffs_2t"], n, 2 * t)
        rd = PD.randousha_model(GL, n, t, dealt_t, dealt_2t)
        assert rs["bad"] == (0, NONE) and rd["bad"] == (0, NONE)
        # every take from the front (preprocessing.rs:126-163): RandBit's a, then the triples' a, then their b (mod.rs:2012-2016, 1717-1726)
        cut = lambda rows, lo, hi: [row[lo:hi] for row in rows]  # noqa: E731
        tg_in = {"a": cut(rs["out"], R, R + T), "b": cut(rs["out"], R + T, R + 2 * T), "rt": cut(rd["out_t"], 0, T), "r2t": cut(rd["out_2t"], 0, T)}
        opened, c = triplegen(n, t, tg_in["a"], tg_in["b"], tg_in["r2t"], tg_in["rt"])
        rb_in = {"a": cut(rs["out"], 0, R), "ta": cut(tg_in["a"], 0, R), "tb": cut(tg_in["b"], 0, R), "tc": cut(c, 0, R)}   # mod.rs:2022-2026
        rb = randbit(n, t, rb_in["a"], rb_in["ta"], rb_in["tb"], rb_in["tc"])
        assert rb["error"] == 0
        pb = PR.prandbit(n, t, inp["contrib_bit"], inp["lk"], rb["out"], fast=True)
        out.update({"sizes": (R, T, K1, K2),
                    "ransha": {"S": dealt, "out": rs["out"]},
                    "randousha": {"S_t": dealt_t, "S_2t": dealt_2t, "out_t": rd["out_t"], "out_2t": rd["out_2t"]},
                    "triplegen": dict(tg_in, opened=opened, c=c),
                    "randbit": dict(rb_in, **{k: rb[k] for k in ("deop", "sq", "sqop", "status", "out")}),
                    "prandbit": dict(pb, b_q=rb["out"]),
                    "r_bits": pb["b_p"], "r_bits2": pb["b_2"]})
    if n_prandint:
        pi = PR.prandint(n, t, inp["contrib_int"], inp["lk"], fast=True)
        out.update({"prandint": pi, "r_int": pi["r_p"]})
    return out
