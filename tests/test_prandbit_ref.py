"""The PRandBit / PRandInt restatement (tests/prandbit_ref.py) against itself and the reference's constructions, on the CPU: f_T from
the closed product equals the interpolated polynomial evaluated at the party's point; converted shares lie on one degree-t
polynomial whose constant term is sum r_T; PRandBit recovers the input bit in Fr and in GF(2^8); the library's set enumeration
(hbmpc_riss_tsets, host only) equals itertools.combinations; a golden file pins the restatement."""
import itertools
import json
import math
import os
import random

import numpy as np
import pytest

from __graft_entry__ import load_package
from tests import prandbit_ref as PR

SHAPES = [(5, 1), (7, 2), (10, 3)]
# l + k per shape with C(n,t) n 2^(l+k) + 1 < q, so that r + b never wraps in Goldilocks (the reference's own capacity check lacks
# the C(n,t) factor): (5,1) is the reference's test shape with l + k = 55 (tests/prandbitd_test.rs)
LK = {(5, 1): 55, (7, 2): 50, (10, 3): 47}
GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "prandbit_small.json")


@pytest.mark.parametrize("n,t", SHAPES)
def test_lk_leaves_room(n, t):
    assert math.comb(n, t) * n * 2 ** LK[(n, t)] + 1 < PR.P_GL and PR.capacity_ok(n, LK[(n, t)])


@pytest.mark.parametrize("n,t", SHAPES)
@pytest.mark.parametrize("field", ["fr", "goldilocks"])
def test_f_T_closed_product_is_the_interpolated_polynomial(n, t, field):
    p = PR.PRIME[field]
    for T in PR.tsets(n, t):
        for j in range(n):
            v = PR.f_prime(p, n, T, j)
            assert v == PR.f_prime_interpolated(p, n, T, j)
            assert (v == 0) == (j in T)


@pytest.mark.parametrize("n,t", SHAPES)
def test_f_T_gf256(n, t):
    for T in PR.tsets(n, t):
        for j in range(n):
            v = PR.f_gf(T, j)
            assert v == PR.f_gf_interpolated(T, j) and (v == 0) == (j in T)


def test_gf256_field():
    assert PR.gf_mul(0x57, 0x83) == 0xC1  # FIPS-197 section 4.2
    for a in range(1, 256):
        assert PR.gf_mul(a, PR.gf_inv(a)) == 1
    assert len({PR.gf_domain_element(j) for j in range(255)}) == 255 and PR.gf_domain_element(1) == 3


@pytest.mark.parametrize("n,t", SHAPES)
def test_converted_shares_lie_on_one_polynomial(n, t):
    rng = random.Random(n * 100 + t)
    sets = PR.tsets(n, t)
    B = 3
    r = [[rng.randrange(0, n * 2 ** LK[(n, t)] + 1) for _ in range(B)] for _ in sets]
    for field in ("fr", "goldilocks"):
        p = PR.PRIME[field]
        sh, sh2 = PR.convert(p, n, t, r)
        xs = [PR.domain_element(p, n, j) for j in range(n)]
        for i in range(B):
            coeffs = PR.lagrange_interpolate(p, xs, [sh[j][i] for j in range(n)])
            assert all(c == 0 for c in coeffs[t + 1:]) and coeffs[0] == sum(r[k][i] for k in range(len(sets))) % p
    x2 = [PR.gf_domain_element(j) for j in range(n)]
    for i in range(B):
        coeffs = PR.gf_lagrange_interpolate(x2, [sh2[j][i] for j in range(n)])
        assert all(c == 0 for c in coeffs[t + 1:]) and coeffs[0] == sum(r[k][i] for k in range(len(sets))) & 1
    # the one-party layout and the vectorised form give the same shares
    for j in (0, n - 1):
        own = [r[k] for k, T in enumerate(sets) if j not in T]
        assert PR.convert(PR.P_FR, n, t, own, parties=[j], own=j)[0][0] == PR.convert(PR.P_FR, n, t, r, parties=[j])[0][0]
    for field in ("fr", "goldilocks"):
        assert PR.convert_fast(PR.PRIME[field], n, t, np.array(r, dtype=np.uint64)) == PR.convert(PR.PRIME[field], n, t, r)


@pytest.mark.parametrize("n,t", SHAPES)
def test_prandbit_recovers_the_bit(n, t):
    B = 2 * (t + 1)
    contrib, bits, b_q = PR.make_inputs(n, t, B, LK[(n, t)], seed=7 * n + t)
    d = PR.prandbit(n, t, contrib, LK[(n, t)], b_q)
    assert not any(any(row) for row in d["bad"])
    assert d["opened"] == [sum(d["sums"][k][i] for k in range(len(d["sums"]))) + bits[i] for i in range(B)]
    vp, v2 = PR.recovered_bits(n, t, d)
    assert vp == bits and v2 == bits
    # every party's r + b share is on the opened polynomial
    xs = [PR.domain_element(PR.P_GL, n, j) for j in range(n)]
    for i in range(B):
        assert PR.lagrange_at_zero(PR.P_GL, xs, [d["rb"][j][i] for j in range(n)]) == d["opened"][i]
    assert PR.prandint(n, t, contrib, LK[(n, t)])["r_p"] == d["r_p"]


def test_fold_verdicts():
    n, t, B, lk = 5, 1, 4, 20
    contrib, _, _ = PR.make_inputs(n, t, B, lk, seed=3, with_bits=False)
    contrib[2][1][3] = (1 << lk) + 1
    contrib[4][0][0] = 1 << lk  # the bound itself is allowed
    sums, bad = PR.fold(contrib, lk)
    assert [(s, T) for s in range(n) for T in range(5) if bad[s][T]] == [(2, 1)]
    assert sums[0][0] == sum(contrib[s][0][0] for s in range(n))
    assert PR.capacity_ok(16, 57) and not PR.capacity_ok(16, 58) and PR.capacity_ok(5, 58) and not PR.capacity_ok(5, 59) and PR.capacity_ok(4, 59)


@pytest.mark.parametrize("n,t", [(4, 1), (5, 1), (7, 2), (10, 3), (13, 4), (16, 5), (6, 0), (3, 3)])
def test_library_enumerates_the_sets_like_itertools(n, t):
    rc, sets = load_package().hbmpc.riss_tsets(n, t)
    assert rc == 0 and sets == list(itertools.combinations(range(n), t))


def test_library_refuses_too_many_sets():
    assert load_package().hbmpc.riss_tsets(19, 6)[0] == 4  # InvalidInput: 27 132 sets
    assert load_package().hbmpc.riss_tsets(3, 4)[0] == 4


def _golden_case(n, t, seed):
    B, lk = t + 1, LK[(n, t)]
    contrib, bits, b_q = PR.make_inputs(n, t, B, lk, seed)
    d = PR.prandbit(n, t, contrib, lk, b_q)
    hx = lambda rows: [[format(v, "x") for v in row] for row in rows]  # noqa: E731
    return {"n": n, "t": t, "lk": lk, "bits": bits, "contrib": [hx(s) for s in contrib], "b_q": hx(b_q), "sums": hx(d["sums"]),
            "r_q": hx(d["r_q"]), "r_p": hx(d["r_p"]), "r_2": d["r_2"], "opened": [format(v, "x") for v in d["opened"]],
            "b_p": hx(d["b_p"]), "b_2": d["b_2"]}


def test_golden_file_pins_the_restatement():
    with open(GOLDEN) as f:
        cases = json.load(f)
    assert [(c["n"], c["t"]) for c in cases] == [(5, 1), (7, 2)]
    for c in cases:
        n, t = c["n"], c["t"]
        un = lambda rows: [[int(v, 16) for v in row] for row in rows]  # noqa: E731
        d = PR.prandbit(n, t, [un(s) for s in c["contrib"]], c["lk"], un(c["b_q"]))
        assert d["sums"] == un(c["sums"]) and d["r_q"] == un(c["r_q"]) and d["r_p"] == un(c["r_p"]) and d["r_2"] == c["r_2"]
        assert d["opened"] == [int(v, 16) for v in c["opened"]] and d["b_p"] == un(c["b_p"]) and d["b_2"] == c["b_2"]
        vp, v2 = PR.recovered_bits(n, t, d)
        assert vp == c["bits"] and v2 == c["bits"]


if __name__ == "__main__":  # regenerate the golden file
    with open(GOLDEN, "w") as f:
        json.dump([_golden_case(5, 1, 11), _golden_case(7, 2, 12)], f, separators=(",", ":"))
