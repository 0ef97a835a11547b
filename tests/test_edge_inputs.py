"""tests/edge_inputs.py without a GPU and without the library: every generated sharing is valid (it opens with status 0 under the
oracle's batch_recover_p0), the single-bit tampering fails exactly the chunks it names, and SITE_TABLE holds -- for every kernel
family each listed intermediate, computed as an integer from the inputs alone, takes each listed edge value for at least one
(party, element) of the inputs tests/test_gpu_wave_edges.py feeds it.  No pair is waived."""
import numpy as np
import pytest

from oracle import spec as S
from tests import edge_inputs as X

R = S.R_MOD


def assert_opens(F, shares, n, deg, t, tag):
    """[party][N] (ints) is a sharing of degree <= deg: the oracle's robust P(0) decode from all n parties reports nothing"""
    rc, _, st = F.O.batch_recover_p0(list(range(n)), F.arr(shares), n, deg, t)
    assert rc == 0 and not st.any(), tag


def assert_all_open(F, ins, n, t, tag, degrees=None):
    for nm, v in ins.items():
        if nm == "w" or v is None:
            continue
        if nm == "rbits":
            for j in range(len(v[0])):
                assert_opens(F, [row[j] for row in v], n, t, t, (tag, nm, j))
        else:
            assert_opens(F, v, n, (degrees or {}).get(nm, t), t, (tag, nm))


def test_value_classes():
    assert len(X.EDGE) == 15 and all(0 <= v < R for v in X.EDGE) and len(set(X.EDGE_GL)) == 9 and all(0 <= v < X.P for v in X.EDGE_GL)
    assert X.B >> 232 == R >> 232 and X.B < R and X.MAXLIMB == X.B - 1 and len(set(X.EDGE)) == 14      # B - 1 and MAXLIMB: one value, listed twice
    assert all((X.MAXLIMB >> 29 * i) & 0x1fffffff == 0x1fffffff for i in range(8))      # all-ones limbs below the top one
    for bit in X.TAMPER_BITS:
        base, bad = X.tamper_value(bit)
        assert base < bad < R and base ^ bad == 1 << bit


@pytest.mark.parametrize("n,t,senders", X.MUL_SHAPES)
def test_mul_inputs(n, t, senders):
    for F in (X.FR, X.GL):
        case = X.mul_case(F, n, t, senders)
        assert case["N"] <= 64
        assert_all_open(F, case["ins"], n, t, (F.name, n, t))
        for p in X.forced_parties(n, t, senders):                                     # the forced columns hold edge values there
            assert all(case["ins"]["x"][p][g] in F.edge for g in range(case["N"] - len(F.edge), case["N"]))
        sites = [X.mul_sites(F, col, n, t, senders) for col in case["cols"]]
        assert X.missing_pairs(F, "mul", sites) == [], (F.name, n, t)


def test_truncpr_inputs():
    """every case of the GPU tests is valid; the table holds over each shape's cases of the main moduli on their own (both instances
    of the kernel together), with the wide moduli's four elements each for c mod 2^m"""
    per_shape = {}
    for n, t, senders, k, m, with_w, count, rot in X.truncpr_cases():
        case = X.truncpr_case(n, t, senders, k, m, with_w, count, rot)
        assert case["N"] <= (4 if count else 64)
        assert_all_open(X.FR, case["ins"], n, t, (n, t, k, m, with_w))
        if with_w:
            assert set(case["ins"]["w"]) <= set(X.W_VALUES) and (count or set(case["ins"]["w"]) == set(X.W_VALUES))
        per_shape.setdefault((n, t), []).extend(X.truncpr_sites(col, n, t, senders, k, m) for col in case["cols"])
    wide = [s for (n, t, senders, k, m, with_w, count, rot) in X.truncpr_cases() if count
            for s in [{"cop_mod": X.truncpr_sites(col, n, t, senders, k, m)["cop_mod"]} for col in X.truncpr_case(n, t, senders, k, m, with_w, count, rot)["cols"]]]
    for (n, t), sites in per_shape.items():
        assert X.missing_pairs(X.FR, "truncpr", sites + wide) == [], (n, t)


def test_truncpr_special_columns():
    """the columns the list of edge values does not give by itself: every bit share MAXLIMB, then r - 1, and the maximal four-term
    loose sum v = r - 1, 2^m r_int = r - 1, r' = r - 1"""
    n, t, k, m = 16, 5, 32, 13
    senders = tuple(range(2 * t + 1))
    cols = X.truncpr_case(n, t, senders, k, m, False)["cols"]
    for b in (X.MAXLIMB, R - 1):
        assert any(all(v == b for row in col["bits"] for v in row) for col in cols)
    assert any(s["two_m_rint"][0] == s["rdash"][0] == R - 1 and col["a"][0] == R - 1
               for col in cols for s in [X.truncpr_sites(col, n, t, senders, k, m)])


@pytest.mark.parametrize("n,t,k,m", X.FPMUL_SHAPES)
def test_fpmul_inputs(n, t, k, m):
    senders = tuple(range(2 * t + 1))
    case = X.fpmul_case(n, t, senders, k, m)
    assert_all_open(X.FR, case["ins"], n, t, (n, t, k, m))
    sites = [X.fpmul_sites(col, n, t, senders, k, m) for col in case["cols"]]
    wide = []                                                   # c mod 2^m < 2^m: the classes above it come from the wide moduli's cases
    for wn, wt, wk, wm, count, rot in X.FPMUL_WIDE:
        wcase = X.fpmul_case(wn, wt, (0, 1, 2), wk, wm, count, rot)
        assert_all_open(X.FR, wcase["ins"], wn, wt, (wk, wm))
        wide += [{"cop_mod": X.fpmul_sites(col, wn, wt, (0, 1, 2), wk, wm)["cop_mod"]} for col in wcase["cols"]]
    assert X.missing_pairs(X.FR, "fpmul", sites + wide) == [], (n, t, k, m)
    assert {v for s in sites for v in s["cop_mod"]} >= {v for v in X.EDGE if v < 1 << m}


@pytest.mark.parametrize("F", [X.FR, X.GL], ids=["fr", "goldilocks"])
@pytest.mark.parametrize("n,t", X.TRIPLE_SHAPES)
def test_triple_inputs(F, n, t):
    case = X.triple_case(F, n, t)
    assert case["N"] % (2 * t + 1) == 0
    assert_all_open(F, case["ins"], n, t, (F.name, n, t), degrees={"r2t": 2 * t})
    for col in case["cols"]:                                                            # rt and r2t share their secret: c opens to a b
        assert X.p0(F, n, list(range(t + 1)), col["rt"]) == X.p0(F, n, list(range(2 * t + 1)), col["r2t"])
    sites = [X.triple_sites(F, col, n, t) for col in case["cols"]]
    assert X.missing_pairs(F, "triplegen", sites) == [], (F.name, n, t)


def failing_chunks(ids, rows, n, t):
    rc, _, st = X.FR.O.batch_recover_p0(list(ids), X.FR.arr(rows), n, t, t)
    assert rc in (0, 8) and set(st.tolist()) <= {0, 8}
    return [int(i) for i in np.flatnonzero(st)]


def opened_pair(ins, ids, N):
    """the senders' rows of a - x | b - y"""
    return [[(ins["ta"][p][g] - ins["x"][p][g]) % R for g in range(N)] + [(ins["tb"][p][g] - ins["y"][p][g]) % R for g in range(N)] for p in ids]


@pytest.mark.parametrize("n,t,senders", [(4, 1, (0, 1, 2)), (7, 2, (6, 1, 3, 0, 4)), (16, 5, tuple(range(11)))])
def test_single_bit_tampering(n, t, senders):
    """one bit per element, on a sender behind a verify row and on one behind the P(0) row: exactly those chunks fail in the oracle's
    decode from the 2t + 1 senders, the honest inputs open clean"""
    k, m = 32, 6
    mt = X.mul_tamper_case(n, t, senders)
    assert_all_open(X.FR, mt["honest"], n, t, "mul")
    assert failing_chunks(senders, opened_pair(mt["ins"], senders, mt["N"]), n, t) == mt["failing"] and len(mt["failing"]) == 16
    tt = X.truncpr_tamper_case(n, t, senders, k, m)
    assert_all_open(X.FR, tt["honest"], n, t, "truncpr")
    cols = [{"a": [tt["ins"]["a"][p][g] for p in range(n)], "rint": [tt["ins"]["rint"][p][g] for p in range(n)],
             "bits": [[tt["ins"]["rbits"][p][j][g] for p in range(n)] for j in range(m)]} for g in range(tt["N"])]
    osh = [X.truncpr_sites(col, n, t, senders, k, m)["osh"] for col in cols]
    assert all(osh[g][p] == tt["ins"]["a"][p][g] for g in range(tt["N"]) for p in range(n))          # the opened share is a itself
    assert failing_chunks(senders, [[osh[g][p] for g in range(tt["N"])] for p in senders], n, t) == tt["failing"] and len(tt["failing"]) == 16
    ft = X.fpmul_tamper_case(n, t, senders, k, m)
    assert_all_open(X.FR, ft["honest"], n, t, "fpmul")
    assert failing_chunks(senders, opened_pair(ft["ins"], senders, ft["N"]), n, t) == ft["failing_first"]
    assert len(ft["failing_first"]) == 16 and len(ft["failing_second"]) == 16
    assert not set(ft["failing_second"]) & {c % ft["N"] for c in ft["failing_first"]}
