"""tests/producers_ref.py (the model of hbmpc_[gl_]dev_ransha_parties / _randousha_parties from the dealt shares on) against
oracle/spec.py's ransha / randousha, which start from the dealers' polynomials: on honest inputs the outputs are equal and every
verifier passes; a lie in one dealt share fails exactly the verifiers the mixing step carries it to."""
import pytest

from tests import producers_ref as PR
from tests.batchrecon_ref import NONE, PRIME, SPEC

SHAPES = [(4, 1), (5, 1), (7, 2), (2, 0), (3, 1)]
FIELDS = ("fr", "goldilocks")


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("n,t", SHAPES)
def test_ransha_equals_the_oracle_on_honest_inputs(field, n, t):
    Sp, K = SPEC[field], 2
    coeffs = [[list(p) for p in row] for row in PR.honest_coeffs(field, n, t, K)]
    want_out, want_ok = Sp.ransha(coeffs, n, t)
    m = PR.ransha_model(field, n, t, PR.deal(field, coeffs, n, t))
    assert m["out"] == want_out
    if n >= 3 * t + 1:
        assert all(want_ok) and m["bad"] == (0, NONE) and m["status"] == [0] * (2 * t * K) and m["summary"] == (0, 0, NONE, 0)
    else:  # recover_secret refuses: every verifier fails every column
        assert not any(want_ok) and m["bad"] == (2 * t * K, 0) and m["status"] == [4] * (2 * t * K) and m["summary"] == (2 * t * K, 2 * t * K, 0, 4)


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("n,t", SHAPES)
def test_randousha_equals_the_oracle_on_honest_inputs(field, n, t):
    Sp, K = SPEC[field], 2
    ct, c2 = PR.double_coeffs(field, n, t, K)
    want_t, want_2t, want_ok = Sp.randousha(ct, c2, n, t)
    m = PR.randousha_model(field, n, t, PR.deal(field, ct, n, t), PR.deal(field, c2, n, 2 * t))
    assert m["out_t"] == want_t and m["out_2t"] == want_2t
    assert all(want_ok) and m["bad"] == (0, NONE)
    G = (n - t - 1) * K
    if field == "fr":
        assert m["st_t"] == [0] * G and m["st_2t"] == [0] * G and m["sel_t"][0::2] == m["sel_2t"][0::2]
    else:
        assert m["st_t"] == [t] * G and m["st_2t"] == [2 * t] * G and m["sel_t"] == m["sel_2t"]


@pytest.mark.parametrize("field", FIELDS)
def test_a_tampered_dealt_share(field):
    """recipient j <= 2t: every RanSha verifier fails the column; j > 2t: none sees it, party j's outputs differ"""
    n, t, K, q = 7, 2, 2, PRIME[field]
    coeffs = [[list(p) for p in row] for row in PR.honest_coeffs(field, n, t, K)]
    dealt = PR.deal(field, coeffs, n, t)
    honest = PR.ransha_model(field, n, t, dealt)
    for j, want in ((1, (2 * t, 1)), (2 * t + 1, (0, NONE))):
        lied = [[list(r) for r in d] for d in dealt]
        lied[3][j][1] = (lied[3][j][1] + 1) % q
        m = PR.ransha_model(field, n, t, lied)
        assert m["bad"] == want
        assert m["out"][j] != honest["out"][j]               # party j mixes what it received, whether a verifier hears of it or not
        assert [m["out"][p] for p in range(n) if p != j] == [honest["out"][p] for p in range(n) if p != j]


@pytest.mark.parametrize("field", FIELDS)
def test_randousha_unequal_secrets_and_a_wrong_degree(field):
    n, t, K, q = 4, 1, 3, PRIME[field]
    ct, c2 = PR.double_coeffs(field, n, t, K)
    c2[0][1][0] = (c2[0][1][0] + 1) % q                      # unequal secrets in column 1: every verifier
    m = PR.randousha_model(field, n, t, PR.deal(field, ct, n, t), PR.deal(field, c2, n, 2 * t))
    assert m["bad"] == (n - t - 1, 1)
    ct, c2 = PR.double_coeffs(field, n, t, K)
    for p in range(n):
        c2[p][2][2 * t] = 0                                  # degree below 2t in column 2
    m = PR.randousha_model(field, n, t, PR.deal(field, ct, n, t), PR.deal(field, c2, n, 2 * t))
    assert m["bad"] == (n - t - 1, 2)
