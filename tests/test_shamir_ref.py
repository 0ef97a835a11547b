"""The model of the integer-point Shamir scheme (tests/shamir_ref.py) against common/share/shamir.rs:44-125: every error in the
reference's order (inputs that trip two checks at once pin the order), round trips, the Goldilocks ids p, p + 1 and 2^64 - 1, and
the zero polynomial.  Runs without a GPU."""
import random

import pytest

from tests import shamir_ref as M
from tests.shamir_ref import FR, GL

P_GL = GL.R_MOD
SPECS = [pytest.param(FR, id="fr"), pytest.param(GL, id="goldilocks")]


def poly(spec, seed, d):
    rng = random.Random(seed)
    return [rng.randrange(spec.R_MOD) for _ in range(d + 1)]


# ---- compute_shares: shamir.rs:51-70 ----
@pytest.mark.parametrize("spec", SPECS)
def test_compute_shares_error_order(spec):
    c = poly(spec, 1, 2)
    with pytest.raises(spec.InvalidInput):                   # 1. ids = None, whatever else
        M.compute_shares(spec, c, 2, None)
    with pytest.raises(spec.InsufficientShares):             # 2. before 3 and 4: too few ids that also hold a zero and a duplicate
        M.compute_shares(spec, c, 2, [0, 0])
    with pytest.raises(spec.InvalidInput):                   # 3. a zero id
        M.compute_shares(spec, c, 2, [1, 0, 2])
    with pytest.raises(spec.InvalidInput):                   # 4. duplicates
        M.compute_shares(spec, c, 2, [1, 2, 2])
    assert len(M.compute_shares(spec, c, 2, [3, 1, 2])) == 3


def test_compute_shares_insufficient_wins_over_zero_and_duplicate():
    """InsufficientShares (code 1) and InvalidInput (code 4) differ, so the order of checks 2 and 3/4 shows in the code"""
    for ids in ([0], [5, 5], [0, 0]):
        with pytest.raises(FR.ShareErr) as e:
            M.compute_shares(FR, poly(FR, 2, 2), 2, ids)
        assert e.value.code == 1


def test_goldilocks_ids_at_and_above_p():
    c = poly(GL, 3, 1)
    with pytest.raises(GL.InvalidInput):                     # id = p is the zero element
        M.compute_shares(GL, c, 1, [1, P_GL])
    got = M.compute_shares(GL, c, 1, [1, P_GL + 1])          # distinct integers, the same point: accepted, two equal rows
    assert got[0] == got[1] == GL.p_eval(c, 1)
    top = (1 << 64) - 1
    got = M.compute_shares(GL, c, 1, [top, 2])
    assert got[0] == GL.p_eval(c, top - P_GL) and top - P_GL == (1 << 32) - 2
    # over Fr no u64 id reaches p
    assert M.compute_shares(FR, poly(FR, 4, 1), 1, [top, P_GL])[1] == FR.p_eval(poly(FR, 4, 1), P_GL)


# ---- recover_secret: shamir.rs:90-125 ----
@pytest.mark.parametrize("spec", SPECS)
def test_recover_secret_error_order(spec):
    c = poly(spec, 5, 2)
    ids = [1, 2, 3, 4]
    vals = M.compute_shares(spec, c, 2, ids)
    with pytest.raises(spec.InvalidInput):                   # 1. no shares
        M.recover_secret(spec, [], [], [])
    with pytest.raises(spec.InvalidInput):                   # 2. duplicate ids, before 3: the degrees differ too
        M.recover_secret(spec, [1, 1, 2], [2, 3, 2], vals[:3])
    with pytest.raises(spec.DegreeMismatch):                 # 3. unequal degrees, before 4: too few for degrees[0] as well
        M.recover_secret(spec, [1, 2], [5, 2], vals[:2])
    with pytest.raises(spec.InsufficientShares):             # 4. too few shares, before 5: a zero id among them
        M.recover_secret(spec, [0, 2], [2, 2], vals[:2])
    with pytest.raises(spec.InvalidInput):                   # 5. a zero id
        M.recover_secret(spec, [0, 2, 3], [2, 2, 2], vals[:3])
    bad = list(vals)
    bad[3] = (bad[3] + 1) % spec.R_MOD
    with pytest.raises(spec.DegreeMismatch):                 # 7. four points off a parabola
        M.recover_secret(spec, ids, [2] * 4, bad)
    co, sec = M.recover_secret(spec, ids, [2] * 4, vals)
    assert co == c and sec == c[0]


def test_recover_secret_duplicate_field_elements():
    """6. distinct integers that are one field element pass checks 2 and 5 and fail inside lagrange_interpolate (mod.rs:141-144);
    with a wrong degree list check 3 answers first"""
    with pytest.raises(GL.InvalidInput):
        M.recover_secret(GL, [1, P_GL + 1], [1, 1], [7, 7])
    with pytest.raises(GL.DegreeMismatch):
        M.recover_secret(GL, [1, P_GL + 1], [1, 2], [7, 7])
    with pytest.raises(GL.InvalidInput):                     # 5 before 6: id = p is zero and p + 1 doubles 1
        M.recover_secret(GL, [1, P_GL + 1, P_GL], [1, 1, 1], [7, 7, 7])


@pytest.mark.parametrize("spec", SPECS)
@pytest.mark.parametrize("ids,d", [([1, 2, 3, 4, 5, 6], 5), ([1, 2, 3, 4, 5, 6], 2), ([7, 1, 3, 20], 3), ([7, 1, 3, 20], 1), ([(1 << 32) + 5, 1, 2], 2),
                                   ([(1 << 64) - 1, 9], 1), ([4], 0)])
def test_round_trip(spec, ids, d):
    c = poly(spec, 100 + d, d)
    c[d] = c[d] or 1
    vals = M.compute_shares(spec, c, d, ids)
    co, sec = M.recover_secret(spec, ids, [d] * len(ids), vals)
    assert co == c and sec == c[0]
    bc, deg = M.batch_interpolate(spec, ids, [[v] for v in vals])
    assert bc[0][:d + 1] == c and not any(bc[0][d + 1:]) and deg == [d]


@pytest.mark.parametrize("spec", SPECS)
def test_zero_polynomial(spec):
    ids = [1, 2, 3]
    assert M.compute_shares(spec, [0, 0, 0], 2, ids) == [0, 0, 0]
    assert M.recover_secret(spec, ids, [2] * 3, [0, 0, 0]) == ([], 0)
    assert M.batch_interpolate(spec, ids, [[0], [0], [0]]) == ([[0, 0, 0]], [0])


@pytest.mark.parametrize("spec", SPECS)
def test_lagrange_basis_is_the_inverse_vandermonde(spec):
    for ids in ([1, 2, 3, 4, 5, 6], [7, 1, 3, 20], [(1 << 32) + 5, 1, 2]):
        basis = M.lagrange_basis(spec, ids)
        for i in range(len(ids)):
            for j, x in enumerate(ids):
                assert spec.p_eval(basis[i], M.f_from(spec, x)) == (1 if i == j else 0)


def test_batch_interpolate_refusals():
    for ids in ([], [1, 1], [0, 1]):
        with pytest.raises(FR.InvalidInput):
            M.batch_interpolate(FR, ids, [[1]] * len(ids))
    for ids in ([1, P_GL + 1], [P_GL, 2]):
        with pytest.raises(GL.InvalidInput):
            M.batch_interpolate(GL, ids, [[1]] * len(ids))
