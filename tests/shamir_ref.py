"""The model of the integer-point Shamir scheme, `Shamirshare` (common/share/shamir.rs:13-126), line by line over oracle/spec.py's
polynomial helpers and error classes -- and over their Goldilocks twins (oracle/spec_gl.py) through the `spec` argument.

A share sits at the field element F::from(id as u64): the id reduced mod p, NOT a root of unity.  The order of the checks is the
reference's; the tests pin it with inputs that trip two checks at once."""
from oracle import spec as FR
from oracle.spec_gl import S as GL

U64 = 1 << 64


def f_from(spec, i):
    """F::from(id as u64)"""
    assert 0 <= i < U64
    return i % spec.R_MOD


def compute_shares(spec, coeffs, degree, ids):
    """shamir.rs:44-88 with the polynomial given instead of drawn: coeffs[0] = secret, coeffs[1..=degree] = DensePolynomial::rand's
    draws.  Returns the share values in the order of ids."""
    if ids is None:                                            # :51-54
        raise spec.InvalidInput()
    if len(ids) < degree + 1:                                  # :57-59
        raise spec.InsufficientShares()
    if any(f_from(spec, i) == 0 for i in ids):                 # :62-64
        raise spec.InvalidInput()
    if len(set(ids)) != len(ids):                              # :67-70, the ids as integers
        raise spec.InvalidInput()
    assert len(coeffs) == degree + 1
    return [spec.p_eval(coeffs, f_from(spec, i)) for i in ids]  # :77-84


def recover_secret(spec, ids, degrees, vals):
    """shamir.rs:90-125.  Returns (trimmed coefficients, secret).  For the zero polynomial the reference indexes result_poly[0] and
    panics; this returns ([], 0), as oracle/spec.py::nonrobust_recover_secret does for the same expression."""
    if len(ids) == 0:                                          # :95-97
        raise spec.InvalidInput()
    if len(set(ids)) != len(ids):                              # :98-101
        raise spec.InvalidInput()
    deg = degrees[0]
    if any(d != deg for d in degrees):                         # :102-105
        raise spec.DegreeMismatch()
    if len(ids) < deg + 1:                                     # :106-108
        raise spec.InsufficientShares()
    if any(f_from(spec, i) == 0 for i in ids):                 # :109-114
        raise spec.InvalidInput()
    xs = [f_from(spec, i) for i in ids]
    poly = spec.lagrange_interpolate(xs, [v % spec.R_MOD for v in vals])  # :120, duplicate field elements: InvalidInput (mod.rs:141-144)
    if spec.p_degree(poly) > deg:                              # :121-123
        raise spec.DegreeMismatch()
    return poly, (poly[0] if poly else 0)


def check_points(spec, ids):
    """the point checks of the batched open (hbmpc_[gl_]shamir_batch_interpolate): recover_secret's without the degrees"""
    if len(ids) == 0 or len(set(ids)) != len(ids) or any(f_from(spec, i) == 0 for i in ids):
        raise spec.InvalidInput()
    if len({f_from(spec, i) for i in ids}) != len(ids):
        raise spec.InvalidInput()


def batch_interpolate(spec, ids, evals):
    """evals[S][G] -> (coeffs[G][S] not trimmed, degree[G]): plain Lagrange through all S points, column by column"""
    check_points(spec, ids)
    xs = [f_from(spec, i) for i in ids]
    S, G = len(ids), len(evals[0])
    basis = [spec.lagrange_interpolate(xs, [1 if j == i else 0 for j in range(S)]) for i in range(S)]  # the Lagrange basis, once
    basis = [b + [0] * (S - len(b)) for b in basis]
    out, deg = [], []
    for g in range(G):
        col = [sum(basis[i][k] * evals[i][g] for i in range(S)) % spec.R_MOD for k in range(S)]
        out.append(col)
        top = max((k for k in range(S) if col[k]), default=0)
        deg.append(top)
    return out, deg


def lagrange_basis(spec, ids):
    """basis[i][k] = coefficient k of L_i over the points F::from(ids): what the host-built table must hold"""
    xs = [f_from(spec, i) for i in ids]
    S = len(ids)
    rows = [spec.lagrange_interpolate(xs, [1 if j == i else 0 for j in range(S)]) for i in range(S)]
    return [r + [0] * (S - len(r)) for r in rows]
