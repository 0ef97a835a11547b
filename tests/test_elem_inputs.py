"""The inputs of tests/elem_inputs.py reach what SITE_TABLE claims, tell every mutation of tests/elem_model.py from the true model, and
the model is the project's specification (oracle/spec.py, oracle/spec_gl.py) restated.  No GPU, no library.

Where a mutation must die.  A mutation of the arithmetic (the stored-word add and subtract, the terms of finalize_mul, the mask, 2^(k-1),
the fold of r') shows at any shape, so it must die at the smallest one, (N, parties) = (1, 1): one element.  A mutation of the indexing
needs more than one party to be a different kernel at all (party 0 of a one-party call has ip = i, one r_bits plane, one pair), and the
swapped remap writes the same cells as the true one wherever the block count equals the party count; such a mutation must die at the
smallest grid-row shape (by elements) at which it is a different kernel, which visible() decides from the shape alone, never from the
outputs.  The in-thread form runs k_beaver_finalize and k_fpmul_middle only, so there every mutation must die that changes one of
those two calls for the field (Goldilocks has no fpmul_middle, hence no in-thread add)."""
import random

import pytest

from oracle import spec as S
from oracle import spec_gl
from tests import elem_inputs as X
from tests import elem_model as M

SPEC = {"fr": S, "goldilocks": spec_gl.S}
IN_THREAD_CALLS = ("beaver_finalize", "fpmul_middle")
INDEXING = ("ex_party0", "public_by_ip", "rbits_m_major", "paired_pair_major")


def shapes_of(call):
    return X.GRID_SHAPES + (X.IN_THREAD_SHAPES if call in IN_THREAD_CALLS else [])


# ---- site coverage --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("call", X.CALLS)
def test_site_coverage(call):
    missing, claimed = [], 0
    for field in X.fields_of(call):
        for prm in X.params_of(call):
            for N, parties in shapes_of(call):
                c = X.case(call, field, N, parties, prm)
                assert c.period % 2 == 1 and c.period <= 255, "an odd period that the two-block shapes hold whole"
                assert c.claims() == (N >= 255)
                if c.claims():
                    claimed += 1
                    missing += [(field, N, parties, prm) + pair for pair in X.missing_pairs(c)]
    assert claimed and missing == []


@pytest.mark.parametrize("call", X.CALLS)
def test_parties_and_elements_differ(call):
    """the per-party arrays differ from party to party and the public operands from element to element: what the indexing mutants need"""
    for field in X.fields_of(call):
        for prm in X.params_of(call):
            c = X.case(call, field, 513, 5, prm)
            for nm, a in c.base.items():
                if nm in X.PUBLIC:                # every edge value (but perhaps zero) and few equal neighbours
                    assert len(set(a)) >= len(X.FLD[field].edge) - 1, (call, nm)
                    assert sum(a[i] == a[i - 1] for i in range(len(a))) * 4 < len(a), (call, nm)
                elif c.parties > 1 and a[0] != []:
                    assert all(a[p] != a[q] for p in range(c.parties) for q in range(p)), (call, nm)


# ---- mutants --------------------------------------------------------------------------------------------------------------------------------
def visible(mut, N, parties):
    """is the mutated kernel a different kernel at this shape?  (from the shape alone)"""
    if mut in INDEXING:
        return parties > 1
    if mut == "remap_swapped":
        return M._written(N, parties, mut) != M._written(N, parties, None)
    return True


def killed(mut, field, N, parties, calls, elems=None):
    """the (call, prm) whose mutated outputs differ from the true ones"""
    out = []
    for call in calls:
        if field not in X.fields_of(call):
            continue
        for prm in X.params_of(call):
            c = X.case(call, field, N, parties, prm)
            ins = c.arrays(tiled=elems is not None)
            if X.run_model(c, ins, None, N, elems) != X.run_model(c, ins, mut, N, elems):
                out.append((call, prm))
    return out


@pytest.mark.parametrize("mut", M.MUTATIONS)
def test_mutant_dies_at_the_smallest_shape(mut):
    for field in ("fr", "goldilocks"):
        if not M.applies(mut, field):
            continue
        shape = min((s for s in X.GRID_SHAPES if visible(mut, *s)), key=lambda s: s[0] * s[1])
        if mut not in INDEXING and mut != "remap_swapped":
            assert shape == (1, 1)
        assert killed(mut, field, *shape, M.MUTATION_CALLS[mut]), (mut, field, shape)


@pytest.mark.parametrize("mut", M.MUTATIONS)
def test_mutant_dies_in_every_call_it_changes(mut):
    """at the shape with the most blocks and parties that do not divide them, every call the mutation changes tells it apart (for some
    parameter set of the call: a mask mutation cannot show at every m)"""
    for field in ("fr", "goldilocks"):
        if not M.applies(mut, field):
            continue
        for call in M.MUTATION_CALLS[mut]:
            if field in X.fields_of(call):
                assert killed(mut, field, 513, 5, [call]), (mut, field, call)


@pytest.mark.parametrize("mut", M.MUTATIONS)
def test_mutant_dies_in_the_in_thread_form(mut):
    N, parties = 65536, 3
    for field in ("fr", "goldilocks"):
        calls = [c for c in M.MUTATION_CALLS[mut] if c in IN_THREAD_CALLS and field in X.fields_of(c)]
        if not M.applies(mut, field) or not calls:
            continue
        period = max(X.case(c, field, N, parties, X.params_of(c)[0]).period for c in calls)
        elems = list(range(2 * period)) + list(range(N - 2 * period, N))
        assert killed(mut, field, N, parties, calls, elems), (mut, field)


def test_every_mutation_is_listed_once():
    assert len(set(M.MUTATIONS)) == len(M.MUTATIONS) == 28
    for field in ("fr", "goldilocks"):
        assert [m for m in M.MUTATIONS if M.applies(m, field)]
    assert sum(M.applies(m, "goldilocks") for m in M.MUTATIONS) == 13


# ---- the model against the specification ----------------------------------------------------------------------------------------------------
def rand_elems(field, seed, count):
    rng, q = random.Random(seed), M.MOD[field]
    return [rng.randrange(q) for _ in range(count)]


def sh(spec, vals):
    return [spec.Share(v, 1, 1) for v in vals]


@pytest.mark.parametrize("field", ("fr", "goldilocks"))
def test_model_equals_spec(field):
    sp, q, n = SPEC[field], M.MOD[field], 200
    assert sp.R_MOD == q
    a, b, c, x, y, d, e = (rand_elems(field, 100 + i, n) for i in range(7))
    A, B, C_, X_, Y = (sh(sp, v) for v in (a, b, c, x, y))
    vals = lambda shares: [s.v for s in shares]      # noqa: E731
    assert M.fr_op(field, "add", a, b) == vals(map(sp.share_add, A, B))
    assert M.fr_op(field, "sub", a, b) == vals(map(sp.share_sub, A, B))
    assert M.fr_op(field, "mul", a, b) == vals(map(sp.share_mul, A, B))
    s = e[0]
    assert M.fr_op_scalar(field, "add", a, s) == [sp.share_add_scalar(v, s).v for v in A]
    assert M.fr_op_scalar(field, "sub", a, s) == [sp.share_sub_scalar(v, s).v for v in A]
    assert M.fr_op_scalar(field, "mul", a, s) == [sp.share_mul_scalar(v, s).v for v in A]
    assert M.fr_op_scalar(field, "rsub", a, s) == [sp.share_from_scalar_sub(s, v).v for v in A]
    assert M.triple_local(field, a, b, c) == vals(map(sp.triple_local, A, B, [sp.Share(v, 1, 2) for v in c]))
    assert M.triple_finalize(field, a, d) == [sp.triple_finalize(v, o).v for v, o in zip(A, d)]
    assert M.triple_finalize_parties(field, [a, b], d) == [[sp.triple_finalize(v, o).v for v, o in zip(row, d)] for row in (A, B)]
    want = [sp.beaver_open_shares(*t) for t in zip(A, B, X_, Y)]
    assert M.beaver_open_shares(field, a, b, x, y) == ([w[0].v for w in want], [w[1].v for w in want])
    assert M.beaver_open_shares_paired(field, [a, b], [b, c], [x, y], [y, x]) == [
        [[sp.share_sub(p, q_).v for p, q_ in zip(u, v)] for u, v in pair] for pair in (((A, X_), (B, Y)), ((B, Y), (C_, X_)))]
    z = [sp.beaver_finalize(*t).v for t in zip(C_, X_, Y, d, e)]
    assert M.beaver_finalize(field, c, x, y, d, e) == z
    assert M.beaver_finalize_parties(field, [c, a], [x, b], [y, x], d, e) == [z, [sp.beaver_finalize(*t).v for t in zip(A, B, X_, d, e)]]


def test_model_equals_spec_truncpr():
    n = 200
    a, rd, ri, cop = (rand_elems("fr", 200 + i, n) for i in range(4))
    A, RD, RI = (sh(S, v) for v in (a, rd, ri))
    for m in sorted(set(X.RDASH_M) | {2, 5}):
        bits = [rand_elems("fr", 300 + 7 * m + j, n) for j in range(m)]
        want = [S.truncpr_rdash([S.Share(bits[j][i], 1, 1) for j in range(m)], m, 1, 1).v for i in range(n)]
        assert M.truncpr_rdash(bits, m, n) == want
        assert M.truncpr_rdash_parties([bits, bits[::-1]], m, n)[0] == want
    for k, m in X.OPEN_KM + [(k, 13) for k in X.K_VALUES]:
        assert M.truncpr_open_share(a, rd, ri, k, m) == [S.truncpr_open_share(*t, k, m).v for t in zip(A, RD, RI)]
    for m in tuple(X.FINALIZE_M) + (0, 1, 8, 248, 4096):
        edge = list(X.FLD["fr"].edge) + [((1 << m) + s) % S.R_MOD for s in (-1, 0, 1)]
        assert [M.mod_pow_2(v, m) % S.R_MOD for v in cop + edge] == [S.mod_pow_2_from_field(v, m) for v in cop + edge]
        assert M.truncpr_finalize(a, rd, cop, m) == [S.truncpr_finalize(*t, m).v for t in zip(A, RD, cop)]
    k, m = 32, 13
    c, x, y, d, e = (rand_elems("fr", 400 + i, n) for i in range(5))
    bits = [rand_elems("fr", 500 + j, n) for j in range(m)]
    z, r1, op = M.fpmul_middle([c], [x], [y], d, e, [bits], [ri], k, m)
    assert z[0] == [S.beaver_finalize(*t).v for t in zip(sh(S, c), sh(S, x), sh(S, y), d, e)]
    assert r1[0] == M.truncpr_rdash(bits, m, n) and op[0] == M.truncpr_open_share(z[0], r1[0], ri, k, m)


@pytest.mark.parametrize("field", ("fr", "goldilocks"))
def test_word_add_and_sub_are_the_field_operations(field):
    q = M.MOD[field]
    pairs = X.add_pairs(field) + X.sub_pairs(field) + list(zip(rand_elems(field, 1, 300), rand_elems(field, 2, 300)))
    for a, b in pairs:
        assert 0 <= a < q and 0 <= b < q
        assert M.add_mod(field, a, b) == (a + b) % q and M.sub_mod(field, a, b) == (a - b) % q


def test_tiled_expectation_is_the_model_of_the_whole_shape():
    """element i of a shape is column i % C: the tiled expectation of the GPU tests equals the model run on all N elements"""
    for call, prm in (("triple_finalize", {}), ("beaver_open_shares_paired", {}), ("truncpr_rdash", {"m": 7}), ("truncpr_finalize", {"m": 33}),
                      ("fpmul_middle", {"k": 32, "m": 7})):
        c = X.case(call, "fr", 257, 2, prm)
        tile = lambda a: [tile(r) for r in a] if isinstance(a[0], list) else [a[i % c.C] for i in range(c.N)]      # noqa: E731
        assert {k: tile(v) for k, v in X.expected(c).items()} == X.run_model(c, c.arrays(), None, c.N)
