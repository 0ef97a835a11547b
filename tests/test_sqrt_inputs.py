"""tests/sqrt_inputs.py without a GPU and without the library: the construction gives the logs it names, the closed form the kernels
compute is ark's loop on every family value, SITE_TABLE holds for both fields (no row is waived; the rows that no input can reach are
asserted unreached), and the inverse patterns realise their slot masks for 8 and for 2 slots from the arrays alone."""
import pytest

from tests import randbit_ref as RB
from tests import sqrt_inputs as X

FIELDS = sorted(X.FIELDS)


def test_family_of_logs():
    logs = [L for _, L in X.LOGS]
    assert len(set(logs)) == len(logs)
    assert len({j << (8 * w) for w in range(4) for j in range(256)}) == 1021
    want = {j << (8 * w) for w in range(4) for j in range(256)} | set(X.NAMED)
    for i in range(32):
        want |= {1 << i, 2**32 - (1 << i), 0xFFFFFFFF ^ (1 << i)}
    for w in (1, 2, 3):                                           # a chosen upper byte over lower windows all 0x00 and all 0xFF
        for b in X.UPPER_BYTES:
            want |= {b << (8 * w), b << (8 * w) | ((1 << (8 * w)) - 1)}
    assert want <= set(logs)
    assert sum(L & 1 for L in logs) > 40                          # the non-residues stay in
    assert {2, 2**31, 0xFFFFFFFE, 0xAAAAAAAA, 0x55555554} <= set(logs)


@pytest.mark.parametrize("field", FIELDS)
def test_construction_and_closed_form(field):
    """log_of(with_log(L)) = L; closed_sqrt = ark_sqrt; root^2 = A; a root exists exactly when L is even -- on every family value"""
    p = X.FIELDS[field].mod
    fam, roots, logs = X.family(p), X.family_roots(p), X.family_logs(p)
    assert len(fam) >= 1100 + len(X.FIELDS[field].edge) - 1
    kinds = {k for _, _, k in fam}
    assert kinds == {"random", "subgroup", "edge"}
    for (A, L, kind), (root, ks), Lg in zip(fam, roots, logs):
        assert 0 <= A < p
        if A == 0:
            assert root == 0 and RB.ark_sqrt(0, p) == 0 and RB.closed_sqrt(0, p) == 0
            continue
        assert X.log_of(A, p) == Lg and (L is None or L == Lg), (kind, hex(A))
        assert RB.ark_sqrt(A, p) == root and RB.closed_sqrt(A, p) == root, (kind, hex(Lg))
        assert (root is not None) == (Lg & 1 == 0), hex(Lg)
        if root is not None:
            assert root * root % p == A
        if kind == "subgroup":                                     # a power of omega: its Montgomery form is a table entry
            assert pow(A, 1 << 32, p) == 1


@pytest.mark.parametrize("field", FIELDS)
def test_site_table(field):
    p = X.FIELDS[field].mod
    got = X.reached(p)
    for row, want in X.SITE_TABLE.items():
        missing = sorted(want - got[row], key=repr)
        assert not missing, (field, row, missing[:8], len(missing))
    for row, never in X.NEVER.items():
        assert not [v for v in got[row] if never(v)], (field, row)
    # the named members do what the table says of them
    by_log = {L: ks for (A, L, _), (root, ks) in zip(X.family(p), X.family_roots(p)) if L is not None}
    assert by_log[0] == [] and by_log[2**31] == [1] and len(by_log[2]) == 31 and by_log[2] == list(range(31, 0, -1))
    assert by_log[1] == [32] and by_log[0xFFFFFFFF] == [32]
    assert X.exps(2) == (2**31 - 1, 2**31 - 1) and X.exps(2**32 - 2) == (1, 1) and X.exps(0) == (0, 0)
    assert all((2**31 - 1 >> (8 * w)) & 255 == (255 if w < 3 else 127) for w in range(4))


def test_the_two_exponents_coincide():
    """what makes two rows unreachable: for every even L, -(L + E) = E modulo 2^32 and L + E < 2^32 (sqrt_inputs docstring)"""
    for _, L in X.LOGS:
        if not L & 1:
            E, V = X.exps(L)
            assert V == E < 2**31 and L + E < 2**32 and (2 * E + L) % 2**32 == 0


@pytest.mark.parametrize("field", FIELDS)
def test_inverse_patterns(field):
    F = X.FIELDS[field]
    vals = X.inverse_case(F, 8)
    assert len(vals) == 256 * 8 and all(0 <= v < F.mod for v in vals)
    for B in (8, 2):                                               # the masks, from the array and the layout rule alone
        got = X.lane_classes(vals, F.mod, B, F.edge)
        assert X.required_classes(B) <= got, (B, sorted(X.required_classes(B) - got, key=repr))
    assert X.slot_of(0, 8) == (0, 0, 0) and X.slot_of(256 * 8 + 257, 8) == (1, 1, 1) and X.slot_of(513, 2) == (1, 1, 0)
    for B in (8, 2):
        tails = X.inverse_tails(F, B)
        assert {N % (256 * B) for N, _ in tails} == set(X.TAIL_R(B)) and max(N for N, _ in tails) <= 4 * 256 * 8
        for N, v in tails:
            assert len(v) == N
            blk, lane, slot = X.slot_of(N - 1, B)                  # element N - 1 is its lane's last live slot
            assert len(X.lanes_of(v, B)[(blk, lane)]) == slot + 1
            last = {v[N - 1]} | ({v[N - 2]} if N > 1 else set())
            assert 0 in last and (N == 1 or last & (set(F.edge) - {0}))
        assert {v[N - 1] == 0 for N, v in tails} == {True, False}


@pytest.mark.parametrize("field", FIELDS)
def test_phase2_inputs(field):
    """the solved shares give the chosen outputs under RB.phase2; the failure layouts give the summaries they name"""
    F = X.FIELDS[field]
    p = F.mod
    which = (X.even_indices(p)[:40] + X.odd_indices(p)[:5] + [X.family_values(p).index(0)])
    sq, a, outs = X.phase2_case(F, 3, which)
    err, first, status, want = RB.phase2(sq, a, p)
    assert err == RB.ZERO_SQUARE and status.count(RB.ST_NO_ROOT) == 5 and status.count(RB.ST_ZERO) == 1
    solved = [(q, i) for q in range(3) for i in range(len(sq)) if outs[q][i] is not None]
    assert len(solved) > 60 and all(want[q][i] == outs[q][i] for q, i in solved)
    assert {outs[q][i] for q, i in solved} >= set(F.edge)        # every edge value is an output: p - 1 and p - 2 among them
    assert any(a[q][i] in F.edge and outs[q][i] is None and status[i] == 0 for q in range(3) for i in range(len(sq)))
    fv = X.family_values(p)
    for name, (idx, (first, nfail)) in X.failure_layouts(F).items():
        err, at, status, _ = RB.phase2([fv[i] for i in idx], [[1] * len(idx)], p)
        assert nfail == sum(1 for s in status if s) and (first >> 32, first & 0xFFFFFFFF) == (status[at], at), name
    lay = X.failure_layouts(F)
    assert lay["first_at_0"][1] == ((2 << 32) | 0, 1) and lay["first_at_last"][1] == ((2 << 32) | 299, 1)
    assert lay["first_in_partial_block"][1][0] == (2 << 32) | 257 and lay["zero_after_non_residues"][1] == ((1 << 32) | 270, 6)
    assert lay["only_non_residues"][1] == ((2 << 32) | 5, 4) and lay["every_element_fails"][1][1] == 300
