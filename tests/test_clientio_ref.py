"""tests/clientio_ref.py (the big-integer model of Input and Output that the GPU tests compare the library with) against the
reference's own algebra: the shares Input leaves open to the client's values; one lying server among exactly 2t + 1 refuses its
element and nothing of the client's value is written; with one server more the lie is corrected.  No library, no GPU."""
import numpy as np
import pytest

from tests import clientio_ref as R
from tests import randbit_ref as RB

SHAPES = [(4, 1), (7, 2)]
FIELDS = ["fr", "goldilocks"]
N = 5


def case(field, n, t, seed):
    """x (nonzero values) and a degree-t sharing of N uniform masks, as ints"""
    x = [v or 1 for v in R.to_ints(RB.fill_random(field, seed, N), field)]
    masks = RB.fill_random(field, seed + 1, N)
    r_sh = R.rows_to_ints(RB.share_all(field, masks, n, t, seed + 2), field)
    return x, R.to_ints(masks, field), r_sh


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("n,t", SHAPES)
def test_honest_input_shares_open_to_the_inputs(field, n, t):
    q = R.PRIME[field]
    x, masks, r_sh = case(field, n, t, 100 * n + t)
    for ids in (tuple(range(2 * t + 1)), tuple(range(n - 1, n - 2 * t - 2, -1)), tuple(range(n))):
        m = R.input_model(field, ids, x, r_sh, n, t)
        assert m["rc"] == 0 and m["status"] == [0] * N and m["summary"] == [0, 0xffffffff, 0]
        assert m["mask"] == masks and m["masked"] == [(a + b) % q for a, b in zip(x, masks)]
        for other in (tuple(range(2 * t + 1)), tuple(range(n))):                  # recover(in_sh) == x, from any 2t + 1 or from all
            o = R.output_model(field, other, m["in_sh"], n, t)
            assert o["rc"] == 0 and o["out"] == x and o["status"] == [0] * N


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("n,t", SHAPES)
def test_one_liar_is_refused_at_2t_plus_1_and_corrected_with_one_more(field, n, t):
    q = R.PRIME[field]
    x, masks, r_sh = case(field, n, t, 200 * n + t)
    g, liar = 3, 1
    honest = R.input_model(field, tuple(range(2 * t + 1)), x, r_sh, n, t)
    lied = [list(row) for row in r_sh]
    lied[liar][g] = (lied[liar][g] + 1) % q
    m = R.input_model(field, tuple(range(2 * t + 1)), x, lied, n, t)
    assert m["rc"] == R.DECODING_ERROR and m["status"][g] == R.DECODING_ERROR and m["summary"] == [1, g, R.DECODING_ERROR]
    assert m["mask"][g] == 0 and m["masked"][g] == 0 and all(m["in_sh"][p][g] == 0 for p in range(n))
    assert x[g] != 0 and m["masked"][g] != x[g]                                   # never x + 0
    for h in range(N):
        if h != g:
            assert m["status"][h] == 0 and m["masked"][h] == honest["masked"][h]
            assert all(m["in_sh"][p][h] == honest["in_sh"][p][h] for p in range(n))
    m = R.input_model(field, tuple(range(2 * t + 2)), x, lied, n, t)             # one OEC round: corrected
    assert m["rc"] == 0 and m["status"] == [1 if h == g else 0 for h in range(N)] and m["summary"] == [0, 0xffffffff, 0]
    assert m["mask"] == masks and m["masked"] == honest["masked"]
    for p in range(n):
        want = honest["in_sh"][p] if p != liar else [(honest["in_sh"][p][h] - (1 if h == g else 0)) % q for h in range(N)]
        assert m["in_sh"][p] == want                                              # the liar's own share follows its own r
    o = R.output_model(field, tuple(range(2 * t + 1)), lied, n, t)                # Output: the same open, the same refusal
    assert o["rc"] == R.DECODING_ERROR and o["out"][g] == 0 and o["status"][g] == R.DECODING_ERROR
    o = R.output_model(field, tuple(range(2 * t + 2)), lied, n, t)
    assert o["rc"] == 0 and o["out"] == masks and o["status"][g] == 1


def test_a_liar_outside_the_sender_set_changes_nothing():
    n, t, field = 7, 2, "fr"
    x, masks, r_sh = case(field, n, t, 77)
    ids = (6, 1, 3, 0, 4)
    honest = R.input_model(field, ids, x, r_sh, n, t)
    lied = [list(row) for row in r_sh]
    lied[2][0] = (lied[2][0] + 5) % R.PRIME[field]
    m = R.input_model(field, ids, x, lied, n, t)
    assert m["status"] == [0] * N and m["masked"] == honest["masked"] and m["mask"] == masks
    assert [m["in_sh"][p] for p in range(n) if p != 2] == [honest["in_sh"][p] for p in range(n) if p != 2]


def test_round_trip_of_the_array_helpers():
    for field in FIELDS:
        v = [0, 1, R.PRIME[field] - 1]
        assert R.to_ints(R.from_ints(v, field), field) == v
        assert R.rows_to_ints(R.rows_from_ints([v, v[::-1]], field), field) == [v, v[::-1]]
        assert R.rows_from_ints([v], field).dtype == np.uint64
