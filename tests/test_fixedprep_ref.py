"""tests/fixedprep_ref.py checked on the CPU: the sizing arithmetic against the issue's table and against the rounding rules stated
one by one, the parties' pool shares open to bits, the Fr, Goldilocks and GF(2^8) bit of an element agree, the restatement's take of
element i is the reference's drain(0..f) order, and the chain takes from the front of every list."""
import pytest

from tests import fixedprep_ref as FR
from tests import prandbit_ref as PR

SHAPES = [(4, 1, 4, 3), (7, 2, 16, 5), (10, 3, 8, 4)]


@pytest.fixture(scope="module", params=SHAPES, ids=lambda s: "n%d_t%d_%d_%d" % s)
def run(request):
    shape = request.param
    return shape, FR.fixedprep(*shape, FR.inputs(*shape))


def test_sizing_table():
    table = {(7, 2, 16): (18, 20, 20, 7), (4, 1, 16): (16, 18, 26, 9), (16, 5, 16): (18, 22, 11, 4),
             (4, 1, 1): (2, 3, 4, 2),        # R = 2, T = 3, ceil(8 / 2), ceil(3 / 2)
             (4, 1, 2): (2, 3, 4, 2),
             (4, 1, 6): (6, 6, 9, 3),        # already a multiple of t + 1 = 2 and of 2t + 1 = 3: nothing is rounded
             (7, 2, 15): (15, 15, 15, 5)}    # ... of 3 and of 5
    for (n, t, nb), want in table.items():
        assert FR.sizes(n, t, nb) == want, (n, t, nb)


def test_sizing_rules():
    for n, t in ((4, 1), (5, 1), (7, 2), (10, 3), (13, 4), (16, 5)):
        for nb in list(range(1, 70)) + [1 << 16, (1 << 16) + 1]:
            R, T, K1, K2 = FR.sizes(n, t, nb)
            assert R % (t + 1) == 0 and nb <= R < nb + t + 1
            assert T % (2 * t + 1) == 0 and R <= T < R + 2 * t + 1
            assert (n - 2 * t) * (K1 - 1) < R + 2 * T <= (n - 2 * t) * K1
            assert (t + 1) * (K2 - 1) < T <= (t + 1) * K2


def test_pool_shares_open_to_bits_and_the_three_fields_agree(run):
    (n, t, nb, ni), m = run
    R = m["sizes"][0]
    fr_bits, gf_bits = PR.recovered_bits(n, t, m["prandbit"])
    gl_bits = FR.open_honest(m["randbit"]["out"], n, t)
    assert len(fr_bits) == R and set(fr_bits) <= {0, 1}
    assert fr_bits == gf_bits == gl_bits
    # the pools are the PRandBit part's outputs, every party's row; the integers are shared with degree t
    assert m["r_bits"] == m["prandbit"]["b_p"] and m["r_bits2"] == m["prandbit"]["b_2"] and m["r_int"] == m["prandint"]["r_p"]
    xs = [PR.domain_element(PR.P_FR, n, j) for j in range(n)]
    for i in range(ni):
        lo = PR.lagrange_at_zero(PR.P_FR, xs[:t + 1], [m["r_int"][j][i] for j in range(t + 1)])
        hi = PR.lagrange_at_zero(PR.P_FR, xs[n - t - 1:], [m["r_int"][j][i] for j in range(n - t - 1, n)])
        assert lo == hi == sum(m["prandint"]["sums"][k][i] for k in range(len(m["prandint"]["sums"]))) % PR.P_FR


def test_takes_are_from_the_front(run):
    (n, t, nb, ni), m = run
    R, T, K1, K2 = m["sizes"]
    for p in range(n):
        lst = m["ransha"]["out"][p]
        assert len(lst) == (n - 2 * t) * K1 >= R + 2 * T
        assert m["randbit"]["a"][p] == lst[:R] and m["triplegen"]["a"][p] == lst[R:R + T] and m["triplegen"]["b"][p] == lst[R + T:R + 2 * T]
        assert m["triplegen"]["rt"][p] == m["randousha"]["out_t"][p][:T] and m["triplegen"]["r2t"][p] == m["randousha"]["out_2t"][p][:T]
        assert m["randbit"]["tc"][p] == m["triplegen"]["c"][p][:R] and m["prandbit"]["b_q"][p] == m["randbit"]["out"][p]
    # the triples are triples
    a, b, c = (FR.open_honest(m["triplegen"][k], n, t) for k in ("a", "b", "c"))
    assert c == [x * y % FR.Q for x, y in zip(a, b)]


def test_the_take_is_the_drain_order():
    """mod.rs:1036-1040: `for _ in 0..N { r_bits.drain(0..f) ... }` -- a list as the pool, drained as the reference drains it"""
    m, N, cursor = 4, 3, 5
    pool = list(range(100, 140))
    ints = list(range(500, 520))
    queue = pool[cursor:]
    drained = [[queue.pop(0) for _ in range(m)] for _ in range(N)]            # element i's bits, in order
    rbits, rint = FR.pool_take(pool, ints, cursor, 2, m, N)
    assert [[rbits[j][i] for j in range(m)] for i in range(N)] == drained and rint == ints[2:2 + N]
    # and the device's take of the same slice (group = m) is that regrouping
    import numpy as np
    src = np.array(pool, dtype=np.uint64)
    got = FR.take_rows(src[cursor:], 1, len(pool), np.zeros(m * N, dtype=np.uint64), m * N, m * N, m)
    assert got.reshape(m, N).tolist() == rbits
