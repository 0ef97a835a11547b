"""tests/sender_sets.py without a GPU and without the library: on the inputs the GPU tests use, the right open from a sender set
differs AT EVERY CHUNK, in value or in status, from the two wrong ones a library could make --

  wrong reading   rows 0 .. S - 1 of the [party][..] arrays decoded as the shares of `ids` (what FpMul's five-launch form did)
  prefix table    the senders' own rows decoded with the ids 0 .. S - 1 (a kernel with the prefix's table, or one that ignores the ids)

-- a sender that lies fails exactly its chunks from 2t + 1 senders, is repaired from 2t + 2, and a wrong share outside the set
changes nothing the open produces.  So a GPU test that passes on these inputs has read the right rows with the right table.

Outcome per set (chunks that differ from the right open / chunks there are; first open: 2 N chunks, second: N):

  (n, t)     S   N   wrong reading       prefix table        liars: first open   second open   from 2t + 2 senders
                     first     second    first     second
  (7, 2)     5   32  64/64     32/32     64/64     32/32     3, N + 5 fail       7, 9 fail
  (7, 2)     5   33  66/66     33/33     66/66     33/33     3, N + 5 fail       7, 9 fail
  (7, 2)     6   32  64/64     32/32     64/64     32/32     -                   -             3, N + 5, 7, 9 repaired
  (16, 5)   11   32  64/64     32/32     64/64     32/32     3, N + 5 fail       7, 9 fail
  (31, 10)  21   32  64/64     32/32     64/64     32/32     3, N + 5 fail       7, 9 fail
  (40, 13)  27   32  64/64     32/32     64/64     32/32     3, N + 5 fail       7, 9 fail

Every wrong open is a failed verification (status 8, value zero) at every chunk: the shares are uniform, so 2t + 1 points that are
not on one polynomial of degree t pass a verify row with probability 1 / r.  TruncPr / FPDivConst at (7, 2) (S = 5, 6) and (16, 5),
N = 20, whose arrays hold row s = sender_ids[s]'s share: 20/20 for the prefix's table, for sorted ids over unsorted rows and for
FpMul's party-id convention applied to that layout; liars at elements 3 and 7 (fail from 2t + 1 senders, repaired from 2t + 2).
"""
import numpy as np
import pytest

from oracle import cref as O
from tests import sender_sets as SS
from tests import test_gpu_truncpr as T

K, M = SS.K_BITS, SS.M_BITS
# (n, t, S, N): what tests/test_gpu_sender_sets.py runs
FPMUL_CASES = [(7, 2, 5, 32), (7, 2, 5, 33), (7, 2, 6, 32), (16, 5, 11, 32), (31, 10, 21, 32), (40, 13, 27, 32)]


def test_the_sets():
    """the issue's sets, literally; each is unsorted, holds party n - 1 and an id >= S and leaves out a low party"""
    assert SS.sender_set(7, 2) == (6, 1, 3, 0, 4) and SS.sender_set(7, 2, 6) == (6, 1, 3, 0, 4, 5)
    assert SS.sender_set(16, 5) == (15, 2, 3, 4, 5, 6, 7, 8, 9, 10, 0)
    assert SS.sender_set(31, 10) == (30,) + tuple(range(2, 21)) + (0,) and len(SS.sender_set(31, 10)) == 21
    assert SS.sender_set(40, 13) == (39,) + tuple(range(2, 27)) + (0,) and len(SS.sender_set(40, 13)) == 27
    for (n, t), by_size in SS.SETS.items():
        for S, ids in by_size.items():
            assert SS.sender_set(n, t, S) == ids and len(ids) == S
            ver, low = SS.liars(ids, t)
            assert (ver == n - 1 and ver >= S if S == 2 * t + 1 else ver == sorted(ids)[2 * t]) and low in ids and low != min(ids)
            assert SS.outsiders(n, ids)[0] < S


def differs_everywhere(ids, rows, n, t, right, right_status):
    """this decode's (value, status) differs from the right one's at every chunk; returns how many chunks that is"""
    rc, val, st = O.batch_recover_p0(list(ids), np.ascontiguousarray(rows), n, t, t)
    assert rc in (0, 8)
    diff = [bool(st[g] != right_status[g] or not np.array_equal(val[g], right[g])) for g in range(len(right))]
    assert all(diff), [g for g, d in enumerate(diff) if not d]
    return len(diff)


def beaver_shares(ins, n):
    """[party][2 N]: every party's shares of a - x, then of b - y"""
    rows = []
    for p in range(n):
        rc, d_sh, e_sh = O.beaver_open_shares(ins["ta"][p], ins["tb"][p], ins["x"][p], ins["y"][p])
        assert rc == 0
        rows.append(np.concatenate([d_sh, e_sh]))
    return np.stack(rows)


def open_from_all(shares, n, t):
    rc, p0, st = O.batch_recover_p0(list(range(n)), np.ascontiguousarray(shares), n, t, t)
    assert rc == 0 and not st.any()
    return p0


@pytest.mark.parametrize("n,t,S,N", FPMUL_CASES)
def test_fpmul_sets_discriminate(n, t, S, N):
    ids = SS.sender_set(n, t, S)
    ins = SS.fpmul_inputs(n, t, N)
    right = SS.fpmul_expected(ins, n, t, N, K, M, ids)
    assert not right["status_first"].any() and not right["status"].any()
    assert right["summary_first"] == right["summary"] == [0, 0xffffffff, 0]
    desh, osh = beaver_shares(ins, n), right["osh"]
    # the right open is THE open: what all n parties' shares give
    assert np.array_equal(np.concatenate([right["dop"], right["eop"]]), open_from_all(desh, n, t)) and np.array_equal(right["cop"], open_from_all(osh, n, t))
    de = np.concatenate([right["dop"], right["eop"]])
    prefix = list(range(S))
    # the wrong reading and the prefix's table, for both opens
    assert differs_everywhere(ids, desh[:S], n, t, de, right["status_first"]) == 2 * N
    assert differs_everywhere(ids, osh[:S], n, t, right["cop"], right["status"][:N]) == N
    assert differs_everywhere(prefix, desh[list(ids)], n, t, de, right["status_first"]) == 2 * N
    assert differs_everywhere(prefix, osh[list(ids)], n, t, right["cop"], right["status"][:N]) == N
    # ... and the sorted ids with unsorted rows (a call that sorted the ids and forgot the rows)
    assert differs_everywhere(sorted(ids), desh[list(ids)], n, t, de, right["status_first"]) > 0

    # the outsider: every element of x, ta and r_int wrong at a party outside the set -- the opens do not move
    out = SS.fpmul_expected(SS.with_wrong_outsider(ins, n, ids, ("x", "ta", "rint")), n, t, N, K, M, ids)
    for nm in ("dop", "eop", "cop", "status", "status_first"):
        assert np.array_equal(out[nm], right[nm]), nm
    assert not np.array_equal(out["z"], right["z"])                                # (its own rows of course differ)

    lied, first, second = SS.fpmul_with_liars(ins, ids, t, N)
    got = SS.fpmul_expected(lied, n, t, N, K, M, ids)
    bad_first, bad_second = np.flatnonzero(got["status_first"]).tolist(), np.flatnonzero(got["status"][:N]).tolist()
    assert bad_first == first and bad_second == second
    de_got = np.concatenate([got["dop"], got["eop"]])
    if S == 2 * t + 1:                                                              # no OEC round: exactly those fail, to zero
        assert set(got["status_first"][first]) == {8} and set(got["status"][second]) == {8}
        assert not de_got[first].any() and not got["cop"][second].any()
        assert got["summary_first"] == [2, first[0], 8] and got["summary"] == [2, second[0], 8]
        keep = [g for g in range(N) if g not in (3, 5) + tuple(second)]             # elements behind a failed first open run on its zero
        assert np.array_equal(got["cop"][keep], right["cop"][keep]) and not np.array_equal(got["cop"][3], right["cop"][3])
    else:                                                                           # one sender to spare: repaired
        assert set(got["status_first"][first]) == {1} and set(got["status"][second]) == {1}
        assert np.array_equal(de_got, de) and np.array_equal(got["cop"], right["cop"])
        assert got["summary_first"] == got["summary"] == [0, 0xffffffff, 0]


TRUNCPR_N = 20


@pytest.mark.parametrize("with_w", [False, True], ids=["truncpr", "fpdivconst"])
@pytest.mark.parametrize("n,t,S", [(7, 2, 5), (7, 2, 6), (16, 5, 11)])
def test_truncpr_sets_discriminate(n, t, S, with_w):
    """TruncPr's arrays hold row s = sender_ids[s]'s share; here they are indexed by party and T.expected(.., ids) takes the senders' rows"""
    ids, N, k, m = SS.sender_set(n, t, S), TRUNCPR_N, 32, 8
    clean = T.random_inputs(n, t, N, m, 9000 + n + S, with_w)
    ins = SS.with_wrong_outsider(clean, n, ids, ("a", "rint"), every=True)         # what the GPU test lays out: the outsiders' rows are wrong
    right = T.expected(ins, n, t, N, k, m, ids)
    assert right["rc"] == 0 and not right["status"].any()                           # ... and change nothing:
    assert np.array_equal(right["cop"], open_from_all(T.expected(clean, n, t, N, k, m, n)["osh"], n, t))
    osh, perm = right["osh"], list(ids) + SS.outsiders(n, ids)
    assert differs_everywhere(list(range(S)), osh[list(ids)], n, t, right["cop"], right["status"]) == N           # the prefix's table
    assert differs_everywhere(sorted(ids), osh[list(ids)], n, t, right["cop"], right["status"]) == N              # ids sorted, rows not
    assert differs_everywhere(ids, osh[[perm[i] for i in ids]], n, t, right["cop"], right["status"]) == N         # FpMul's convention on this layout
    lied, bad = SS.truncpr_with_liars(ins, ids, t)
    got = T.expected(lied, n, t, N, k, m, ids)
    assert np.flatnonzero(got["status"]).tolist() == bad
    if S == 2 * t + 1:
        assert got["rc"] == 8 and set(got["status"][bad]) == {8} and not got["cop"][bad].any()
    else:
        assert got["rc"] == 0 and set(got["status"][bad]) == {1} and np.array_equal(got["cop"], right["cop"])


def test_expected_with_a_count_is_the_prefix():
    """T.expected's last parameter: a count means parties 0 .. count - 1, as before"""
    n, t, N, k, m = 7, 2, 9, 32, 4
    ins = T.random_inputs(n, t, N, m, 123, False)
    a, b = T.expected(ins, n, t, N, k, m, 2 * t + 1), T.expected(ins, n, t, N, k, m, list(range(2 * t + 1)))
    assert all(np.array_equal(a[nm], b[nm]) for nm in ("rdash", "osh", "cop", "out", "status")) and a["rc"] == b["rc"] == 0
