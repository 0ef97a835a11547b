"""The model of hbmpc_[gl_]dev_batchrecon_parties (tests/batchrecon_ref.py) checked against itself and against the model of RandBit's
opens (open_model of tests/test_gpu_randbit_parties.py) where both apply: d = t and senders 0 .. 2t.  No GPU work, but it guards the
GPU tests' reference.  The pinned cases: exact sender sets open honest inputs with every status 0; the lie with a root at recipient j
fails every other recipient and the chunk (exact sets) or is repaired everywhere (all n senders)."""
import pytest

from tests import batchrecon_ref as BR

SHAPES = [(4, 1, 1), (5, 1, 2), (7, 2, 2), (7, 2, 4), (10, 3, 3), (16, 5, 5), (16, 5, 10)]
OK = (0, 0, BR.NONE, 0)


def sets_of(n, t, d):
    S = d + t + 1
    return tuple(range(S)), tuple(range(n - S, n))


@pytest.mark.parametrize("n,t,d", SHAPES)
def test_exact_sets_open_honest_inputs(n, t, d):
    G = 2
    secrets, x = BR.honest("fr", n, t, d, G)
    for ids in sets_of(n, t, d):
        m = BR.model("fr", n, t, d, x, ids, ids[::-1])
        assert m["opened"] == secrets
        assert not any(m["rstatus"]) and not any(m["status"]) and m["summary_first"] == OK and m["summary"] == OK
        q = BR.PRIME["fr"]
        al = [BR.SPEC["fr"].domain_element(n, j) for j in range(n)]
        for j in range(n):  # z_j is the chunk's polynomial of secrets at recipient j's point
            assert m["Z"][j] == [sum(pow(al[j], k, q) * secrets[g * (d + 1) + k] for k in range(d + 1)) % q for g in range(G)]


def test_goldilocks_opens_honest_inputs():
    for n, t, d in ((4, 1, 1), (7, 2, 4)):
        secrets, x = BR.honest("goldilocks", n, t, d, 2)
        m = BR.model("goldilocks", n, t, d, x, *sets_of(n, t, d))
        assert m["opened"] == secrets and not any(m["rstatus"]) and not any(m["status"])


@pytest.mark.parametrize("n,t,d", SHAPES)
def test_lie_with_exact_sets(n, t, d):
    """party 1 lies to everyone but recipient j: rstatus 8 at every recipient except j, chunk status 8 and zeros; the neighbouring chunk
    stays intact"""
    G, g, j = 3, 1, 2
    secrets, x = BR.honest("fr", n, t, d, G)
    ids = sets_of(n, t, d)[0]
    assert 1 in ids and j in ids
    m = BR.model("fr", n, t, d, BR.lie("fr", x, n, d, g, j), ids, ids)
    M = d + 1
    for r in range(n):
        assert m["rstatus"][r * G + g] == (0 if r == j else 8), r
        assert m["rstatus"][r * G] == 0 and m["rstatus"][r * G + 2] == 0
        assert m["Z"][r][g] == 0 or r == j
    assert m["status"] == [0, 8, 0]
    assert m["opened"] == secrets[:M] + [0] * M + secrets[2 * M:]
    assert m["summary_first"] == (n - 1, n - 1, g if j else G + g, 8) and m["summary"] == (1, 1, g, 8)


@pytest.mark.parametrize("n,t,d", [s for s in SHAPES if s[0] > s[1] + s[2] + 1])
def test_lie_with_all_senders(n, t, d):
    """the same lie with all n senders: the fallback repairs every recipient (rstatus 1 at the others, 0 at j) and the secrets open"""
    G, g, j = 3, 1, 2
    secrets, x = BR.honest("fr", n, t, d, G)
    ids = tuple(range(n))
    m = BR.model("fr", n, t, d, BR.lie("fr", x, n, d, g, j), ids, ids)
    for r in range(n):
        assert m["rstatus"][r * G + g] == (0 if r == j else 1), r
    assert m["status"] == [0, 0, 0] and m["opened"] == secrets
    assert m["summary_first"] == (n - 1, 0, BR.NONE, 0) and m["summary"] == OK


def test_lie_outside_the_eval_senders_changes_only_y():
    n, t, d, G = 7, 2, 2, 2
    secrets, x = BR.honest("fr", n, t, d, G)
    ids = tuple(range(n - (d + t + 1), n))  # party 1 is not among them
    assert 1 not in ids
    a, b = BR.model("fr", n, t, d, x, ids, ids), BR.model("fr", n, t, d, BR.lie("fr", x, n, d, 0, 3), ids, ids)
    assert a["Y"] != b["Y"] and a["Y"][0] == b["Y"][0]
    for k in ("Z", "opened", "rstatus", "status", "summary_first", "summary"):
        assert a[k] == b[k], k


def test_agrees_with_the_model_of_randbits_opens():
    """d = t and prefix senders 0 .. 2t: open_model of tests/test_gpu_randbit_parties.py is the same call (it folds both status arrays
    into one buffer, recipient 0's bytes rewritten by the second decode)"""
    from tests import test_gpu_randbit_parties as RBP
    for field, n, t in (("fr", 4, 1), ("goldilocks", 7, 2), ("fr", 10, 3)):
        G = 3
        secrets, x = BR.honest(field, n, t, t, G)
        for xs in (x, BR.lie(field, x, n, t, 1, 2)):
            ids = tuple(range(2 * t + 1))
            m = BR.model(field, n, t, t, xs, ids, ids)
            opened, rst, s1, s2 = RBP.open_model(field, n, t, xs)
            assert m["opened"] == opened and m["summary_first"] == s1 and m["summary"] == s2
            assert m["status"] == rst[:G] and m["rstatus"][G:] == rst[G:]
