"""Sender sets that are no prefix 0 .. S - 1, for the calls that take sender ids (Mul, FpMul: PARTY ids; TruncPr / FPDivConst: the
ids of the rows in the decode call's order), the oracle composition of FpMul for any sender set, and the places where a wrong
share must, or must not, show.  Plain Python integers and oracle/ alone: no library, no GPU.

Every set is in a fixed, unsorted arrival order, contains party n - 1, leaves out a low party and holds at least one id >= S: a
call that read rows 0 .. S - 1, or used the table of the prefix, or sorted nothing, opens something else from it.
tests/test_sender_sets.py proves that on the very inputs the GPU tests (tests/test_gpu_sender_sets.py, tests/test_gpu_truncpr.py,
tests/test_gpu_mul.py) feed the library.
"""
import numpy as np

from oracle import cref as O
from tests import edge_inputs as X


def _spread(n, count):
    """party n - 1 first, then parties 2, 3, .. and party 0 last: party 1 is left out"""
    return (n - 1,) + tuple(range(2, count)) + (0,)


# (n, t) -> {S: ids}
SETS = {
    (7, 2): {5: (6, 1, 3, 0, 4), 6: (6, 1, 3, 0, 4, 5)},
    (16, 5): {11: _spread(16, 11)},
    (31, 10): {21: _spread(31, 21)},          # t + 1 = 11: the last size the decode's pair form takes
    (40, 13): {27: _spread(40, 27)},          # t + 1 = 14: beyond it (FpMul only)
}
K_BITS, M_BITS = 32, 6                        # TruncPr's k and m in the FpMul cases


def sender_set(n, t, S=None):
    ids = SETS[(n, t)][2 * t + 1 if S is None else S]
    assert len(ids) == len(set(ids)) and n - 1 in ids and min(set(range(n)) - set(ids)) < len(ids) <= max(ids) and list(ids) != sorted(ids)
    return ids


def outsiders(n, ids):
    return [p for p in range(n) if p not in ids]


def liars(ids, t):
    """(a sender behind a verify row, a sender behind the P(0) row): the highest of the 2t + 1 lowest senders, which the decode
    verifies first -- with S = 2t + 1 that is party n - 1, whose id is beyond every prefix -- and the second lowest sender"""
    low, ver = X.split_senders(ids, t)
    return ver[t - 1], low[1]


def summary_tail(status):
    """n_failed, first_failed, first_error of a decode that left these status bytes (1: repaired by an OEC round; a failed chunk is 8)"""
    bad = np.flatnonzero(np.asarray(status) > 1)
    return [len(bad), int(bad[0]) if len(bad) else 0xffffffff, 8 if len(bad) else 0]


def share_all(secrets, n, d, seed):
    """[n][N] degree-d sharings of N secrets (random higher coefficients), via the oracle"""
    N = secrets.shape[0]
    co = O.fill_random(seed, N * (d + 1)).reshape(N, d + 1, 4)
    co[:, 0] = secrets
    rc, sh = O.compute_shares(co, n, d)
    assert rc == 0
    return sh


_inputs = {}


def fpmul_inputs(n, t, N, m=M_BITS):
    """x, y, the triple, r_int and the m bit arrays as degree-t sharings of uniform elements (the steps are algebra); computed once
    per shape and never modified: the tampering below works on copies"""
    key = (n, t, N, m)
    if key not in _inputs:
        seed = 7000 + 100 * n + N
        ins = {nm: share_all(O.fill_random(seed + j, N), n, t, seed + 10 + j) for j, nm in enumerate(("x", "y", "ta", "tb", "tc", "rint"))}
        ins["rbits"] = np.stack([share_all(O.fill_random(seed + 20 + j, N), n, t, seed + 40 + j) for j in range(m)], axis=1)
        _inputs[key] = ins
    return _inputs[key]


def _copy(ins):
    return {nm: (v.copy() if isinstance(v, np.ndarray) else v) for nm, v in ins.items()}


def _wrong(arr, party, el=None):
    """party's share (of element el, or its whole row) replaced by its neighbour's: a valid field element on the wrong polynomial"""
    donor = (party + 1) % arr.shape[0]
    if el is None:
        assert not np.array_equal(arr[party], arr[donor])
        arr[party] = arr[donor]
    else:
        assert not np.array_equal(arr[party, ..., el, :], arr[donor, ..., el, :])
        arr[party, ..., el, :] = arr[donor, ..., el, :]


def with_wrong_outsider(ins, n, ids, names, every=False):
    """the lowest party outside the set (or every such party) holds wrong shares of every element of the named inputs"""
    out = _copy(ins)
    for nm in names:
        for p in outsiders(n, ids)[:n if every else 1]:
            _wrong(out[nm], p)
    return out


# element, input, which liar, the open it shows in (FpMul: chunk g of a - x, chunk N + g of b - y, chunk g of the second open)
FPMUL_LIES = ((3, "ta", "verify", "first"), (5, "tb", "p0", "first"), (7, "rint", "p0", "second"), (9, "rbits", "verify", "second"))


def fpmul_with_liars(ins, ids, t, N):
    """a sender behind a verify row lies about a at element 3 and about bit 0 at element 9, one behind the P(0) row about b at
    element 5 and about r_int at element 7 (one lie per chunk: an OEC round with one sender to spare repairs each).  Returns the
    inputs, the chunks of the first open [0, 2 N) and those of the second [0, N) that see a lie."""
    ver, low = liars(ids, t)
    out = _copy(ins)
    for el, nm, who, _ in FPMUL_LIES:
        _wrong(out[nm], ver if who == "verify" else low, el)
    return out, [3, N + 5], [7, 9]


TRUNCPR_LIES = (3, 7)


def truncpr_with_liars(ins, ids, t):
    """the same for TruncPr / FPDivConst, whose arrays here are indexed by PARTY (the GPU test lays them out in the call's order):
    the verify-row liar about a at element 3, the P(0)-row liar about r_int at element 7"""
    ver, low = liars(ids, t)
    out = _copy(ins)
    _wrong(out["a"], ver, TRUNCPR_LIES[0])
    _wrong(out["rint"], low, TRUNCPR_LIES[1])
    return out, list(TRUNCPR_LIES)


def fpmul_expected(ins, n, t, N, k, m, ids=None):
    """beaver_open_shares, batch_recover_p0, beaver_finalize, truncpr_rdash, the integer formula of truncpr.rs:275-297,
    batch_recover_p0 again, truncpr_finalize -- both opens from the shares of the PARTIES `ids` (default: 0 .. 2t)"""
    from tests import test_gpu_mul as M              # (here, so that those modules can import this one for the sets)
    from tests import test_gpu_truncpr as T
    ids = list(range(2 * t + 1)) if ids is None else list(ids)
    mul = M.expected(X.FR, ins, n, t, N, ids)
    tr = T.expected({"a": mul["out"], "w": None, "rbits": ins["rbits"], "rint": ins["rint"]}, n, t, N, k, m, ids)
    return {"dop": mul["deop"][:N], "eop": mul["deop"][N:], "z": mul["out"], "rdash": tr["rdash"], "osh": tr["osh"], "cop": tr["cop"], "out": tr["out"],
            "status": np.concatenate([tr["status"], mul["status"][N:]]),               # [0, N) the second open's, [N, 2 N) b - y of the first
            "status_first": mul["status"],
            "summary_first": summary_tail(mul["status"]), "summary": summary_tail(tr["status"])}
