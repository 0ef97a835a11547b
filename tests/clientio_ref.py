"""Input and Output restated (honeybadger/input/input.rs:489-506, 85-100, 300-301; honeybadger/output/output.rs:157-177) for the
tests, in Python big integers over both fields, on the oracle's recover_secret -- never on the library.

Input: the client opens one mask per value with RobustShare::recover_secret(shares, n, t) from the S servers that answered,
broadcasts masked = x + mask, and server p keeps masked - r_p.  Output: the client opens the result shares the same way.

The reference aborts at the first element that does not open (`?`).  The device calls run on: they report that element in its
status byte and in the summary, and -- the rule this model pins down -- REFUSE it: its mask, its masked value and every party's
share are zero, never x + 0, which would be the client's value in the clear.  `rc` is what the reference returns.

status per element: 0 the lowest 2t + 1 senders agree (optimistic pass), 1 an OEC round over all S repaired it (fallback), else
recover_secret's error code (8: DecodingError)."""
from __future__ import annotations

import numpy as np

from oracle import cref as O
from oracle import cref_gl as OG
from oracle import spec as S

PRIME = {"fr": S.R_MOD, "goldilocks": OG.P}
DECODING_ERROR = 8


# ---- element arrays <-> python ints -------------------------------------------------------------------------------------
def to_ints(arr, field):
    arr = np.asarray(arr, dtype=np.uint64)
    if field == "goldilocks":
        return [int(v) for v in arr.reshape(-1)]
    f = arr.reshape(-1, 4)
    return [int(r[0]) | (int(r[1]) << 64) | (int(r[2]) << 128) | (int(r[3]) << 192) for r in f]


def from_ints(vals, field):
    if field == "goldilocks":
        return np.array([int(v) for v in vals], dtype=np.uint64)
    out = np.zeros((len(vals), 4), dtype=np.uint64)
    for i, v in enumerate(vals):
        for k in range(4):
            out[i, k] = (v >> (64 * k)) & 0xFFFFFFFFFFFFFFFF
    return out


def rows_to_ints(arr, field):
    """[party][N] elements -> a list of N-lists"""
    return [to_ints(row, field) for row in np.asarray(arr, dtype=np.uint64)]


def rows_from_ints(rows, field):
    return np.stack([from_ints(row, field) for row in rows])


def _oracle(field):
    return O if field == "fr" else OG


def open_element(field, ids, vals, n, t):
    """RobustShare::recover_secret(shares, n, t) of one element from the shares `vals` of the parties `ids` (arrival order; every
    share has degree t): (status, P(0)).  It sorts by id, tries the optimistic pass on the lowest 2t + 1 and then OEC over all S;
    which of the two succeeded is told apart by asking the oracle again with the lowest 2t + 1 alone (no OEC round there)."""
    orc = _oracle(field)
    rc, _, sec = orc.recover_secret(list(ids), [t] * len(ids), from_ints(vals, field), n, t)
    if rc != 0:
        return rc, 0
    secret = to_ints(sec, field)[0]
    if len(ids) == 2 * t + 1:
        return 0, secret
    low = sorted(range(len(ids)), key=lambda i: ids[i])[:2 * t + 1]
    rc2, _, sec2 = orc.recover_secret([ids[i] for i in low], [t] * len(low), from_ints([vals[i] for i in low], field), n, t)
    if rc2 == 0:
        assert to_ints(sec2, field)[0] == secret
        return 0, secret
    return 1, secret


def _summary(status):
    """n_failed, first_failed, first_error as the device summary reports them (its first word is not compared)"""
    bad = [g for g, s in enumerate(status) if s > 1]
    return [len(bad), bad[0] if bad else 0xffffffff, status[bad[0]] if bad else 0]


def output_model(field, ids, sh, n, t):
    """sh: [party][N] ints.  {"out": [N], "status": [N], "summary": [3], "rc": the reference's result (the first error, or 0)}.
    An element that does not open reads zero in `out`, as the decode leaves it."""
    N = len(sh[0])
    out, status = [], []
    for g in range(N):
        st, v = open_element(field, ids, [sh[p][g] for p in ids], n, t)
        status.append(st)
        out.append(v if st < 2 else 0)
    bad = [s for s in status if s > 1]
    return {"out": out, "status": status, "summary": _summary(status), "rc": bad[0] if bad else 0}


def input_model(field, ids, x, r_sh, n, t):
    """x: [N] ints, r_sh: [party][N] ints.  {"mask", "masked": [N], "in_sh": [party][N], "status", "summary", "rc"}.
    THE FAILURE RULE: element g is opened iff status[g] < 2; one that is not has mask = masked = 0 and in_sh[p][g] = 0 for every p."""
    q = PRIME[field]
    op = output_model(field, ids, r_sh, n, t)
    N = len(x)
    mask, masked, in_sh = op["out"], [], [[0] * N for _ in range(n)]
    for g in range(N):
        ok = op["status"][g] < 2
        masked.append((x[g] + mask[g]) % q if ok else 0)
        for p in range(n):
            in_sh[p][g] = (masked[g] - r_sh[p][g]) % q if ok else 0
    return {"mask": mask, "masked": masked, "in_sh": in_sh, "status": op["status"], "summary": op["summary"], "rc": op["rc"]}
