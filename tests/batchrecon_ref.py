"""BatchReconNode restated (honeybadger/batch_recon/batch_recon.rs: init_batch_reconstruct_many :144-185, the EvalBatch arm
:371-391, the RevealBatch arm :451-467) for the tests, in Python big integers over both fields, on oracle/spec.py -- never on the
library.

The call (hbmpc_[gl_]dev_batchrecon_parties) for all n parties: party p holds x_p[N], N = G (d + 1), in chunks of d + 1 values.
  encode      y[p][j][g] = sum_k alpha_j^k x_p[g (d + 1) + k]                                          (:157-165)
  EvalBatch   recipient j runs batch_recover_secret on the listed eval senders' y[.][j][g] and keeps P(0) -> z[j][g]   (:384-391)
  RevealBatch everyone runs batch_recover_secret on the listed reveal senders' z[.][g] and keeps the d + 1 coefficients: the
              opened values of chunk g                                                                 (:457-467)
The reference aborts at the first decode that fails.  The device call runs on: the chunk gives zeros, is counted in the summary, and
the next step runs on that zero.

A status byte is 0 when the verify rows of the lowest d + t + 1 senders pass (optimistic), 1 when the fallback (recover_secret's OEC
over all S senders) recovers, else the error code (8: DecodingError) with zeros as the result.
A summary is (n_fallback, n_failed, first_failed, first_error): chunks that left the optimistic pass, chunks that failed, the lowest
failed chunk (0xffffffff: none) and its error."""
from __future__ import annotations

import functools
import random

from oracle import spec as S_FR
from oracle import spec_gl

SPEC = {"fr": S_FR, "goldilocks": spec_gl.S}
PRIME = {"fr": S_FR.R_MOD, "goldilocks": spec_gl.P}
DECODING_ERROR = 8
NONE = 0xFFFFFFFF


@functools.lru_cache(maxsize=None)
def _basis(field, ids_needed, n, d, t):
    return SPEC[field].batch_basis(list(ids_needed), n, d, t)


def decode(field, senders, vals, n, d, t):
    """batch_recover_secret of ONE chunk from the values `vals` of the parties `senders` (any order): (status, coefficients [d + 1])"""
    Sp, q = SPEC[field], PRIME[field]
    m, needed = d + 1, d + t + 1
    srt = sorted(zip(senders, vals))
    basis, verify = _basis(field, tuple(s for s, _ in srt[:needed]), n, d, t)
    if all(sum(verify[s][i] * srt[i][1] for i in range(m)) % q == srt[s][1] % q for s in range(needed)):
        return 0, [sum((basis[i][k] if k < len(basis[i]) else 0) * srt[i][1] for i in range(m)) % q for k in range(m)]
    try:
        coeffs, _ = Sp.recover_secret([Sp.Share(v, sid, d) for sid, v in srt], n, t)
    except Sp.ShareErr as e:
        return e.code, [0] * m
    return 1, (list(coeffs) + [0] * m)[:m]


def summary(status):
    bad = [g for g, s in enumerate(status) if s > 1]
    return (sum(1 for s in status if s), len(bad), bad[0] if bad else NONE, status[bad[0]] if bad else 0)


@functools.lru_cache(maxsize=None)
def _powers(field, n, d):
    Sp, q = SPEC[field], PRIME[field]
    return [[pow(Sp.domain_element(n, j), k, q) for k in range(d + 1)] for j in range(n)]


def encode(field, x, n, d):
    """x [party][N] -> y [party][recipient][G]"""
    q, M, pw = PRIME[field], d + 1, _powers(field, n, d)
    G = len(x[0]) // M
    return [[[sum(pw[j][k] * xp[g * M + k] for k in range(M)) % q for g in range(G)] for j in range(n)] for xp in x]


def reveal_model(field, z, n, d, t, reveal_senders):
    """the RevealBatch arm alone, z [recipient][G] -> {"opened": [N], "status": [G], "summary"}"""
    G = len(z[0])
    opened, status = [], []
    for g in range(G):
        st, co = decode(field, reveal_senders, [z[j][g] for j in reveal_senders], n, d, t)
        status.append(st)
        opened += co
    return {"opened": opened, "status": status, "summary": summary(status)}


def model(field, n, t, d, x, eval_senders, reveal_senders):
    """x [party][N] ints -> {"Y": [party][recipient][G], "Z": [recipient][G], "opened": [N], "rstatus": [n G], "status": [G],
    "summary_first", "summary"}"""
    M = d + 1
    assert len(x) == n and len(x[0]) % M == 0 and len(x[0]) > 0
    G = len(x[0]) // M
    y = encode(field, x, n, d)
    z = [[0] * G for _ in range(n)]
    rstatus = [0] * (n * G)
    for j in range(n):
        for g in range(G):
            st, co = decode(field, eval_senders, [y[p][j][g] for p in eval_senders], n, d, t)
            rstatus[j * G + g] = st
            z[j][g] = co[0]
    out = reveal_model(field, z, n, d, t, reveal_senders)
    out.update({"Y": y, "Z": z, "rstatus": rstatus, "summary_first": summary(rstatus)})
    return out


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
def share_secrets(field, secrets, n, d, seed):
    """a degree-d sharing of every secret: x [party][N]"""
    Sp, q = SPEC[field], PRIME[field]
    rnd = random.Random(seed)
    al = [Sp.domain_element(n, p) for p in range(n)]
    x = [[0] * len(secrets) for _ in range(n)]
    for i, s in enumerate(secrets):
        poly = [s % q] + [rnd.randrange(q) for _ in range(d)]
        for p in range(n):
            x[p][i] = Sp.p_eval(poly, al[p])
    return x


@functools.lru_cache(maxsize=None)
def honest(field, n, t, d, G, seed=0):
    """(secrets [N], x [party][N]) of G chunks, computed once per shape; treat as read-only"""
    rnd = random.Random(7919 * n + 131 * d + 17 * G + seed + (1 if field == "fr" else 2))
    secrets = [rnd.randrange(PRIME[field]) for _ in range(G * (d + 1))]
    return secrets, share_secrets(field, secrets, n, d, seed + 99)


def lie(field, x, n, d, g, j, party=1, delta=5):
    """a copy of x in which `party` adds delta to element 1 and -alpha_j delta to element 0 of chunk g: the error polynomial
    delta (X - alpha_j) of its EvalBatch messages has a root at recipient j's point, so j alone is not lied to"""
    q = PRIME[field]
    a_j = SPEC[field].domain_element(n, j)
    out = [list(row) for row in x]
    out[party][g * (d + 1) + 1] = (out[party][g * (d + 1) + 1] + delta) % q
    out[party][g * (d + 1)] = (out[party][g * (d + 1)] - a_j * delta) % q
    return out
