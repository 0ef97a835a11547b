"""The square-root kernels (csrc/kernels_sqrt.hpp, and sqrt_core inside csrc/kernels_randbit_wg.hpp) on the chosen discrete logs and
slot patterns of tests/sqrt_inputs.py, bit for bit against tests/randbit_ref.py: every output of every call is compared, nothing is
sampled.  tests/test_sqrt_inputs.py proves without a GPU what these inputs reach (SITE_TABLE); tests/test_host_tables.py proves the
tables and an integer model of the kernels on the same values."""
import functools

import numpy as np
import pytest

from __graft_entry__ import load_package
from tests import randbit_ref as RB
from tests import sqrt_inputs as SX
from tests import test_gpu_randbit as RG
from tests import test_gpu_randbit_parties as RP

pytestmark = pytest.mark.gpu
CONFIGS = RG.CONFIGS


@pytest.fixture(scope="module")
def pkg():
    return load_package()


@pytest.fixture(scope="module")
def stream():
    torch = pytest.importorskip("torch")
    return torch.cuda.Stream(device=torch.device("cuda", 0))


def check_sqrt_inverse(eng, field, vals, want_root=None):
    """fr_sqrt and fr_inverse of `vals`: EVERY root, has_root, inverse and ok byte against ark_sqrt / ark_inverse"""
    p = RB.PRIME[field]
    a = RB.from_ints(vals, field)
    rc, root, has = eng.fr_sqrt(a)
    assert rc == 0, eng.last_error()
    rc, inv, ok = eng.fr_inverse(a)
    assert rc == 0, eng.last_error()
    N = len(vals)
    assert len(has) == N and len(ok) == N
    rv, iv = RB.to_ints(root, field), RB.to_ints(inv, field)
    for i, x in enumerate(vals):
        if want_root is not None:
            w = want_root[i]
            assert (int(has[i]), rv[i]) == ((0, 0) if w is None else (1, w)), (i, hex(x))
        wi = RB.ark_inverse(x, p)
        assert (int(ok[i]), iv[i]) == ((0, 0) if wi is None else (1, wi)), (i, hex(x))


@pytest.mark.parametrize("field,impl", CONFIGS)
def test_sqrt_and_inverse_over_the_family(pkg, field, impl):
    """the whole family in two seeded orders (a value meets different lanes and blocks), N no multiple of 256"""
    p = RB.PRIME[field]
    roots = SX.family_roots(p)
    eng = RG.engine(pkg, field, impl)
    try:
        for seed in (11, 12):
            vals, idx = SX.permuted(p, seed, extra=3 if len(roots) % 256 else 4)
            assert len(vals) % 256 and len(vals) > 8 * 256
            want = [roots[i][0] if i is not None else RB.ark_sqrt(vals[k], p) for k, i in enumerate(idx)]
            check_sqrt_inverse(eng, field, vals, want)
    finally:
        eng.close()


@pytest.mark.parametrize("field,impl", CONFIGS)
def test_inverse_slot_patterns(pkg, field, impl):
    """Montgomery's trick over the slots of a lane: every zero mask of tests/sqrt_inputs.py for 8 slots (u29, Goldilocks) and 2 slots
    (sat32) in one block, and the tails N = 256 B k + r with a zero and an edge value in the last live slots"""
    F = SX.FIELDS[field]
    eng = RG.engine(pkg, field, impl)
    try:
        check_sqrt_inverse(eng, field, SX.inverse_case(F, 8))
        for B in (8, 2):
            for N, vals in SX.inverse_tails(F, B):
                check_sqrt_inverse(eng, field, vals)
    finally:
        eng.close()


@functools.lru_cache(maxsize=None)
def family_phase2(field, parties):
    """(sq, a, RB.phase2 of them) over the whole family, once per field and party count"""
    F = SX.FIELDS[field]
    sq, a, _ = SX.phase2_case(F, parties)
    return sq, a, RB.phase2(sq, a, F.mod)


def summary_of(status):
    bad = [(s << 32) | i for i, s in enumerate(status) if s]
    return (min(bad) if bad else 2**64 - 1, len(bad))


def check_finalize(eng, field, sq, a, want_phase2, want_summary=None):
    parties = len(a)
    err, first, st, want = want_phase2
    arr_a = np.stack([RB.from_ints(row, field) for row in a])
    rc, out, status, summ = RG.finalize(eng, field, arr_a, RB.from_ints(sq, field), parties)
    assert rc == 0, eng.last_error()
    assert [int(s) for s in status] == st
    assert summ == summary_of(st) and (want_summary is None or summ == want_summary)
    assert (first is None) == (summ[1] == 0) and (first is None or (summ[0] >> 32, summ[0] & 0xFFFFFFFF) == (st[first], first))
    for q in range(parties):
        assert RB.to_ints(out[q], field) == want[q], f"party {q}"


@pytest.mark.parametrize("field,impl", CONFIGS)
@pytest.mark.parametrize("parties", [1, 3, 16])
def test_finalize_over_the_family(pkg, field, impl, parties):
    """squares with every chosen L (even, odd and zero), shares solved so that the OUTPUT is an edge value, and edge values as shares:
    the whole out and status against RB.phase2"""
    sq, a, want = family_phase2(field, parties)
    assert len(sq) % 256 and want[0] == RB.ZERO_SQUARE
    eng = RG.engine(pkg, field, impl)
    try:
        check_finalize(eng, field, sq, a, want)
    finally:
        eng.close()


@functools.lru_cache(maxsize=None)
def layout_phase2(field):
    F = SX.FIELDS[field]
    out = {}
    for name, (idx, summ) in SX.failure_layouts(F).items():
        sq, a, _ = SX.phase2_case(F, 3, tuple(idx))
        out[name] = (sq, a, RB.phase2(sq, a, F.mod), summ)
    return out


@pytest.mark.parametrize("field,impl", CONFIGS)
def test_finalize_failure_layouts(pkg, field, impl):
    """where the failures lie: the first at index 0, at N - 1, in the last partial block; a zero after several non-residues; only
    non-residues; every element failing -- each with the (first, n_failed) it must report"""
    eng = RG.engine(pkg, field, impl)
    try:
        for name, (sq, a, want, summ) in layout_phase2(field).items():
            check_finalize(eng, field, sq, a, want, summ)
    finally:
        eng.close()


# ---- the all-parties call: sqrt_core in t + 1 lanes of a workgroup (one launch) and in k_randbit_finalize (nine launches) -----------
PARTY_SHAPES = [("goldilocks", 5, 1), ("fr", 4, 1), ("fr", 16, 5)]


def parties_inputs(field, n, t):
    """shares whose secrets a = with_log(La) make the opened squares run over the family's even L (L = 2 La; La and La + 2^31 are +-a,
    the two output bits), then three more chunks with a zero secret and a square of chosen odd L (the same delta on every party's tc
    share) in the first, the last and a middle lane -> (shares, the expected (status, log) per element)"""
    p = RB.PRIME[field]
    M = t + 1
    evens = [L for _, L in SX.LOGS if not L & 1]
    named = [L for L in SX.NAMED if not L & 1]
    las = [(L >> 1) | ((i & 1) << 31) for i, L in enumerate(evens)]
    las += [(L >> 1) | ((~i & 1) << 31) for i, L in enumerate(named)]          # the named ones again, with the other sign
    while len(las) % M:
        las.append((named[len(las) % len(named)] >> 1) | 1 << 31)
    base = len(las)
    las += [(L >> 1) for L in (named * 3)[:3 * M]]
    N = len(las)
    rng = np.random.default_rng(N + n)
    avals = [SX.with_log(p, La, 1 if i % 5 == 0 else int(rng.integers(2, 2**62))) for i, La in enumerate(las)]
    expect = [(RB.ST_OK, (2 * La) & SX.M32) for La in las]
    odd = [L for _, L in SX.LOGS if L & 1]
    zeros, deltas = [], {}
    for c, (zl, ol) in enumerate(((0, t), (t, 0), (t // 2, (t // 2 + 1) % M))):
        zeros.append(base + c * M + zl)
        if ol != zl:
            i = base + c * M + ol
            L = odd[(17 * c + n) % len(odd)]
            deltas[i] = (SX.with_log(p, L, 3 + c) - avals[i] * avals[i]) % p
            expect[i] = (RB.ST_NO_ROOT, L)
    for i in zeros:
        avals[i] = 0
        expect[i] = (RB.ST_ZERO, None)
    a = RB.from_ints(avals, field)
    ta, tb = RB.fill_random(field, 61 + n, N), RB.fill_random(field, 62 + n, N)
    sec = {"a": a, "ta": ta, "tb": tb, "tc": RB.product(field, ta, tb)}
    sh = {k: RB.share_all(field, v, n, t, 70 + n + i) for i, (k, v) in enumerate(sec.items())}
    for i in zeros:
        sh["a"][:, i] = 0                                                  # the constant sharing of zero
    for i, d in deltas.items():
        col = RB.to_ints(sh["tc"][:, i], field)
        sh["tc"][:, i] = RB.from_ints([(v + d) % p for v in col], field)
    return sh, expect, avals


@pytest.mark.parametrize("field,n,t", PARTY_SHAPES)
def test_randbit_parties_over_the_family(pkg, stream, field, n, t):
    p = RB.PRIME[field]
    sh, expect, avals = parties_inputs(field, n, t)
    N = len(expect)
    assert N % (t + 1) == 0
    m = RP.model(field, n, t, sh)
    # the inputs are what they claim: every open succeeds, the opened squares have the chosen logs and statuses
    assert m["sm_de"][1] == 0 and m["sm_sq"][1] == 0 and m["status"] == [st for st, _ in expect]
    for i, (st, L) in enumerate(expect):
        if st == RB.ST_OK:
            assert m["sqop"][i] == avals[i] * avals[i] % p
        if L is not None and (i % 97 == 0 or st != RB.ST_OK):
            assert SX.log_of(m["sqop"][i], p) == L
    assert m["rb"] == summary_of(m["status"]) and m["rb"][1] >= 5
    eng = RP.engine(pkg, field)
    try:
        RP.both_forms_match(eng, stream, field, n, t, sh, m)
    finally:
        eng.close()
