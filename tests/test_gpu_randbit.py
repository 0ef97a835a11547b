"""RandBit on the device against its restatement (tests/randbit_ref.py): sqrt and inverse bit for bit, phase 2 for several party
counts with the reference's error precedence, and the whole pipeline (hbmpc_pipe_randbit_create) over both fields."""
import random

import numpy as np
import pytest

from __graft_entry__ import load_package
from tests import randbit_ref as RB

pytestmark = pytest.mark.gpu
CONFIGS = [("fr", "u29"), ("fr", "sat32"), ("goldilocks", None)]
SIZES = [1, 63, 64, 65, 4097, (1 << 20) + 3]


@pytest.fixture(scope="module")
def pkg():
    return load_package()


def engine(pkg, field, impl):
    eng = pkg.Engine(0, field=field)
    if impl:
        eng.set_impl(impl)
    return eng


def values(field, N, seed):
    """N canonical elements: random values (half of them squares), squares, the edge cases, zero, non-residues"""
    p = RB.PRIME[field]
    rng = random.Random(seed)
    om = RB.omega(p)
    special = [0, 1, p - 1, om * om % p, pow(om, 2**31 - 2, p), 7, om]
    out = []
    for i in range(min(N, 3000)):
        k = i % 4
        out.append(special[i % len(special)] if k == 0 else pow(rng.randrange(1, p), 2, p) if k == 1 else rng.randrange(0, p))
    arr = RB.from_ints(out, field)
    if N > len(out):  # the bulk: uniform random elements from the oracle's generator
        arr = np.concatenate([arr, RB.fill_random(field, seed, N - len(out))])
    return arr[:N]


def sample(N, seed, k=2000):
    if N <= 5000:
        return np.arange(N)
    rng = np.random.default_rng(seed)
    return np.unique(np.concatenate([np.arange(3000), rng.choice(N, k, replace=False), [N - 1]]))


@pytest.mark.parametrize("field,impl", CONFIGS)
@pytest.mark.parametrize("N", SIZES)
def test_sqrt_and_inverse_match_ark(pkg, field, impl, N):
    p = RB.PRIME[field]
    eng = engine(pkg, field, impl)
    try:
        a = values(field, N, 100 + N)
        rc, root, has = eng.fr_sqrt(a)
        assert rc == 0, eng.last_error()
        rc, inv, ok = eng.fr_inverse(a)
        assert rc == 0, eng.last_error()
        cols = sample(N, N)
        av, rv, iv = RB.to_ints(a[cols], field), RB.to_ints(root[cols], field), RB.to_ints(inv[cols], field)
        for k, x in enumerate(av):
            want = RB.ark_sqrt(x, p)
            assert (has[cols[k]], rv[k]) == ((0, 0) if want is None else (1, want)), (cols[k], hex(x))
            wi = RB.ark_inverse(x, p)
            assert (ok[cols[k]], iv[k]) == ((0, 0) if wi is None else (1, wi)), (cols[k], hex(x))
    finally:
        eng.close()


def finalize(eng, field, a_shares, sq, parties):
    """hbmpc_[gl_]dev_randbit_finalize_parties through device buffers -> (rc, out, status, (first, n_failed))"""
    N = sq.shape[0]
    eb = eng.ebytes
    bufs = [eng.dev_alloc(max(1, x)) for x in (parties * N * eb, N * eb, parties * N * eb, N, 16)]
    try:
        eng.h2d(bufs[0], a_shares)
        eng.h2d(bufs[1], sq)
        rc = eng.randbit_finalize_parties(bufs[0], bufs[1], N, parties, bufs[2], bufs[3], bufs[4])
        eng.sync()
        out = eng._new((parties, N))
        status = np.zeros(N, dtype=np.uint8)
        summ = np.zeros(16, dtype=np.uint8)
        eng.d2h(out, bufs[2])
        eng.d2h(status, bufs[3])
        eng.d2h(summ, bufs[4])
        eng.sync()
        return rc, out, status, (int(summ[:8].view(np.uint64)[0]), int(summ[8:12].view(np.uint32)[0]))
    finally:
        for b in bufs:
            eng.dev_free(b)


@pytest.mark.parametrize("field,impl", CONFIGS)
@pytest.mark.parametrize("parties", [1, 5, 16])
def test_finalize_matches_phase2(pkg, field, impl, parties):
    p = RB.PRIME[field]
    eng = engine(pkg, field, impl)
    try:
        N = 777
        rng = random.Random(parties)
        sqv = [pow(rng.randrange(1, p), 2, p) for _ in range(N)]
        sq = RB.from_ints(sqv, field)
        a = RB.fill_random(field, 5 + parties, parties * N).reshape((parties, N) + sq.shape[1:])
        rc, out, status, summ = finalize(eng, field, a, sq, parties)
        assert rc == 0, eng.last_error()
        err, first, st, want = RB.phase2(sqv, [RB.to_ints(a[q], field) for q in range(parties)], p)
        assert err == 0 and summ == (2**64 - 1, 0) and list(status) == st
        for q in range(parties):
            assert RB.to_ints(out[q], field) == want[q]
    finally:
        eng.close()


@pytest.mark.parametrize("field,impl", CONFIGS)
def test_finalize_error_precedence(pkg, field, impl):
    p = RB.PRIME[field]
    eng = engine(pkg, field, impl)
    try:
        base = [pow(k + 2, 2, p) for k in range(20)]
        for bad, want in (({2: 7, 9: 0}, (RB.ZERO_SQUARE, 9)), ({2: 7, 7: 7}, (RB.NO_SQUARE_ROOT, 2))):
            sqv = list(base)
            for i, v in bad.items():
                sqv[i] = v
            a = RB.fill_random(field, 77, 3 * len(sqv)).reshape((3, len(sqv)) + RB.from_ints([1], field).shape[1:])
            rc, out, status, (first, nfail) = finalize(eng, field, a, RB.from_ints(sqv, field), 3)
            assert rc == 0
            err, idx, st, exp = RB.phase2(sqv, [RB.to_ints(a[q], field) for q in range(3)], p)
            assert (err, idx) == want and list(status) == st and nfail == len(bad)
            assert (first >> 32, first & 0xFFFFFFFF) == (st[idx], idx)
            for q in range(3):
                assert RB.to_ints(out[q], field) == exp[q]
    finally:
        eng.close()


PIPE_SHAPES = [("goldilocks", 5, 1), ("fr", 4, 1), ("goldilocks", 4, 1), ("fr", 16, 5), ("goldilocks", 16, 5)]


def _stream():
    torch = pytest.importorskip("torch")
    return torch.cuda.Stream(device=torch.device("cuda", 0)).cuda_stream


@pytest.mark.parametrize("field,n,t", PIPE_SHAPES)
@pytest.mark.parametrize("big", [False, True])
def test_pipeline_matches_restatement(pkg, field, n, t, big):
    eng = engine(pkg, field, None)
    try:
        N = ((1 << 18) // (t + 1)) * (t + 1) if big else 40 * (t + 1)
        sec, sh = RB.pipeline_inputs(field, n, t, N, 1000 + n + N)
        rb = pkg.pipelines.RandBit(eng, n, t, N, stream=_stream())
        rb.upload(sh["a"], sh["ta"], sh["tb"], sh["tc"])
        rb.run(check=True)
        out, sq, sqop = rb.download("out"), rb.download("sq"), rb.download("sqop")
        assert not rb.status().any() and rb.rb_summary() == (2**64 - 1, 0)
        # every output opens to a bit
        rc, bits, st = eng.batch_recover_p0(list(range(n)), out, n, t, t)
        assert rc == 0 and not st.any()
        assert set(RB.to_ints(bits, field)) <= {0, 1}
        cols = sample(N, 9)
        wsq, wop, (err, first, status, want) = RB.pipeline_columns(field, sec, sh, cols)
        assert err == 0 and RB.to_ints(sqop[cols], field) == wop
        for q in range(n):
            assert RB.to_ints(sq[q][cols], field) == wsq[q]
            assert RB.to_ints(out[q][cols], field) == want[q]
        # replay of the captured run: the same bytes
        rb.capture()
        rb.upload_named("out", np.zeros_like(out))
        rb.replay()
        rb.sync()
        assert np.array_equal(rb.download("out"), out)
        rb.close()
    finally:
        eng.close()


@pytest.mark.parametrize("field,n,t", [("goldilocks", 5, 1), ("fr", 16, 5)])
def test_pipeline_errors(pkg, field, n, t):
    eng = engine(pkg, field, None)
    try:
        N = 30 * (t + 1)
        sec, sh = RB.pipeline_inputs(field, n, t, N, 77)
        # a tampered a share of party 0 in two elements: the opens decode from exactly 2t + 1 senders, so those chunks fail
        bad = {k: v.copy() for k, v in sh.items()}
        for i in (3, 17):
            bad["a"][0, i] = bad["a"][1, i]
        rb = pkg.pipelines.RandBit(eng, n, t, N, stream=_stream())
        rb.upload(bad["a"], bad["ta"], bad["tb"], bad["tc"])
        rb.run(check=False)
        rst = rb.bytes_of("rstatus_de", n * 2 * N // (t + 1))
        de_first = rb.bytes_of("summary_de_first", 16).view(np.uint32)
        assert de_first[1] > 0 and rst.any()
        with pytest.raises(RuntimeError, match=f"ShareErrorCode {int(de_first[3])}"):
            rb.run(check=True)
        # a = 0 in one element: phase 2's ZeroSquare
        z = {k: v.copy() for k, v in sh.items()}
        z["a"][:, 5] = 0
        rb.upload(z["a"], z["ta"], z["tb"], z["tc"])
        with pytest.raises(RuntimeError, match=f"ShareErrorCode {RB.ZERO_SQUARE}"):
            rb.run(check=True)
        assert rb.status()[5] == RB.ST_ZERO and rb.rb_summary() == ((1 << 32) | 5, 1)
        rb.close()
        # N not a multiple of t + 1 (rand_bit.rs:253-255)
        with pytest.raises(RuntimeError, match="ShareErrorCode 4"):
            pkg.pipelines.RandBit(eng, n, t, N + 1)
    finally:
        eng.close()
