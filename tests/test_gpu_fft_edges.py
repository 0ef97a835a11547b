"""The lane-per-chunk FFT encode kernels (k_eval_fft1, k_eval_fftP and its fold form, k_eval_fft1_triple, k_eval_fft1_mix; Fr / U29 and
Goldilocks) on the bound-edge inputs of tests/fft_inputs.py: every instantiation the library compiles, full tiles followed by a one-row
tile, n = 256 and n = size / 2 + 1.  tests/test_fft_inputs.py proves without a GPU that the inputs reach their sites and pins the kernel
each call takes first.

Every output element of every route is compared with the oracle (oracle.cref, oracle.cref_gl), then the routes with each other.  That the
FFT kernel produced the bytes, not the generic kernel behind it, is checked through the table cache: only the generic and the wide kernel
build the point table of n, so after the FFT calls of a fresh context the first forced-generic call adds exactly one table."""
import numpy as np
import pytest

from __graft_entry__ import load_package
from tests import fft_inputs as X
from tests.gpu_util import configure, dev_buf, fetch

pytestmark = pytest.mark.gpu
CANARY = 0xEEEEEEEEEEEEEEEE


def groups():
    """(field, n) -> the chunk-major shapes of that domain, (family, shape); a fresh context each, so that its cache has not seen n.
    Shapes only: the cases are built inside the tests, collection needs no model"""
    out = {}
    for field in ("fr", "goldilocks"):
        for sh in X.fft1_shapes():
            out.setdefault((field, sh[2]), []).append(("fft1", sh))
        for sh in X.fftP_shapes():
            out.setdefault((field, sh[2]), []).append(("fftP", sh))
    return out


GROUPS = groups()


def case_of(field, family, shape):
    return X.chunk_case(field, "fft1", shape[2], shape[1] - 1) if family == "fft1" else X.fftP_case(field, *shape)


def batch_sizes(c):
    small = (c.LOG, c.d + 1, c.n) in X.SMALL_G_FFT1 if c.family == "fft1" else (c.P, c.d + 1, c.n) in X.SMALL_G_FFTP
    return (c.G,) + (X.SMALL_G if small else ())


def encode(eng, x, n, d, want, tag):
    """vandermonde_apply and compute_shares, every element against the oracle"""
    rc, y = eng.vandermonde_apply(x, n, d)
    assert rc == 0 and np.array_equal(y, want), (tag, "vandermonde_apply", eng.last_error())
    rc, y2 = eng.compute_shares(x, n, d)
    assert rc == 0 and np.array_equal(y2, want), (tag, "compute_shares", eng.last_error())
    return y


@pytest.mark.parametrize("field,n", sorted(GROUPS), ids=["%s-n%d" % k for k in sorted(GROUPS)])
def test_chunk_major_edges(field, n):
    F = X.FIELDS[field]
    eng = load_package().Engine(0, field=field)
    try:
        configure(eng, X.K_FFT)
        runs = []
        for family, shape in GROUPS[(field, n)]:
            c = case_of(field, family, shape)
            for G in batch_sizes(c):
                x = c.array(G)
                rc, want = F.O.vandermonde_apply(x, n, c.d)
                assert rc == 0
                runs.append((c.d, x, want, encode(eng, x, n, c.d, want, (field, n, c.d, G, X.K_FFT))))
        # the FFT kernels ran, not the fallback: nothing so far built the point table alpha{n}, so the first generic call adds exactly it
        for i, (d, x, want, y_fft) in enumerate(runs):
            before = eng.cache_stats()["tables"]
            eng.set_force_generic(True)
            try:
                y_gen = encode(eng, x, n, d, want, (field, n, d, "generic"))
            finally:
                eng.set_force_generic(False)
            assert eng.cache_stats()["tables"] - before == (1 if i == 0 else 0), (field, n, d, i)
            configure(eng, "default")                                     # a batch this small: the wave-per-chunk kernels
            y_wide = encode(eng, x, n, d, want, (field, n, d, "default"))
            assert np.array_equal(y_fft, y_gen) and np.array_equal(y_fft, y_wide)
            if field == "fr":
                eng.set_impl("sat32")
                try:
                    rc, y_sat = eng.vandermonde_apply(x, n, d)
                finally:
                    eng.set_impl("u29")
                assert rc == 0 and np.array_equal(y_sat, want), (n, d, "sat32")
            configure(eng, X.K_FFT)
    finally:
        eng.close()


@pytest.mark.parametrize("field", ["fr", "goldilocks"])
def test_a_fall_through_is_what_the_table_check_sees(field):
    """the control of the check above: (100, 33) has d + 1 = 34 coefficients, beyond the fold kernel's 32, so the same knobs give the generic
    kernel -- and then the point table is already there when the forced-generic call comes"""
    F = X.FIELDS[field]
    n, d = 100, 33
    x = F.arr([[(7 * g + k) % F.mod for k in range(d + 1)] for g in range(65)])
    rc, want = F.O.vandermonde_apply(x, n, d)
    assert rc == 0
    eng = load_package().Engine(0, field=field)
    try:
        configure(eng, X.K_FFT)
        encode(eng, x, n, d, want, (field, "fall-through"))
        before = eng.cache_stats()["tables"]
        eng.set_force_generic(True)
        encode(eng, x, n, d, want, (field, "generic"))
        assert eng.cache_stats()["tables"] == before
    finally:
        eng.close()


@pytest.fixture(scope="module")
def engines():
    pkg = load_package()
    es = {"fr": pkg.Engine(0), "goldilocks": pkg.Engine(0, field="goldilocks")}
    yield es
    for e in es.values():
        e.close()


STRIDED = [(field, family, sh) for field in ("fr", "goldilocks") for family, shapes in (("fft1", X.STRIDED_FFT1), ("fftP", X.STRIDED_FFTP))
           for sh in shapes]


@pytest.mark.parametrize("field,family,shape", STRIDED, ids=["%s-%s-%d-%d-%d" % ((f, fam) + sh) for f, fam, sh in STRIDED])
def test_strided_and_party_batched_outputs(engines, field, family, shape):
    """hbmpc_dev_vandermonde_apply_strided with a row stride of G + 5 (the gaps and what lies behind the last row keep their canary bytes)
    and hbmpc_dev_vandermonde_apply_parties with 3 parties (party p holds the rows rolled by 64 p)"""
    F, eng, c = X.FIELDS[field], engines[field], case_of(field, family, shape)
    n, d, G, eb = c.n, c.d, c.G, eng.ebytes
    stride, tail = G + 5, 7
    configure(eng, X.K_FFT)
    x = c.array()
    rc, want = F.O.vandermonde_apply(x, n, d)
    assert rc == 0
    x_d, y_d = dev_buf(eng, x), eng.dev_alloc((n * stride + tail) * eb)
    try:
        eng.h2d(y_d, np.full((n * stride + tail,) + F.tail, CANARY, dtype=np.uint64))
        assert eng.dev_vandermonde_apply_strided(x_d, G, n, d, y_d, stride) == 0, eng.last_error()
        flat = fetch(eng, y_d, (n * stride + tail,) + F.tail)
        eng.sync()
        y = flat[:n * stride].reshape((n, stride) + F.tail)
        assert np.array_equal(y[:, :G], want)
        assert np.all(y[:, G:] == np.uint64(CANARY)) and np.all(flat[n * stride:] == np.uint64(CANARY))
    finally:
        eng.dev_free(x_d), eng.dev_free(y_d)
    parties = 3
    xs = np.stack([np.roll(x, -64 * p, axis=0) for p in range(parties)])
    wants = np.stack([F.O.vandermonde_apply(np.ascontiguousarray(xs[p]), n, d)[1] for p in range(parties)])
    x_d, y_d = dev_buf(eng, xs), eng.dev_alloc((parties * n * G + tail) * eb)
    try:
        eng.h2d(y_d, np.full((parties * n * G + tail,) + F.tail, CANARY, dtype=np.uint64))
        assert eng.dev_vandermonde_apply_parties(x_d, G, n, d, parties, y_d) == 0, eng.last_error()
        flat = fetch(eng, y_d, (parties * n * G + tail,) + F.tail)
        eng.sync()
        assert np.array_equal(flat[:parties * n * G].reshape((parties, n, G) + F.tail), wants)
        assert np.all(flat[parties * n * G:] == np.uint64(CANARY))
    finally:
        eng.dev_free(x_d), eng.dev_free(y_d)
        configure(eng, "default")


@pytest.mark.parametrize("field", ["fr", "goldilocks"])
@pytest.mark.parametrize("LOG,cnt,n", X.triple_shapes())
def test_triple_edges(engines, field, LOG, cnt, n):
    """hbmpc_dev_triple_encode_parties with a null workspace (a declined launcher is then an error, not the two-step form), 1 and 3
    parties, against the oracle's products and encode"""
    F, eng = X.FIELDS[field], engines[field]
    d, eb = cnt - 1, eng.ebytes
    configure(eng, "default")
    for parties in (1, 3):
        t = X.triple_case(field, LOG, cnt, n, parties)
        G = t["G"]
        a, b, r = (F.arr([v for party in t[k] for v in party]) for k in ("a", "b", "r2t"))
        rc, loc = F.O.triple_local(a, b, r)
        assert rc == 0 and np.array_equal(loc, F.arr([v for party in t["c"] for row in party for v in row]))
        loc = loc.reshape((parties, G, cnt) + F.tail)
        want = np.stack([F.O.vandermonde_apply(np.ascontiguousarray(loc[p]), n, d)[1] for p in range(parties)])
        ptrs = [dev_buf(eng, v) for v in (a, b, r)]
        y_d = eng.dev_alloc(parties * n * G * eb)
        try:
            eng.h2d(y_d, np.full((parties, n, G) + F.tail, CANARY, dtype=np.uint64))
            assert eng.dev_triple_encode_parties(ptrs[0], ptrs[1], ptrs[2], G, n, d, parties, 0, y_d) == 0, eng.last_error()
            y = fetch(eng, y_d, (parties, n, G) + F.tail)
            eng.sync()
            assert np.array_equal(y, want), (field, LOG, cnt, n, parties)
        finally:
            for p in ptrs + [y_d]:
                eng.dev_free(p)


def mix_params():
    return [(field, n) for field in ("fr", "goldilocks") for n in X.MIX_N[field]]


@pytest.mark.parametrize("field,n", mix_params())
def test_mix_edges(engines, field, n):
    """the producers' mixing step where the kernel writes the lists itself (k_eval_fft1_mix): two slices, a K that is no multiple of 64;
    the lists, the party-major other rows and the plain rows against the oracle's encode of the transposed input"""
    F, eng = X.FIELDS[field], engines[field]
    eb, d, K = eng.ebytes, n - 1, X.mix_K(field, n)
    G = n * K
    configure(eng, "default")
    assert K % 64 and eng.apply_rows_lists_in_kernel(G, n, d)
    x = F.arr(X.mix_rows(field, n))                                       # [G][n]
    rc, want = F.O.vandermonde_apply(x, n, d)
    assert rc == 0
    xr = np.ascontiguousarray(np.swapaxes(x, 0, 1))                       # the n input rows
    row0, rows = n // 3, max(1, n // 2)
    nother, k1 = n - rows, K // 3
    other_rows = [r for r in range(n) if not row0 <= r < row0 + rows]
    w4 = want.reshape((n, n, K) + F.tail)                                 # [row][party][k]
    want_others = np.ascontiguousarray(np.swapaxes(w4[other_rows], 0, 1))             # [party][r'][k]
    want_lists = np.ascontiguousarray(np.moveaxis(w4[row0:row0 + rows], 0, 2))         # [party][k][row]
    na, nb = k1, K - k1 - 1                                               # two slices: [0, k1) and [k1 + 1, K); element k1 is dropped
    x_d, tmp_d, y_d = dev_buf(eng, xr), eng.dev_alloc(G * n * eb), eng.dev_alloc(n * G * eb)
    la_d, lb_d, ot_d = eng.dev_alloc(n * na * rows * eb), eng.dev_alloc(n * (nb + 2) * rows * eb), eng.dev_alloc(n * nother * K * eb)
    try:
        for with_others in (True, False):
            eng.h2d(y_d, np.full((n, G) + F.tail, CANARY, dtype=np.uint64))
            eng.h2d(la_d, np.full((n, na, rows) + F.tail, CANARY, dtype=np.uint64))
            eng.h2d(lb_d, np.full((n, nb + 2, rows) + F.tail, CANARY, dtype=np.uint64))
            eng.h2d(ot_d, np.full((n, nother, K) + F.tail, CANARY, dtype=np.uint64))
            slices = [(la_d, na * rows, 0, na), (lb_d, (nb + 2) * rows, k1 + 1, nb)]
            rc = eng.dev_vandermonde_apply_rows_split(x_d, G, G, n, d, 0, y_d, row0, rows, K, slices, ot_d if with_others else None)
            assert rc == 0, eng.last_error()                              # no workspace: only the list-writing kernel can take the call
            la, lb = fetch(eng, la_d, (n, na, rows) + F.tail), fetch(eng, lb_d, (n, nb + 2, rows) + F.tail)
            ot, y = fetch(eng, ot_d, (n, nother, K) + F.tail), fetch(eng, y_d, (n, G) + F.tail)
            eng.sync()
            assert np.array_equal(la, want_lists[:, :k1]) and np.array_equal(lb[:, :nb], want_lists[:, k1 + 1:]), (field, n, with_others)
            assert np.all(lb[:, nb:] == np.uint64(CANARY))
            if with_others:
                assert np.array_equal(ot, want_others) and np.all(y == np.uint64(CANARY))
            else:
                assert np.array_equal(y[other_rows], want[other_rows]) and np.all(ot == np.uint64(CANARY))
        eng.h2d(y_d, np.full((n, G) + F.tail, CANARY, dtype=np.uint64))
        assert eng.dev_vandermonde_apply_rows(x_d, G, G, n, d, tmp_d, y_d) == 0, eng.last_error()
        y = fetch(eng, y_d, (n, G) + F.tail)
        eng.sync()
        assert np.array_equal(y, want)
    finally:
        for p in (x_d, tmp_d, y_d, la_d, lb_d, ot_d):
            eng.dev_free(p)
