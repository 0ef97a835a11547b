"""The matrix-core kernels (k_mfma_bfly, k_mfma_rows and their team, SUB, DEG, TRIPLE and Goldilocks variants) on the adversarial
inputs of tests/mfma_inputs.py: for every output row and digit the chunks with the largest and smallest digit sum, chunks whose T
accumulator alone is negative, chunks on the slow path of reduce_words (one subtraction; top word equal to r's) alone in a fast tile, as
a whole tile and last in the ragged tile, claimed values with one bit flipped at the word and lane-half boundaries of verify_tile, and the
operand pairs of sub_mod_r.  tests/test_mfma_inputs.py proves without a GPU that the inputs reach all of that, and pins the kernel each
(call, knobs, batch) below takes.

Every output element, status byte, ncoeffs entry and summary of every route is compared with the oracle (oracle.cref, oracle.cref_gl),
never with another route of the library alone; then the routes with each other, byte for byte."""
import numpy as np
import pytest

from __graft_entry__ import load_package
from oracle import cref as O
from oracle import cref_gl as OG
from tests import mfma_inputs as X
from tests import test_gpu_wave_edges as W
from tests.test_gpu_mul import pkg_eng  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu
K_OFF = "mc0,small0"                   # no matrix cores: the lane kernels and the FFTs


def configure(eng, knobs):
    """the knob strings of the planners' dump tools (tests/test_mfma_inputs.py::test_routes_are_pinned) applied to a context"""
    mode, mn = 1, 0
    eng.set_small_batch_chunks(8192)
    eng.set_matrix_core_workgroups(0)
    for tok in knobs.split(","):
        if tok.startswith("mc"):
            mode = int(tok[2:])
        elif tok.startswith("min"):
            mn = int(tok[3:])
        elif tok == "small0":
            eng.set_small_batch_chunks(0)
        elif tok == "wgs8":
            eng.set_matrix_core_workgroups(8)
        else:
            assert tok == "default", tok
    eng.set_matrix_cores(mode, mn if mn else 65536)      # 65 536: every threshold back at its default (each is capped there)


@pytest.fixture(scope="module")
def eng():
    e = load_package().Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def eng_gl():
    e = load_package().Engine(0, field="goldilocks")
    yield e
    e.close()


def agree(res):
    """the routes with each other, byte for byte"""
    first = next(iter(res))
    for name, got in res.items():
        for u, v in zip(got, res[first]):
            assert np.array_equal(u, v), (name, first)


def dev_buf(eng, arr):
    p = eng.dev_alloc(max(arr.nbytes, 16))
    eng.h2d(p, np.ascontiguousarray(arr))
    return p


def fetch(eng, ptr, shape, dtype=np.uint64):
    out = np.zeros(shape, dtype=dtype)
    eng.d2h(out, ptr)
    return out


# ---- encode ------------------------------------------------------------------------------------------------------------------------
def encode_routes(eng, x, n, d, routes):
    rc0, want = O.vandermonde_apply(x, n, d)
    assert rc0 == 0
    res = {}
    for knobs in routes:
        configure(eng, knobs)
        rc, y = eng.vandermonde_apply(x, n, d)
        assert rc == 0 and np.array_equal(y, want), knobs
        rc, y2 = eng.compute_shares(x, n, d)
        assert rc == 0 and np.array_equal(y2, want), knobs
        res[knobs] = (y,)
    agree(res)
    return want


@pytest.mark.parametrize("n,d", X.PAIR_SHAPES)
def test_point_pairs_chunk_major(eng, n, d):
    """k_mfma_bfly through 8 workgroups over more than 16 tiles; (13, 4): points without a partner, (16, 15): m = 16, (31, 10): two roles"""
    case = X.pair_case(n, d)
    assert (case.G + 31) // 32 > 16
    encode_routes(eng, X.fr_array(case.x), n, d, (X.K_PAIRS, X.K_TEAM, X.K_ROWS, K_OFF))


@pytest.mark.parametrize("n,d", X.ROW_ENCODE_SHAPES)
def test_one_row_per_point(eng, n, d):
    """k_mfma_rows as an encode (hbmpc_set_matrix_cores(ctx, 3, ..)), then the workgroup-per-tile kernel, the point pairs and the FFT"""
    case = X.row_encode_case(n, d)
    encode_routes(eng, X.fr_array(case.x), n, d, (X.K_ROWS, X.K_TEAM, X.K_PAIRS, K_OFF))


def test_workgroup_per_tile_encode_small_domain(eng):
    n, d, t = X.TEAM_SHAPES[0]
    case = X.row_encode_case(n, d)
    encode_routes(eng, X.fr_array(case.x), n, d, (X.K_TEAM, X.K_PAIRS, K_OFF))


def test_point_pairs_inputs_as_rows(eng):
    """hbmpc_dev_vandermonde_apply_rows at (16, 15): the rows read in place by the point-pair kernel (no workspace given), strided"""
    n, d = X.ROWS_IN_SHAPE
    case = X.pair_case(n, d)
    x = X.fr_array(case.x)
    G, stride = case.G, case.G + 24
    rc0, want = O.vandermonde_apply(x, n, d)
    assert rc0 == 0
    xr = np.full((d + 1, stride, 4), 0xEEEEEEEEEEEEEEEE, dtype=np.uint64)
    xr[:, :G] = x.transpose(1, 0, 2)
    res = {}
    x_d, y_d, tmp_d = dev_buf(eng, xr), eng.dev_alloc(n * G * 32), eng.dev_alloc(G * (d + 1) * 32)
    try:
        for knobs, tmp in ((X.K_PAIRS, 0), (K_OFF, tmp_d)):
            configure(eng, knobs)
            eng.h2d(y_d, np.full((n, G, 4), 0xEEEEEEEEEEEEEEEE, dtype=np.uint64))
            assert eng.dev_vandermonde_apply_rows(x_d, stride, G, n, d, tmp, y_d) == 0, eng.last_error()
            y = fetch(eng, y_d, (n, G, 4))
            eng.sync()
            assert np.array_equal(y, want), knobs
            res[knobs] = (y,)
    finally:
        for p in (x_d, y_d, tmp_d):
            eng.dev_free(p)
    agree(res)


def test_point_pairs_all_parties_in_one_launch(eng):
    """hbmpc_dev_vandermonde_apply_parties at (16, 5), P = 3: k_mfma_bfly<.., LISTS> over the P G chunks; party p holds the chunks rolled
    by p tiles.  (This branch tests the table's bound word before it launches, as the per-party one does.)"""
    n, d, parties = X.PARTIES_SHAPE
    case = X.pair_case(n, d)
    x0 = X.fr_array(case.x)
    G = case.G
    x = np.stack([np.roll(x0, 32 * p, axis=0) for p in range(parties)])
    want = np.stack([O.vandermonde_apply(np.ascontiguousarray(x[p]), n, d)[1] for p in range(parties)])
    res = {}
    x_d, y_d = dev_buf(eng, x), eng.dev_alloc(parties * n * G * 32)
    try:
        for knobs in (X.K_PAIRS, K_OFF):
            configure(eng, knobs)
            eng.h2d(y_d, np.full((parties, n, G, 4), 0xEEEEEEEEEEEEEEEE, dtype=np.uint64))
            assert eng.dev_vandermonde_apply_parties(x_d, G, n, d, parties, y_d) == 0, eng.last_error()
            y = fetch(eng, y_d, (parties, n, G, 4))
            eng.sync()
            assert np.array_equal(y, want), knobs
            res[knobs] = (y,)
    finally:
        eng.dev_free(x_d), eng.dev_free(y_d)
    agree(res)


def test_triple_encode_with_the_products_inside(eng):
    """k_mfma_bfly<.., TRIPLE> at (16, 5), 16 parties: b = 2^261 mod r and r2t = 0, so the kernel's x = (a b - r2t) / 2^261 is a, chosen
    against the table of alpha^i 2^261; against triple_local + vandermonde_apply of the oracle for EVERY party"""
    n, d, parties = X.TRIPLE_SHAPE
    case = X.triple_case(n, d)
    G, m = case.G, d + 1
    assert parties * G >= 1 << 14
    a0 = X.fr_array(case.x)
    a = np.stack([np.roll(a0, 32 * p, axis=0) for p in range(parties)]).reshape(parties * G * m, 4)
    b = np.ascontiguousarray(np.broadcast_to(X.fr_array([X.MM.RADIX % X.R])[0], a.shape))
    r = np.zeros_like(a)
    rc, loc = O.triple_local(a, b, r)
    assert rc == 0
    want = np.stack([O.vandermonde_apply(np.ascontiguousarray(loc.reshape(parties, G, m, 4)[p]), n, d)[1] for p in range(parties)])
    res = {}
    ptrs = [dev_buf(eng, v) for v in (a, b, r)]
    y_d, tmp_d = eng.dev_alloc(parties * n * G * 32), eng.dev_alloc(a.nbytes)
    try:
        for knobs in ("default", K_OFF):
            configure(eng, knobs)
            eng.h2d(y_d, np.full((parties, n, G, 4), 0xEEEEEEEEEEEEEEEE, dtype=np.uint64))
            assert eng.dev_triple_encode_parties(ptrs[0], ptrs[1], ptrs[2], G, n, d, parties, tmp_d if knobs == K_OFF else 0, y_d) == 0, eng.last_error()
            y = fetch(eng, y_d, (parties, n, G, 4))
            eng.sync()
            assert np.array_equal(y, want), knobs
            res[knobs] = (y,)
    finally:
        for p in ptrs + [y_d, tmp_d]:
            eng.dev_free(p)
    agree(res)


def test_inverse_transform_with_degrees(eng):
    """hbmpc_dev_batch_interpolate through all 16 shares of a full domain: k_mfma_bfly<.., DEG> (coefficients and degrees) and the
    instance without degrees; the oracle's decode with t = 0 gives the coefficients, the degree is their highest nonzero index"""
    n = X.DEG_N
    case = X.inverse_case(n)
    G, stride = case.G, case.G + 8
    sh = X.fr_array(case.x).transpose(1, 0, 2)                     # [party][G]
    ids = [5, 0, 11, 3, 7, 1, 12, 2, 9, 4, 15, 6, 8, 10, 13, 14]   # an arrival order
    rc0, co0, nco0, st0 = O.batch_recover(list(range(n)), np.ascontiguousarray(sh), n, n - 1, 0)
    assert rc0 == 0 and not st0.any()
    nz = co0.reshape(G, n, 4).any(axis=2)
    deg0 = np.where(nz.any(axis=1), n - 1 - np.argmax(nz[:, ::-1], axis=1), 0).astype(np.uint32)
    assert deg0.min() == 0 and deg0.max() == n - 1
    ev = np.full((n, stride, 4), 0xEEEEEEEEEEEEEEEE, dtype=np.uint64)
    ev[:, :G] = sh[ids]
    res = {}
    ev_d, c_d, dg_d = dev_buf(eng, ev), eng.dev_alloc(G * n * 32), eng.dev_alloc(G * 4)
    try:
        for knobs in (X.K_PAIRS, K_OFF):
            configure(eng, knobs)
            for with_degrees in (True, False):
                eng.h2d(c_d, np.full((G, n, 4), 0xEEEEEEEEEEEEEEEE, dtype=np.uint64))
                eng.h2d(dg_d, np.full(G, 0xEEEEEEEE, dtype=np.uint32))
                assert eng.dev_batch_interpolate(ids, ev_d, stride, G, n, c_d, dg_d if with_degrees else 0) == 0, eng.last_error()
                co, dg = fetch(eng, c_d, (G, n, 4)), fetch(eng, dg_d, (G,), np.uint32)
                eng.sync()
                assert np.array_equal(co, co0), (knobs, with_degrees)
                if with_degrees:
                    assert np.array_equal(dg, deg0), knobs
                    res[knobs] = (co, dg)
    finally:
        for p in (ev_d, c_d, dg_d):
            eng.dev_free(p)
    agree(res)


# ---- decode ------------------------------------------------------------------------------------------------------------------------
def summary_of(st):
    bad = np.flatnonzero(st > 1)
    return [int((st != 0).sum()), len(bad), int(bad[0]) if len(bad) else 0xFFFFFFFF, int(st[bad[0]]) if len(bad) else 0]


def dev_decode(eng, ids, ev, n, d, t, p0, eb):
    """hbmpc_[gl_]dev_batch_recover[_p0] with every output buffer: (out, status, ncoeffs, summary)"""
    G, ow, tail = ev.shape[1], 1 if p0 else d + 1, (4,) if eb == 32 else ()
    ev_d, out_d, st_d, nc_d, su_d = dev_buf(eng, ev), eng.dev_alloc(G * ow * eb), eng.dev_alloc(G), eng.dev_alloc(G * 4), eng.dev_alloc(64)
    try:
        eng.h2d(out_d, np.full((G, ow) + tail, 0xEEEEEEEEEEEEEEEE, dtype=np.uint64))
        eng.h2d(st_d, np.full(G, 0xEE, dtype=np.uint8))
        eng.h2d(nc_d, np.full(G, 0xEEEEEEEE, dtype=np.uint32))
        rc = eng.dev_batch_recover(ids, ev_d, G, n, d, t, out_d, 0 if p0 else nc_d, st_d, su_d, 0, p0=p0)
        assert rc == 0, eng.last_error()
        got = (fetch(eng, out_d, (G, ow) + tail), fetch(eng, st_d, (G,), np.uint8), fetch(eng, nc_d, (G,), np.uint32), fetch(eng, su_d, (4,), np.uint32))
        eng.sync()
        return got
    finally:
        for p in (ev_d, out_d, st_d, nc_d, su_d):
            eng.dev_free(p)


def decode_routes(eng, Or, case, field, routes):
    """a tile of tampered copies (one claimed value with one bit flipped), then the case's chunks: full and P(0), every route against the
    oracle -- coefficients, status, ncoeffs, summary -- and the routes with each other"""
    n, d, t = case.n, case.d, case.t
    y = X.evals_of(case, field)
    bad, info = X.tampered(case, y, field)
    ev = np.ascontiguousarray(np.concatenate([bad, y], axis=1))
    ids = list(range(n))
    rc0, co0, nco0, st0 = Or.batch_recover(ids, ev, n, d, t)
    hit = [k for k, (_, sender, _) in enumerate(info) if sender is not None]
    assert [int(g) for g in np.flatnonzero(st0)] == hit, "exactly the tampered chunks, as the oracle says"
    clean = np.ones(ev.shape[1], dtype=bool)
    clean[hit] = False
    want_free = X.fr_array(case.x) if field == "fr" else np.array(case.x, dtype=np.uint64)
    assert np.array_equal(ev[:d + 1, 32:].swapaxes(0, 1), want_free)
    eb = 32 if field == "fr" else 8
    res = {}
    for knobs in routes:
        configure(eng, knobs)
        co, st, nco, su = dev_decode(eng, ids, ev, n, d, t, False, eb)
        assert np.array_equal(st, st0) and np.array_equal(nco, nco0) and np.array_equal(co, co0), knobs
        assert su.tolist() == summary_of(st0), (knobs, su.tolist())
        p0v, st1, _, su1 = dev_decode(eng, ids, ev, n, d, t, True, eb)
        assert np.array_equal(st1, st0) and np.array_equal(p0v[:, 0], co0[:, 0]), knobs
        assert su1.tolist() == summary_of(st0), (knobs, su1.tolist())
        res[knobs] = (co, st, nco, su, p0v, st1, su1)
    agree(res)


@pytest.mark.parametrize("n,d,t", X.DECODE_SHAPES)
def test_decode_rows_full_and_p0(eng, n, d, t):
    """k_mfma_rows: one role and two, with an OEC tail behind it and without ((16, 10, 5): every sender is needed); (43, 14, 13) is beyond
    it (13 verify rows of 15 inputs do not fit the LDS: the lane kernel, pinned as such) and (31, 14, 10) is the 15-input shape it covers"""
    decode_routes(eng, O, X.decode_case(n, d, t), "fr", (X.K_DECODE, K_OFF))


@pytest.mark.parametrize("n,d,t", X.TEAM_SHAPES)
def test_workgroup_per_tile_decode_and_encode(eng, n, d, t):
    decode_routes(eng, O, X.decode_case(n, d, t), "fr", (X.K_TEAM, X.K_DECODE))
    if (n, d, t) != X.TEAM_SHAPES[0]:
        encode_routes(eng, X.fr_array(X.row_encode_case(n, d).x), n, d, (X.K_TEAM, K_OFF))


def test_sub_decode_operand_pairs(pkg_eng):  # noqa: F811
    """FpMul's four-launch form (k_mfma_rows<.., SUB>) on the operand pairs of sub_mod_r, behind interpolation rows and verify rows,
    in both halves; all three forms against the full oracle composition of tests/test_gpu_wave_edges.py"""
    pkg, e = pkg_eng
    n, t = X.SUB_SHAPE
    case = X.sub_case(n, t)
    ins = W.arrays(W.X.FR, case, n)
    want = W.check_fpmul(pkg, e, n, t, case["N"], X.SUB_K, X.SUB_M, ins, ("sub", n, t))
    assert want["summary_first"] == W.NOTHING_FAILED[1:] and want["summary"] == W.NOTHING_FAILED[1:]


# ---- Goldilocks --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,d,t", X.GL_SHAPES)
def test_goldilocks_rows(eng_gl, n, d, t):
    """k_mfma_rows_gl with the thresholds at 1, encode and decode: the largest w2, results that wrap 64 bits and results that need the
    final subtraction of p.  (64, 21, 21) has 22 inputs, beyond the kernel's 16: the same inputs through the kernels that take it)"""
    case = X.gl_encode_case(n, d)
    x = np.array(case.x, dtype=np.uint64)
    rc0, want = OG.vandermonde_apply(x, n, d)
    assert rc0 == 0
    res = {}
    for knobs in (X.K_TEAM, K_OFF):
        configure(eng_gl, knobs)
        rc, y = eng_gl.vandermonde_apply(x, n, d)
        assert rc == 0 and np.array_equal(y, want), knobs
        res[knobs] = (y,)
    agree(res)
    decode_routes(eng_gl, OG, X.gl_decode_case(n, d, t), "gl", (X.K_TEAM, K_OFF))
