"""The FixedPrep handle (hbmpc_pipe_fixedprep_create, csrc/capi_pipelines_fixedprep.hip) against its restatement
(tests/fixedprep_ref.py), bit for bit: every named buffer of the handle and of its six parts that the composition defines, at three
shapes whose cuts fall differently and at one shape beyond PRandBit's one-launch tables -- (13, 4, 5, 2), also against the Python
restatement: it takes about half a second on the CPU; the one-launch forms against the separate launches; capture + replay against
eager; a dealer whose dealt share is rewritten between deal() and finish(); takes from the pools into an FpMul handle; the halves
that may be absent; and config C1 from the dealers' polynomials to a client's fixed-point products through handles only.

Workspaces the parts document as unspecified (Y, Z, the producers' x / y / poly) are not compared."""
import ctypes as C

import numpy as np
import pytest

from __graft_entry__ import load_package
from oracle import spec as S
from tests import fixedprep_ref as FR
from tests import prandbit_ref as PR
from tests import producers_ref as PD

pytestmark = pytest.mark.gpu
SHAPES = [(4, 1, 4, 3), (7, 2, 16, 5), (10, 3, 8, 4), (13, 4, 5, 2)]
INSUFFICIENT_SHARES, INVALID_INPUT, TYPE_MISMATCH, DECODING_ERROR = 1, 4, 5, 8
SENTINEL = np.uint64(0xC3C3C3C3C3C3C3C3)
GL = "goldilocks"


@pytest.fixture(scope="module")
def pkg():
    return load_package()


@pytest.fixture(scope="module")
def engines(pkg):
    fr, gl = pkg.Engine(0, field="fr"), pkg.Engine(0, field="goldilocks")
    yield fr, gl
    fr.close()
    gl.close()


@pytest.fixture(scope="module")
def stream(engines):
    st = engines[1].stream_create()
    yield st
    engines[1].sync(st)
    engines[1].stream_destroy(st)


def gl_arr(rows):
    return np.array(rows, dtype=np.uint64)


def make(pkg, engines, shape, stream):
    """a handle with the restatement's inputs uploaded"""
    fr, gl = engines
    n, t, nb, ni = shape
    inp = FR.inputs(*shape)
    prep = pkg.pipelines.FixedPrep(gl, fr, n, t, nb, ni, inp["lk"], stream=stream)
    if nb:
        prep.rs.upload(gl_arr(inp["coeffs"]))
        prep.rd.upload(gl_arr(inp["coeffs_t"]), gl_arr(inp["coeffs_2t"]))
        prep.pb.upload_named("contrib", gl_arr(inp["contrib_bit"]))
    if ni:
        prep.pi.upload_named("contrib", gl_arr(inp["contrib_int"]))
    return prep


def collect(prep):
    """every buffer the composition defines, as bytes: {(part, name): array}"""
    n, t = prep.n, prep.t
    got = {}
    if prep.n_prandbit:
        R, T, K1, K2 = prep.R, prep.T, prep.K1, prep.K2
        l1, l2 = (n - 2 * t) * K1, (t + 1) * K2
        gl_shapes = {"ransha": (prep.rs, {"S": (n, n, K1), "out": (n, l1)}),
                     "randousha": (prep.rd, {"S_t": (n, n, K2), "S_2t": (n, n, K2), "out_t": (n, l2), "out_2t": (n, l2)}),
                     "triplegen": (prep.tg, {k: (n, T) for k in ("a", "b", "rt", "r2t", "c")} | {"opened": (T,)}),
                     "randbit": (prep.rb, {k: (n, R) for k in ("a", "ta", "tb", "tc", "sq", "out")} | {"sqop": (R,), "deop": (2 * R,)})}
        for part, (h, names) in gl_shapes.items():
            for name, shp in names.items():
                got[(part, name)] = h.download_named(name, shp).copy()
        got[("randbit", "status")] = prep.rb.status().copy()
        for name in ("b_q", "sums", "bad", "r_p", "r_2", "r_q", "rb", "opened", "b_p", "b_2"):
            got[("prandbit", name)] = prep.pb.download_named(name).copy()
        got[("fixedprep", "r_bits")] = prep.download_named("r_bits").copy()
        got[("fixedprep", "r_bits2")] = prep.download_named("r_bits2").copy()
        got[("verdict", "")] = np.array(prep.verdict(), dtype=np.uint64)
        got[("summary", "")] = prep.summary().copy()
    if prep.n_prandint:
        for name in ("sums", "bad", "r_p"):
            got[("prandint", name)] = prep.pi.download_named(name).copy()
        got[("fixedprep", "r_int")] = prep.download_named("r_int").copy()
    return got


def expected(shape):
    n, t, nb, ni = shape
    m = FR.fixedprep(*shape, FR.inputs(*shape))
    flat_fr = lambda rows: PR.rows_from_ints(rows, "fr").reshape(-1, 4)  # noqa: E731
    want = {}
    if nb:
        for part in ("ransha", "randousha", "triplegen", "randbit"):
            for name, v in m[part].items():
                want[(part, name)] = np.array(v, dtype=np.uint8 if name == "status" else np.uint64)
        pb = m["prandbit"]
        for name in ("b_q", "sums", "r_q", "rb", "opened"):
            want[("prandbit", name)] = gl_arr(pb[name]).reshape(-1)
        for name in ("bad", "r_2", "b_2"):
            want[("prandbit", name)] = np.array(pb[name], dtype=np.uint8).reshape(-1)
        for name in ("r_p", "b_p"):
            want[("prandbit", name)] = flat_fr(pb[name])
        want[("fixedprep", "r_bits")] = flat_fr(m["r_bits"])
        want[("fixedprep", "r_bits2")] = np.array(m["r_bits2"], dtype=np.uint8).reshape(-1)
        want[("verdict", "")] = np.array([0, 0xFFFFFFFF], dtype=np.uint64)
        want[("summary", "")] = np.array([0, 0, 0xFFFFFFFF, 0], dtype=np.uint32)
    if ni:
        pi = m["prandint"]
        want[("prandint", "sums")] = gl_arr(pi["sums"]).reshape(-1)
        want[("prandint", "bad")] = np.array(pi["bad"], dtype=np.uint8).reshape(-1)
        want[("prandint", "r_p")] = flat_fr(pi["r_p"])
        want[("fixedprep", "r_int")] = flat_fr(m["r_int"])
    return m, want


def assert_same(got, want, tag):
    assert set(got) == set(want), (tag, set(got) ^ set(want))
    for key in want:
        g, w = np.asarray(got[key]).reshape(-1), np.asarray(want[key]).reshape(-1)
        assert g.shape == w.shape and np.array_equal(g.astype(np.uint64), w.astype(np.uint64)), (tag, key, np.argwhere(g != w)[:4].tolist())


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "n%d_t%d_%d_%d" % s)
def test_every_defined_buffer_equals_the_restatement(pkg, engines, stream, shape):
    prep = make(pkg, engines, shape, stream)
    try:
        assert prep.available() == (0, 0)                       # empty until the first run
        prep.run(check=True)
        _, want = expected(shape)
        assert_same(collect(prep), want, shape)
        n, t, nb, ni = shape
        assert prep.available() == (FR.sizes(n, t, nb)[0], ni)
    finally:
        prep.close()


FUSED = ("triplegen", "fpmul", "truncpr", "mul", "input", "batchrecon", "producers", "randbit", "prandbit")


def set_fused(pkg, engines, zero):
    """every hbmpc_set_fused_* of both contexts at 0 (separate launches everywhere), or back at the defaults"""
    H = pkg.hbmpc
    for eng in engines:
        per_field = lambda d: d[eng.field]  # noqa: E731
        defaults = {"triplegen": 1024, "fpmul": 2048, "truncpr": H.FUSED_TRUNCPR_DEFAULT, "mul": H.FUSED_MUL_DEFAULT, "input": H.FUSED_INPUT_DEFAULT,
                    "batchrecon": per_field(H.FUSED_BATCHRECON_DEFAULT), "producers": per_field(H.FUSED_PRODUCERS_DEFAULT),
                    "randbit": per_field(H.FUSED_RANDBIT_DEFAULT), "prandbit": H.FUSED_PRANDBIT_DEFAULT}
        for name in FUSED:
            rc = getattr(eng.L, "hbmpc_set_fused_" + name)(eng.ctx, C.c_size_t(0 if zero else defaults[name]))
            assert rc in (0, TYPE_MISMATCH), (name, rc)          # a setter of the other field's call may refuse the context


@pytest.mark.parametrize("shape", [(4, 1, 4, 3), (7, 2, 16, 5)], ids=lambda s: "n%d_t%d_%d_%d" % s)
def test_forms_and_replay_give_the_same_bytes(pkg, engines, stream, shape):
    """the defaults (one launch wherever a call has that form) against separate launches everywhere, and capture() + replay() against
    eager -- after the outputs were overwritten, so the replay has to write them again"""
    res = {}
    try:
        for form in ("default", "separate"):
            set_fused(pkg, engines, form == "separate")
            prep = make(pkg, engines, shape, stream)
            try:
                prep.run(check=True)
                res[form] = collect(prep)
                if form == "default":
                    prep.capture()
                    for h, name in ((prep, "r_bits"), (prep, "r_int"), (prep.rb, "out"), (prep.tg, "c")):
                        nbytes = h.buffer(name)[1] * (32 if name.startswith("r_") else 8)
                        engines[1].h2d(h.buffer(name)[0], np.full(nbytes // 8, SENTINEL, dtype=np.uint64), stream)
                    prep.replay()
                    prep.sync()
                    res["replay"] = collect(prep)
                    assert prep.available() == (prep.R, prep.n_prandint)        # a replay refills: the cursors are reset
            finally:
                prep.close()
    finally:
        set_fused(pkg, engines, False)
    assert_same(res["separate"], res["default"], (shape, "separate"))
    assert_same(res["replay"], res["default"], (shape, "replay"))
    assert_same(res["default"], expected(shape)[1], shape)


def test_byzantine_dealer(pkg, engines, stream):
    """deal(), one dealt share of the ransha part rewritten, finish(): the verdict counts it, a checked finish returns DecodingError
    (the reference aborts where a verifier says no), an unchecked one ShareSuccess"""
    shape = (7, 2, 16, 5)
    n, t = shape[:2]
    prep = make(pkg, engines, shape, stream)
    try:
        K1 = prep.K1
        for check in (False, True):
            prep.deal()
            S_ = prep.rs.download_named("S", (n, n, K1))
            S_[0, 1, 0] = (int(S_[0, 1, 0]) + 1) % FR.Q           # dealer 0's share for recipient 1, column 0
            prep.rs.upload_named("S", S_)
            if check:
                with pytest.raises(RuntimeError, match="ShareErrorCode %d" % DECODING_ERROR):
                    prep.finish(check=True)
            else:
                prep.finish(check=False)                          # raises on any code but ShareSuccess
            bad, first = prep.verdict()
            assert bad >= 1 and first == 0
        prep.run(check=True)                                      # an honest run of the same handle afterwards
        assert prep.verdict() == (0, 0xFFFFFFFF)
        assert_same(collect(prep), expected(shape)[1], "after the lie")
    finally:
        prep.close()


def test_take(pkg, engines, stream):
    """N = 3 at m = 4, then N = 1 at m = 4, into FpMul handles' rbits / rint: the restatement's pool slices at cursors 0 and 12 (bits), 0
    and 3 (integers); available counts down; an overdraw is InsufficientShares with nothing written and the cursors unchanged; run()
    resets the cursors"""
    fr, gl = engines
    shape = (7, 2, 16, 5)
    n, t, nb, ni = shape
    m_model, _ = expected(shape)
    R = m_model["sizes"][0]
    prep = make(pkg, engines, shape, stream)
    k, m = 16, 4
    fps = [pkg.pipelines.FpMul(fr, n, t, N, k, m, stream=stream) for N in (3, 1, 2)]
    try:
        prep.run(check=True)
        cur_b = cur_i = 0
        for fp in fps[:2]:
            N = fp.N
            prep.take(fp)
            want = [FR.pool_take(m_model["r_bits"][p], m_model["r_int"][p], cur_b, cur_i, m, N) for p in range(n)]
            rbits = fp.download_named("rbits", (n, m, N))
            rint = fp.download_named("rint", (n, N))
            for p in range(n):
                assert np.array_equal(rbits[p].reshape(-1, 4), PR.from_ints([v for row in want[p][0] for v in row], "fr")), (N, p)
                assert np.array_equal(rint[p], PR.from_ints(want[p][1], "fr")), (N, p)
            cur_b, cur_i = cur_b + m * N, cur_i + N
            assert prep.available() == (R - cur_b, ni - cur_i)
        assert (cur_b, cur_i) == (16, 4) and prep.available() == (2, 1)
        # overdraws: 2 elements want 8 bits (2 left) / 2 integers (1 left) -- each pool alone, and both
        fp = fps[2]
        for rb_d, ri_d in ((fp.rbits, fp.rint), (fp.rbits, 0), (0, fp.rint)):
            fr.h2d(fp.rbits, np.full((n, m, 2, 4), SENTINEL, dtype=np.uint64), stream)
            fr.h2d(fp.rint, np.full((n, 2, 4), SENTINEL, dtype=np.uint64), stream)
            assert prep.take_raw(m, 2, rb_d, ri_d) == INSUFFICIENT_SHARES
            assert (fp.download_named("rbits", (n, m, 2)) == SENTINEL).all() and (fp.download_named("rint", (n, 2)) == SENTINEL).all()
            assert prep.available() == (2, 1)
        assert prep.take_raw(m, 2, 0, 0) == INVALID_INPUT and prep.take_raw(0, 1, fp.rbits, fp.rint) == INVALID_INPUT
        assert prep.take_raw(m, 0, fp.rbits, fp.rint) == INVALID_INPUT and prep.available() == (2, 1)
        assert fps[0].eng.L.hbmpc_pipe_fixedprep_take(fps[0].h, C.c_size_t(m), C.c_size_t(1), C.c_void_p(fp.rbits), None) == INVALID_INPUT  # not a fixedprep
        prep.run(check=True)
        assert prep.available() == (R, ni)
    finally:
        for h in fps + [prep]:
            h.close()


def test_create_refusals_and_absent_halves(pkg, engines, stream):
    fr, gl = engines
    L = fr.L
    z = C.c_size_t

    def create(a, b, n, t, nb, ni, lk):
        h = C.c_void_p(1234)
        rc = L.hbmpc_pipe_fixedprep_create(a.ctx, b.ctx, z(n), z(t), z(nb), z(ni), z(lk), C.c_void_p(stream), C.byref(h))
        assert (h.value is None) == (rc != 0), rc
        if rc == 0:
            L.hbmpc_pipe_destroy(h)
        return rc
    assert create(fr, gl, 4, 1, 4, 3, 40) == 0
    assert create(gl, fr, 4, 1, 4, 3, 40) == TYPE_MISMATCH and create(fr, fr, 4, 1, 4, 3, 40) == TYPE_MISMATCH
    assert create(gl, gl, 4, 1, 4, 3, 40) == TYPE_MISMATCH
    assert create(fr, gl, 4, 1, 0, 0, 40) == INVALID_INPUT                      # both halves absent
    assert create(fr, gl, 4, 2, 4, 3, 40) == INVALID_INPUT                      # n <= 2t
    assert create(fr, gl, 4, 1, 4, 3, 62) == fr.FIELD_CAPACITY                  # the RISS parts' capacity rule
    assert create(fr, gl, 4, 1, 0, 3, 62) == fr.FIELD_CAPACITY
    # one half absent: its parts and buffers are unknown names, the other half runs and equals the restatement
    for shape in ((4, 1, 4, 0), (4, 1, 0, 3)):
        prep = make(pkg, engines, shape, stream)
        try:
            prep.run(check=True)
            assert_same(collect(prep), expected(shape)[1], shape)
            h = C.c_void_p()
            absent = ("prandint",) if shape[3] == 0 else ("ransha", "randousha", "triplegen", "randbit", "prandbit")
            for name in absent:
                assert L.hbmpc_pipe_part(prep.h, name.encode(), C.byref(h)) == INVALID_INPUT
            for name in (("r_int",) if shape[3] == 0 else ("r_bits", "r_bits2")):
                assert L.hbmpc_pipe_buffer(prep.h, name.encode(), None, None) == INVALID_INPUT
            assert prep.available() == (FR.sizes(4, 1, shape[2])[0] if shape[2] else 0, shape[3])
        finally:
            prep.close()
    # a NULL stream: the handle works on a stream of its own
    prep = make(pkg, engines, (4, 1, 4, 3), 0)
    try:
        prep.run(check=True)
        assert_same(collect(prep), expected((4, 1, 4, 3))[1], "own stream")
    finally:
        prep.close()


def test_c1_from_polynomials_to_fixed_point_products(pkg, engines, stream):
    """config C1 (n = 4, t = 1) through handles only: the dealers' polynomials -> Preprocessing (Fr triples), FixedPrep (the pools) and an
    Fr RanSha (the input masks) -> Input of two fixed-point vectors -> FpMul, fed by take() and by device copies of the triples ->
    Output.  The client's values equal the restatement's chain bit for bit, and each lies within one unit of the last place of
    x y / 2^m: TruncPr's rounding rule (truncpr.rs:215-220), not a measured tolerance.  k, m and the value range are those of
    tests/test_gpu_pipelines.py's FPMul tests (k = 16, m = 4, values below 2^((k - 2) / 2))."""
    fr, gl = engines
    pl = pkg.pipelines
    n, t, N, k, m = 4, 1, 5, 16, 4
    rng = np.random.default_rng(41)
    half = (k - 2) // 2
    xs, ys = ([int(v) for v in rng.integers(0, 1 << half, N)] for _ in range(2))
    NT = 6                                                                       # triples: a multiple of 2t + 1 that covers N
    shape = (n, t, m * N, N)
    model, _ = expected(shape)
    pre = pl.Preprocessing(fr, n, t, NT, stream=stream)
    masks = pl.RanSha(fr, n, t, -(-2 * N // (n - 2 * t)), stream=stream)
    prep = make(pkg, engines, shape, stream)
    ix, iy = pl.Input(fr, n, t, N, stream=stream), pl.Input(fr, n, t, N, stream=stream)
    fp, op = pl.FpMul(fr, n, t, N, k, m, stream=stream), pl.Output(fr, n, t, N, stream=stream)
    handles = [pre, masks, prep, ix, iy, fp, op]
    try:
        co_rs = [[list(p) for p in row] for row in PD.honest_coeffs("fr", n, t, pre.K_rs, 3)]
        co_t, co_2t = PD.double_coeffs("fr", n, t, pre.K_rd, 4)
        co_mask = [[list(p) for p in row] for row in PD.honest_coeffs("fr", n, t, masks.K, 5)]
        as_fr = lambda co: np.stack([PR.rows_from_ints(row, "fr") for row in co])  # noqa: E731
        pre.rs.upload(as_fr(co_rs))
        pre.rd.upload(as_fr(co_t), as_fr(co_2t))
        masks.upload(as_fr(co_mask))
        pre.run(check=True)
        masks.run(check=True)
        prep.run(check=True)
        ix.upload_named("x", PR.from_ints(xs, "fr"))
        iy.upload_named("x", PR.from_ints(ys, "fr"))
        l_mask = masks.nout
        assert fr.take_rows([(masks.out, l_mask, ix.r, N, N, 1), (masks.out + N * 32, l_mask, iy.r, N, N, 1)], n, stream) == 0
        ix.run(check=True)
        iy.run(check=True)
        assert fr.take_rows([(ix.out, N, fp.x, N, N, 1), (iy.out, N, fp.y, N, N, 1), (pre.tg.a, NT, fp.ta, N, N, 1), (pre.tg.b, NT, fp.tb, N, N, 1),
                             (pre.tg.c, NT, fp.tc, N, N, 1)], n, stream) == 0
        prep.take(fp)
        fp.run(check=True)
        fr.d2d(op.sh, fp.out, n * N * 32, stream)
        op.run(check=True)
        got = PR.to_ints(op.download(), "fr")
        # the restatement's chain on the secrets (every step is linear in the shares or an open): z = x y by Beaver, then TruncPr with
        # r' = sum_j 2^j bit_j and r'' = the PRandInt integer (truncpr.rs:215-220, 277-297 through oracle/spec.py)
        bits, _ = PR.recovered_bits(n, t, model["prandbit"])
        sums = model["prandint"]["sums"]
        want = []
        for i in range(N):
            z = xs[i] * ys[i] % S.R_MOD
            r_dash = sum(bits[i * m + j] << j for j in range(m))
            r_int = sum(sums[s][i] for s in range(len(sums))) % S.R_MOD
            c_open = (z + S.pow2_f(k - 1) + r_int * S.pow2_f(m) + r_dash) % S.R_MOD
            want.append((z - (S.mod_pow_2_from_field(c_open, m) - r_dash)) * S.inv(S.pow2_f(m)) % S.R_MOD)
        assert got == want
        for v, x, y in zip(got, xs, ys):
            assert v in ((x * y) >> m, ((x * y) >> m) + 1), (v, x, y)
        assert prep.available() == (0, 0)
    finally:
        for h in handles:
            h.close()
