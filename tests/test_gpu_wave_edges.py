"""The wave-per-element kernels (k_mul_wave, k_truncpr_wave with and without a multiplier, k_fpmul_wave, k_triplegen_wg) and
their multi-launch forms (k_truncpr_front among them) on the adversarial inputs of tests/edge_inputs.py: constant and forced
sharings of edge values, inputs solved so that the intermediates ARE edge values (differences of 0, 1, 2^232, values between
0x73EDA7 2^232 and r, all-ones limbs), and single-bit tampering.  tests/test_edge_inputs.py proves without a GPU that those inputs
reach every listed intermediate with every listed value.

Every caller-visible buffer, status byte and summary of every form is compared with the composition of oracle calls and Python
integers that the call replaces -- never with another form of the library alone -- and then the forms with each other, byte for
byte.  No element is left out of a comparison."""
import ctypes as C

import numpy as np
import pytest

from oracle import cref as O
from tests import edge_inputs as X
from tests import test_gpu_mul as M
from tests import test_gpu_truncpr as T
from tests.sender_sets import fpmul_expected, fpmul_inputs, summary_tail
from tests.test_gpu_mul import pkg_eng, pkg_gl  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
NOTHING_FAILED = [0, 0, 0xffffffff, 0]
NEVER = (1 << 64) - 1


def arrays(F, case, n):
    """the case's nested lists of integers as the arrays the calls take"""
    out = {}
    for nm, v in case["ins"].items():
        if nm == "rbits" and not v[0]:
            out[nm] = np.zeros((n, 0, case["N"], 4), dtype=np.uint64)
        else:
            out[nm] = None if v is None else F.arr(v)
    return out


# ---- Mul -------------------------------------------------------------------------------------------------------------------------
def run_mul(pkg, eng, F, n, t, N, ins, ids, forms=M.FORMS, desh_marker=None):
    """hbmpc_[gl_]dev_mul_parties with these sender ids under each threshold setting; {form: buffers}.  desh_marker: what the
    separate launches' workspace holds before each call (the one launch leaves it alone), returned as "desh" """
    mp = pkg.pipelines.Mul(eng, n, t, N)
    got = {}
    try:
        mp.upload(ins["x"], ins["y"], ins["ta"], ins["tb"], ins["tc"])
        for form, fused in forms:
            eng.set_fused_mul(fused)
            eng.h2d(mp.out, F.arr([[0] * N] * n))
            eng.h2d(mp.deop, F.arr([0] * (2 * N)))
            if desh_marker is not None:
                mp.upload_named("desh", desh_marker)
            assert M.raw_call(eng, mp, ids, n, t, N) == 0
            got[form] = M.collect(eng, mp)
            if desh_marker is not None:
                got[form]["desh"] = mp.download("desh").copy()
    finally:
        eng.set_fused_mul(pkg.hbmpc.FUSED_MUL_DEFAULT)
        mp.close()
    return got


def mul_all_forms(pkg, eng, n, t, N, ins, ids):
    """one launch and three on the u29 context, three on sat32"""
    res = run_mul(pkg, eng, X.FR, n, t, N, ins, ids)
    eng.set_impl("sat32")
    try:
        res["sat32"] = run_mul(pkg, eng, X.FR, n, t, N, ins, ids, forms=M.FORMS[1:])["multi"]
    finally:
        eng.set_impl("u29")
    return res


def assert_forms_agree(res, names, tag):
    base = next(iter(res))
    for form, got in res.items():
        for nm in names:
            assert np.array_equal(got[nm], res[base][nm]), (tag, form, nm)


MUL_BUFFERS = ("out", "deop", "dop", "eop", "status", "summary")


@pytest.mark.parametrize("n,t,senders", X.MUL_SHAPES)
def test_mul_edges(pkg_eng, n, t, senders):
    """(4, 1): no lane sharing; (16, 5): quads; (31, 10): pairs; (46, 15): the tail load loop; (64, 21): 22-term rows, a lane per row
    (all-ones limbs in every term: the fold interval is crossed three times); (7, 2): senders unsorted and no prefix"""
    pkg, eng = pkg_eng
    case = X.mul_case(X.FR, n, t, senders)
    ins, N = arrays(X.FR, case, n), case["N"]
    want = M.expected(X.FR, ins, n, t, N, senders)
    assert want["rc"] == 0 and not want["status"].any()
    res = mul_all_forms(pkg, eng, n, t, N, ins, senders)
    for form, got in res.items():
        M.assert_equals_oracle(got, want, form)
        assert got["summary"].tolist() == NOTHING_FAILED, form
        z = X.FR.ints(got["out"])                                                        # and z is what the inputs were solved for
        assert all(z[p][g] == X.mul_sites(X.FR, col, n, t, senders)["z"][p] for g, col in enumerate(case["cols"]) for p in (0, n - 1)), form
    assert_forms_agree(res, MUL_BUFFERS, (n, t))


@pytest.mark.parametrize("n,t,senders", X.MUL_SHAPES)
def test_mul_edges_goldilocks(pkg_gl, n, t, senders):
    """hbmpc_gl_dev_mul_parties with the Goldilocks classes (0, 1, 2^32 +- 1, 2^63, p - 2^32, p - 1, ...)"""
    pkg, eng = pkg_gl
    case = X.mul_case(X.GL, n, t, senders)
    ins, N = arrays(X.GL, case, n), case["N"]
    want = M.expected(X.GL, ins, n, t, N, senders)
    assert want["rc"] == 0 and not want["status"].any()
    res = run_mul(pkg, eng, X.GL, n, t, N, ins, senders)
    for form, got in res.items():
        M.assert_equals_oracle(got, want, form)
        assert got["summary"].tolist() == NOTHING_FAILED, form
    assert_forms_agree(res, MUL_BUFFERS, (n, t))


# ---- TruncPr and FPDivConst --------------------------------------------------------------------------------------------------------
def truncpr_all_forms(pkg, eng, n, t, N, k, m, ins, check=False):
    """one launch and three on the u29 context, three on sat32"""
    res = T.run_forms(pkg, eng, n, t, N, k, m, ins, check=check)
    eng.set_impl("sat32")
    try:
        res["sat32"] = T.run_forms(pkg, eng, n, t, N, k, m, ins)["three"]
    finally:
        eng.set_impl("u29")
    return res


def check_truncpr(pkg, eng, n, t, senders, k, m, with_w, count, rot):
    case = X.truncpr_case(n, t, senders, k, m, with_w, count, rot)
    ins, N = arrays(X.FR, case, n), case["N"]
    want = T.expected(ins, n, t, N, k, m, len(senders))
    assert want["rc"] == 0 and not want["status"].any()
    res = truncpr_all_forms(pkg, eng, n, t, N, k, m, ins)
    names = (("c",) if with_w else ()) + ("rdash", "osh", "cop", "out", "status", "summary")
    for form, got in res.items():
        T.assert_equals_oracle(got, want, with_w, (form, n, t, k, m))
        assert got["summary"].tolist() == NOTHING_FAILED, (form, n, t, k, m)
    assert_forms_agree(res, names, (n, t, k, m, with_w))


@pytest.mark.parametrize("with_w", [False, True], ids=["truncpr", "fpdivconst"])
@pytest.mark.parametrize("m", X.TRUNCPR_M)
def test_truncpr_edges(pkg_eng, m, with_w):
    """m on both sides of every fold boundary of r' (6 terms between folds), at (4, 1), (16, 5), (31, 10), (64, 21); k in {1, 32, 250};
    w in {0, 1, r - 1, MAXLIMB, 2^128 - 1}; every bit share MAXLIMB, then r - 1; the maximal four-term loose sum"""
    pkg, eng = pkg_eng
    for si, (n, t) in enumerate(X.TRUNCPR_SHAPES):
        check_truncpr(pkg, eng, n, t, tuple(range(2 * t + 1)), X.truncpr_k(with_w, m, si), m, with_w, 0, 0)


@pytest.mark.parametrize("with_w", [False, True], ids=["truncpr", "fpdivconst"])
def test_truncpr_wide_moduli(pkg_eng, with_w):
    """m in {29, 31, 32, 33, 64, 232, 254, 255, 256, 264}: the mask of c mod 2^m on both sides of a word and of r's width, four
    elements each at (4, 1); whichever form the library takes there, the bytes are the oracle's"""
    pkg, eng = pkg_eng
    cases = [c for c in X.truncpr_cases() if c[6] and c[5] == with_w]
    assert [c[4] for c in cases] == list(X.TRUNCPR_WIDE_M)
    for case in cases:
        check_truncpr(pkg, eng, *case)


# ---- FpMul -----------------------------------------------------------------------------------------------------------------------
FPMUL_FORMS = {"one": (1 << 20, NEVER), "four": (0, 0), "five": (0, NEVER)}      # hbmpc_set_fused_fpmul, hbmpc_set_fpmul_pair_decode
FPMUL_NAMES = ("dop", "eop", "z", "rdash", "osh", "cop", "out")


def run_fpmul(pkg, eng, n, t, N, k, m, ins, forms_known=True, forms=tuple(FPMUL_FORMS)):
    """the three forms, set as tests/test_gpu_pipelines.py::test_fpmul_one_launch_equals_five sets them; defaults restored"""
    res = {}
    marker = O.fill_random(77, 2 * n * N).reshape(n, 2, N, 4)
    try:
        for form, (fused, pair_min) in ((f, FPMUL_FORMS[f]) for f in forms):
            assert eng.L.hbmpc_set_fused_fpmul(eng.ctx, C.c_size_t(fused)) == 0
            assert eng.L.hbmpc_set_fpmul_pair_decode(eng.ctx, C.c_size_t(pair_min)) == 0
            eng.set_matrix_cores(True, 32 if form == "four" else 65536)
            fp = pkg.pipelines.FpMul(eng, n, t, N, k, m)
            try:
                fp.upload(ins["x"], ins["y"], ins["ta"], ins["tb"], ins["tc"], np.ascontiguousarray(ins["rbits"]), ins["rint"])
                fp.upload_named("desh", marker)                   # the five launches' workspace: the one launch leaves it alone
                fp.run(check=False)
                wrote_desh = not np.array_equal(fp.download_named("desh", (n, 2, N)), marker)
                if forms_known:                                   # (the four-launch form: t + 1 <= 11 and whole 32-element tiles)
                    assert wrote_desh == (form == "five" or (form == "four" and (t + 1 > 11 or N % 32 != 0))), ("which form ran", form)
                got = {nm: fp.download_named(nm, (N,) if nm in ("dop", "eop", "cop") else (n, N)).copy() for nm in FPMUL_NAMES}
                for nm, arr in (("status", np.zeros(2 * N, dtype=np.uint8)), ("summary", np.zeros(4, dtype=np.uint32)), ("summary_first", np.zeros(4, dtype=np.uint32))):
                    eng.d2h(arr, fp.buffer(nm)[0])
                    got[nm] = arr
                eng.sync()
                res[form] = got
            finally:
                fp.close()
    finally:
        eng.L.hbmpc_set_fused_fpmul(eng.ctx, C.c_size_t(2048))
        eng.L.hbmpc_set_fpmul_pair_decode(eng.ctx, C.c_size_t(8192))
        eng.set_matrix_cores(True, 65536)
    return res


def check_fpmul(pkg, eng, n, t, N, k, m, ins, tag, forms_known=True, forms=tuple(FPMUL_FORMS)):
    want = fpmul_expected(ins, n, t, N, k, m)
    res = run_fpmul(pkg, eng, n, t, N, k, m, ins, forms_known, forms)
    for form, got in res.items():
        for nm in FPMUL_NAMES + ("status",):
            assert np.array_equal(got[nm], want[nm]), (tag, form, nm)
        assert got["summary_first"].tolist()[1:] == want["summary_first"] and got["summary"].tolist()[1:] == want["summary"], (tag, form)
    assert_forms_agree(res, FPMUL_NAMES + ("status", "summary", "summary_first"), tag)
    return want


@pytest.mark.parametrize("n,t,k,m", X.FPMUL_SHAPES)
def test_fpmul_edges(pkg_eng, n, t, k, m):
    """the union of the Mul and the TruncPr inputs (whole 32-element tiles, so that the four-launch form is one), each form against
    the full oracle composition; then one case of uniform elements through the same comparison"""
    pkg, eng = pkg_eng
    case = X.fpmul_case(n, t, tuple(range(2 * t + 1)), k, m, tile=32)
    ins, N = arrays(X.FR, case, n), case["N"]
    want = check_fpmul(pkg, eng, n, t, N, k, m, ins, ("edge", n, t))
    assert want["summary_first"] == NOTHING_FAILED[1:] and want["summary"] == NOTHING_FAILED[1:]
    N = 32
    names = ("x", "y", "ta", "tb", "tc", "rint")
    rnd = {nm: T.share_all(O.fill_random(40 + j, N), n, t, 50 + j) for j, nm in enumerate(names)}
    rnd["rbits"] = np.stack([T.share_all(O.fill_random(60 + j, N), n, t, 80 + j) for j in range(m)], axis=1)
    check_fpmul(pkg, eng, n, t, N, k, m, rnd, ("random", n, t))


def test_fpmul_wide_moduli(pkg_eng):
    """m = 255, 256, 264, where c mod 2^m is c: every class of the opened value reaches the mask.  Whichever form the library takes"""
    pkg, eng = pkg_eng
    for n, t, k, m, count, rot in X.FPMUL_WIDE:
        case = X.fpmul_case(n, t, (0, 1, 2), k, m, count, rot)
        check_fpmul(pkg, eng, n, t, case["N"], k, m, arrays(X.FR, case, n), ("wide", k, m), forms_known=False)


# ---- triple generation -------------------------------------------------------------------------------------------------------------
def triple_expected(F, ins, n, t, N):
    """triple_local, BatchRecon's two opens (the encode, the recipients' P(0) decodes, the coefficient decode), triple_finalize"""
    m, G, ids = 2 * t + 1, N // (2 * t + 1), list(range(n))
    loc = [F.O.triple_local(ins["a"][p], ins["b"][p], ins["r2t"][p])[1] for p in range(n)]
    Y = np.stack([F.O.vandermonde_apply(loc[p].reshape((G, m) + F.tail), n, 2 * t)[1] for p in range(n)])      # [party][recipient][chunk]
    Z, st1 = [], []
    for j in range(n):
        rc, z, st = F.O.batch_recover_p0(ids, np.ascontiguousarray(Y[:, j]), n, 2 * t, t)    # a failed chunk: zero, status = its error
        assert rc == (8 if st.any() else 0)
        Z.append(z), st1.append(st)
    Z = np.stack(Z)
    rc, opened, nco, st2 = F.O.batch_recover(ids, Z, n, 2 * t, t)
    assert rc == 0
    opened = np.ascontiguousarray(opened).reshape((N,) + F.tail)
    c = np.stack([F.O.triple_finalize(ins["rt"][p], opened)[1] for p in range(n)])
    return {"c": c, "Y": Y, "Z": Z, "opened": opened, "status": np.concatenate([st2] + st1[1:]), "status_first": np.concatenate(st1)}


TRIPLE_FORMS = (("one", 1 << 20), ("four", 0))


def run_triplegen(pkg, eng, n, t, N, ins, forms=TRIPLE_FORMS):
    G = N // (2 * t + 1)
    res = {}
    try:
        for form, fused in forms:
            assert eng.L.hbmpc_set_fused_triplegen(eng.ctx, C.c_size_t(fused)) == 0
            tg = pkg.pipelines.TripleGen(eng, n, t, N)
            try:
                tg.upload(ins["a"], ins["b"], ins["r2t"], ins["rt"])
                tg.run(check=False)
                got = {"c": tg.download_c().copy(), "Y": tg.download_named("Y", (n, n, G)).copy(), "Z": tg.download_named("Z", (n, G)).copy(),
                       "opened": tg.download_named("opened", (N,)).copy()}
                for nm, arr in (("status", np.zeros(n * G, dtype=np.uint8)), ("summary", np.zeros(4, dtype=np.uint32)), ("summary_first", np.zeros(4, dtype=np.uint32))):
                    eng.d2h(arr, tg.buffer(nm)[0])
                    got[nm] = arr
                eng.sync()
                res[form] = got
            finally:
                tg.close()
    finally:
        eng.L.hbmpc_set_fused_triplegen(eng.ctx, C.c_size_t(1024))
    return res


@pytest.mark.parametrize("field", ["fr", "goldilocks"])
@pytest.mark.parametrize("n,t", X.TRIPLE_SHAPES)
def test_triplegen_edges(pkg_eng, pkg_gl, n, t, field):
    """the one launch (n = 3t + 1 in {4, 7, 16}) and the four, each against the oracle; constant and forced sharings such that
    a_p b_p - r2t_p and opened + rt_p are edge values; c opens to a b"""
    (pkg, eng), F = (pkg_eng, X.FR) if field == "fr" else (pkg_gl, X.GL)
    case = X.triple_case(F, n, t)
    ins, N = arrays(F, case, n), case["N"]
    want = triple_expected(F, ins, n, t, N)
    assert not want["status"].any()
    res = run_triplegen(pkg, eng, n, t, N, ins)
    for form, got in res.items():
        for nm in ("c", "Y", "Z", "opened", "status"):
            assert np.array_equal(got[nm], want[nm]), (form, nm)
        assert got["summary"].tolist() == NOTHING_FAILED and got["summary_first"].tolist() == NOTHING_FAILED, form
        rc, ab, st = F.O.batch_recover_p0(list(range(n)), got["c"], n, t, t)
        secret = {nm: F.ints(F.O.batch_recover_p0(list(range(n)), ins[nm], n, t, t)[1]) for nm in ("a", "b")}
        assert rc == 0 and not st.any() and F.ints(ab) == [a * b % F.mod for a, b in zip(secret["a"], secret["b"])], form
    assert_forms_agree(res, ("c", "Y", "Z", "opened", "status", "summary", "summary_first"), (n, t, field))


# ---- single-bit tampering ----------------------------------------------------------------------------------------------------------
TAMPER_SHAPES = [(4, 1, (0, 1, 2)), (7, 2, (6, 1, 3, 0, 4)), (16, 5, tuple(range(11)))]


@pytest.mark.parametrize("n,t,senders", TAMPER_SHAPES)
def test_mul_single_bit_tampering(pkg_eng, n, t, senders):
    """a sender's share of a (behind a verify row) or of b (behind the P(0) row) with one clear bit set, bits 0, 28, 29, 57, 58, 231,
    232, 253 -- the limb boundaries of the comparison: exactly those 16 chunks fail, open to zero and are counted, as in the oracle"""
    pkg, eng = pkg_eng
    case = X.mul_tamper_case(n, t, senders)
    ins, N = arrays(X.FR, case, n), case["N"]
    want = M.expected(X.FR, ins, n, t, N, senders)
    assert want["rc"] == 8 and [int(i) for i in np.flatnonzero(want["status"])] == case["failing"]
    res = mul_all_forms(pkg, eng, n, t, N, ins, senders)
    for form, got in res.items():
        M.assert_equals_oracle(got, want, form)
        assert not got["deop"][case["failing"]].any(), form
        assert got["summary"].tolist()[1:] == summary_tail(want["status"]) == [16, case["failing"][0], 8], form
    assert_forms_agree(res, MUL_BUFFERS, (n, t))


@pytest.mark.parametrize("n,t", [(4, 1), (7, 2), (16, 5)])
def test_truncpr_single_bit_tampering(pkg_eng, n, t):
    """the same through TruncPr (the inputs make the opened share the share of a itself, so it differs in that one bit)"""
    pkg, eng = pkg_eng
    k, m, senders = 32, 6, tuple(range(2 * t + 1))
    case = X.truncpr_tamper_case(n, t, senders, k, m)
    ins, N = arrays(X.FR, case, n), case["N"]
    want = T.expected(ins, n, t, N, k, m, len(senders))
    assert want["rc"] == 8 and [int(i) for i in np.flatnonzero(want["status"])] == case["failing"]
    res = truncpr_all_forms(pkg, eng, n, t, N, k, m, ins, check=True)
    for form, got in res.items():
        T.assert_equals_oracle(got, want, False, form)
        assert not got["cop"][case["failing"]].any(), form
        assert got["summary"].tolist()[1:] == summary_tail(want["status"]) == [16, case["failing"][0], 8], form
    assert_forms_agree(res, ("rdash", "osh", "cop", "out", "status", "summary"), (n, t))


@pytest.mark.parametrize("n,t", [(4, 1), (7, 2), (16, 5)])
def test_fpmul_single_bit_tampering(pkg_eng, n, t):
    """the Mul tampering in the first open (the steps after it run on zero), then the same bits in the second open, in all three forms"""
    pkg, eng = pkg_eng
    k, m, senders = 32, 6, tuple(range(2 * t + 1))
    case = X.fpmul_tamper_case(n, t, senders, k, m)
    ins, N = arrays(X.FR, case, n), case["N"]
    want = check_fpmul(pkg, eng, n, t, N, k, m, ins, ("tamper", n, t), forms_known=True)
    assert want["summary_first"] == [16, case["failing_first"][0], 8] and want["summary"] == [16, case["failing_second"][0], 8]
    assert [int(i) for i in np.flatnonzero(want["status"][:N])] == case["failing_second"]
    assert [N + int(i) for i in np.flatnonzero(want["status"][N:])] == [c for c in case["failing_first"] if c >= N]
    assert not want["cop"][case["failing_second"]].any() and not np.concatenate([want["dop"], want["eop"]])[case["failing_first"]].any()


# ---- the decode counters behind the summaries ------------------------------------------------------------------------------------------
# A one-launch call whose opens fail, then an honest one-launch call on the same stream with nothing in between: the first must
# count exactly what the oracle fails, the second must report nothing -- the last workgroup of the first left every counter it
# used at zero.  n = 4, t = 1 and 5 elements: two workgroups (fewer than the 16 sub-tickets), the second with one live wave;
# two chunks for the workgroup kernel.  One bit of one sender's share is flipped per failing chunk.
def flip_bit(arr, party, el):
    arr[(party, el) + (0,) * (arr.ndim - 2)] ^= np.uint64(1)


def test_mul_counters_after_a_failed_call(pkg_eng):
    pkg, eng = pkg_eng
    n, t, N, ids = 4, 1, 5, (0, 1, 2)
    honest = M.inputs(M.FR, n, t, N, 9100)
    bad = M.tampered(honest)
    flip_bit(bad["ta"], 1, 4)                                                            # a - x of element 4: chunk 4
    flip_bit(bad["tb"], 2, 0)                                                            # b - y of element 0: chunk N
    marker = O.fill_random(78, 2 * n * N).reshape(n, 2, N, 4)
    for ins, failing in ((bad, [4, N]), (honest, [])):
        want = M.expected(M.FR, ins, n, t, N, ids)
        assert [int(i) for i in np.flatnonzero(want["status"])] == failing
        got = run_mul(pkg, eng, X.FR, n, t, N, ins, ids, forms=M.FORMS[:1], desh_marker=marker)["one"]
        assert np.array_equal(got["desh"], marker), "the separate launches ran"           # their workspace: the one launch leaves it alone
        M.assert_equals_oracle(got, want, failing)
        assert got["summary"].tolist()[1:] == summary_tail(want["status"]) == ([2, 4, 8] if failing else NOTHING_FAILED[1:])
    assert got["summary"].tolist() == NOTHING_FAILED
    multi = run_mul(pkg, eng, X.FR, n, t, N, honest, ids, forms=M.FORMS[1:], desh_marker=marker)["multi"]
    assert not np.array_equal(multi["desh"], marker)                                     # (the marker does tell the forms apart)


@pytest.mark.parametrize("with_w", [False, True], ids=["truncpr", "fpdivconst"])
def test_truncpr_counters_after_a_failed_call(pkg_eng, with_w):
    """(the call has no workspace and every buffer holds the same bytes in both forms, so nothing a caller can see tells which form
    ran: that this shape under this threshold takes the one launch is pinned by tests/test_protocol_routes.py on the planner itself)"""
    pkg, eng = pkg_eng
    n, t, N, k, m = 4, 1, 5, 32, 4
    honest = T.random_inputs(n, t, N, m, 9200, with_w)
    bad = dict(honest, a=honest["a"].copy())
    flip_bit(bad["a"], 1, 4)
    for ins, failing in ((bad, [4]), (honest, [])):
        want = T.expected(ins, n, t, N, k, m, 2 * t + 1)
        assert [int(i) for i in np.flatnonzero(want["status"])] == failing
        got = T.run_forms(pkg, eng, n, t, N, k, m, ins, forms=T.FORMS[:1])["one"]
        T.assert_equals_oracle(got, want, with_w, failing)
        assert got["summary"].tolist()[1:] == summary_tail(want["status"]) == ([1, 4, 8] if failing else NOTHING_FAILED[1:])
    assert got["summary"].tolist() == NOTHING_FAILED


def test_fpmul_counters_after_a_failed_call(pkg_eng):
    """both pairs of counters: the first open's ([24], [25]) and the second's ([0], [1])"""
    pkg, eng = pkg_eng
    n, t, N, k, m = 4, 1, 5, 32, 4
    honest = fpmul_inputs(n, t, N, m)
    bad = {nm: v.copy() for nm, v in honest.items()}
    flip_bit(bad["ta"], 1, 4)                                                            # the first open, chunk 4
    flip_bit(bad["rint"], 2, 2)                                                          # the second open, chunk 2
    for ins, first, second in ((bad, [1, 4, 8], [1, 2, 8]), (honest, NOTHING_FAILED[1:], NOTHING_FAILED[1:])):
        want = check_fpmul(pkg, eng, n, t, N, k, m, ins, ("counters", first), forms=("one",))   # (asserts that the one launch ran)
        assert want["summary_first"] == first and want["summary"] == second


@pytest.mark.parametrize("field", ["fr", "goldilocks"])
def test_triplegen_counters_after_a_failed_call(pkg_eng, pkg_gl, field):
    """the recipients' decodes ([24], [25]).  The revealed values' decode ([0], [1]) reads what the kernel itself wrote -- every
    party is a sender of every recipient's decode, so a tampered chunk reveals n zeros, which lie on the zero polynomial: no input
    makes it fail.  (Y, Z and c hold the same bytes in both forms -- c is the four launches' workspace before it is their output -- so
    which form ran is pinned by tests/test_protocol_routes.py on the planner, not here)"""
    (pkg, eng), F = (pkg_eng, M.FR) if field == "fr" else (pkg_gl, M.GL)
    n, t, G = 4, 1, 2
    N = G * (2 * t + 1)
    r = F.O.fill_random(9402, N)
    honest = {"a": F.share_all(F.O.fill_random(9400, N), n, t, 9410), "b": F.share_all(F.O.fill_random(9401, N), n, t, 9411),
              "r2t": F.share_all(r, n, 2 * t, 9412), "rt": F.share_all(r, n, t, 9413)}
    bad = {nm: v.copy() for nm, v in honest.items()}
    flip_bit(bad["a"], 1, 4)                                                             # chunk 1, for every recipient
    for ins, first in ((bad, [n, 1, 8]), (honest, NOTHING_FAILED[1:])):
        want = triple_expected(F, ins, n, t, N)
        assert summary_tail(want["status_first"]) == first and not want["status"][:G].any()
        got = run_triplegen(pkg, eng, n, t, N, ins, forms=TRIPLE_FORMS[:1])["one"]
        for nm in ("c", "Y", "Z", "opened", "status"):
            assert np.array_equal(got[nm], want[nm]), (first, nm)
        assert got["summary_first"].tolist()[1:] == first and got["summary"].tolist() == NOTHING_FAILED
    assert got["summary_first"].tolist() == NOTHING_FAILED
