"""hbmpc_dev_fpmul_parties and hbmpc_[gl_]dev_mul_parties with sender sets that are no prefix 0 .. S - 1 (tests/sender_sets.py), in
every form the calls have: FpMul's one launch, its four launches (the decode's pair form) and its five, Mul with an OEC round.
sender_ids are PARTY ids: every form opens from exactly those parties' rows of the [party][..] arrays.

Every caller-visible buffer, status byte and summary is compared with the oracle composition of tests/sender_sets.py --
never with another form of the library alone -- and then the forms with each other, byte for byte.  tests/test_sender_sets.py
proves without a GPU that on these inputs a call that read rows 0 .. S - 1, or decoded with the prefix's table, differs from that
composition at every chunk of both opens."""
import ctypes as C

import numpy as np
import pytest

from oracle import cref as O
from tests import sender_sets as SS
from tests import test_gpu_mul as M
from tests import test_gpu_wave_edges as W
from tests.test_gpu_mul import pkg_eng, pkg_gl  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
K, MB = SS.K_BITS, SS.M_BITS
INPUTS = ("ta", "tb", "tc", "x", "y", "rbits", "rint")
OUTPUTS = {"deop": lambda n, N: (2 * N,), "z": lambda n, N: (n, N), "rdash": lambda n, N: (n, N), "osh": lambda n, N: (n, N), "cop": lambda n, N: (N,),
           "out": lambda n, N: (n, N)}
ALL = W.FPMUL_NAMES + ("status", "summary", "summary_first")


def raw_fpmul(eng, fp, ids, n, t, N, k=K, m=MB):
    b = {nm: fp.buffer(nm)[0] for nm in INPUTS + ("desh", "deop", "z", "rdash", "osh", "cop", "out", "status", "summary_first", "summary")}
    return eng.dev_fpmul_parties(list(ids), b["ta"], b["tb"], b["tc"], b["x"], b["y"], b["rbits"], b["rint"], k, m, N, n, t, b["desh"], b["deop"], b["z"],
                                 b["rdash"], b["osh"], b["cop"], b["out"], b["status"], b["summary_first"], b["summary"])


def five_launches(form, S, t, N):
    """whether the call writes its [party][2][N] workspace under this setting: the one launch needs exactly 2t + 1 senders, the
    decode's pair form (four launches) those, t + 1 <= 11 and whole 32-element tiles"""
    return S != 2 * t + 1 or form == "five" or (form == "four" and (t + 1 > 11 or N % 32 != 0))


def run_fpmul_ids(pkg, eng, n, t, N, ins, ids):
    """the raw call with these party ids under the three settings of W.FPMUL_FORMS; every output holds a marker before each call
    and which form ran is asserted from the workspace.  {form: buffers}; defaults restored"""
    S, res = len(ids), {}
    marker = {nm: O.fill_random(900 + j, int(np.prod(sh(n, N)))).reshape(sh(n, N) + (4,)) for j, (nm, sh) in enumerate(OUTPUTS.items())}
    marker["desh"] = O.fill_random(77, 2 * n * N).reshape(n, 2, N, 4)
    try:
        for form, (fused, pair_min) in W.FPMUL_FORMS.items():
            assert eng.L.hbmpc_set_fused_fpmul(eng.ctx, C.c_size_t(fused)) == 0
            assert eng.L.hbmpc_set_fpmul_pair_decode(eng.ctx, C.c_size_t(pair_min)) == 0
            eng.set_matrix_cores(True, 32 if form == "four" else 65536)
            fp = pkg.pipelines.FpMul(eng, n, t, N, K, MB, open_senders=S)
            try:
                fp.upload(ins["x"], ins["y"], ins["ta"], ins["tb"], ins["tc"], np.ascontiguousarray(ins["rbits"]), ins["rint"])
                for nm, arr in marker.items():
                    fp.upload_named(nm, arr)
                eng.h2d(fp.buffer("status")[0], np.full(2 * N, 0x5A, dtype=np.uint8))
                for nm in ("summary", "summary_first"):
                    eng.h2d(fp.buffer(nm)[0], np.full(4, 0x5A5A5A5A, dtype=np.uint32))
                eng.sync()
                assert raw_fpmul(eng, fp, ids, n, t, N) == 0, form
                wrote_desh = not np.array_equal(fp.download_named("desh", (n, 2, N)), marker["desh"])
                assert wrote_desh == five_launches(form, S, t, N), ("which form ran", form)
                got = {nm: fp.download_named(nm, (N,) if nm in ("dop", "eop", "cop") else (n, N)).copy() for nm in W.FPMUL_NAMES}
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


def check_fpmul_ids(pkg, eng, n, t, N, ins, ids, tag):
    """every form against the oracle's composition for these senders, then the forms with each other"""
    want = SS.fpmul_expected(ins, n, t, N, K, MB, ids)
    res = run_fpmul_ids(pkg, eng, n, t, N, ins, ids)
    for form, got in res.items():
        for nm in W.FPMUL_NAMES + ("status",):
            assert np.array_equal(got[nm], want[nm]), (tag, form, nm)
        assert got["summary_first"].tolist()[1:] == want["summary_first"] and got["summary"].tolist()[1:] == want["summary"], (tag, form)
    W.assert_forms_agree(res, ALL, tag)
    return want


def fpmul_honest_outsider_liars(pkg, eng, n, t, N, S=None):
    """honest senders and a party outside the set whose every share of x, ta and r_int is wrong: nothing fails and the opens are
    the honest ones; then the two liars inside the set.  Returns the oracle's results for the lies and the chunks lied about."""
    ids = SS.sender_set(n, t, S)
    ins = SS.fpmul_inputs(n, t, N)
    honest = SS.fpmul_expected(ins, n, t, N, K, MB, ids)
    want = check_fpmul_ids(pkg, eng, n, t, N, SS.with_wrong_outsider(ins, n, ids, ("x", "ta", "rint")), ids, ("outsider", n, t, N))
    assert want["summary_first"] == want["summary"] == W.NOTHING_FAILED[1:] and not want["status"].any()
    for nm in ("dop", "eop", "cop"):
        assert np.array_equal(want[nm], honest[nm]), nm
    lied, first, second = SS.fpmul_with_liars(ins, ids, t, N)
    return honest, check_fpmul_ids(pkg, eng, n, t, N, lied, ids, ("liars", n, t, N)), first, second


def assert_liars_fail(want, N, first, second):
    """from 2t + 1 senders: exactly the chunks lied about fail, open to zero, and the later steps ran on that zero (z, r', the
    opened share and the output are the oracle's, which computed them from those zeros)"""
    assert want["summary_first"] == [2, first[0], 8] and want["summary"] == [2, second[0], 8]
    assert np.flatnonzero(want["status"][:N]).tolist() == second and (N + np.flatnonzero(want["status"][N:])).tolist() == [c for c in first if c >= N]
    assert not np.concatenate([want["dop"], want["eop"]])[first].any() and not want["cop"][second].any()


@pytest.mark.parametrize("n,t", [(7, 2), (16, 5), (31, 10)])
def test_fpmul_every_form(pkg_eng, n, t):
    """S = 2t + 1 and N = 32, whole 32-element tiles: one launch, four (t + 1 = 3, 6 and 11, the last size the pair form takes) and five"""
    pkg, eng = pkg_eng
    _, want, first, second = fpmul_honest_outsider_liars(pkg, eng, n, t, 32)
    assert_liars_fail(want, 32, first, second)


@pytest.mark.parametrize("n,t,N", [(40, 13, 32), (7, 2, 33)])
def test_fpmul_four_falls_back_to_five(pkg_eng, n, t, N):
    """t + 1 = 14 > 11, and a batch that is no whole number of tiles: the four-launch setting runs the five launches -- the same call
    with the same senders must open the same values whatever the batch size and the thresholds"""
    pkg, eng = pkg_eng
    assert five_launches("four", 2 * t + 1, t, N)
    _, want, first, second = fpmul_honest_outsider_liars(pkg, eng, n, t, N)
    assert_liars_fail(want, N, first, second)


def test_fpmul_with_an_oec_round(pkg_eng):
    """S = 2t + 2 at (7, 2): separate launches whatever the setting, and the liars' chunks are repaired as the oracle repairs them"""
    pkg, eng = pkg_eng
    n, t, N = 7, 2, 32
    honest, want, first, second = fpmul_honest_outsider_liars(pkg, eng, n, t, N, S=2 * t + 2)
    assert want["summary_first"] == want["summary"] == W.NOTHING_FAILED[1:]
    assert np.flatnonzero(want["status"][:N]).tolist() == second and set(want["status"][second]) == {1} and want["status"][N + 5] == 1
    for nm in ("dop", "eop", "cop"):
        assert np.array_equal(want[nm], honest[nm]), nm
    truthful = [p for p in range(n) if p not in SS.liars(SS.sender_set(n, t, 2 * t + 2), t)]
    assert np.array_equal(want["out"][truthful], honest["out"][truthful])          # (a liar's own output share follows its own inputs)


def test_fpmul_refused_calls(pkg_eng):
    """a null sender_ids, an unsorted list with a duplicate, one with an id = n: InvalidInput (4) under both hbmpc_set_fused_fpmul
    settings, and the opened values and the output keep their markers"""
    pkg, eng = pkg_eng
    n, t, N = 7, 2, 32
    ins = SS.fpmul_inputs(n, t, N)
    marker = {"deop": O.fill_random(300, 2 * N), "out": O.fill_random(301, n * N).reshape(n, N, 4)}
    fp = pkg.pipelines.FpMul(eng, n, t, N, K, MB)
    try:
        fp.upload(ins["x"], ins["y"], ins["ta"], ins["tb"], ins["tc"], np.ascontiguousarray(ins["rbits"]), ins["rint"])
        for nm, arr in marker.items():
            fp.upload_named(nm, arr)
        eng.sync()
        b = [fp.buffer(nm)[0] for nm in INPUTS]
        outs = [fp.buffer(nm)[0] for nm in ("desh", "deop", "z", "rdash", "osh", "cop", "out", "status", "summary_first", "summary")]
        for fused in (1 << 20, 0):
            assert eng.L.hbmpc_set_fused_fpmul(eng.ctx, C.c_size_t(fused)) == 0
            assert eng.L.hbmpc_dev_fpmul_parties(eng.ctx, None, C.c_size_t(2 * t + 1), *(C.c_void_p(p) for p in b), C.c_size_t(K), C.c_size_t(MB),
                                                 C.c_size_t(N), C.c_size_t(n), C.c_size_t(t), *(C.c_void_p(p) for p in outs), C.c_void_p(0)) == 4
            assert raw_fpmul(eng, fp, (6, 1, 3, 1, 4), n, t, N) == 4 and raw_fpmul(eng, fp, (6, 1, 3, 0, n), n, t, N) == 4
        eng.sync()
        assert np.array_equal(fp.download_named("deop", (2 * N,)), marker["deop"]) and np.array_equal(fp.download_named("out", (n, N)), marker["out"])
    finally:
        eng.L.hbmpc_set_fused_fpmul(eng.ctx, C.c_size_t(2048))
        fp.close()


@pytest.mark.parametrize("field", ["fr", "goldilocks"])
def test_mul_with_an_oec_round(pkg_eng, pkg_gl, field):
    """Mul from the (7, 2) set of 2t + 2 senders, one of which lies about a at element 3 and one about b at element 5; the party
    outside the set holds wrong shares of a throughout.  Both threshold settings (with an OEC round the call is never one launch):
    the chunks are repaired exactly as the oracle repairs them"""
    (pkg, eng), F = (pkg_eng, M.FR) if field == "fr" else (pkg_gl, M.GL)
    n, t, N = 7, 2, 30
    ids = SS.sender_set(n, t, 2 * t + 2)
    honest_ins = M.inputs(F, n, t, N, 4242)
    honest = M.expected(F, honest_ins, n, t, N, ids)
    ins = M.tampered(honest_ins)
    ver, low = SS.liars(ids, t)
    out_p = SS.outsiders(n, ids)[0]
    ins["ta"][out_p] = ins["ta"][(out_p + 1) % n]
    ins["ta"][ver, 3] = ins["ta"][(ver + 1) % n, 3]
    ins["tb"][low, 5] = ins["tb"][(low + 1) % n, 5]
    want = M.expected(F, ins, n, t, N, ids)
    assert want["rc"] == 0 and np.flatnonzero(want["status"]).tolist() == [3, N + 5] and set(want["status"][[3, N + 5]]) == {1}
    assert np.array_equal(want["deop"], honest["deop"])
    mp = pkg.pipelines.Mul(eng, n, t, N, open_senders=len(ids))
    got = {}
    try:
        mp.upload(ins["x"], ins["y"], ins["ta"], ins["tb"], ins["tc"])
        for form, fused in M.FORMS:
            eng.set_fused_mul(fused)
            eng.h2d(mp.out, F.zeros((n, N)))
            eng.h2d(mp.deop, F.zeros((2 * N,)))
            assert M.raw_call(eng, mp, ids, n, t, N) == 0
            got[form] = M.collect(eng, mp)
            M.assert_equals_oracle(got[form], want, form)
            assert got[form]["summary"].tolist() == [2, 0, 0xffffffff, 0], form      # two chunks through the fallback, none failed
        M.assert_same_bytes(got, ids)
    finally:
        eng.set_fused_mul(pkg.hbmpc.FUSED_MUL_DEFAULT)
        mp.close()
