"""Multiply (Beaver) for all parties on one GPU (hbmpc_[gl_]dev_mul_parties, hbmpc_pipe_mul_create): the one-launch form (a wave per
element, csrc/kernels_mul_wave.hpp) and the multi-launch form (the opened shares, the P(0) decode of 2 N values, finalize_mul)
against the oracle's restatements and Python big ints -- never against the library itself -- and against each other, byte for
byte."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from __graft_entry__ import ROOT, load_package
from oracle import cref as O
from oracle import cref_gl as OG
from oracle import spec as S
from tests import sender_sets as SS

pytestmark = pytest.mark.gpu
FORMS = (("one", 1 << 20), ("multi", 0))      # hbmpc_set_fused_mul: always (where the call qualifies) / never


class Field:
    def __init__(self, name, oracle, mod, tail):
        self.name, self.O, self.mod, self.tail = name, oracle, mod, tail

    def from_ints(self, vals):
        return O.ints_to_u256(vals) if self.tail else np.array(vals, dtype=np.uint64)

    def to_ints(self, arr):
        return O.u256_to_ints(arr) if self.tail else [int(v) for v in np.asarray(arr).reshape(-1)]

    def zeros(self, shape):
        return np.zeros(tuple(shape) + self.tail, dtype=np.uint64)

    def share_all(self, secrets, n, d, seed):
        """[n][N] degree-d sharings of N secrets (random higher coefficients), via the oracle"""
        N = secrets.shape[0]
        co = self.O.fill_random(seed, N * (d + 1)).reshape((N, d + 1) + self.tail)
        co[:, 0] = secrets
        rc, sh = self.O.compute_shares(co, n, d)
        assert rc == 0
        return sh


FR = Field("fr", O, S.R_MOD, (4,))
GL = Field("goldilocks", OG, OG.P, ())


@pytest.fixture(scope="module")
def pkg_eng():
    pkg = load_package()
    e = pkg.Engine(0)
    yield pkg, e
    e.close()


@pytest.fixture(scope="module")
def pkg_gl():
    pkg = load_package()
    e = pkg.Engine(0, field="goldilocks")
    yield pkg, e
    e.close()


_inputs = {}


def inputs(F, n, t, N, seed):
    """x, y and a triple (a, b, c = a b in plain integers) as degree-t sharings of uniform elements; computed once per shape and
    never modified (tests that tamper take copies)"""
    key = (F.name, n, t, N, seed)
    if key not in _inputs:
        sec = {nm: F.O.fill_random(seed + j, N) for j, nm in enumerate(("x", "y", "ta", "tb"))}
        ints = {nm: F.to_ints(v) for nm, v in sec.items()}
        sec["tc"] = F.from_ints([a * b % F.mod for a, b in zip(ints["ta"], ints["tb"])])
        ins = {nm: F.share_all(v, n, t, seed + 10 + j) for j, (nm, v) in enumerate(sec.items())}
        ins["xy"] = [a * b % F.mod for a, b in zip(ints["x"], ints["y"])]
        _inputs[key] = ins
    return _inputs[key]


def tampered(ins):
    return {nm: (v.copy() if isinstance(v, np.ndarray) else v) for nm, v in ins.items()}


def expected(F, ins, n, t, N, ids):
    """the composition of oracle calls that the call replaces: the shares every party opens, the P(0) decode of the senders' 2 N
    values, finalize_mul per party"""
    desh = []
    for p in range(n):
        rc, d_sh, e_sh = F.O.beaver_open_shares(ins["ta"][p], ins["tb"][p], ins["x"][p], ins["y"][p])
        assert rc == 0
        desh.append(np.concatenate([d_sh, e_sh]))
    desh = np.stack(desh)                                                          # [party][2 N]
    rows = np.ascontiguousarray(desh[[min(i, n - 1) for i in ids]])                 # the senders' rows (an id >= n is refused anyway)
    rc, de, st = F.O.batch_recover_p0(list(ids), rows, n, t, t)                     # a failed chunk: zero, status = its error
    if rc not in (0, 8):
        return {"rc": rc}
    out = np.stack([F.O.beaver_finalize(ins["tc"][p], ins["x"][p], ins["y"][p], de[:N], de[N:])[1] for p in range(n)])
    return {"out": out, "deop": de, "status": st, "rc": rc}


def collect(eng, mp, stream=0):
    N = mp.N
    got = {nm: mp.download(nm).copy() for nm in ("out", "deop", "dop", "eop")}
    for nm, arr in (("status", np.zeros(2 * N, dtype=np.uint8)), ("summary", np.zeros(4, dtype=np.uint32))):
        eng.d2h(arr, mp.buffer(nm)[0], stream)
        got[nm] = arr
    eng.sync(stream)
    assert np.array_equal(got["dop"], got["deop"][:N]) and np.array_equal(got["eop"], got["deop"][N:])
    return got


def run_forms(pkg, eng, F, n, t, N, ins, open_senders=None, stream=0, check=False, graph=False):
    """the same inputs through both forms; returns {form: buffers}.  The default threshold is put back."""
    res = {}
    try:
        for form, fused in FORMS:
            eng.set_fused_mul(fused)
            mp = pkg.pipelines.Mul(eng, n, t, N, stream=stream, open_senders=open_senders)
            try:
                mp.upload(ins["x"], ins["y"], ins["ta"], ins["tb"], ins["tc"])
                if check:
                    with pytest.raises(RuntimeError, match="ShareErrorCode 8"):     # the decode's error: DecodingError
                        mp.run(check=True)
                mp.run(check=False)
                res[form] = collect(eng, mp, stream)
                if graph:
                    mp.capture()
                    eng.h2d(mp.out, F.zeros((n, N)), stream)
                    mp.replay()
                    again = collect(eng, mp, stream)
                    for nm in again:
                        assert np.array_equal(again[nm], res[form][nm]), (form, nm)
            finally:
                mp.close()
    finally:
        eng.set_fused_mul(pkg.hbmpc.FUSED_MUL_DEFAULT)
    return res


def assert_equals_oracle(got, want, tag):
    for nm in ("out", "deop", "status"):
        assert np.array_equal(got[nm], want[nm]), (tag, nm)


def assert_same_bytes(res, tag):
    for nm in res["multi"]:
        assert np.array_equal(res["one"][nm], res["multi"][nm]), (tag, nm)


def assert_opens_to_xy(F, out, ins, n, t):
    rc, p0, st = F.O.batch_recover_p0(list(range(n)), out, n, t, t)
    assert rc == 0 and not st.any() and F.to_ints(p0) == ins["xy"]


# (4, 1, 1 / 3 / 5): 1, 3 and 1 live waves in the last workgroup; (16, 5, ..): table rows shared by four lanes; (31, 10, ..): by two;
# (46, 15, ..): no sharing, and 3 P = 138 operand items reach the tail load loop; (64, 21, ..): every lane is a party; (9, 2, ..):
# n > 3t + 1; (70, 2, ..): n > 64, where "one" must take the multi-launch form
SHAPES = [(4, 1, 1), (4, 1, 3), (4, 1, 5), (7, 2, 67), (16, 5, 200), (10, 3, 33), (31, 10, 18), (46, 15, 6), (64, 21, 5), (9, 2, 20), (70, 2, 5)]


@pytest.mark.parametrize("n,t,N", SHAPES)
def test_exact_identity_both_forms(pkg_eng, n, t, N):
    """out, deop and status of both forms equal the oracle's composition, the summary says nothing failed, and the forms agree"""
    pkg, eng = pkg_eng
    ins = inputs(FR, n, t, N, 1000 * n + N)
    want = expected(FR, ins, n, t, N, range(2 * t + 1))
    assert want["rc"] == 0 and not want["status"].any()
    res = run_forms(pkg, eng, FR, n, t, N, ins)
    for form, got in res.items():
        assert_equals_oracle(got, want, form)
        assert got["summary"].tolist() == [0, 0, 0xffffffff, 0], form
    assert_same_bytes(res, (n, t, N))


@pytest.mark.parametrize("n,t,N", [(7, 2, 67), (16, 5, 200)])
def test_output_opens_to_the_product(pkg_eng, n, t, N):
    """with c = a b, the n parties' shares of z open to x y mod r"""
    pkg, eng = pkg_eng
    ins = inputs(FR, n, t, N, 1000 * n + N)
    for form, got in run_forms(pkg, eng, FR, n, t, N, ins).items():
        assert_opens_to_xy(FR, got["out"], ins, n, t)


def raw_call(eng, mp, ids, n, t, N, **kw):
    b = {nm: mp.buffer(nm)[0] for nm in ("ta", "tb", "tc", "x", "y", "desh", "deop", "out", "status", "summary")}
    b.update(kw)
    return eng.dev_mul_parties(list(ids), b["ta"], b["tb"], b["tc"], b["x"], b["y"], N, n, t, b["desh"], b["deop"], b["out"], b["status"], b["summary"])


@pytest.mark.parametrize("n,t,N,ids", [(7, 2, 30, (6, 1, 3, 0, 4)), (9, 2, 20, (8, 2, 5, 7, 0)), (31, 10, 18, SS.sender_set(31, 10))])
def test_sender_sets(pkg_eng, n, t, N, ids):
    """sender_ids are party ids, unsorted and not a prefix: both forms open from exactly those parties' shares.  A party outside
    the set holds a wrong share of a at one element: nothing may change."""
    pkg, eng = pkg_eng
    ins = tampered(inputs(FR, n, t, N, 555 + n))
    outsider = next(p for p in range(n) if p not in ids)
    ins["ta"][outsider, 2] = ins["ta"][ids[0], 2]
    want = expected(FR, ins, n, t, N, ids)
    assert want["rc"] == 0 and not want["status"].any()
    mp = pkg.pipelines.Mul(eng, n, t, N)
    got = {}
    try:
        mp.upload(ins["x"], ins["y"], ins["ta"], ins["tb"], ins["tc"])
        for form, fused in FORMS:
            eng.set_fused_mul(fused)
            eng.h2d(mp.out, FR.zeros((n, N)))
            eng.h2d(mp.deop, FR.zeros((2 * N,)))
            assert raw_call(eng, mp, ids, n, t, N) == 0
            got[form] = collect(eng, mp)
            assert_equals_oracle(got[form], want, form)
            assert got[form]["summary"].tolist() == [0, 0, 0xffffffff, 0], form
        assert_same_bytes(got, ids)
    finally:
        eng.set_fused_mul(pkg.hbmpc.FUSED_MUL_DEFAULT)
        mp.close()


@pytest.mark.parametrize("extra", [0, 1])
def test_default_threshold_boundary(pkg_eng, extra):
    """at the library's own threshold: FUSED_MUL_DEFAULT elements (the last one-launch size) and one more (the first multi-launch
    size) are both exact"""
    pkg, eng = pkg_eng
    n, t, N = 4, 1, pkg.hbmpc.FUSED_MUL_DEFAULT + extra
    ins = inputs(FR, n, t, N, 31 + extra)
    want = expected(FR, ins, n, t, N, range(2 * t + 1))
    mp = pkg.pipelines.Mul(eng, n, t, N)
    try:
        mp.upload(ins["x"], ins["y"], ins["ta"], ins["tb"], ins["tc"])
        mp.run(check=True)
        got = collect(eng, mp)
    finally:
        mp.close()
    assert_equals_oracle(got, want, N)
    assert got["summary"].tolist() == [0, 0, 0xffffffff, 0]


def test_pair_decode_size(pkg_eng):
    """8 192 elements at n = 16, t = 5: from hbmpc_set_fpmul_pair_decode's default on the multi-launch form lets the decode form
    a - x and b - y as it loads them.  Senders that are no prefix, one of them lying about b at the last element: both forms
    fail chunk 2 N - 1 alone and agree with the oracle and with each other."""
    pkg, eng = pkg_eng
    n, t, N = 16, 5, 8192
    ids = (15, 2, 3, 4, 5, 6, 7, 8, 9, 10, 0)
    ins = tampered(inputs(FR, n, t, N, 8192))
    ins["tb"][7, N - 1] = ins["tb"][1, N - 1]
    want = expected(FR, ins, n, t, N, ids)
    assert want["rc"] == 8 and [int(i) for i in np.flatnonzero(want["status"])] == [2 * N - 1]
    mp = pkg.pipelines.Mul(eng, n, t, N)
    got = {}
    try:
        mp.upload(ins["x"], ins["y"], ins["ta"], ins["tb"], ins["tc"])
        for form, fused in FORMS:
            eng.set_fused_mul(fused)
            eng.h2d(mp.out, FR.zeros((n, N)))
            assert raw_call(eng, mp, ids, n, t, N) == 0
            got[form] = collect(eng, mp)
            assert_equals_oracle(got[form], want, form)
            assert got[form]["summary"].tolist()[1:] == [1, 2 * N - 1, 8], form
        assert_same_bytes(got, "pair decode")
    finally:
        eng.set_fused_mul(pkg.hbmpc.FUSED_MUL_DEFAULT)
        mp.close()


def test_lying_sender(pkg_eng):
    """sender 1 lies about a at element 4, sender 3 about b at element 9.  Opened from 2t + 1 senders there is no OEC round: chunk
    4 and chunk N + 9 fail, open to zero, finalize_mul runs on those zeros, a checked run raises.  Opened from all n they are
    repaired."""
    pkg, eng = pkg_eng
    n, t, N = 7, 2, 30
    honest_ins = inputs(FR, n, t, N, 4242)
    honest = expected(FR, honest_ins, n, t, N, range(2 * t + 1))
    ins = tampered(honest_ins)
    ins["ta"][1, 4] = ins["ta"][2, 4]
    ins["tb"][3, 9] = ins["tb"][4, 9]
    want = expected(FR, ins, n, t, N, range(2 * t + 1))
    assert want["rc"] == 8
    res = run_forms(pkg, eng, FR, n, t, N, ins, check=True)
    for form, got in res.items():
        st = got["status"]
        assert st[4] == 8 and st[N + 9] == 8 and int(np.count_nonzero(st)) == 2, form
        assert not got["deop"][4].any() and not got["deop"][N + 9].any(), form
        assert np.array_equal(got["deop"][N + 4], honest["deop"][N + 4]) and np.array_equal(got["deop"][9], honest["deop"][9]), form
        assert got["summary"].tolist()[1:] == [2, 4, 8], form                       # n_failed, first_failed, first_error
        assert_equals_oracle(got, want, form)                                       # out: the oracle's beaver_finalize on those opened values
    assert_same_bytes(res, "2t+1 senders")
    want = expected(FR, ins, n, t, N, range(n))                                     # OEC rounds available: never the one-launch form
    assert want["rc"] == 0 and np.array_equal(want["out"], honest["out"])
    res = run_forms(pkg, eng, FR, n, t, N, ins, open_senders=n)
    for form, got in res.items():
        st = got["status"]
        assert st[4] == 1 and st[N + 9] == 1 and int(np.count_nonzero(st)) == 2, form
        assert got["summary"].tolist()[1] == 0, form
        assert_equals_oracle(got, want, form)
    assert_same_bytes(res, "n senders")


def test_refused_calls_write_nothing(pkg_eng, pkg_gl):
    """too few senders, a repeated id, an id >= n: the error the decode gives for that case (the oracle's), and out, deop, status and
    summary keep their marker in both threshold settings; open_senders outside [2t + 1, n] and the other field's context are refused"""
    pkg, eng = pkg_eng
    n, t, N = 7, 2, 20
    ins = inputs(FR, n, t, N, 99)
    mp = pkg.pipelines.Mul(eng, n, t, N)
    marker = {"out": O.fill_random(300, n * N).reshape(n, N, 4), "deop": O.fill_random(301, 2 * N)}
    st_marker, sm_marker = np.full(2 * N, 0x5A, dtype=np.uint8), np.full(4, 0x5A5A5A5A, dtype=np.uint32)
    try:
        mp.upload(ins["x"], ins["y"], ins["ta"], ins["tb"], ins["tc"])
        for nm, arr in marker.items():
            mp.upload_named(nm, arr)
        eng.h2d(mp.buffer("status")[0], st_marker)
        eng.h2d(mp.buffer("summary")[0], sm_marker)
        eng.sync()
        for fused in (1 << 20, 0):
            eng.set_fused_mul(fused)
            for ids in (tuple(range(2 * t)), (0, 1, 2, 3, 3), (0, 1, 2, 3, n)):
                want_rc = expected(FR, ins, n, t, N, ids)["rc"]
                assert want_rc not in (0, 8)
                assert raw_call(eng, mp, ids, n, t, N) == want_rc, ids
            for nm in ("ta", "tb", "tc", "x", "y", "desh", "deop", "out"):
                assert raw_call(eng, mp, range(2 * t + 1), n, t, N, **{nm: 0}) == 4, nm
            assert raw_call(eng, mp, range(2 * t + 1), n, t, 0) == 4 and raw_call(eng, mp, range(2 * t + 1), 0, t, N) == 4
            assert raw_call(eng, mp, range(2 * t + 1), 256, t, N) == 4
        eng.sync()
        for nm, arr in marker.items():
            assert np.array_equal(mp.download(nm), arr), nm
        st_now, sm_now = np.zeros(2 * N, dtype=np.uint8), np.zeros(4, dtype=np.uint32)
        eng.d2h(st_now, mp.buffer("status")[0])
        eng.d2h(sm_now, mp.buffer("summary")[0])
        eng.sync()
        assert np.array_equal(st_now, st_marker) and np.array_equal(sm_now, sm_marker)
        for fused in (1 << 20, 0):                                                  # and the good calls: status and summary are optional
            eng.set_fused_mul(fused)
            assert raw_call(eng, mp, range(2 * t + 1), n, t, N) == 0 and raw_call(eng, mp, range(2 * t + 1), n, t, N, status=0, summary=0) == 0
        eng.sync()
        for bad in (2 * t, n + 1):
            with pytest.raises(RuntimeError, match="ShareErrorCode 4"):
                pkg.pipelines.Mul(eng, n, t, N, open_senders=bad)
        # the Fr call on a Goldilocks context, and the Goldilocks call on an Fr context: TypeMismatch (5)
        _, gl = pkg_gl
        ids = (C.c_size_t * (2 * t + 1))(*range(2 * t + 1))
        ptrs = [C.c_void_p(mp.buffer(nm)[0]) for nm in ("ta", "tb", "tc", "x", "y")]
        tail = [C.c_size_t(N), C.c_size_t(n), C.c_size_t(t)] + [C.c_void_p(mp.buffer(nm)[0]) for nm in ("desh", "deop", "out")] + [None, None, None]
        assert eng.L.hbmpc_dev_mul_parties(gl.ctx, ids, C.c_size_t(2 * t + 1), *ptrs, *tail) == 5
        assert eng.L.hbmpc_gl_dev_mul_parties(eng.ctx, ids, C.c_size_t(2 * t + 1), *ptrs, *tail) == 5
    finally:
        eng.set_fused_mul(pkg.hbmpc.FUSED_MUL_DEFAULT)
        mp.close()


def test_pipeline_as_hip_graph(pkg_eng):
    """on an explicit stream: capture, zero `out`, replay -- the eager run's bytes, for both forms"""
    pkg, eng = pkg_eng
    n, t, N = 16, 5, 200
    ins = inputs(FR, n, t, N, 1000 * n + N)
    want = expected(FR, ins, n, t, N, range(2 * t + 1))
    st = eng.stream_create()
    try:
        res = run_forms(pkg, eng, FR, n, t, N, ins, stream=st, graph=True)
    finally:
        eng.sync(st)
        eng.stream_destroy(st)
    for form, got in res.items():
        assert_equals_oracle(got, want, form)
    assert_same_bytes(res, "graph")


@pytest.mark.parametrize("n,t,N", [(4, 1, 5), (16, 5, 200)])
def test_goldilocks(pkg_gl, n, t, N):
    """the three hbmpc_gl_* launches under both threshold settings against the Goldilocks oracle; out opens to x y mod p"""
    pkg, eng = pkg_gl
    ins = inputs(GL, n, t, N, 77 * n + N)
    want = expected(GL, ins, n, t, N, range(2 * t + 1))
    assert want["rc"] == 0
    res = run_forms(pkg, eng, GL, n, t, N, ins)
    for form, got in res.items():
        assert_equals_oracle(got, want, form)
        assert got["summary"].tolist() == [0, 0, 0xffffffff, 0], form
        assert_opens_to_xy(GL, got["out"], ins, n, t)
    assert_same_bytes(res, (n, t, N))


def test_cpp_wrapper():
    """tests/cpp/test_mul_pipeline (include/hbmpc_pipelines.hpp's Mul at n = 4, t = 1, N = 5: c = a b opens to x y) in a child process"""
    exe = os.path.join(ROOT, "tests", "cpp", "test_mul_pipeline")
    assert os.path.exists(exe), "built by make -C tests/cpp -f mul.mk (build())"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
