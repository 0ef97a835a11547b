"""RanSha and DouSha + RanDouSha for all parties as one device call each (hbmpc_[gl_]dev_ransha_parties / _randousha_parties): the
one-launch form (csrc/kernels_producers_wg.hpp, a workgroup per column) against the separate launches (hbmpc_set_fused_producers(ctx, 0)),
byte for byte in every buffer a caller can see, and both against the big-integer model of tests/producers_ref.py -- never against the
library itself.

Every device call of this file runs on a stream of its own and is waited for with a deadline (`wait`): a kernel that does not finish
ends the session instead of blocking it."""
import ctypes as C
import functools
import time

import numpy as np
import pytest

from __graft_entry__ import load_package
from tests import edge_inputs as EI
from tests import producers_ref as PR
from tests.batchrecon_ref import NONE, PRIME, SPEC

pytestmark = pytest.mark.gpu
SHAPES = [(4, 1), (5, 1), (7, 2), (13, 4), (16, 5), (16, 1)]
FIELDS = ("fr", "goldilocks")
KINDS = ("ransha", "randousha")
FORCED = 1 << 20
LIMIT = 60.0  # seconds a device call may take before the session is ended
FLD = {"fr": EI.FR, "goldilocks": EI.GL}
MARK = 0x5C
OUT = {"ransha": ("dealt_t", "out_t", "yv_t", "status", "summary", "bad"),
       "randousha": ("dealt_t", "dealt_2t", "out_t", "out_2t", "yv_t", "yv_2t", "sel_t", "sel_2t", "st_t", "st_2t", "bad")}


@pytest.fixture(scope="module")
def pkg():
    return load_package()


@pytest.fixture(scope="module")
def stream():
    torch = pytest.importorskip("torch")
    return torch.cuda.Stream(device=torch.device("cuda", 0))


def wait(stream, what):
    """the stream's work so far, under a time limit"""
    import torch
    ev = torch.cuda.Event()
    ev.record(stream)
    t0 = time.monotonic()
    while not ev.query():
        if time.monotonic() - t0 > LIMIT:
            pytest.exit(f"{what}: the device call did not finish within {LIMIT} s", returncode=3)
        time.sleep(0.0002)


def default_threshold(eng):
    return load_package().hbmpc.FUSED_PRODUCERS_DEFAULT[eng.field]


class Call:
    """the buffers of one call shape on the device; run() returns every output as bytes"""

    def __init__(self, eng, stream, kind, n, t, K):
        self.eng, self.stream, self.s, self.kind = eng, stream, stream.cuda_stream, kind
        self.n, self.t, self.K = n, t, K
        eb, dou = eng.ebytes, kind == "randousha"
        nver = n - t - 1 if dou else 2 * t
        self.nver, G = nver, max(nver * K, 1)
        self.out_rows = t + 1 if dou else n - 2 * t
        sz = {"ws": (2 * n * n * K + max(nver * n, 2 * t, t + 1) * K) * eb, "bad": 8}
        for sfx, deg in (("t", t), ("2t", 2 * t)) if dou else (("t", t),):
            sz.update({"coeffs_" + sfx: n * K * (deg + 1) * eb, "dealt_" + sfx: n * n * K * eb, "out_" + sfx: n * K * self.out_rows * eb,
                       "yv_" + sfx: max(n * nver * K, 1) * eb})
            if dou:
                sz.update({"sel_" + sfx: G * eb * (2 if eng.field == "fr" else 1), "st_" + sfx: G * (1 if eng.field == "fr" else 4)})
        if not dou:
            sz.update({"status": G, "summary": 16})
        self.size = sz
        self.ptr = {k: eng.dev_alloc(v) for k, v in sz.items()}
        self.outputs = OUT[kind]

    def close(self):
        for p in self.ptr.values():
            self.eng.dev_free(p)

    def fill(self, names, byte):
        for k in names:
            self.eng.h2d(self.ptr[k], np.full(self.size[k], byte, dtype=np.uint8), self.s)

    def read(self):
        out = {k: np.zeros(self.size[k], dtype=np.uint8) for k in self.outputs}
        for k, arr in out.items():
            self.eng.d2h(arr, self.ptr[k], self.s)
        wait(self.stream, "download")
        return out

    def upload(self, name, vals):
        self.eng.h2d(self.ptr[name], FLD[self.eng.field].arr(vals), self.s)

    def call(self, threshold, from_coeffs, S=None, null=(), K=None, n=None, t=None, eng=None):
        """one hbmpc_[gl_]dev_ransha_parties / _randousha_parties with the threshold at `threshold` (None: as the context has it) -> rc;
        eng: another context (of the other field, on the same buffers: for calls that are refused)"""
        eng = eng or self.eng
        if threshold is not None:
            eng.set_fused_producers(threshold)
        p = {k: (0 if k in null else v) for k, v in self.ptr.items()}
        K, n, t = self.K if K is None else K, self.n if n is None else n, self.t if t is None else t
        if self.kind == "ransha":
            S = 2 * t + 1 if S is None else S
            rc = eng.ransha_parties(p["coeffs_t"] if from_coeffs else 0, p["dealt_t"], K, n, t, S, p["out_t"], p["yv_t"], p["ws"], p["status"],
                                         p["summary"], p["bad"], stream=self.s)
        else:
            co = (p["coeffs_t"], p["coeffs_2t"]) if from_coeffs is True else (0, 0) if not from_coeffs else from_coeffs
            rc = eng.randousha_parties(co[0], co[1], p["dealt_t"], p["dealt_2t"], K, n, t, p["out_t"], p["out_2t"], p["yv_t"], p["yv_2t"], p["ws"],
                                            p["sel_t"], p["sel_2t"], p["st_t"], p["st_2t"], p["bad"], stream=self.s)
        wait(self.stream, f"{self.kind}_parties(n={n}, t={t}, K={K}, threshold={threshold})")
        return rc

    def run(self, threshold, inputs, from_coeffs, S=None):
        """inputs: {"coeffs_t": .., ["coeffs_2t"]} or {"dealt_t": .., ["dealt_2t"]} as nested lists"""
        self.fill(self.outputs, 0xA5)
        for k, v in inputs.items():
            self.upload(k, v)
        rc = self.call(threshold, from_coeffs, S)
        assert rc == 0, self.eng.last_error()
        return self.read()


def as_bytes(field, kind, m, dealt, S_extra=None):
    """the model's outputs as the bytes the device writes; S_extra = (K, fill): RanSha with more than 2t + 1 verify senders keeps the last
    verifier's status bytes and summary"""
    F = FLD[field]
    el = lambda v: np.ascontiguousarray(F.arr(v)).view(np.uint8).reshape(-1)  # noqa: E731
    u32 = lambda s: np.array(s, dtype=np.uint32).view(np.uint8)  # noqa: E731
    if kind == "ransha":
        status = np.array(m["status"], dtype=np.uint8)
        summ = m["summary"]
        if S_extra and len(status):
            K = S_extra
            last = m["status"][-K:]
            status = np.concatenate([np.array(last, dtype=np.uint8), np.full(len(status) - K, 0xA5, dtype=np.uint8)])
            summ = PR.summary(last)
        if not len(status):  # no verifier: neither is written
            status, summ = np.full(1, 0xA5, dtype=np.uint8), None
        return {"dealt_t": el(dealt[0]), "out_t": el(m["out"]), "yv_t": el(m["yv"]) if len(m["status"]) else np.full(F.arr([0]).nbytes, 0xA5, dtype=np.uint8),
                "status": status, "summary": u32(summ) if summ else np.full(16, 0xA5, dtype=np.uint8), "bad": u32(m["bad"])}
    out = {"bad": u32(m["bad"])}
    none = len(m["st_t"]) == 0
    for i, sfx in enumerate(("t", "2t")):
        out["dealt_" + sfx], out["out_" + sfx] = el(dealt[i]), el(m["out_" + sfx])
        out["yv_" + sfx] = np.full(F.arr([0]).nbytes, 0xA5, dtype=np.uint8) if none else el(m["yv_" + sfx])
        out["sel_" + sfx] = np.full(F.arr([0]).nbytes * (2 if field == "fr" else 1), 0xA5, dtype=np.uint8) if none else el(m["sel_" + sfx])
        st = np.array(m["st_" + sfx], dtype=np.uint8 if field == "fr" else np.uint32).view(np.uint8)
        out["st_" + sfx] = np.full(1 if field == "fr" else 4, 0xA5, dtype=np.uint8) if none else st
    return out


def assert_same(kind, a, b, what):
    for k in OUT[kind]:
        assert np.array_equal(a[k], b[k]), (k, what)


def model_of(field, kind, n, t, dealt, S=None):
    return PR.ransha_model(field, n, t, dealt[0], S) if kind == "ransha" else PR.randousha_model(field, n, t, dealt[0], dealt[1])


def lists(c):
    return [[list(p) for p in row] for row in c]


def coeffs_of(field, kind, n, t, K, seed=0):
    if kind == "ransha":
        return [lists(PR.honest_coeffs(field, n, t, K, seed))]
    return list(PR.double_coeffs(field, n, t, K, seed))


def deal_of(field, n, t, coeffs):
    return [PR.deal(field, c, n, (i + 1) * t) for i, c in enumerate(coeffs)]


@functools.lru_cache(maxsize=None)
def honest_case(field, kind, n, t, K):
    """(coeffs, dealt, model) of the honest inputs of a shape, computed once; treat as read-only"""
    coeffs = coeffs_of(field, kind, n, t, K)
    dealt = deal_of(field, n, t, coeffs)
    return coeffs, dealt, model_of(field, kind, n, t, dealt)


def inputs_of(kind, coeffs=None, dealt=None):
    names = ("t",) if kind == "ransha" else ("t", "2t")
    src, pre = (coeffs, "coeffs_") if coeffs is not None else (dealt, "dealt_")
    return {pre + sfx: src[i] for i, sfx in enumerate(names)}


def forms_match(eng, stream, kind, n, t, coeffs, dealt, want, forms=(FORCED, 0), S=None, modes=(True, False)):
    """the call in each form and each input mode: every output equal among them and, where `want` is given, to the model's bytes"""
    K = len(dealt[0][0][0])
    c = Call(eng, stream, kind, n, t, K)
    got = []
    try:
        for from_coeffs in modes:
            if from_coeffs and coeffs is None:
                continue
            for th in forms:
                got.append(c.run(th, inputs_of(kind, coeffs if from_coeffs else None, dealt), from_coeffs, S))
    finally:
        c.close()
        eng.set_fused_producers(default_threshold(eng))
    for g in got[1:]:
        assert_same(kind, got[0], g, "the forms differ")
    if want is not None:
        assert_same(kind, got[0], as_bytes(eng.field, kind, want, dealt, K if S and S > 2 * t + 1 else None), "differs from the model")
    return got[0]


def test_device_calls_exist(pkg):
    """the four calls and the setter, callable through hbmpc.py: null buffers are refused with InvalidInput"""
    L = pkg.lib()
    for nm in ("hbmpc_dev_ransha_parties", "hbmpc_gl_dev_ransha_parties", "hbmpc_dev_randousha_parties", "hbmpc_gl_dev_randousha_parties",
               "hbmpc_set_fused_producers"):
        assert hasattr(L, nm), nm
    for field in FIELDS:
        eng = pkg.Engine(0, field=field)
        try:
            eng.set_fused_producers(pkg.hbmpc.FUSED_PRODUCERS_DEFAULT[field])
            assert eng.ransha_parties(0, 0, 2, 4, 1, 3, 0, 0, 0) == 4
            assert eng.randousha_parties(0, 0, 0, 0, 2, 4, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0) == 4
        finally:
            eng.close()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n,t", SHAPES)
@pytest.mark.parametrize("field", FIELDS)
def test_both_forms_byte_for_byte_and_the_model(pkg, stream, field, n, t, kind):
    eng = pkg.Engine(0, field=field)
    try:
        for K in (1, 2, 3):
            coeffs, dealt, want = honest_case(field, kind, n, t, K)
            got = forms_match(eng, stream, kind, n, t, coeffs, dealt, want)
            assert got["bad"].view(np.uint32).tolist() == [0, NONE]
        for K in (3, 4, 5):  # around a threshold of 4: bytes only (the model's interpolations are the slow part)
            coeffs = coeffs_of(field, kind, n, t, K, seed=5)
            dealt = deal_of(field, n, t, coeffs)
            got = forms_match(eng, stream, kind, n, t, coeffs, dealt, None, forms=(4, 0))
            assert got["bad"].view(np.uint32).tolist() == [0, NONE]
    finally:
        eng.close()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n,t", [(4, 1), (16, 5)])
@pytest.mark.parametrize("field", FIELDS)
def test_one_launch_leaves_the_workspace_alone(pkg, stream, field, n, t, kind):
    """the forms write the same bytes, so only the workspace tells them apart: the separate launches write it, one launch does not --
    a call that quietly took the separate launches under a forced threshold fails here"""
    K = 2
    coeffs, dealt, _ = honest_case(field, kind, n, t, K)
    eng = pkg.Engine(0, field=field)
    c = Call(eng, stream, kind, n, t, K)
    try:
        touched = {}
        for th in (FORCED, 0):
            c.fill(("ws",), MARK)
            c.run(th, inputs_of(kind, coeffs), True)
            ws = np.zeros(c.size["ws"], dtype=np.uint8)
            eng.d2h(ws, c.ptr["ws"], c.s)
            wait(stream, "download")
            touched[th] = bool((ws != MARK).any())
        assert not touched[FORCED]
        if kind == "ransha":  # the verifiers' decode keeps its coefficients there; RanDouSha's separate launches need it for some shapes only
            assert touched[0]
    finally:
        c.close()
        eng.set_fused_producers(default_threshold(eng))
        eng.close()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("field", FIELDS)
def test_shapes_outside_the_kernel(pkg, stream, field, kind):
    """t = 0, n < 3t + 1, n = 17 with every party a verify sender, a Sat32 context: the model's bytes through the separate launches"""
    K = 2
    eng = pkg.Engine(0, field=field)
    try:
        for n, t, S in ((1, 0, None), (2, 0, None), (3, 1, None), (5, 2, None), (17, 5, 17)):
            coeffs = coeffs_of(field, kind, n, t, K)
            dealt = deal_of(field, n, t, coeffs)
            want = model_of(field, kind, n, t, dealt, S)
            got = forms_match(eng, stream, kind, n, t, coeffs, dealt, want, S=S if kind == "ransha" else None)
            refused = kind == "ransha" and n < 3 * t + 1
            assert got["bad"].view(np.uint32).tolist() == ([2 * t * K, 0] if refused else [0, NONE]), (n, t)
        if field == "fr":
            eng.set_impl("sat32")
            coeffs, dealt, want = honest_case(field, kind, 4, 1, K)
            forms_match(eng, stream, kind, 4, 1, coeffs, dealt, want)
    finally:
        eng.close()


def solve_top(field, n, i, tops):
    """dealer 0's top coefficient so that sum_p alpha_i^p top_p = 0 (alpha_i^0 = 1)"""
    q, a = PRIME[field], SPEC[field].domain_element(n, i)
    return -sum(pow(a, p, q) * tops[p] for p in range(1, n)) % q


@pytest.mark.parametrize("field", FIELDS)
def test_ransha_a_wrong_degree(pkg, stream, field):
    """one verifier's mixed polynomial loses its top coefficient: bad == (1, k); all top coefficients zero and all-zero polynomials in a
    column: every verifier fails it"""
    n, t, K, k, i = 7, 2, 3, 1, 1
    eng = pkg.Engine(0, field=field)
    try:
        honest = honest_case(field, "ransha", n, t, K)[2]
        co = coeffs_of(field, "ransha", n, t, K)
        co[0][0][k][t] = solve_top(field, n, i, [co[0][p][k][t] for p in range(n)])
        dealt = deal_of(field, n, t, co)
        want = model_of(field, "ransha", n, t, dealt)
        assert want["bad"] == (1, k)
        got = forms_match(eng, stream, "ransha", n, t, co, dealt, want)
        assert got["bad"].view(np.uint32).tolist() == [1, k]
        assert [r[: k * (n - 2 * t)] for r in want["out"]] == [r[: k * (n - 2 * t)] for r in honest["out"]]  # the other columns' outputs untouched
        for zero_all in (False, True):
            co = coeffs_of(field, "ransha", n, t, K)
            for p in range(n):
                co[0][p][k] = [0] * (t + 1) if zero_all else co[0][p][k][:t] + [0]
            dealt = deal_of(field, n, t, co)
            want = model_of(field, "ransha", n, t, dealt)
            assert want["bad"] == (2 * t, k)
            forms_match(eng, stream, "ransha", n, t, co, dealt, want)
    finally:
        eng.close()


@pytest.mark.parametrize("field", FIELDS)
def test_randousha_a_wrong_degree_and_unequal_secrets(pkg, stream, field):
    n, t, K, k, i = 7, 2, 3, 2, 4
    eng = pkg.Engine(0, field=field)
    try:
        co = coeffs_of(field, "randousha", n, t, K)
        co[1][0][k][2 * t] = solve_top(field, n, i, [co[1][p][k][2 * t] for p in range(n)])  # the degree-2t side only, verifier i only
        dealt = deal_of(field, n, t, co)
        want = model_of(field, "randousha", n, t, dealt)
        assert want["bad"] == (1, k)
        forms_match(eng, stream, "randousha", n, t, co, dealt, want)
        for what in ("top", "zero", "secret"):
            co = coeffs_of(field, "randousha", n, t, K)
            for p in range(n):
                if what == "top":
                    co[1][p][k][2 * t] = 0
                elif what == "zero":
                    co[0][p][k], co[1][p][k] = [0] * (t + 1), [0] * (2 * t + 1)
            if what == "secret":
                co[1][3][k][0] = (co[1][3][k][0] + 1) % PRIME[field]
            dealt = deal_of(field, n, t, co)
            want = model_of(field, "randousha", n, t, dealt)
            assert want["bad"] == (n - t - 1, k), what
            forms_match(eng, stream, "randousha", n, t, co, dealt, want)
    finally:
        eng.close()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("field", FIELDS)
def test_a_byzantine_dealer(pkg, stream, field, kind):
    """one dealt share of dealer p for recipient j changed (dealt mode).  RanSha: j <= 2t, every verifier fails the column; j > 2t, no
    verifier sees it and party j's outputs differ.  RanDouSha (the degree-2t array alone): every verifier reads all n parties"""
    n, t, K, k, p = 7, 2, 3, 1, 3
    eng = pkg.Engine(0, field=field)
    try:
        _, dealt, honest = honest_case(field, kind, n, t, K)
        for j in (1, 2 * t, 2 * t + 1, n - 1):
            lied = [[[list(r) for r in d] for d in arr] for arr in dealt]
            lied[-1][p][j][k] = (lied[-1][p][j][k] + 1) % PRIME[field]
            want = model_of(field, kind, n, t, lied)
            nver = 2 * t if kind == "ransha" else n - t - 1
            assert want["bad"] == ((nver, k) if kind == "randousha" or j <= 2 * t else (0, NONE)), j
            key = "out" if kind == "ransha" else "out_2t"
            assert want[key][j] != honest[key][j] and want[key][(j + 1) % n] == honest[key][(j + 1) % n]
            got = forms_match(eng, stream, kind, n, t, None, lied, want, modes=(False,))
            assert got["bad"].view(np.uint32).tolist() == list(want["bad"])
    finally:
        eng.close()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n,t", [(4, 1), (16, 5)])
@pytest.mark.parametrize("field", FIELDS)
def test_field_edge_values(pkg, stream, field, n, t, kind):
    """the field's edge values as coefficients and as dealt shares (which then lie on no polynomial)"""
    K, edge = 2, FLD[field].edge
    eng = pkg.Engine(0, field=field)
    try:
        degs = (t,) if kind == "ransha" else (t, 2 * t)
        coeffs = [[[[edge[(p * 7 + k * 3 + c + s) % len(edge)] for c in range(d + 1)] for k in range(K)] for p in range(n)] for s, d in enumerate(degs)]
        dealt = deal_of(field, n, t, coeffs)
        forms_match(eng, stream, kind, n, t, coeffs, dealt, model_of(field, kind, n, t, dealt))
        dealt = [[[[edge[(p * 5 + j * 3 + k + s) % len(edge)] for k in range(K)] for j in range(n)] for p in range(n)] for s in range(len(degs))]
        forms_match(eng, stream, kind, n, t, None, dealt, model_of(field, kind, n, t, dealt), modes=(False,))
    finally:
        eng.close()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("threshold", [FORCED, 0])
def test_refusals_write_nothing(pkg, stream, threshold, kind):
    n, t, K = 7, 2, 2
    coeffs, dealt, want = honest_case("fr", kind, n, t, K)
    eng, gl = pkg.Engine(0, field="fr"), pkg.Engine(0, field="goldilocks")
    c = Call(eng, stream, kind, n, t, K)
    try:
        for k, v in inputs_of(kind, coeffs).items():
            c.upload(k, v)
        c.fill(c.outputs, MARK)
        cases = [("null dealt", dict(null=("dealt_t",))), ("null out", dict(null=("out_t",))), ("null yv", dict(null=("yv_t",))), ("null ws", dict(null=("ws",))),
                 ("null bad", dict(null=("bad",))), ("neither coeffs nor dealt", dict(from_coeffs=False, null=("dealt_t",))), ("K = 0", dict(K=0)),
                 ("n <= 2t", dict(n=4)), ("n > 255", dict(n=256)), ("K >= 2^19", dict(K=1 << 19)),
                 # a dealt block of n n K elements reaches 4 GiB with K still below 2^19 (2 065 columns over Fr, 8 257 over Goldilocks; one
                 # column fewer is below 4 GiB); nothing of that size exists: the call is refused before it touches a buffer
                 ("a block of 4 GiB", dict(n=255, t=2, K=(1 << 32) // (32 * 255 * 255) + 1)),
                 ("a block of 4 GiB, Goldilocks", dict(n=255, t=2, K=(1 << 32) // (8 * 255 * 255) + 1, eng=gl)),
                 ("t beyond any n", dict(t=1 << 63)), ("t beyond any n", dict(t=(1 << 63) + 3))]
        assert (1 << 32) // (32 * 255 * 255) + 1 < 1 << 19 and (1 << 32) // (8 * 255 * 255) + 1 < 1 << 19 and 255 * 255 * 2065 * 32 >= 1 << 32
        if kind == "ransha":
            cases += [("S < 2t + 1", dict(S=2 * t)), ("S > n", dict(S=n + 1))]
        else:
            cases += [("null dealt_2t", dict(null=("dealt_2t",))), ("null sel", dict(null=("sel_2t",))), ("null st", dict(null=("st_t",))),
                      ("one coefficient array", dict(from_coeffs=(c.ptr["coeffs_t"], 0)))]
        for what, kw in cases:
            assert c.call(threshold, kw.pop("from_coeffs", True), **kw) == 4, what
        # TypeMismatch: either field's call on the other field's context
        L, p = pkg.lib(), c.ptr
        v = lambda *names: [C.c_void_p(p[k]) for k in names]  # noqa: E731
        sz = [C.c_size_t(x) for x in (K, n, t)]
        for pfx, ctx in (("hbmpc_", gl.ctx), ("hbmpc_gl_", eng.ctx)):
            if kind == "ransha":
                rc = getattr(L, pfx + "dev_ransha_parties")(ctx, *v("coeffs_t", "dealt_t"), *sz, C.c_size_t(2 * t + 1),
                                                            *v("out_t", "yv_t", "ws", "status", "summary", "bad"), C.c_void_p(c.s))
            else:
                rc = getattr(L, pfx + "dev_randousha_parties")(ctx, *v("coeffs_t", "coeffs_2t", "dealt_t", "dealt_2t"), *sz,
                                                               *v("out_t", "out_2t", "yv_t", "yv_2t", "ws", "sel_t", "sel_2t", "st_t", "st_2t", "bad"),
                                                               C.c_void_p(c.s))
            wait(stream, "a refused call")
            assert rc == 5
        got = c.read()
        for k in c.outputs:
            assert (got[k] == MARK).all(), (k, "a refused call wrote to it")
        if kind == "ransha":  # the optional buffers may be null
            assert c.call(threshold, True, null=("status", "summary")) == 0, eng.last_error()
            got, wb = c.read(), as_bytes("fr", kind, want, dealt)
            for k in ("dealt_t", "out_t", "yv_t", "bad"):
                assert np.array_equal(got[k], wb[k]), k
            assert (got["status"] == MARK).all() and (got["summary"] == MARK).all()
    finally:
        c.close()
        eng.close()
        gl.close()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("threshold", [FORCED, 0])
@pytest.mark.parametrize("field", FIELDS)
def test_capture_and_replay(pkg, stream, field, threshold, kind):
    """the call inside a capture, replayed twice with the inputs changed in between: the eager bytes of each input"""
    n, t, K = 7, 2, 3
    eng = pkg.Engine(0, field=field)
    c = Call(eng, stream, kind, n, t, K)
    try:
        coeffs, dealt, want = honest_case(field, kind, n, t, K)
        lied = [[[list(r) for r in d] for d in arr] for arr in dealt]
        lied[-1][2][1][2] = (lied[-1][2][1][2] + 1) % PRIME[field]
        want_lied = model_of(field, kind, n, t, lied)
        assert want_lied["bad"][0] != 0
        c.run(threshold, inputs_of(kind, None, dealt), False)  # eager first: tables and scratch exist
        eng.graph_begin(c.s)
        try:
            rc = c.eng.ransha_parties(0, c.ptr["dealt_t"], K, n, t, 2 * t + 1, c.ptr["out_t"], c.ptr["yv_t"], c.ptr["ws"], c.ptr["status"], c.ptr["summary"],
                                      c.ptr["bad"], stream=c.s) if kind == "ransha" else \
                c.eng.randousha_parties(0, 0, c.ptr["dealt_t"], c.ptr["dealt_2t"], K, n, t, c.ptr["out_t"], c.ptr["out_2t"], c.ptr["yv_t"], c.ptr["yv_2t"],
                                        c.ptr["ws"], c.ptr["sel_t"], c.ptr["sel_2t"], c.ptr["st_t"], c.ptr["st_2t"], c.ptr["bad"], stream=c.s)
        finally:
            g = eng.graph_end(c.s)
        assert rc == 0, eng.last_error()
        try:
            for inp, w in ((lied, want_lied), (dealt, want)):
                outs = tuple(k for k in c.outputs if not k.startswith("dealt"))
                c.fill(outs, 0xA5)
                for k, v in inputs_of(kind, None, inp).items():
                    c.upload(k, v)
                eng.graph_launch(g, c.s)
                wait(stream, "the replayed graph")
                assert_same(kind, c.read(), as_bytes(field, kind, w, inp), "the replayed graph")
        finally:
            eng.graph_destroy(g)
    finally:
        c.close()
        eng.set_fused_producers(default_threshold(eng))
        eng.close()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("field", FIELDS)
def test_default_threshold_routes(pkg, stream, field, kind):
    """at the library's defaults, K = default and default + 1 columns: the bytes of the separate launches (the only case at this size)"""
    n, t = 4, 1
    dflt = pkg.hbmpc.FUSED_PRODUCERS_DEFAULT[field]
    eng = pkg.Engine(0, field=field)
    try:
        F = FLD[field]
        rnd = np.random.default_rng(11)
        for K in (max(dflt, 1), dflt + 1):
            c = Call(eng, stream, kind, n, t, K)
            try:
                inputs = {}
                for sfx, deg in (("t", t), ("2t", 2 * t)) if kind == "randousha" else (("t", t),):
                    vals = rnd.integers(1, 1 << 62, size=(n, K, deg + 1), dtype=np.uint64).astype(object)
                    if sfx == "2t":
                        vals[:, :, 0] = inputs["coeffs_t"][:, :, 0]
                    inputs["coeffs_" + sfx] = vals
                got = [c.run(th, inputs, True) for th in (None, 0)]
                assert_same(kind, got[0], got[1], f"K = {K}")
                assert got[0]["bad"].view(np.uint32).tolist() == [0, NONE]
            finally:
                c.close()
                eng.set_fused_producers(default_threshold(eng))
        assert F.mod > 1 << 62
    finally:
        eng.close()


@pytest.mark.parametrize("n,t,N", [(4, 1, 6), (16, 5, 66)])
@pytest.mark.parametrize("field", FIELDS)
def test_into_the_consumer(pkg, stream, field, n, t, N):
    """ransha_parties and randousha_parties write a, b, r_t, r_2t for hbmpc_[gl_]dev_triplegen_parties: c equals the Preprocessing handle's
    from the same polynomials -- three launches against the handle's many"""
    F, eb = FLD[field], FLD[field].arr([0]).nbytes
    K_rs, K_rd = -(-2 * N // (n - 2 * t)), -(-N // (t + 1))
    co_rs = coeffs_of(field, "ransha", n, t, K_rs, seed=3)
    co_rd = coeffs_of(field, "randousha", n, t, K_rd, seed=4)
    eng = pkg.Engine(0, field=field)
    s = stream.cuda_stream
    pp = pkg.pipelines.Preprocessing(eng, n, t, N, stream=s)
    rs, rd = Call(eng, stream, "ransha", n, t, K_rs), Call(eng, stream, "randousha", n, t, K_rd)
    G = N // (2 * t + 1)
    sz = {"a": n * N * eb, "b": n * N * eb, "rt": n * N * eb, "r2t": n * N * eb, "Y": n * n * G * eb, "Z": n * G * eb, "opened": N * eb, "c": n * N * eb}
    tg = {k: eng.dev_alloc(v) for k, v in sz.items()}
    try:
        pp.rs.upload(F.arr(co_rs[0]))
        pp.rd.upload(F.arr(co_rd[0]), F.arr(co_rd[1]))
        pp.run(check=True)
        wait(stream, "Preprocessing.run")
        want_c = np.ascontiguousarray(pp.tg.download_named("c", (n, N)))
        o1 = rs.run(None, inputs_of("ransha", co_rs), True)
        o2 = rd.run(None, inputs_of("randousha", co_rd), True)
        assert o1["bad"].view(np.uint32).tolist() == [0, NONE] and o2["bad"].view(np.uint32).tolist() == [0, NONE]
        lists_rs = o1["out_t"].reshape(n, -1)
        for name, block in (("a", lists_rs[:, : N * eb]), ("b", lists_rs[:, N * eb: 2 * N * eb]), ("rt", o2["out_t"].reshape(n, -1)[:, : N * eb]),
                            ("r2t", o2["out_2t"].reshape(n, -1)[:, : N * eb])):
            eng.h2d(tg[name], np.ascontiguousarray(block), s)
        fn = getattr(pkg.lib(), ("hbmpc_" if field == "fr" else "hbmpc_gl_") + "dev_triplegen_parties")
        rc = fn(eng.ctx, *(C.c_void_p(tg[k]) for k in ("a", "b", "r2t", "rt")), C.c_size_t(N), C.c_size_t(n), C.c_size_t(t),
                *(C.c_void_p(tg[k]) for k in ("Y", "Z", "opened", "c")), None, None, None, C.c_void_p(s))
        assert rc == 0, eng.last_error()
        wait(stream, "triplegen_parties")
        got_c = np.zeros(sz["c"], dtype=np.uint8)
        eng.d2h(got_c, tg["c"], s)
        wait(stream, "download")
        assert np.array_equal(got_c, want_c.view(np.uint8).reshape(-1))
    finally:
        for p in tg.values():
            eng.dev_free(p)
        rs.close()
        rd.close()
        pp.close()
        eng.close()
