"""BatchRecon for all parties as one device call (hbmpc_[gl_]dev_batchrecon_parties, hbmpc_pipe_batchrecon_create): its one-launch
form (csrc/kernels_batchrecon_wg.hpp, a workgroup per chunk of d + 1 elements) against its three launches
(hbmpc_set_fused_batchrecon(ctx, 0)) and against the composition of the three public calls the definition names
(hbmpc_dev_vandermonde_apply_parties, hbmpc_dev_batch_recover_slots twice), byte for byte in every buffer a caller can see, and all of
them against the big-integer model of tests/batchrecon_ref.py -- never against the library itself.

Every device call of this file runs on a stream of its own and is waited for with a deadline (`wait`): a kernel that does not finish
ends the session instead of blocking it."""
import ctypes as C
import functools
import random
import time

import numpy as np
import pytest

from __graft_entry__ import load_package
from tests import batchrecon_ref as BR
from tests import edge_inputs as EI

pytestmark = pytest.mark.gpu
SHAPES = [("fr", 4, 1, 1), ("fr", 4, 1, 2), ("fr", 5, 1, 2), ("fr", 7, 2, 2), ("fr", 16, 5, 1), ("fr", 16, 5, 5), ("fr", 16, 5, 10),
          ("goldilocks", 4, 1, 1), ("goldilocks", 7, 2, 4), ("goldilocks", 16, 5, 5), ("goldilocks", 16, 5, 10)]
CHUNKS = [1, 3, 41]  # one workgroup; fewer workgroups than the summaries' fan-in of 16; not a multiple of it
FORCED = 1 << 20
LIMIT = 60.0  # seconds a device call may take before the session is ended
FLD = {"fr": EI.FR, "goldilocks": EI.GL}
OUTPUTS = ("Y", "Z", "opened", "rstatus", "status", "summary_first", "summary")
OK = (0, 0, BR.NONE, 0)
MARK = 0x5C


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


def engine(pkg, field, impl=None):
    eng = pkg.Engine(0, field=field)
    if impl:
        eng.set_impl(impl)
    return eng


def default_threshold(eng):
    return load_package().hbmpc.FUSED_BATCHRECON_DEFAULT[eng.field]


def sender_sets(n, t, d):
    """(eval senders, reveal senders): a prefix, a suffix, a scattered eval set with a different scattered reveal set, unsorted lists"""
    S = d + t + 1
    rnd = random.Random(100 * n + 10 * t + d)
    sc1, sc2 = sorted(rnd.sample(range(n), S)), sorted(rnd.sample(range(n), S))
    if n > S:
        while sc2 == sc1:
            sc2 = sorted(rnd.sample(range(n), S))
    un1, un2 = list(sc2), list(range(S))
    rnd.shuffle(un1), rnd.shuffle(un2)
    return [(tuple(range(S)), tuple(range(S))), (tuple(range(n - S, n)), tuple(range(n - S, n))), (tuple(sc1), tuple(sc2)), (tuple(un1), tuple(un2))]


@functools.lru_cache(maxsize=None)
def model_of_honest(field, n, t, d, G, ids1, ids2):
    secrets, x = BR.honest(field, n, t, d, G)
    return BR.model(field, n, t, d, x, ids1, ids2)


# ---- the device call ----------------------------------------------------------------------------------------------------------------
class Call:
    """the buffers of one call shape on the device; run() returns every output as bytes"""

    def __init__(self, eng, stream, n, t, d, N):
        self.eng, self.stream, self.s = eng, stream, stream.cuda_stream
        self.n, self.t, self.d, self.N = n, t, d, N
        eb, G = eng.ebytes, max(1, N // (d + 1))
        self.G = G
        self.size = {"x": n * max(N, 1) * eb, "Y": n * n * G * eb, "Z": n * G * eb, "opened": max(N, 1) * eb, "rstatus": n * G, "status": G,
                     "summary_first": 16, "summary": 16}
        self.ptr = {k: eng.dev_alloc(v) for k, v in self.size.items()}

    def close(self):
        for p in self.ptr.values():
            self.eng.dev_free(p)

    def fill(self, names, byte):
        for k in names:
            self.eng.h2d(self.ptr[k], np.full(self.size[k], byte, dtype=np.uint8), self.s)

    def read(self, names=OUTPUTS):
        out = {k: np.zeros(self.size[k], dtype=np.uint8) for k in names}
        for k, arr in out.items():
            self.eng.d2h(arr, self.ptr[k], self.s)
        wait(self.stream, "download")
        return out

    def upload(self, x):
        self.eng.h2d(self.ptr["x"], FLD[self.eng.field].arr(x), self.s)

    def call(self, threshold, ids1, ids2, null=(), N=None, n=None, d=None, t=None):
        """one hbmpc_[gl_]dev_batchrecon_parties with the threshold at `threshold` (None: as the context has it) -> rc"""
        if threshold is not None:
            self.eng.set_fused_batchrecon(threshold)
        p = {k: (0 if k in null else v) for k, v in self.ptr.items()}
        rc = self.eng.batchrecon_parties(list(ids1), list(ids2), p["x"], self.N if N is None else N, self.n if n is None else n,
                                         self.d if d is None else d, self.t if t is None else t, p["Y"], p["Z"], p["opened"], p["rstatus"], p["status"],
                                         p["summary_first"], p["summary"], stream=self.s)
        wait(self.stream, f"batchrecon_parties(n={self.n}, t={self.t}, d={self.d}, N={self.N}, threshold={threshold})")
        return rc

    def run(self, threshold, ids1, ids2):
        self.fill(OUTPUTS, 0xA5)
        rc = self.call(threshold, ids1, ids2)
        assert rc == 0, self.eng.last_error()
        return self.read()

    def compose(self, ids1, ids2):
        """the three public calls of the definition, what a caller wrote before the call existed"""
        e, p, n, t, d, G = self.eng, self.ptr, self.n, self.t, self.d, self.G
        self.fill(OUTPUTS, 0xA5)
        assert e.dev_vandermonde_apply_parties(p["x"], G, n, d, n, p["Y"], stream=self.s) == 0, e.last_error()
        assert e.dev_batch_recover_slots(list(ids1), list(ids1), p["Y"], n * G, n * G, n, d, t, p["Z"], p0=True, status_d=p["rstatus"],
                                         summary_d=p["summary_first"], stream=self.s) == 0, e.last_error()
        assert e.dev_batch_recover_slots(list(ids2), list(ids2), p["Z"], G, G, n, d, t, p["opened"], p0=False, status_d=p["status"],
                                         summary_d=p["summary"], stream=self.s) == 0, e.last_error()
        wait(self.stream, "the composition of the three public calls")
        return self.read()


def as_bytes(field, m):
    """the model's outputs as the bytes the device writes"""
    F = FLD[field]
    el = lambda v: np.ascontiguousarray(F.arr(v)).view(np.uint8).reshape(-1)  # noqa: E731
    summ = lambda s: np.array(s, dtype=np.uint32).view(np.uint8)  # noqa: E731
    return {"Y": el(m["Y"]), "Z": el(m["Z"]), "opened": el(m["opened"]), "rstatus": np.array(m["rstatus"], dtype=np.uint8),
            "status": np.array(m["status"], dtype=np.uint8), "summary_first": summ(m["summary_first"]), "summary": summ(m["summary"])}


def assert_same(a, b, what):
    for k in OUTPUTS:
        assert np.array_equal(a[k], b[k]), (k, what)


def all_forms_match(eng, stream, field, n, t, d, x, ids1, ids2, want, forms=(FORCED, 0), composition=True):
    """the call in each form and the composition: every output equal among them and equal to `want` (the model's outputs)"""
    c = Call(eng, stream, n, t, d, len(x[0]))
    try:
        c.upload(x)
        got = [c.run(th, ids1, ids2) for th in forms]
        if composition:
            got.append(c.compose(ids1, ids2))
    finally:
        c.close()
        eng.set_fused_batchrecon(default_threshold(eng))
    for g in got[1:]:
        assert_same(got[0], g, "the forms differ")
    assert_same(got[0], as_bytes(field, want), "differs from the model")
    return got[0]


def test_device_call_exists(pkg):
    """both symbols, the setter and the handle's create, callable through hbmpc.py: a null buffer is refused with InvalidInput"""
    L = pkg.lib()
    for nm in ("hbmpc_dev_batchrecon_parties", "hbmpc_gl_dev_batchrecon_parties", "hbmpc_set_fused_batchrecon", "hbmpc_pipe_batchrecon_create"):
        assert hasattr(L, nm), nm
    for field in ("fr", "goldilocks"):
        eng = engine(pkg, field)
        try:
            assert callable(eng.batchrecon_parties) and callable(eng.set_fused_batchrecon)
            eng.set_fused_batchrecon(pkg.hbmpc.FUSED_BATCHRECON_DEFAULT[field])
            assert eng.batchrecon_parties([0, 1, 2], [0, 1, 2], 0, 2, 4, 1, 1, 0, 0, 0) == 4
            assert L.hbmpc_pipe_batchrecon_create(eng.ctx, *[C.c_size_t(v) for v in (4, 1, 1, 2, 0, 0)], C.c_void_p(0), None) == 4
        finally:
            eng.close()


@pytest.mark.parametrize("field,n,t,d", SHAPES)
@pytest.mark.parametrize("chunks", CHUNKS)
def test_all_forms_byte_for_byte(pkg, stream, field, n, t, d, chunks):
    secrets, x = BR.honest(field, n, t, d, chunks)
    eng = engine(pkg, field)
    try:
        for ids1, ids2 in sender_sets(n, t, d):
            want = model_of_honest(field, n, t, d, chunks, ids1, ids2)
            assert want["opened"] == secrets and want["summary_first"] == OK and want["summary"] == OK
            all_forms_match(eng, stream, field, n, t, d, x, ids1, ids2, want)
    finally:
        eng.close()


# ---- the lie: party 1's error polynomial has a root at recipient j's point --------------------------------------------------------------
@pytest.mark.parametrize("field,n,t,d", [("fr", 7, 2, 2), ("goldilocks", 7, 2, 2), ("fr", 16, 5, 5)])
@pytest.mark.parametrize("inside", [True, False])
def test_lie_with_exact_sets(pkg, stream, field, n, t, d, inside):
    """in chunk 0, a middle chunk and the last chunk, with recipient j inside the reveal set and outside it.  Outside, every reveal that is
    used is zero: the chunk "opens" to zero with status 0 while rstatus and summary_first show the failures"""
    G, S, M = 5, d + t + 1, d + 1
    secrets, x = BR.honest(field, n, t, d, G)
    ids1 = tuple(range(S))
    j = 2 if inside else n - 1
    ids2 = tuple(range(S)) if inside else tuple(range(n - 1 - S, n - 1))
    assert (j in ids2) == inside and 1 in ids1
    eng = engine(pkg, field)
    try:
        for g in (0, 2, G - 1):
            xs = BR.lie(field, x, n, d, g, j)
            want = BR.model(field, n, t, d, xs, ids1, ids2)
            # what the model must say, spelled out
            assert [want["rstatus"][r * G + g] for r in range(n)] == [0 if r == j else 8 for r in range(n)]
            assert sum(1 for s in want["rstatus"] if s) == n - 1 and want["summary_first"][:2] == (n - 1, n - 1) and want["summary_first"][3] == 8
            assert want["status"] == [8 if (inside and k == g) else 0 for k in range(G)]
            assert want["summary"] == ((1, 1, g, 8) if inside else OK)
            assert want["opened"] == [0 if k // M == g else s for k, s in enumerate(secrets)]
            all_forms_match(eng, stream, field, n, t, d, xs, ids1, ids2, want)
    finally:
        eng.close()


@pytest.mark.parametrize("field,n,t,d", [("fr", 7, 2, 2), ("goldilocks", 7, 2, 2), ("fr", 16, 5, 5)])
def test_lie_with_all_senders_is_repaired(pkg, stream, field, n, t, d):
    """S1 = S2 = n: the three launches with their robust decodes; rstatus 1 at every recipient but j, the secrets intact"""
    G, j = 5, 2
    secrets, x = BR.honest(field, n, t, d, G)
    ids = tuple(range(n))
    eng = engine(pkg, field)
    try:
        for g in (0, 2, G - 1):
            xs = BR.lie(field, x, n, d, g, j)
            want = BR.model(field, n, t, d, xs, ids, ids)
            assert [want["rstatus"][r * G + g] for r in range(n)] == [0 if r == j else 1 for r in range(n)]
            assert want["opened"] == secrets and not any(want["status"]) and want["summary"] == OK and want["summary_first"] == (n - 1, 0, BR.NONE, 0)
            all_forms_match(eng, stream, field, n, t, d, xs, ids, ids, want)
    finally:
        eng.close()


def test_lie_outside_the_eval_senders_changes_only_y(pkg, stream):
    field, n, t, d, G = "fr", 7, 2, 2, 3
    secrets, x = BR.honest(field, n, t, d, G)
    ids = tuple(range(n - (d + t + 1), n))
    assert 1 not in ids
    xs = BR.lie(field, x, n, d, 1, 3)
    eng = engine(pkg, field)
    try:
        a = all_forms_match(eng, stream, field, n, t, d, x, ids, ids, BR.model(field, n, t, d, x, ids, ids))
        b = all_forms_match(eng, stream, field, n, t, d, xs, ids, ids, BR.model(field, n, t, d, xs, ids, ids))
    finally:
        eng.close()
    assert not np.array_equal(a["Y"], b["Y"])
    for k in OUTPUTS[1:]:
        assert np.array_equal(a[k], b[k]), k


# ---- field edge values ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field,n,t,d", [("fr", 4, 1, 1), ("fr", 16, 5, 10), ("fr", 7, 2, 2), ("goldilocks", 4, 1, 1), ("goldilocks", 16, 5, 5)])
def test_edge_values(pkg, stream, field, n, t, d):
    """the values of tests/edge_inputs.py as secrets (random sharings of them) and as constant sharings (every party holds the value)"""
    F, M = FLD[field], d + 1
    vals = list(F.edge)
    vals += [vals[i % len(vals)] for i in range(-len(vals) % M)]
    shared = BR.share_secrets(field, vals, n, d, 31 * n + d)
    const = [list(vals) for _ in range(n)]
    x = [a + b for a, b in zip(shared, const)]
    ids1, ids2 = sender_sets(n, t, d)[2]
    want = BR.model(field, n, t, d, x, ids1, ids2)
    assert want["opened"] == vals + vals and not any(want["rstatus"]) and not any(want["status"])
    eng = engine(pkg, field)
    try:
        all_forms_match(eng, stream, field, n, t, d, x, ids1, ids2, want)
    finally:
        eng.close()


# ---- counters ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field", ["fr", "goldilocks"])
def test_failing_call_leaves_clean_counters(pkg, stream, field):
    """a failing one-launch call, then an honest one on the same stream: the second reports nothing in either summary"""
    n, t, d, G = 7, 2, 2, 19
    secrets, x = BR.honest(field, n, t, d, G)
    ids = tuple(range(d + t + 1))
    xs = BR.lie(field, BR.lie(field, x, n, d, 3, 2), n, d, 17, 4)
    eng = engine(pkg, field)
    c = Call(eng, stream, n, t, d, len(x[0]))
    try:
        c.upload(xs)
        bad = c.run(FORCED, ids, ids)
        assert_same(bad, as_bytes(field, BR.model(field, n, t, d, xs, ids, ids)), "the failing call")
        assert bad["summary"].view(np.uint32).tolist() == [2, 2, 3, 8] and bad["summary_first"].view(np.uint32)[1] == 2 * (n - 1)
        c.upload(x)
        good = c.run(FORCED, ids, ids)
        assert_same(good, as_bytes(field, BR.model(field, n, t, d, x, ids, ids)), "the honest call after it")
        assert good["summary"].view(np.uint32).tolist() == list(OK) and good["summary_first"].view(np.uint32).tolist() == list(OK)
    finally:
        c.close()
        eng.close()


# ---- refusals write nothing -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("threshold", [FORCED, 0])
def test_refusals_write_nothing(pkg, stream, threshold):
    n, t, d, G = 7, 2, 2, 2
    N, S = G * (d + 1), d + t + 1
    ids = tuple(range(S))
    secrets, x = BR.honest("fr", n, t, d, G)
    eng = engine(pkg, "fr")
    gl = engine(pkg, "goldilocks")
    c = Call(eng, stream, n, t, d, N)
    try:
        c.upload(x)
        c.fill(OUTPUTS, MARK)
        cases = [("null x", dict(null=("x",))), ("null y_ws", dict(null=("Y",))), ("null z_out", dict(null=("Z",))), ("null opened_out", dict(null=("opened",))),
                 ("N = 0", dict(N=0)), ("N % (d + 1) != 0", dict(N=N - 1)), ("d = 0", dict(d=0)), ("n = 0", dict(n=0)), ("n > 255", dict(n=256)),
                 ("n < 3t + 1", dict(t=3)), ("d + t + 1 > S1", dict(ids1=ids[:-1])), ("d + t + 1 > S2", dict(ids2=ids[:-1])),
                 ("duplicate id", dict(ids1=ids[:-1] + (ids[0],))), ("duplicate reveal id", dict(ids2=(1,) + ids[1:])),
                 ("id out of range", dict(ids1=ids[:-1] + (n,))), ("reveal id out of range", dict(ids2=ids[:-1] + (n,))),
                 ("no eval senders", dict(ids1=())), ("no reveal senders", dict(ids2=()))]
        for what, kw in cases:
            i1, i2 = kw.pop("ids1", ids), kw.pop("ids2", ids)
            assert c.call(threshold, i1, i2, **kw) == 4, what
        # TypeMismatch: either field's call on the other field's context
        p = c.ptr
        L = pkg.lib()
        arr = (C.c_size_t * S)(*ids)
        for fn, ctx in ((L.hbmpc_dev_batchrecon_parties, gl.ctx), (L.hbmpc_gl_dev_batchrecon_parties, eng.ctx)):
            rc = fn(ctx, arr, C.c_size_t(S), arr, C.c_size_t(S), C.c_void_p(p["x"]), C.c_size_t(N), C.c_size_t(n), C.c_size_t(d), C.c_size_t(t),
                    *(C.c_void_p(p[k]) for k in OUTPUTS), C.c_void_p(c.s))
            wait(stream, "a refused call")
            assert rc == 5
        got = c.read()
        for k in OUTPUTS:
            assert (got[k] == MARK).all(), (k, "a refused call wrote to it")
        # the optional buffers may be null
        assert c.call(threshold, ids, ids, null=("rstatus", "status", "summary_first", "summary")) == 0, eng.last_error()
        got = c.read()
        want = as_bytes("fr", BR.model("fr", n, t, d, x, ids, ids))
        for k in ("Y", "Z", "opened"):
            assert np.array_equal(got[k], want[k]), k
        for k in ("rstatus", "status", "summary_first", "summary"):
            assert (got[k] == MARK).all(), k
    finally:
        c.close()
        eng.close()
        gl.close()


# ---- routing --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field", ["fr", "goldilocks"])
def test_routing_gives_the_same_bytes(pkg, stream, field):
    """at the default threshold and one chunk above it, n = 17, Sat32 and set_force_generic: the same bytes as the model"""
    n, t, d = 4, 1, 1
    ids = tuple(range(d + t + 1))
    dflt = pkg.hbmpc.FUSED_BATCHRECON_DEFAULT[field]
    eng = engine(pkg, field)
    try:
        for G in (max(dflt, 1), dflt + 1):
            secrets, x = BR.honest(field, n, t, d, G)
            all_forms_match(eng, stream, field, n, t, d, x, ids, ids[::-1], model_of_honest(field, n, t, d, G, ids, ids[::-1]), forms=(None,), composition=False)
        secrets, x = BR.honest(field, 17, 5, 5, 3)
        ids17 = tuple(range(6, 17))
        all_forms_match(eng, stream, field, 17, 5, 5, x, ids17, ids17, model_of_honest(field, 17, 5, 5, 3, ids17, ids17), forms=(FORCED, 0))
        secrets, x = BR.honest(field, n, t, d, 3)
        xs = BR.lie(field, x, n, d, 1, 2)
        want = BR.model(field, n, t, d, xs, ids, ids)
        eng.set_force_generic(True)
        all_forms_match(eng, stream, field, n, t, d, xs, ids, ids, want, forms=(FORCED,))
        eng.set_force_generic(False)
        if field == "fr":
            eng.set_impl("sat32")
            all_forms_match(eng, stream, field, n, t, d, xs, ids, ids, want, forms=(FORCED,))
    finally:
        eng.close()


# ---- the handle -------------------------------------------------------------------------------------------------------------------------
def handle_outputs(bp):
    out = {k: np.ascontiguousarray(bp.download(k)).view(np.uint8).reshape(-1) for k in ("Y", "Z", "opened")}
    out["rstatus"] = bp.status("rstatus").reshape(-1)
    out["status"] = bp.status()
    out["summary_first"] = bp.summary_first().view(np.uint8)
    out["summary"] = bp.summary().view(np.uint8)
    return out


@pytest.mark.parametrize("field", ["fr", "goldilocks"])
def test_handle_run_checked_capture_replay(pkg, stream, field):
    n, t, d, G = 7, 2, 2, 3
    F = FLD[field]
    secrets, x = BR.honest(field, n, t, d, G)
    ids = tuple(range(d + t + 1))
    eng = engine(pkg, field)
    bp = pkg.pipelines.BatchRecon(eng, n, t, d, G * (d + 1), stream=stream.cuda_stream)
    try:
        bp.upload(F.arr(x))
        bp.run(check=True)
        wait(stream, "BatchRecon.run")
        eager = handle_outputs(bp)
        assert_same(eager, as_bytes(field, BR.model(field, n, t, d, x, ids, ids)), "the handle's run")
        assert F.ints(bp.download("opened")) == secrets
        # capture and replay with the outputs zeroed in between give the eager bytes
        bp.capture()
        for k in ("Y", "Z", "opened"):
            bp.upload_named(k, np.zeros_like(bp.download(k)))
        for k, nb in (("rstatus", n * G), ("status", G), ("summary_first", 16), ("summary", 16)):
            eng.h2d(bp.buffer(k)[0], np.zeros(nb, dtype=np.uint8), stream.cuda_stream)
        bp.replay()
        wait(stream, "BatchRecon.replay")
        assert_same(handle_outputs(bp), eager, "the replayed graph")
        # a checked run on the lie returns DecodingError
        bp.upload(F.arr(BR.lie(field, x, n, d, 1, 2)))
        with pytest.raises(RuntimeError, match="ShareErrorCode 8"):
            bp.run(check=True)
        wait(stream, "BatchRecon.run on the lie")
    finally:
        bp.close()
        eng.close()


@pytest.mark.parametrize("field", ["fr", "goldilocks"])
def test_handle_byzantine_recipients_between_the_arms(pkg, stream, field):
    """deal(), overwrite the Z rows of t recipients, finish() with reveal_senders = n: status 1 and the honest secrets; with t + 1 rows
    overwritten: status 8 and zeros.  (The only way the reveal arm's fallback can succeed: the first arm leaves either 0 or at least
    n - d zero reveals.)"""
    n, t, d, G = 7, 2, 2, 3
    F = FLD[field]
    secrets, x = BR.honest(field, n, t, d, G)
    ids1, ids2 = tuple(range(d + t + 1)), tuple(range(n))
    honest_z = BR.model(field, n, t, d, x, ids1, ids2)["Z"]
    eng = engine(pkg, field)
    bp = pkg.pipelines.BatchRecon(eng, n, t, d, G * (d + 1), reveal_senders=n, stream=stream.cuda_stream)
    try:
        bp.upload(F.arr(x))
        for liars, status, opened in (((1, 4), 1, secrets), ((0, 3, 6), 8, [0] * len(secrets))):
            bp.deal()
            wait(stream, "BatchRecon.deal")
            assert F.ints(bp.download("Z")) == honest_z
            z = [list(row) for row in honest_z]
            for r in liars:
                z[r] = [(v + 1 + r) % F.mod for v in z[r]]
            bp.upload_named("Z", F.arr(z))
            bp.finish()
            wait(stream, "BatchRecon.finish")
            want = BR.reveal_model(field, z, n, d, t, ids2)
            assert want["status"] == [status] * G and want["opened"] == opened
            assert bp.status().tolist() == want["status"] and F.ints(bp.download("opened")) == opened
            assert bp.summary().tolist() == list(want["summary"])
    finally:
        bp.close()
        eng.close()
