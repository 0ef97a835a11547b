"""RandBit for all parties as one device call (hbmpc_[gl_]dev_randbit_parties): its one-launch form (csrc/kernels_randbit_wg.hpp, a
workgroup per chunk of t + 1 elements) against its nine launches (hbmpc_set_fused_randbit(ctx, 0)) byte for byte in every buffer a
caller can see, and both against the restatement: tests/randbit_ref.py for honest shares, and for tampered shares the model below
(BatchRecon of degree t from senders 0 .. 2t in plain integers: a chunk that fails its verification opens to zero), which is itself
checked against randbit_ref on the honest inputs.

Every device call of this file runs on a stream of its own and is waited for with a deadline (`wait`): a kernel that does not finish
ends the session instead of blocking it."""
import functools
import time

import numpy as np
import pytest

from __graft_entry__ import load_package
from tests import edge_inputs as EI
from tests import randbit_ref as RB

pytestmark = pytest.mark.gpu
SHAPES = [("goldilocks", 4, 1), ("goldilocks", 5, 1), ("goldilocks", 7, 3), ("goldilocks", 16, 5), ("fr", 4, 1), ("fr", 7, 3), ("fr", 16, 5)]
CHUNKS = [1, 3, 41]  # one workgroup; fewer workgroups than the summaries' fan-in of 16; not a multiple of it
FORCED = 1 << 20
DECODING_ERROR = 8
LIMIT = 60.0  # seconds a device call may take before the session is ended
FLD = {"fr": EI.FR, "goldilocks": EI.GL}
OUTPUTS = ("deop", "sq", "sqop", "out", "status", "rst_de", "rst_sq", "sm_de_first", "sm_de", "sm_sq_first", "sm_sq", "rb")


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


# ---- the model: the call in plain integers, tampered shares included --------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _tables(field, n, t):
    F = FLD[field]
    al = [F.S.domain_element(n, j) for j in range(n)]
    basis = EI.lagrange_basis(F, n, tuple(range(t + 1)))  # basis[i][k]: coefficient k of L_i over senders 0 .. t
    return al, [(list(b) + [0] * (t + 1))[:t + 1] for b in basis]


def _interp(field, n, t, v):
    """coefficients [t + 1] of the polynomial through senders 0 .. t of v [2t + 1], or None when senders t + 1 .. 2t are not on it"""
    q = RB.PRIME[field]
    al, basis = _tables(field, n, t)
    co = [sum(v[i] * basis[i][k] for i in range(t + 1)) % q for k in range(t + 1)]
    for s in range(t + 1, 2 * t + 1):
        if sum(c * pow(al[s], k, q) for k, c in enumerate(co)) % q != v[s]:
            return None
    return co


def open_model(field, n, t, x):
    """BatchRecon of x [party][G (t + 1)] as the call runs it -> (opened [G (t + 1)], status bytes [n G], summary of the recipients'
    decodes, summary of the revealed values' decode)"""
    q = RB.PRIME[field]
    al, _ = _tables(field, n, t)
    M = t + 1
    G = len(x[0]) // M
    pw = [[pow(al[j], k, q) for k in range(M)] for j in range(n)]
    rst, opened, bad1, bad2 = [0] * (n * G), [], [], []
    for g in range(G):
        z = []
        for j in range(n):
            y = [sum(pw[j][k] * x[p][g * M + k] for k in range(M)) % q for p in range(2 * t + 1)]
            co = _interp(field, n, t, y)
            z.append(0 if co is None else co[0])
            if co is None:
                rst[j * G + g] = DECODING_ERROR
                bad1.append(j * G + g)
        co = _interp(field, n, t, z[:2 * t + 1])
        rst[g] = 0 if co is not None else DECODING_ERROR
        if co is None:
            bad2.append(g)
        opened += [0] * M if co is None else co
    summ = lambda bad: (len(bad), len(bad), min(bad) if bad else 0xFFFFFFFF, DECODING_ERROR if bad else 0)  # noqa: E731
    return opened, rst, summ(bad1), summ(bad2)


def model(field, n, t, sh):
    """every output of the call from the parties' shares (arrays [n][N]) -> dict of OUTPUTS in integers / byte lists"""
    q = RB.PRIME[field]
    a, ta, tb, tc = ([RB.to_ints(sh[k][p], field) for p in range(n)] for k in ("a", "ta", "tb", "tc"))
    N = len(a[0])
    x = [[(u - v) % q for u, v in zip(ta[p], a[p])] + [(u - v) % q for u, v in zip(tb[p], a[p])] for p in range(n)]
    deop, rst_de, s1, s2 = open_model(field, n, t, x)
    d, e = deop[:N], deop[N:]
    sq = [[(c - di * ei - di * ai - ei * ai) % q for c, di, ei, ai in zip(tc[p], d, e, a[p])] for p in range(n)]
    sqop, rst_sq, s3, s4 = open_model(field, n, t, sq)
    err, first, status, out = RB.phase2(sqop, a, q)
    nfail = sum(1 for s in status if s)
    rb = (2**64 - 1 if first is None else (status[first] << 32) | first, nfail)
    return {"deop": deop, "sq": sq, "sqop": sqop, "out": out, "status": status, "rst_de": rst_de, "rst_sq": rst_sq, "sm_de_first": s1, "sm_de": s2,
            "sm_sq_first": s3, "sm_sq": s4, "rb": rb}


@functools.lru_cache(maxsize=None)
def honest(field, n, t, N):
    """(secrets, shares) and the model's outputs, computed once per shape"""
    sec, sh = RB.pipeline_inputs(field, n, t, N, 4000 + 7 * n + N)
    return sec, sh, model(field, n, t, sh)


def test_model_matches_restatement_on_honest_shares():
    """the model of this file against tests/randbit_ref.py where both apply (no GPU work, but it guards the GPU tests' reference)"""
    for field, n, t in (("goldilocks", 7, 3), ("fr", 4, 1)):
        N = 3 * (t + 1)
        sec, sh, m = honest(field, n, t, N)
        wsq, wop, (err, first, status, want) = RB.pipeline_columns(field, sec, sh, np.arange(N))
        assert err == 0 and m["sq"] == wsq and m["sqop"] == wop and m["out"] == want and m["status"] == status
        assert not any(m["rst_de"]) and not any(m["rst_sq"]) and m["rb"] == (2**64 - 1, 0) and m["sm_de"] == (0, 0, 0xFFFFFFFF, 0)


# ---- the device call ----------------------------------------------------------------------------------------------------------------
class Call:
    """the buffers of one call shape on the device; run() returns every output as bytes"""

    def __init__(self, eng, stream, n, t, N):
        self.eng, self.stream, self.s = eng, stream, stream.cuda_stream
        self.n, self.t, self.N = n, t, N
        eb, G = eng.ebytes, max(1, N // (t + 1))
        Np = max(1, N)
        self.size = {"a": n * Np * eb, "ta": n * Np * eb, "tb": n * Np * eb, "tc": n * Np * eb, "desh": 2 * n * Np * eb, "Y": 2 * n * n * G * eb,
                     "Z": 2 * n * G * eb, "deop": 2 * Np * eb, "sq": n * Np * eb, "sqop": Np * eb, "out": n * Np * eb, "status": Np, "rst_de": 2 * n * G,
                     "rst_sq": n * G, "sm_de_first": 16, "sm_de": 16, "sm_sq_first": 16, "sm_sq": 16, "rb": 16}
        self.ptr = {k: eng.dev_alloc(v) for k, v in self.size.items()}

    def close(self):
        for p in self.ptr.values():
            self.eng.dev_free(p)

    def fill(self, names, byte):
        for k in names:
            self.eng.h2d(self.ptr[k], np.full(self.size[k], byte, dtype=np.uint8), self.s)

    def read(self, names):
        out = {k: np.zeros(self.size[k], dtype=np.uint8) for k in names}
        for k, arr in out.items():
            self.eng.d2h(arr, self.ptr[k], self.s)
        wait(self.stream, "download")
        return out

    def call(self, threshold, null=(), N=None, n=None, t=None):
        """one hbmpc_[gl_]dev_randbit_parties with the threshold at `threshold` (None: as the context has it) -> rc"""
        if threshold is not None:
            self.eng.set_fused_randbit(threshold)
        p = {k: (0 if k in null else v) for k, v in self.ptr.items()}
        rc = self.eng.randbit_parties(p["a"], p["ta"], p["tb"], p["tc"], self.N if N is None else N, self.n if n is None else n, self.t if t is None else t,
                                      p["desh"], p["Y"], p["Z"], p["deop"], p["sq"], p["sqop"], p["out"], p["status"], p["rst_de"], p["rst_sq"],
                                      p["sm_de_first"], p["sm_de"], p["sm_sq_first"], p["sm_sq"], p["rb"], stream=self.s)
        wait(self.stream, f"randbit_parties(n={self.n}, t={self.t}, N={self.N}, threshold={threshold})")
        return rc

    def run(self, sh, threshold):
        for k in ("a", "ta", "tb", "tc"):
            self.eng.h2d(self.ptr[k], sh[k], self.s)
        self.fill(OUTPUTS + ("desh",), 0xA5)
        rc = self.call(threshold)
        assert rc == 0, self.eng.last_error()
        return self.read(OUTPUTS + ("desh",))


def as_bytes(field, m, n, t, N):
    """the model's outputs as the bytes the device writes"""
    el = lambda v: np.ascontiguousarray(RB.from_ints(v, field)).view(np.uint8).reshape(-1)  # noqa: E731
    summ = lambda s: np.array(s, dtype=np.uint32).view(np.uint8)  # noqa: E731
    rb = np.zeros(16, dtype=np.uint8)
    rb[:8] = np.array([m["rb"][0]], dtype=np.uint64).view(np.uint8)
    rb[8:12] = np.array([m["rb"][1]], dtype=np.uint32).view(np.uint8)
    out = {"deop": el(m["deop"]), "sq": el([v for row in m["sq"] for v in row]), "sqop": el(m["sqop"]), "out": el([v for row in m["out"] for v in row]),
           "status": np.array(m["status"], dtype=np.uint8), "rst_de": np.array(m["rst_de"], dtype=np.uint8), "rst_sq": np.array(m["rst_sq"], dtype=np.uint8),
           "rb": rb}
    out.update({k: summ(m[k]) for k in ("sm_de_first", "sm_de", "sm_sq_first", "sm_sq")})
    return out


def default_threshold(eng):
    return load_package().hbmpc.FUSED_RANDBIT_DEFAULT[eng.field]


def both_forms_match(eng, stream, field, n, t, sh, want, forms=(FORCED, 0)):
    """the call in each form: every output equal between the forms and equal to `want` (a model's outputs)"""
    N = sh["a"].shape[1]
    c = Call(eng, stream, n, t, N)
    try:
        got = [c.run(sh, th) for th in forms]
    finally:
        c.close()
        eng.set_fused_randbit(default_threshold(eng))
    exp = as_bytes(field, want, n, t, N)
    for k in OUTPUTS + ("desh",):
        for g in got[1:]:
            assert np.array_equal(got[0][k], g[k]), (k, "the two forms differ")
    for k in OUTPUTS:
        assert np.array_equal(got[0][k], exp[k]), (k, "differs from the restatement")
    return got[0]


def test_device_call_exists(pkg):
    """both symbols and the setter, callable through hbmpc.py: a null buffer is refused with InvalidInput by either field's call"""
    for field in ("fr", "goldilocks"):
        eng = engine(pkg, field)
        try:
            assert callable(eng.randbit_parties) and callable(eng.set_fused_randbit)
            eng.set_fused_randbit(pkg.hbmpc.FUSED_RANDBIT_DEFAULT[field])
            assert eng.randbit_parties(*([0] * 4), 4, 4, 1, *([0] * 15)) == 4
        finally:
            eng.close()
    assert hasattr(pkg.lib(), "hbmpc_dev_randbit_parties") and hasattr(pkg.lib(), "hbmpc_gl_dev_randbit_parties")


@pytest.mark.parametrize("field,n,t", SHAPES)
@pytest.mark.parametrize("chunks", CHUNKS)
def test_both_forms_byte_for_byte(pkg, stream, field, n, t, chunks):
    N = chunks * (t + 1)
    sec, sh, m = honest(field, n, t, N)
    # the model is the restatement here: every column of tests/randbit_ref.py's pipeline
    wsq, wop, (err, first, status, want) = RB.pipeline_columns(field, sec, sh, np.arange(N))
    assert err == 0 and (m["sq"], m["sqop"], m["out"], m["status"]) == (wsq, wop, want, status)
    q = RB.PRIME[field]
    assert m["deop"] == [(x - y) % q for k in ("ta", "tb") for x, y in zip(RB.to_ints(sec[k], field), RB.to_ints(sec["a"], field))]
    eng = engine(pkg, field)
    try:
        got = both_forms_match(eng, stream, field, n, t, sh, m)
        # every output opens to a bit (with the largest fault bound the decoder admits for this n)
        out = got["out"].view(np.uint64).reshape((n, N) + sh["a"].shape[2:])
        rc, bits, st = eng.batch_recover_p0(list(range(n)), out, n, t, min(t, (n - 1) // 3))
        assert rc == 0 and not st.any(), eng.last_error()
        assert set(RB.to_ints(bits, field)) <= {0, 1}
    finally:
        eng.close()


def tampered(field, n, t, N, edit):
    sec, sh, _ = honest(field, n, t, N)
    bad = {k: v.copy() for k, v in sh.items()}
    edit(bad, sec)
    return bad


ADV_SHAPES = [("goldilocks", 5, 1), ("goldilocks", 16, 5), ("fr", 7, 3), ("fr", 16, 5)]


@pytest.mark.parametrize("field,n,t", ADV_SHAPES)
def test_tampered_shares(pkg, stream, field, n, t):
    """a tampered a share of party 0 in two chunks (both opens fail there), a tampered tc share of party 2 (only the second open fails),
    a tamper in chunk 0 and in the last chunk"""
    M, G = t + 1, 5
    N = G * M

    def a_two_chunks(bad, sec):
        for i in (M + 1, 3 * M):
            bad["a"][0, i] = bad["a"][1, i]

    def tc_party_2(bad, sec):
        bad["tc"][2, 2 * M] = bad["tc"][1, 2 * M]

    def first_and_last(bad, sec):
        bad["ta"][1, 0] = bad["ta"][0, 0]
        bad["tb"][0, N - 1] = bad["tb"][2, N - 1]

    eng = engine(pkg, field)
    try:
        for edit in (a_two_chunks, tc_party_2, first_and_last):
            sh = tampered(field, n, t, N, edit)
            m = model(field, n, t, sh)
            # party 0 is a sender of every recipient's decode: all n recipients of a tampered chunk fail, reveal zero, and zeros lie on
            # the zero polynomial -- the revealed values' decode then passes and the chunk opens to zero
            if edit is a_two_chunks:  # d- and e-chunks 1 and 3
                assert m["sm_de_first"] == (4 * n, 4 * n, 1, DECODING_ERROR) and m["sm_de"][1] == 0 and m["deop"][M:2 * M] == [0] * M
                assert m["rst_de"][2 * G + 1] == DECODING_ERROR and m["rst_de"][1] == 0 and m["sm_sq_first"][1] == 0
            if edit is tc_party_2:    # only the second open fails
                assert m["sm_de_first"][1] == 0 and m["sm_de"][1] == 0 and m["sm_sq_first"] == (n, n, 2, DECODING_ERROR)
                assert m["sqop"][2 * M:3 * M] == [0] * M and m["status"][2 * M] == RB.ST_ZERO
            if edit is first_and_last:  # d-chunk 0 and e-chunk G - 1 (chunk 2 G - 1 of the open)
                assert m["sm_de_first"] == (2 * n, 2 * n, 0, DECODING_ERROR) and m["rst_de"][2 * G + 2 * G - 1] == DECODING_ERROR
            both_forms_match(eng, stream, field, n, t, sh, m)
    finally:
        eng.close()


@pytest.mark.parametrize("field", ["goldilocks", "fr"])
def test_counters_after_a_failed_call(pkg, stream, field):
    """a one-launch call whose two opens fail (the recipients' decodes of d-chunk 0 and of the squares' chunk 1), then an honest
    one-launch call directly after it on the same engine and stream: the first counts what the model fails, the second reports
    nothing in any of the four summaries -- the last workgroup of the first left the counter pairs [24], [26] (and [0], [28], which
    no input can drive: the revealed values' decodes read what the kernel wrote) at zero.  Two chunks at n = 4, t = 1"""
    n, t, G = 4, 1, 2
    M = t + 1
    N = G * M

    def both_opens(bad, sec):
        bad["ta"][1, 0] = bad["ta"][0, 0]
        bad["tc"][2, M] = bad["tc"][1, M]

    sh = tampered(field, n, t, N, both_opens)
    m = model(field, n, t, sh)
    assert m["sm_de_first"] == (n, n, 0, DECODING_ERROR) and m["sm_sq_first"] == (n, n, 1, DECODING_ERROR)
    _, hsh, hm = honest(field, n, t, N)
    assert all(hm[k] == (0, 0, 0xFFFFFFFF, 0) for k in ("sm_de_first", "sm_de", "sm_sq_first", "sm_sq"))
    eng = engine(pkg, field)
    try:
        both_forms_match(eng, stream, field, n, t, sh, m, forms=(FORCED,))
        both_forms_match(eng, stream, field, n, t, hsh, hm, forms=(FORCED,))
    finally:
        eng.close()


def _no_root_delta(field, a):
    """delta with a^2 + delta a non-residue (ark's sqrt has no root)"""
    q = RB.PRIME[field]
    for delta in range(1, 200):
        if RB.ark_sqrt((a * a + delta) % q, q) is None:
            return delta
    raise AssertionError("no non-residue found")


@pytest.mark.parametrize("field,n,t", ADV_SHAPES)
def test_phase2_failures(pkg, stream, field, n, t):
    """a = 0 (RB_ZERO, summary ((1 << 32) | i, 1)); the same delta on every party's tc share: a^2 + delta without a root (RB_NO_ROOT, zero
    shares for every party); delta = -a^2 (RB_ZERO); one element of each kind in one call: `first` keeps phase2's precedence"""
    q = RB.PRIME[field]
    M, G = t + 1, 4
    N = G * M
    sec, _, _ = honest(field, n, t, N)
    av = RB.to_ints(sec["a"], field)

    def add_tc(bad, i, delta):
        col = RB.to_ints(bad["tc"][:, i], field)
        bad["tc"][:, i] = RB.from_ints([(v + delta) % q for v in col], field)

    def zero_a(i):
        def edit(bad, sec):
            bad["a"][:, i] = 0  # the constant sharing of zero: the secret a = 0
        return edit

    def no_root(i):
        return lambda bad, sec: add_tc(bad, i, _no_root_delta(field, av[i]))

    def zero_square(i):
        return lambda bad, sec: add_tc(bad, i, -av[i] * av[i])

    def all_three(bad, sec):
        no_root(1)(bad, sec), zero_square(N - 2)(bad, sec), zero_a(M + 1)(bad, sec), no_root(N - 1)(bad, sec)

    cases = [(zero_a(5 % N), (RB.ST_ZERO, 5 % N, 1)), (no_root(M), (RB.ST_NO_ROOT, M, 1)), (zero_square(N - 1), (RB.ST_ZERO, N - 1, 1)),
             (all_three, (RB.ST_ZERO, M + 1, 4))]
    eng = engine(pkg, field)
    try:
        for edit, (st, i, nfail) in cases:
            sh = tampered(field, n, t, N, edit)
            m = model(field, n, t, sh)
            assert m["rb"] == ((st << 32) | i, nfail) and m["status"][i] == st and all(row[i] == 0 for row in m["out"])
            assert m["sm_de"][1] == 0 and m["sm_sq"][1] == 0  # these are valid sharings: every open succeeds
            both_forms_match(eng, stream, field, n, t, sh, m)
    finally:
        eng.close()


@pytest.mark.parametrize("field,n,t", [("goldilocks", 16, 5), ("fr", 16, 5), ("fr", 4, 1)])
def test_field_edge_values(pkg, stream, field, n, t):
    """the edge values of tests/edge_inputs.py as the secrets a (0, 1, p - 1, the values around 2^32 over Goldilocks, all-ones limbs and the
    top-limb boundary over Fr), and as constant sharings of a (every party's share IS the edge value)"""
    F = FLD[field]
    M = t + 1
    G = -(-2 * len(F.edge) // M)
    N = G * M

    def edit(bad, sec):
        for i, v in enumerate(F.edge):
            sec_i = RB.from_ints([v], field)
            sec_a = sec["a"].copy()
            sec_a[i] = sec_i[0]
            bad["a"][:, i] = RB.share_all(field, sec_a[i:i + 1], n, t, 900 + i)[:, 0]
            bad["a"][:, len(F.edge) + i] = sec_i[0]

    sh = tampered(field, n, t, N, edit)
    m = model(field, n, t, sh)
    assert m["status"][0] == RB.ST_ZERO and m["status"][1] == RB.ST_OK and m["sm_de"][1] == 0 and m["sm_sq"][1] == 0
    eng = engine(pkg, field)
    try:
        both_forms_match(eng, stream, field, n, t, sh, m)
    finally:
        eng.close()


def test_routing(pkg, stream):
    """the default threshold: a call at it and one a chunk above it give the bytes of the forced forms; n = 17, a Sat32 context and
    set_force_generic fall back to the nine launches with the threshold at 2^20 and give the same bytes"""
    for field, n, t in (("goldilocks", 4, 1), ("fr", 4, 1)):
        default = pkg.hbmpc.FUSED_RANDBIT_DEFAULT[field]
        eng = engine(pkg, field)
        try:
            for G in (max(default, 1), default + 1):
                N = G * (t + 1)
                sec, sh = RB.pipeline_inputs(field, n, t, N, 31 + G)
                c = Call(eng, stream, n, t, N)
                try:
                    eng.set_fused_randbit(default)
                    got = [c.run(sh, None), c.run(sh, FORCED), c.run(sh, 0)]
                finally:
                    c.close()
                    eng.set_fused_randbit(default)
                for k in OUTPUTS + ("desh",):
                    assert np.array_equal(got[0][k], got[1][k]) and np.array_equal(got[0][k], got[2][k]), (field, G, k)
                assert not got[0]["status"].any() and not got[0]["rst_sq"].any()
        finally:
            eng.close()
    # outside the kernel: the same bytes as the restatement with the threshold at 2^20
    sec, sh, m = honest("goldilocks", 17, 5, 18)
    eng = engine(pkg, "goldilocks")
    try:
        both_forms_match(eng, stream, "goldilocks", 17, 5, sh, m)
    finally:
        eng.close()
    sec, sh, m = honest("fr", 4, 1, 6)
    for setup in (lambda e: e.set_impl("sat32"), lambda e: e.set_force_generic(True)):
        eng = engine(pkg, "fr")
        try:
            setup(eng)
            both_forms_match(eng, stream, "fr", 4, 1, sh, m)
        finally:
            eng.close()


@pytest.mark.parametrize("field", ["goldilocks", "fr"])
def test_refused_calls_write_nothing(pkg, stream, field):
    """N not a multiple of t + 1, N = 0, n < 2t + 1, a null buffer: InvalidInput and every output byte as it was, in both forms"""
    n, t, N = 4, 1, 6
    sec, sh, _ = honest(field, n, t, N)
    eng = engine(pkg, field)
    c = Call(eng, stream, n, t, N)
    names = OUTPUTS + ("desh", "Y", "Z")
    try:
        for k in ("a", "ta", "tb", "tc"):
            eng.h2d(c.ptr[k], sh[k], c.s)
        cases = [dict(N=N - 1), dict(N=0), dict(t=2), dict(null=("sqop",)), dict(null=("a",)), dict(null=("rb",)), dict(null=("rst_de",)), dict(n=0),
                 dict(n=256, t=1)]
        for th in (FORCED, 0):
            for kw in cases:
                c.fill(names, 0x5C)
                assert c.call(th, **kw) == 4, (th, kw)
                got = c.read(names)
                for k in names:
                    assert (got[k] == 0x5C).all(), (th, kw, k)
    finally:
        c.close()
        eng.close()


@pytest.mark.parametrize("field,n,t", [("goldilocks", 5, 1), ("fr", 16, 5)])
def test_graph_replay(pkg, stream, field, n, t):
    """the pipeline at 3 chunks, captured and replayed with the outputs zeroed in between: the bytes of the eager run"""
    N = 3 * (t + 1)
    sec, sh, m = honest(field, n, t, N)
    eng = engine(pkg, field)
    try:
        rb = pkg.pipelines.RandBit(eng, n, t, N, stream=stream.cuda_stream)
        rb.upload(sh["a"], sh["ta"], sh["tb"], sh["tc"])
        rb.run(check=True)
        wait(stream, "pipeline run")
        names = ("out", "sq", "sqop")
        eager = {k: rb.download(k) for k in names}
        assert RB.to_ints(eager["sqop"], field) == m["sqop"] and rb.rb_summary() == (2**64 - 1, 0)
        for q in range(n):
            assert RB.to_ints(eager["out"][q], field) == m["out"][q]
        rb.capture()
        wait(stream, "capture")
        for k in names:
            rb.upload_named(k, np.zeros_like(eager[k]))
        rb.replay()
        wait(stream, "replay")
        for k in names:
            assert np.array_equal(rb.download(k), eager[k]), k
        assert rb.rb_summary() == (2**64 - 1, 0) and not rb.status().any()
        rb.close()
    finally:
        eng.close()
