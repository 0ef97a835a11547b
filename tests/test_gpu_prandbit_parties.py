"""PRandBit / PRandInt for all parties as one device call (hbmpc_dev_prandbit_parties, hbmpc_dev_prandint_parties): the one-launch form
(csrc/kernels_prandbit_wg.hpp, a workgroup per chunk of t + 1 elements) against the separate launches (hbmpc_set_fused_prandbit(ctx, 0))
byte for byte in every buffer a caller can see, and both against the restatement: tests/prandbit_ref.py for honest inputs, and for
tampered shares the model below (BatchRecon of degree t from senders 0 .. 2t in plain integers: a chunk that fails its verification
opens to zero), which is itself checked against prandbit_ref on the honest inputs.

Every device call of this file runs on a stream of its own and is waited for with a deadline (`wait`): a kernel that does not finish
ends the session instead of blocking it.  (The handle-lifetime test, which runs last of the handle tests and only what they have run,
synchronises through the handle: one of its handles owns a stream that no event of the caller's can be recorded on.)"""
import functools
import math
import time

import numpy as np
import pytest

from __graft_entry__ import load_package
from tests import prandbit_ref as PR

pytestmark = pytest.mark.gpu
ONE_LAUNCH_SHAPES = [(4, 1), (5, 1), (7, 2), (10, 3), (12, 3)]  # (12,3): 150 KB of the 160 KB LDS, the largest layout that fits
OTHER_SHAPES = [(13, 4), (16, 5)]  # their coefficient tables do not fit a workgroup's LDS: always the separate launches
CHUNKS = [1, 3, 41]  # one workgroup; fewer workgroups than the summaries' fan-in of 16; not a multiple of it
FORCED = 1 << 20
INVALID_INPUT, TYPE_MISMATCH, DECODING_ERROR, FIELD_CAPACITY = 4, 5, 8, 104
LIMIT = 60.0  # seconds a device call may take before the session is ended
P = PR.P_GL
OUTPUTS = ("sums", "bad", "r_p", "r_2", "r_q", "rb", "opened", "b_p", "b_2", "rstatus", "summary_first", "summary")
INT_OUTPUTS = ("sums", "bad", "r_p")
NO_FAILURE = (0, 0, 0xFFFFFFFF, 0)


@pytest.fixture(scope="module")
def pkg():
    return load_package()


@pytest.fixture(scope="module")
def stream():
    torch = pytest.importorskip("torch")
    return torch.cuda.Stream(device=torch.device("cuda", 0))


@pytest.fixture(scope="module")
def engines(pkg):
    fr, gl = pkg.Engine(0, field="fr"), pkg.Engine(0, field="goldilocks")
    yield fr, gl
    fr.close()
    gl.close()


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


def lk_for(n, t):
    """l + k with C(n,t) n 2^(l+k) + 1 < q, so that r + b never wraps in Goldilocks: 55, 55, 55, 53, 52, 50, 47 for the shapes here"""
    lk = 55
    while math.comb(n, t) * n * 2**lk + 1 >= P:
        lk -= 1
    return lk


# ---- the model: the call in plain integers, offending values and tampered shares included -------------------------------------------
@functools.lru_cache(maxsize=None)
def _alpha(n):
    return [PR.domain_element(P, n, j) for j in range(n)]


def _interp(n, t, v):
    """coefficients [t + 1] of the polynomial through senders 0 .. t of v [2t + 1], or None when senders t + 1 .. 2t are not on it"""
    al = _alpha(n)
    co = PR.lagrange_interpolate(P, al[:t + 1], list(v[:t + 1]))
    for s in range(t + 1, 2 * t + 1):
        if PR.poly_eval(P, co, al[s]) != v[s]:
            return None
    return co


def open_model(n, t, x):
    """BatchRecon of x [party][G (t + 1)] as the call runs it with 2t + 1 senders -> (opened [G (t + 1)], status bytes [n G], summary of
    the recipients' decodes, summary of the revealed values' decode)"""
    al, M = _alpha(n), t + 1
    G = len(x[0]) // M
    pw = [[pow(al[j], k, P) for k in range(M)] for j in range(n)]
    rst, opened, bad1, bad2 = [0] * (n * G), [], [], []
    for g in range(G):
        z = []
        for j in range(n):
            y = [sum(pw[j][k] * x[p][g * M + k] for k in range(M)) % P for p in range(2 * t + 1)]
            co = _interp(n, t, y)
            z.append(0 if co is None else co[0])
            if co is None:
                rst[j * G + g] = DECODING_ERROR
                bad1.append(j * G + g)
        co = _interp(n, t, z[:2 * t + 1])
        rst[g] = 0 if co is not None else DECODING_ERROR
        if co is None:
            bad2.append(g)
        opened += [0] * M if co is None else co
    summ = lambda bad: (len(bad), len(bad), min(bad) if bad else 0xFFFFFFFF, DECODING_ERROR if bad else 0)  # noqa: E731
    return opened, rst, summ(bad1), summ(bad2)


def fold_model(contrib, lk):
    """numpy's wrapping sum over the senders and the verdict matrix: 1 where any value of (sender, set) exceeds 2^lk"""
    return contrib.sum(axis=0, dtype=np.uint64), (contrib > np.uint64(1 << lk)).any(axis=2).astype(np.uint8)


def model(n, t, contrib, b_q, lk):
    """every output of hbmpc_dev_prandbit_parties from contrib [n][Tn][B] and b_q [n][B] (numpy uint64) -> dict of OUTPUTS in integers"""
    sums, bad = fold_model(contrib, lk)
    B = contrib.shape[2]
    r_p, r_2 = PR.convert_fast(PR.P_FR, n, t, sums)
    r_q = PR.convert_fast(P, n, t, sums)[0]
    rb = [[(r_q[j][i] + int(b_q[j][i])) % P for i in range(B)] for j in range(n)]
    opened, rst, s1, s2 = open_model(n, t, rb)
    b_p, b_2 = PR.finalize(opened, r_p, r_2)
    return {"sums": sums, "bad": bad, "r_p": r_p, "r_2": r_2, "r_q": r_q, "rb": rb, "opened": opened, "b_p": b_p, "b_2": b_2, "rstatus": rst,
            "summary_first": s1, "summary": s2}


def as_bytes(m):
    """the model's outputs as the bytes the device writes"""
    by = lambda a: np.ascontiguousarray(a).view(np.uint8).reshape(-1)  # noqa: E731
    out = {"sums": by(m["sums"]), "bad": by(m["bad"])}
    for k in ("r_p", "b_p"):
        if k in m:
            out[k] = by(PR.rows_from_ints(m[k], "fr"))
    for k in ("r_q", "rb"):
        if k in m:
            out[k] = by(np.array(m[k], dtype=np.uint64))
    for k in ("r_2", "b_2", "rstatus"):
        if k in m:
            out[k] = by(np.array(m[k], dtype=np.uint8))
    if "opened" in m:
        out["opened"] = by(np.array(m["opened"], dtype=np.uint64))
    for k in ("summary_first", "summary"):
        if k in m:
            out[k] = by(np.array(m[k], dtype=np.uint32))
    return out


def edge_columns(contrib, lk, seed):
    """columns of all 0, all 1, all exactly 2^lk (allowed), odd only, even only -- a batch too short for all five takes them in turn"""
    B = contrib.shape[2]
    for col in range(min(B, 5)):
        kind = col if B >= 5 else (col + seed) % 5
        if kind == 0:
            contrib[:, :, col] = 0
        elif kind == 1:
            contrib[:, :, col] = 1
        elif kind == 2:
            contrib[:, :, col] = np.uint64(1 << lk)
        elif kind == 3:
            contrib[:, :, col] |= np.uint64(1)
        else:
            contrib[:, :, col] &= ~np.uint64(1)
    return contrib


@functools.lru_cache(maxsize=None)
def honest(n, t, G):
    """(contrib, bits, b_q, lk) with the edge columns, and the model's outputs, computed once per shape"""
    B, lk = G * (t + 1), lk_for(n, t)
    contrib, bits, b_q = PR.make_inputs(n, t, B, lk, seed=77 + 13 * n + G)
    contrib = edge_columns(np.array(contrib, dtype=np.uint64), lk, n + G)
    b_q = np.array(b_q, dtype=np.uint64)
    for a in (contrib, b_q):
        a.setflags(write=False)
    return contrib, bits, b_q, lk, model(n, t, contrib, b_q, lk)


def equals_restatement(n, t, contrib, b_q, lk, m):
    """PR.prandbit itself on the same inputs: sums, bad, r_q, r_p, r_2, rb, opened, b_p, b_2 of the model (whose bytes the device's are
    compared with) are the restatement's"""
    d = PR.prandbit(n, t, contrib.tolist(), lk, b_q.tolist(), fast=True)
    assert [list(map(int, row)) for row in m["sums"]] == d["sums"] and m["bad"].tolist() == d["bad"]
    for k in ("r_p", "r_2", "r_q", "rb", "opened", "b_p", "b_2"):
        assert m[k] == d[k], k


def test_model_matches_restatement_on_honest_inputs():
    """the model of this file against tests/prandbit_ref.py where both apply (no GPU work, but it guards the GPU tests' reference)"""
    assert [lk_for(n, t) for n, t in ((4, 1), (5, 1), (7, 2), (10, 3), (12, 3), (13, 4), (16, 5))] == [55, 55, 55, 53, 52, 50, 47]
    for n, t in ((4, 1), (7, 2)):
        contrib, bits, b_q, lk, m = honest(n, t, 3)
        equals_restatement(n, t, contrib, b_q, lk, m)
        assert not any(m["rstatus"]) and m["summary_first"] == NO_FAILURE and m["summary"] == NO_FAILURE
        assert PR.recovered_bits(n, t, m) == (bits, bits)


# ---- the device call ----------------------------------------------------------------------------------------------------------------
class Call:
    """the buffers of one call shape on the device; run() returns every output as bytes"""

    def __init__(self, fr, gl, stream, n, t, B):
        self.fr, self.gl, self.stream, self.s = fr, gl, stream, stream.cuda_stream
        self.n, self.t, self.B = n, t, B
        Tn, G, Bp = math.comb(n, t), max(1, B // (t + 1)), max(1, B)
        self.Tn = Tn
        self.size = {"contrib": n * Tn * Bp * 8, "b_q": n * Bp * 8, "sums": Tn * Bp * 8, "bad": n * Tn, "r_p": n * Bp * 32, "r_2": n * Bp, "r_q": n * Bp * 8,
                     "rb": n * Bp * 8, "Y": n * n * G * 8, "Z": n * G * 8, "opened": Bp * 8, "b_p": n * Bp * 32, "b_2": n * Bp, "rstatus": n * G,
                     "summary_first": 16, "summary": 16}
        self.ptr = {k: fr.dev_alloc(v) for k, v in self.size.items()}

    def close(self):
        for p in self.ptr.values():
            self.fr.dev_free(p)

    def fill(self, names, byte):
        for k in names:
            self.fr.h2d(self.ptr[k], np.full(self.size[k], byte, dtype=np.uint8), self.s)

    def read(self, names):
        out = {k: np.zeros(self.size[k], dtype=np.uint8) for k in names}
        for k, arr in out.items():
            self.fr.d2h(arr, self.ptr[k], self.s)
        wait(self.stream, "download")
        return out

    def call(self, threshold, null=(), fr=None, gl=None, open_senders=0, **kw):
        """one hbmpc_dev_prandbit_parties with the threshold at `threshold` (None: as the context has it) -> rc"""
        fr = self.fr if fr is None else fr
        if threshold is not None:
            fr.set_fused_prandbit(threshold)
        p = {k: (0 if k in null else v) for k, v in self.ptr.items()}
        v = dict(n=self.n, t=self.t, B=self.B, lk=lk_for(self.n, self.t))
        v.update(kw)
        rc = fr.prandbit_parties(self.gl if gl is None else gl, p["contrib"], p["b_q"], v["n"], v["t"], v["B"], v["lk"], p["sums"], p["bad"], p["r_p"], p["r_2"],
                                 p["r_q"], p["rb"], p["Y"], p["Z"], p["opened"], p["b_p"], p["b_2"], p["rstatus"], p["summary_first"], p["summary"],
                                 open_senders=open_senders, stream=self.s)
        wait(self.stream, f"prandbit_parties(n={self.n}, t={self.t}, B={self.B}, threshold={threshold})")
        return rc

    def call_int(self, threshold, null=(), **kw):
        if threshold is not None:
            self.fr.set_fused_prandbit(threshold)
        p = {k: (0 if k in null else v) for k, v in self.ptr.items()}
        v = dict(n=self.n, t=self.t, B=self.B, lk=lk_for(self.n, self.t))
        v.update(kw)
        rc = self.fr.prandint_parties(p["contrib"], v["n"], v["t"], v["B"], v["lk"], p["sums"], p["bad"], p["r_p"], stream=self.s)
        wait(self.stream, f"prandint_parties(n={self.n}, t={self.t}, B={self.B}, threshold={threshold})")
        return rc

    def upload(self, contrib, b_q=None):
        self.fr.h2d(self.ptr["contrib"], np.ascontiguousarray(contrib), self.s)
        if b_q is not None:
            self.fr.h2d(self.ptr["b_q"], np.ascontiguousarray(b_q), self.s)

    def run(self, contrib, b_q, threshold, lk=None, **kw):
        self.upload(contrib, b_q)
        self.fill(OUTPUTS + ("Y", "Z"), 0xA5)
        rc = self.call(threshold, **({} if lk is None else {"lk": lk}), **kw)
        assert rc == 0, self.fr.last_error()
        return self.read(OUTPUTS + ("Y", "Z"))


def took_one_launch(got):
    """which form ran, from the workspaces: the separate launches write every sender's messages to Y and the revealed values to Z, the
    one launch keeps both in LDS and leaves the workspaces as they were (0xA5 here)"""
    untouched = [bool((got[k] == 0xA5).all()) for k in ("Y", "Z")]
    assert untouched[0] == untouched[1]
    return untouched[0]


def both_forms_match(engines, pkg, stream, n, t, contrib, b_q, want, lk=None, forms=(FORCED, 0), compare=OUTPUTS, one_launch=None):
    """the call in each form: every output equal between the forms, and the outputs named by `compare` equal to `want` (a model's).
    one_launch: whether the threshold at 2^20 takes the kernel (default: the shapes whose tables fit); at 0 it never does"""
    fr, gl = engines
    c = Call(fr, gl, stream, n, t, contrib.shape[2])
    try:
        got = [c.run(contrib, b_q, th, lk) for th in forms]
    finally:
        c.close()
        fr.set_fused_prandbit(pkg.hbmpc.FUSED_PRANDBIT_DEFAULT)
    exp = as_bytes(want)
    for th, g in zip(forms, got):
        assert took_one_launch(g) == (th == FORCED and ((n, t) in ONE_LAUNCH_SHAPES if one_launch is None else one_launch)), (th, "the wrong form ran")
    for k in OUTPUTS:
        for g in got[1:]:
            assert np.array_equal(got[0][k], g[k]), (k, "the two forms differ")
    for k in compare:
        assert np.array_equal(got[0][k], exp[k]), (k, "differs from the restatement")
    return got[0]


def test_device_call_exists(pkg, engines):
    """the symbols and the setter, callable through hbmpc.py: a null buffer is refused with InvalidInput"""
    fr, gl = engines
    assert callable(fr.prandbit_parties) and callable(fr.prandint_parties) and callable(fr.set_fused_prandbit)
    fr.set_fused_prandbit(pkg.hbmpc.FUSED_PRANDBIT_DEFAULT)
    assert fr.prandbit_parties(gl, 0, 0, 4, 1, 2, 55, *([0] * 12)) == INVALID_INPUT
    assert fr.prandint_parties(0, 4, 1, 2, 55, 0, 0, 0) == INVALID_INPUT
    for sym in ("hbmpc_dev_prandbit_parties", "hbmpc_dev_prandint_parties", "hbmpc_set_fused_prandbit"):
        assert hasattr(pkg.lib(), sym)


@pytest.mark.parametrize("n,t,chunks", [(n, t, G) for n, t in ONE_LAUNCH_SHAPES for G in CHUNKS if (n, t) != (12, 3) or G == 1])
def test_both_forms_byte_for_byte(pkg, engines, stream, n, t, chunks):
    contrib, bits, b_q, lk, m = honest(n, t, chunks)
    equals_restatement(n, t, contrib, b_q, lk, m)
    assert not m["bad"].any() and not any(m["rstatus"]) and m["summary"] == NO_FAILURE
    assert PR.recovered_bits(n, t, m) == (bits, bits)  # the output shares hold the input bits, over Fr and over GF(2^8)
    both_forms_match(engines, pkg, stream, n, t, contrib, b_q, m)


@pytest.mark.parametrize("n,t", OTHER_SHAPES)
def test_shapes_outside_the_kernel(pkg, engines, stream, n, t):
    """forcing the threshold up does not change the form; the bytes equal the restatement"""
    contrib, bits, b_q, lk, m = honest(n, t, 1)
    assert PR.recovered_bits(n, t, m) == (bits, bits) and m["summary"] == NO_FAILURE
    if (n, t) == (13, 4):  # at (16,5) the restatement takes 3 s more: there the model shares its arithmetic (convert_fast, finalize)
        equals_restatement(n, t, contrib, b_q, lk, m)
    both_forms_match(engines, pkg, stream, n, t, contrib, b_q, m)


@pytest.mark.parametrize("n,t", [(5, 1), (10, 3)])
def test_sums_at_the_capacity_bound(pkg, engines, stream, n, t):
    """every contribution exactly 2^(l+k) with l + k the largest the capacity rule admits: folded sums of n 2^(l+k) (max_r of
    tests/test_gpu_prandbit.py), and columns one below it; r + b wraps in Goldilocks here, which the model follows"""
    lk = 61 - math.ceil(math.log2(n))
    assert PR.capacity_ok(n, lk) and not PR.capacity_ok(n, lk + 1)
    G = 3
    B = G * (t + 1)
    _, _, b_q, _, _ = honest(n, t, G)
    contrib = np.full((n, math.comb(n, t), B), 1 << lk, dtype=np.uint64)
    contrib[0, :, 1::2] -= np.uint64(1)
    m = model(n, t, contrib, b_q, lk)
    assert int(m["sums"].max()) == n << lk and not m["bad"].any()
    both_forms_match(engines, pkg, stream, n, t, contrib, b_q, m, lk=lk)


@pytest.mark.parametrize("n,t", [(7, 2), (10, 3)])
def test_offending_values(pkg, engines, stream, n, t):
    """2^(l+k) + 1 and 2^64 - 1 at one sender, at several senders, at all senders in one set: the verdict bytes are the expected matrix,
    the sums numpy's wrapping sums, and both forms give the same bytes everywhere (a sum beyond 2^62 is outside the conversion's
    contract, so its shares are compared between the forms only)"""
    G = 3
    honest_c, _, b_q, lk, _ = honest(n, t, G)
    Tn, B = honest_c.shape[1], honest_c.shape[2]
    over, top = np.uint64((1 << lk) + 1), np.uint64(2**64 - 1)

    def one_sender(c, want):
        c[2, 1, 0], c[2, Tn - 1, B - 1] = over, top
        want[2, 1] = want[2, Tn - 1] = 1

    def several_senders(c, want):
        for s, T, i, v in ((0, 0, 0, top), (3, 0, 1, over), (n - 1, 2, B - 1, top), (1, Tn - 1, t + 1, over)):
            c[s, T, i] = v
            want[s, T] = 1

    def all_senders_one_set(c, want):
        c[:, 3, t + 2] = top
        c[:, 3, 0] = over
        want[:, 3] = 1

    for edit in (one_sender, several_senders, all_senders_one_set):
        contrib, want = honest_c.copy(), np.zeros((n, Tn), dtype=np.uint8)
        edit(contrib, want)
        sums, bad = fold_model(contrib, lk)
        assert np.array_equal(bad, want)
        both_forms_match(engines, pkg, stream, n, t, contrib, b_q, {"sums": sums, "bad": want}, compare=("sums", "bad"))


@pytest.mark.parametrize("n,t", [(5, 1), (7, 2), (10, 3)])
def test_tampered_shares(pkg, engines, stream, n, t):
    """b_q of one party among 0 .. 2t plus 5 in one chunk of three: that chunk's decodes fail with DecodingError, it opens to zero and the
    summaries count it; the other chunks are untouched.  The same change at a party beyond 2t alters that party's rb and nothing opened"""
    G, M = 3, t + 1
    contrib, bits, hb_q, lk, hm = honest(n, t, G)
    for party in (0, 2 * t):
        b_q = hb_q.copy()
        b_q[party, M + 1] = (int(b_q[party, M + 1]) + 5) % P
        m = model(n, t, contrib, b_q, lk)
        # a sender of every recipient's decode: all n recipients of chunk 1 fail and reveal zero; zeros lie on the zero polynomial,
        # so the revealed values' decode passes and the chunk opens to zero
        assert m["summary_first"] == (n, n, 1, DECODING_ERROR) and m["summary"] == NO_FAILURE
        assert [m["rstatus"][j * G + 1] for j in range(n)] == [0] + [DECODING_ERROR] * (n - 1) and sum(1 for s in m["rstatus"] if s) == n - 1
        assert m["opened"][M:2 * M] == [0] * M and m["opened"][:M] == hm["opened"][:M] and m["opened"][2 * M:] == hm["opened"][2 * M:]
        for j in range(n):
            assert m["b_p"][j][:M] == hm["b_p"][j][:M] and m["b_p"][j][2 * M:] == hm["b_p"][j][2 * M:]
            assert m["b_p"][j][M:2 * M] == [(-v) % PR.P_FR for v in m["r_p"][j][M:2 * M]]
        both_forms_match(engines, pkg, stream, n, t, contrib, b_q, m)
    party = 2 * t + 1
    b_q = hb_q.copy()
    b_q[party, M + 1] = (int(b_q[party, M + 1]) + 5) % P
    m = model(n, t, contrib, b_q, lk)
    changed = {k for k in OUTPUTS if not np.array_equal(as_bytes(m)[k], as_bytes(hm)[k])}
    assert changed == {"rb"} and m["rb"][party][M + 1] == (hm["rb"][party][M + 1] + 5) % P
    assert sum(1 for j in range(n) for i in range(G * M) if m["rb"][j][i] != hm["rb"][j][i]) == 1
    both_forms_match(engines, pkg, stream, n, t, contrib, b_q, m)


def test_counters_after_a_failed_call(pkg, engines, stream):
    """a one-launch call whose recipients' decodes fail in chunk 1, then an honest one-launch call directly after it on the same
    engines and stream: the first counts what the model fails, the second reports nothing in either summary -- the last workgroup of
    the first left the counter pair [24] (and [0], which no input can drive: the revealed values' decode reads what the kernel wrote)
    at zero.  Two chunks at n = 5, t = 1; both_forms_match asserts that the kernel ran"""
    n, t, G = 5, 1, 2
    M = t + 1
    contrib, _, hb_q, lk, hm = honest(n, t, G)
    b_q = hb_q.copy()
    b_q[0, M + 1] = (int(b_q[0, M + 1]) + 5) % P
    m = model(n, t, contrib, b_q, lk)
    assert m["summary_first"] == (n, n, 1, DECODING_ERROR) and m["summary"] == NO_FAILURE
    assert hm["summary_first"] == NO_FAILURE and hm["summary"] == NO_FAILURE
    both_forms_match(engines, pkg, stream, n, t, contrib, b_q, m, forms=(FORCED,))
    both_forms_match(engines, pkg, stream, n, t, contrib, hb_q, hm, forms=(FORCED,))


def test_sat32_context_takes_the_separate_launches(pkg, engines, stream):
    """a Sat32 Fr context never takes the kernel: with the threshold forced up it gives the bytes of U29"""
    n, t = 7, 2
    contrib, bits, b_q, lk, m = honest(n, t, 3)
    fr, gl = engines
    sat = pkg.Engine(0, field="fr")
    try:
        sat.set_impl("sat32")
        both_forms_match((sat, gl), pkg, stream, n, t, contrib, b_q, m, one_launch=False)
        gl.set_single_launch_decode(False)  # the decodes' several-launch form: outside the kernel too, the same bytes
        both_forms_match(engines, pkg, stream, n, t, contrib, b_q, m, forms=(FORCED,), one_launch=False)
    finally:
        gl.set_single_launch_decode(True)
        sat.close()


@pytest.mark.parametrize("n,t", [(7, 2), (10, 3)])
def test_all_senders_open_the_same_values(pkg, engines, stream, n, t):
    """open_senders = n on honest inputs (the decodes' OEC path): opened, b_p and b_2 as with 2t + 1; open_senders = 2t + 1 is the default"""
    contrib, bits, b_q, lk, m = honest(n, t, 3)
    fr, gl = engines
    c = Call(fr, gl, stream, n, t, contrib.shape[2])
    try:
        exp = as_bytes(m)
        for S in (n, 2 * t + 2, 2 * t + 1):
            got = c.run(contrib, b_q, FORCED, open_senders=S)
            assert took_one_launch(got) == (S == 2 * t + 1)  # an OEC round exists beyond 2t + 1 senders: the separate launches
            for k in ("sums", "bad", "r_p", "r_2", "r_q", "rb", "opened", "b_p", "b_2"):
                assert np.array_equal(got[k], exp[k]), (S, k)
            assert not got["rstatus"].any() and got["summary"].view(np.uint32)[1] == 0
    finally:
        c.close()
        fr.set_fused_prandbit(pkg.hbmpc.FUSED_PRANDBIT_DEFAULT)


@pytest.mark.parametrize("n,t", [(5, 1), (10, 3)])
def test_prandint(pkg, engines, stream, n, t):
    """PRandInt at B = 1, t + 1, 63, 65 (a short last workgroup): one launch against the separate launches against the restatement"""
    fr, gl = engines
    lk = lk_for(n, t)
    for B in (1, t + 1, 63, 65):
        contrib, _, _ = PR.make_inputs(n, t, B, lk, seed=500 + B + n, with_bits=False)
        contrib = edge_columns(np.array(contrib, dtype=np.uint64), lk, B)
        contrib[n - 1, 0, B - 1] = np.uint64((1 << lk) + 1)  # one verdict, in the last element
        d = PR.prandint(n, t, contrib.tolist(), lk, fast=True)
        exp = as_bytes({"sums": np.array(d["sums"], dtype=np.uint64), "bad": np.array(d["bad"], dtype=np.uint8), "r_p": d["r_p"]})
        assert d["bad"][n - 1][0] == 1 and sum(map(sum, d["bad"])) == 1
        c = Call(fr, gl, stream, n, t, B)
        try:
            got = []
            for th in (FORCED, 0):
                c.upload(contrib)
                c.fill(INT_OUTPUTS, 0xA5)
                assert c.call_int(th) == 0, fr.last_error()
                got.append(c.read(INT_OUTPUTS))
        finally:
            c.close()
            fr.set_fused_prandbit(pkg.hbmpc.FUSED_PRANDBIT_DEFAULT)
        for k in INT_OUTPUTS:
            assert np.array_equal(got[0][k], got[1][k]), (B, k, "the two forms differ")
            assert np.array_equal(got[0][k], exp[k]), (B, k, "differs from the restatement")


def test_against_the_composition(pkg, engines, stream):
    """honest inputs at (7,2): pipelines.PRandBit.run (the composition of eight calls, all n senders) opens the same values"""
    n, t = 7, 2
    contrib, bits, b_q, lk, m = honest(n, t, 3)
    fr, gl = engines
    B = contrib.shape[2]
    pb = pkg.pipelines.PRandBit(gl, fr, n, t, B, stream=stream.cuda_stream)
    try:
        pb.upload_named("contrib", contrib)
        pb.upload_named("b_q", b_q)
        pb.run(lk)
        wait(stream, "pipelines.PRandBit.run")
        comp = {"opened": pb.download_named("opened", np.uint64, (B,)), "b_p": pb.download_named("b_p", np.uint64, (n, B, 4)),
                "b_2": pb.download_named("b_2", np.uint8, (n, B))}
    finally:
        pb.close()
    got = both_forms_match(engines, pkg, stream, n, t, contrib, b_q, m)
    for k, v in comp.items():
        assert np.array_equal(got[k], v.view(np.uint8).reshape(-1)), k


def test_default_threshold_routes(pkg, engines, stream):
    """with the context's own threshold: a call at it and one a chunk above it give the bytes of the forced forms"""
    n, t = 4, 1
    default = pkg.hbmpc.FUSED_PRANDBIT_DEFAULT
    fr, gl = engines
    for G in (max(default, 1), default + 1):
        B, lk = G * (t + 1), lk_for(n, t)
        contrib, _, b_q = PR.make_inputs(n, t, B, lk, seed=31 + G)
        contrib, b_q = np.array(contrib, dtype=np.uint64), np.array(b_q, dtype=np.uint64)
        c = Call(fr, gl, stream, n, t, B)
        try:
            fr.set_fused_prandbit(default)
            got = [c.run(contrib, b_q, None), c.run(contrib, b_q, FORCED), c.run(contrib, b_q, 0)]
        finally:
            c.close()
            fr.set_fused_prandbit(default)
        assert [took_one_launch(g) for g in got] == [G <= default, True, False]
        for k in OUTPUTS:
            assert np.array_equal(got[0][k], got[1][k]) and np.array_equal(got[0][k], got[2][k]), (G, k)
        assert not got[0]["rstatus"].any() and not got[0]["bad"].any()


def test_refused_calls_write_nothing(pkg, engines, stream):
    """every error code of the call, in both forms, with poisoned output buffers: a refused call has written nothing"""
    n, t, G = 4, 1, 3
    contrib, bits, b_q, lk, _ = honest(n, t, G)
    B = contrib.shape[2]
    fr, gl = engines
    gl2 = pkg.Engine(0, field="goldilocks")
    c = Call(fr, gl, stream, n, t, B)
    names = OUTPUTS + ("Y", "Z")
    try:
        c.upload(contrib, b_q)
        cases = [(dict(B=B - 1), INVALID_INPUT), (dict(t=2), INVALID_INPUT), (dict(n=3), INVALID_INPUT), (dict(n=0), INVALID_INPUT),
                 (dict(n=256, t=1), INVALID_INPUT), (dict(n=300, t=0, B=1), INVALID_INPUT), (dict(n=40, t=13, B=14), INVALID_INPUT),
                 (dict(lk=60), FIELD_CAPACITY), (dict(lk=64), FIELD_CAPACITY), (dict(fr=gl2), TYPE_MISMATCH), (dict(gl=fr), TYPE_MISMATCH),
                 (dict(open_senders=2), INVALID_INPUT), (dict(open_senders=n + 1), INVALID_INPUT), (dict(B=0), 0)]
        cases += [(dict(null=(k,)), INVALID_INPUT) for k in ("contrib", "b_q", "sums", "bad", "r_p", "r_2", "r_q", "rb", "Y", "Z", "opened", "b_p", "b_2",
                                                            "rstatus")]
        for th in (FORCED, 0):
            for kw, want in cases:
                c.fill(names, 0x5C)
                kw = dict(kw)
                if "fr" in kw:  # the threshold is read from the Fr context of the call; a Goldilocks context in its place is refused first
                    assert c.call(None, **kw) == want, (th, kw)
                else:
                    assert c.call(th, **kw) == want, (th, kw)
                got = c.read(names)
                for k in names:
                    assert (got[k] == 0x5C).all(), (th, kw, k)
        for th in (FORCED, 0):  # PRandInt: any B; the same shape and capacity checks
            for kw, want in [(dict(t=2), INVALID_INPUT), (dict(n=256, t=1), INVALID_INPUT), (dict(lk=60), FIELD_CAPACITY), (dict(null=("r_p",)), INVALID_INPUT),
                             (dict(null=("contrib",)), INVALID_INPUT), (dict(B=0), 0)]:
                c.fill(INT_OUTPUTS, 0x5C)
                assert c.call_int(th, **kw) == want, (th, kw)
                got = c.read(INT_OUTPUTS)
                for k in INT_OUTPUTS:
                    assert (got[k] == 0x5C).all(), (th, kw, k)
        assert fr.L.hbmpc_dev_prandbit_parties(None, gl.ctx, *([None] * 22)) == INVALID_INPUT
        assert fr.L.hbmpc_dev_prandbit_parties(fr.ctx, None, *([None] * 22)) == INVALID_INPUT
    finally:
        c.close()
        gl2.close()
        fr.set_fused_prandbit(pkg.hbmpc.FUSED_PRANDBIT_DEFAULT)


# ---- the handles (hbmpc_pipe_prandbit_create, hbmpc_pipe_prandint_create) ---------------------------------------------------------------
HANDLE_OUTPUTS = OUTPUTS  # the handle's buffers carry the call's names


@pytest.mark.parametrize("n,t", [(5, 1), (10, 3)])
def test_handle_run_capture_replay(pkg, engines, stream, n, t):
    """create, upload by name, run (checked), capture and replay with the outputs cleared in between: the bytes of the eager run, which
    are the restatement's; unknown buffer names are InvalidInput (that destroy frees the block: test_handle_destroy_frees_the_block)"""
    import ctypes as C
    contrib, bits, b_q, lk, m = honest(n, t, 3)
    B = contrib.shape[2]
    fr, gl = engines
    pb = pkg.pipelines.PRandBitPipe(gl, fr, n, t, B, lk, stream=stream.cuda_stream)
    try:
        assert pb.buffer("contrib")[1] == contrib.size and pb.buffer("b_p")[1] == n * B and pb.buffer("bad")[1] == n * math.comb(n, t)
        assert pb.buffer("rstatus")[1] == n * 3 and pb.buffer("Y")[1] == n * n * 3 and pb.buffer("Z")[1] == n * 3
        for name in ("no_such_buffer", "a", "out"):
            assert fr.L.hbmpc_pipe_buffer(pb.h, name.encode(), None, None) == INVALID_INPUT
            assert fr.L.hbmpc_pipe_upload(pb.h, name.encode(), contrib.ctypes.data_as(C.c_void_p), C.c_size_t(1)) == INVALID_INPUT
        pb.upload_named("contrib", contrib)
        pb.upload_named("b_q", b_q)
        pb.run(check=True)
        wait(stream, "handle run")
        exp = as_bytes(m)
        eager = {k: pb.download_named(k) for k in HANDLE_OUTPUTS}
        for k in HANDLE_OUTPUTS:
            assert np.array_equal(eager[k].view(np.uint8).reshape(-1), exp[k]), k
        assert tuple(int(v) for v in pb.summary()) == NO_FAILURE and pb.open_summary() == [NO_FAILURE, NO_FAILURE]
        pb.capture()
        wait(stream, "capture")
        for k in HANDLE_OUTPUTS:
            pb.upload_named(k, np.full_like(eager[k], 0x5C if eager[k].dtype == np.uint8 else 0))
        pb.replay()
        wait(stream, "replay")
        for k in HANDLE_OUTPUTS:
            assert np.array_equal(pb.download_named(k), eager[k]), k
    finally:
        pb.close()


def test_handle_checked_mode_and_prandint(pkg, engines, stream):
    """checked mode returns DecodingError (8) for a tampered share of a sender, and the unchecked run gives the model's bytes; the PRandInt
    handle gives the restatement's shares; shapes and contexts a handle refuses"""
    n, t, G = 7, 2, 3
    contrib, bits, hb_q, lk, hm = honest(n, t, G)
    B = contrib.shape[2]
    fr, gl = engines
    b_q = hb_q.copy()
    b_q[1, t + 2] = (int(b_q[1, t + 2]) + 5) % P
    m = model(n, t, contrib, b_q, lk)
    pb = pkg.pipelines.PRandBitPipe(gl, fr, n, t, B, lk, stream=stream.cuda_stream)
    try:
        pb.upload_named("contrib", contrib)
        pb.upload_named("b_q", b_q)
        with pytest.raises(RuntimeError, match=f"ShareErrorCode {DECODING_ERROR}"):
            pb.run(check=True)
        pb.run(check=False)
        wait(stream, "handle run")
        exp = as_bytes(m)
        for k in HANDLE_OUTPUTS:
            assert np.array_equal(pb.download_named(k).view(np.uint8).reshape(-1), exp[k]), k
        assert pb.open_summary() == [m["summary_first"], m["summary"]] and m["summary_first"][1] == n
    finally:
        pb.close()
    pi = pkg.pipelines.PRandIntPipe(fr, n, t, B - 1, lk, stream=stream.cuda_stream)
    try:
        pi.upload_named("contrib", np.ascontiguousarray(contrib[:, :, :B - 1]))
        pi.run(check=False)
        wait(stream, "PRandInt handle run")
        assert np.array_equal(pi.download_named("r_p").view(np.uint8).reshape(-1), as_bytes({"sums": hm["sums"], "bad": hm["bad"],
                                                                                            "r_p": [row[:B - 1] for row in hm["r_p"]]})["r_p"])
        assert not pi.download_named("bad").any()
        with pytest.raises(AttributeError):
            pi.b_q
    finally:
        pi.close()
    for args, code in (((gl, fr, n, t, B - 1, lk), INVALID_INPUT), ((gl, fr, 6, 2, 6, lk), INVALID_INPUT), ((fr, gl, n, t, B, lk), TYPE_MISMATCH)):
        with pytest.raises(RuntimeError, match=f"ShareErrorCode {code}"):
            pkg.pipelines.PRandBitPipe(*args, stream=stream.cuda_stream)
    with pytest.raises(RuntimeError, match=f"ShareErrorCode {TYPE_MISMATCH}"):
        pkg.pipelines.PRandIntPipe(gl, n, t, B, lk, stream=stream.cuda_stream)


def test_handle_destroy_frees_the_block(pkg, engines, stream):
    """create / run / capture / destroy in a loop leaves the device's free memory where it was: the arena (1.9 MB at this shape, 20
    handles = 38 MB) goes back with the handle -- both for a caller's stream and for stream = NULL, where the handle owns its stream and
    its destructor also drains it, drops the graph and releases the stream with its scratch.  The bound is the 8 MB of
    tests/test_gpu_table_cache.py: far below the 38 MB that leaked arenas would hold.  The handle without a stream of the caller's gives
    the bytes of the other."""
    import torch
    n, t = 10, 3
    contrib, bits, b_q, lk, m = honest(n, t, 41)
    B = contrib.shape[2]
    fr, gl = engines
    arena = pkg.pipelines.PRandBitPipe(gl, fr, n, t, B, lk, stream=stream.cuda_stream)
    assert sum(arena.buffer(k)[1] * arena._EB[k] for k in arena._EB) > (1 << 20)
    arena.close()

    def cycle(st):
        pb = pkg.pipelines.PRandBitPipe(gl, fr, n, t, B, lk, stream=st)
        try:
            pb.upload_named("contrib", contrib)
            pb.upload_named("b_q", b_q)
            pb.run(check=True)
            pb.sync()
            got = {k: pb.download_named(k) for k in ("opened", "b_p", "b_2")}
            pb._rc(pb.eng.L.hbmpc_pipe_capture(pb.h), "capture")  # (the Python wrapper's capture() insists on a caller's stream)
            pb.replay()
            pb.sync()
        finally:
            pb.close()
        return got

    exp = as_bytes(m)
    for st in (stream.cuda_stream, 0):
        first = cycle(st)  # first use: tables, scratch and runtime-internal allocations happen once
        for k, v in first.items():
            assert np.array_equal(v.view(np.uint8).reshape(-1), exp[k]), (st, k)
        torch.cuda.synchronize()
        free0, _ = torch.cuda.mem_get_info()
        for _ in range(20):
            cycle(st)
        torch.cuda.synchronize()
        free1, _ = torch.cuda.mem_get_info()
        assert free0 - free1 < (8 << 20), (st, free0, free1)
    pi_free = []
    for _ in range(2):  # the PRandInt handle the same way
        torch.cuda.synchronize()
        pi_free.append(torch.cuda.mem_get_info()[0])
        for _ in range(20):
            pi = pkg.pipelines.PRandIntPipe(fr, n, t, B, lk, stream=stream.cuda_stream)
            pi.upload_named("contrib", contrib)
            pi.run(check=False)
            pi.sync()
            pi.close()
    assert pi_free[0] - pi_free[1] < (8 << 20), pi_free


def test_c99_caller_through_the_handles():
    """tests/cpp/test_prandbit_handle.c, built by its own .mk"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.check_call(["make", "-C", os.path.join(root, "tests", "cpp"), "-f", "prandbit_handle.mk"], stdout=subprocess.DEVNULL)
    p = subprocess.run([os.path.join(root, "tests", "cpp", "test_prandbit_handle")], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "PRandBit handle calls passed" in p.stdout, p.stdout[-2000:] + p.stderr[-2000:]


def test_cpp_wrappers_of_the_handles():
    """tests/cpp/test_prandbit_pipe.cpp: PRandBitPipe / PRandIntPipe of include/hbmpc_pipelines.hpp, built by the same .mk"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.check_call(["make", "-C", os.path.join(root, "tests", "cpp"), "-f", "prandbit_handle.mk"], stdout=subprocess.DEVNULL)
    p = subprocess.run([os.path.join(root, "tests", "cpp", "test_prandbit_pipe")], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "PRandBit pipeline wrappers passed" in p.stdout, p.stdout[-2000:] + p.stderr[-2000:]
