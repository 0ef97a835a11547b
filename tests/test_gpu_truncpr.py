"""TruncPr and FPDivConst for all parties on one GPU (hbmpc_dev_truncpr_parties, hbmpc_pipe_truncpr_create): the one-launch form
(a wave per element, csrc/kernels_truncpr_wave.hpp) and the three-launch form (k_truncpr_front, the P(0) decode, the last step)
against the oracle's element-wise restatements and Python big ints -- never against the library itself -- and against each
other, byte for byte."""
import numpy as np
import pytest

from __graft_entry__ import load_package
from oracle import cref as O
from oracle import spec as S
from tests import golden_util as GU
from tests import sender_sets as SS

pytestmark = pytest.mark.gpu
R = S.R_MOD
FORMS = (("one", 1 << 20), ("three", 0))     # hbmpc_set_fused_truncpr: always (where the call qualifies) / never


@pytest.fixture(scope="module")
def pkg_eng():
    pkg = load_package()
    e = pkg.Engine(0)
    yield pkg, e
    e.close()


def share_all(secrets_u256, n, d, seed):
    """[n][N] degree-d sharings of N secrets (random higher coefficients), via the oracle"""
    N = secrets_u256.shape[0]
    co = O.fill_random(seed, N * (d + 1)).reshape(N, d + 1, 4)
    co[:, 0] = secrets_u256
    rc, sh = O.compute_shares(co, n, d)
    assert rc == 0
    return sh


def open_all(shares, n, t):
    rc, p0, st = O.batch_recover_p0(list(range(n)), shares, n, t, t)
    assert rc == 0 and not st.any()
    return p0


def random_inputs(n, t, N, m, seed, with_w):
    """a, r_int and the m bit arrays as sharings of uniform field elements (the steps are algebra, not range-limited), w uniform"""
    ins = {"a": share_all(O.fill_random(seed, N), n, t, seed + 1), "rint": share_all(O.fill_random(seed + 2, N), n, t, seed + 3)}
    ins["rbits"] = (np.stack([share_all(O.fill_random(seed + 10 + j, N), n, t, seed + 50 + j) for j in range(m)], axis=1) if m
                    else np.zeros((n, 0, N, 4), dtype=np.uint64))
    ins["w"] = O.fill_random(seed + 4, N) if with_w else None
    return ins


def expected(ins, n, t, N, k, m, senders):
    """the composition of oracle calls and big ints that the call replaces: c, r', open_sh per party, the open, the output.
    senders: a count (the open is from parties 0 .. senders - 1) or the list of the parties whose shares are opened, in arrival order"""
    ids = list(range(senders)) if isinstance(senders, (int, np.integer)) else list(senders)
    a, w = ins["a"], ins["w"]
    v = np.stack([O.fr_binop("mul", a[p], w) for p in range(n)]) if w is not None else a
    rd = np.stack([O.truncpr_rdash(np.ascontiguousarray(ins["rbits"][p]), m)[1] for p in range(n)])
    vi, ri, rdi = O.u256_to_ints(v), O.u256_to_ints(ins["rint"]), O.u256_to_ints(rd)
    osh = O.ints_to_u256([[(vi[p][i] + (1 << (k - 1)) + (ri[p][i] << m) + rdi[p][i]) % R for i in range(N)] for p in range(n)])  # truncpr.rs:275-297
    rc, cop, st = O.batch_recover_p0(ids, np.ascontiguousarray(osh[ids]), n, t, t)   # a failed chunk: zero, status = its error
    out = np.stack([O.truncpr_finalize(v[p], rd[p], cop, m)[1] for p in range(n)])
    return {"c": v, "rdash": rd, "osh": osh, "cop": cop, "out": out, "status": st, "rc": rc}


def make_pipe(pkg, eng, n, t, N, k, m, ins, stream=0, open_senders=None):
    """TruncPr, or with a multiplier FpDivConst (which runs TruncPr with 2 k_fixed bits and m = f); w is uploaded as it is"""
    if ins["w"] is None:
        tp = pkg.pipelines.TruncPr(eng, n, t, N, k, m, stream=stream, open_senders=open_senders)
    else:
        assert k % 2 == 0
        tp = pkg.pipelines.FpDivConst(eng, n, t, N, k // 2, m, stream=stream, open_senders=open_senders)
        assert (tp.k, tp.m) == (k, m)
        tp.upload_named("w", ins["w"])
    tp.upload(ins["a"], np.ascontiguousarray(ins["rbits"]), ins["rint"])
    return tp


def collect(eng, tp, with_w, stream=0):
    n, N = tp.n, tp.N
    got = {nm: tp.download(nm).copy() for nm in (("c",) if with_w else ()) + ("rdash", "osh", "cop", "out")}
    for nm, arr in (("status", np.zeros(N, dtype=np.uint8)), ("summary", np.zeros(4, dtype=np.uint32))):
        eng.d2h(arr, tp.buffer(nm)[0], stream)
        got[nm] = arr
    eng.sync(stream)
    return got


def run_forms(pkg, eng, n, t, N, k, m, ins, open_senders=None, stream=0, check=False, graph=False, forms=FORMS):
    """the same inputs through both forms; returns {form: buffers}.  The default threshold is put back."""
    H = pkg.hbmpc
    res = {}
    try:
        for form, fused in forms:
            eng.set_fused_truncpr(fused)
            tp = make_pipe(pkg, eng, n, t, N, k, m, ins, stream=stream, open_senders=open_senders)
            try:
                if check:
                    with pytest.raises(RuntimeError, match="ShareErrorCode 8"):   # the decode's error: DecodingError
                        tp.run(check=True)
                tp.run(check=False)
                res[form] = collect(eng, tp, ins["w"] is not None, stream)
                if graph:
                    tp.capture()
                    eng.h2d(tp.out, np.zeros((n, N, 4), dtype=np.uint64), stream)
                    tp.replay()
                    assert GU.eq(tp.download("out"), res[form]["out"]), form
            finally:
                tp.close()
    finally:
        eng.set_fused_truncpr(H.FUSED_TRUNCPR_DEFAULT)
    return res


def assert_equals_oracle(got, want, with_w, tag):
    for nm in (("c",) if with_w else ()) + ("rdash", "osh", "cop", "out", "status"):
        assert np.array_equal(got[nm], want[nm]), (tag, nm)


def assert_same_bytes(res, tag):
    for nm in res["three"]:
        assert np.array_equal(res["one"][nm], res["three"][nm]), (tag, nm)


# the issue's shapes, and (4, 1, 3, ..) so that the last workgroup of the wave-per-element kernel has 1, 3 and 1 (N = 1, 3, 5) live waves
SHAPES = [(4, 1, 5, 32, 4), (4, 1, 1, 32, 4), (4, 1, 3, 32, 4), (7, 2, 67, 32, 8), (16, 5, 200, 32, 16), (10, 3, 33, 16, 0), (31, 10, 18, 48, 24),
          (7, 2, 30, 32, 13)]


@pytest.mark.parametrize("with_w", [False, True], ids=["truncpr", "fpdivconst"])
@pytest.mark.parametrize("n,t,N,k,m", SHAPES)
def test_exact_identity_both_forms(pkg_eng, n, t, N, k, m, with_w):
    """every buffer of both forms equals the oracle / big-int composition: c = a w, r', open_sh per party, cop its open,
    out[p] = truncpr_finalize(v[p], r'[p], cop, m); status and summary say nothing failed"""
    pkg, eng = pkg_eng
    ins = random_inputs(n, t, N, m, 1000 * n + N, with_w)
    want = expected(ins, n, t, N, k, m, 2 * t + 1)
    assert want["rc"] == 0
    res = run_forms(pkg, eng, n, t, N, k, m, ins)
    for form, got in res.items():
        assert_equals_oracle(got, want, with_w, form)
        assert not got["status"].any() and got["summary"].tolist() == [0, 0, 0xffffffff, 0], form
    assert_same_bytes(res, (n, t, N, k, m, with_w))


def test_meaning_division_by_public_constants(pkg_eng):
    """FPDivConst with k = 16, f = 8 (TruncPr runs with 2k = 32, m = 8): x in (-2^15, 2^15), denominators 1 .. N as i << f.  The opened
    value x w + 2^31 + 2^8 r'' + r' is nonnegative and below r, so d = floor(c / 2^m) + u with u in {0, 1}: the output opens to
    floor(x w / 2^f) or that plus one (mathematical floor for negative x), mod r."""
    pkg, eng = pkg_eng
    H = pkg.hbmpc
    n, t, N, k, f = 7, 2, 40, 16, 8
    rng = np.random.default_rng(0xD17)
    xs = [int(v) for v in rng.integers(-(1 << 15) + 1, 1 << 15, N)]
    xs[0], xs[1], xs[2] = -(1 << 15) + 1, (1 << 15) - 1, 0
    den = [i << f for i in range(1, N + 1)]
    rints = [int(v) for v in rng.integers(0, 1 << 40, N)]
    bits = rng.integers(0, 2, (f, N))
    ws = [((1 << (2 * f)) + (b >> 1)) // b for b in den]                         # fpdiv/mod.rs:44
    rdash = [sum(int(bits[j][i]) << j for j in range(f)) for i in range(N)]
    for i in range(N):                                                              # the bounds behind the statement
        assert -(1 << 15) < xs[i] < (1 << 15) and 0 < ws[i] <= 1 << f and rints[i] < 1 << 40 and rdash[i] < 1 << f
        assert 0 <= xs[i] * ws[i] + (1 << (2 * k - 1)) + (rints[i] << f) + rdash[i] < R
    sa = share_all(O.ints_to_u256([x % R for x in xs]), n, t, 61)                  # negatives as r - |x|
    srint = share_all(O.ints_to_u256(rints), n, t, 62)
    sbits = np.stack([share_all(O.ints_to_u256([int(v) for v in bits[j]]), n, t, 70 + j) for j in range(f)], axis=1)
    try:
        for form, fused in FORMS:
            eng.set_fused_truncpr(fused)
            fd = pkg.pipelines.FpDivConst(eng, n, t, N, k, f)
            try:
                w = fd.set_denominators(O.ints_to_u256(den))
                assert O.u256_to_ints(w) == ws
                fd.upload(sa, np.ascontiguousarray(sbits), srint)
                fd.run()
                got = O.u256_to_ints(open_all(fd.download("out"), n, t))
                assert O.u256_to_ints(open_all(fd.download("c"), n, t)) == [(x * w_) % R for x, w_ in zip(xs, ws)]
            finally:
                fd.close()
            for i in range(N):
                fl = (xs[i] * ws[i]) >> f                                           # Python's >> is the mathematical floor
                assert got[i] in (fl % R, (fl + 1) % R), (form, i, xs[i], den[i])
    finally:
        eng.set_fused_truncpr(H.FUSED_TRUNCPR_DEFAULT)


@pytest.mark.parametrize("with_w", [False, True], ids=["truncpr", "fpdivconst"])
def test_failure_path(pkg_eng, with_w):
    """one party among the first 2t + 1 holds a wrong share of a at two elements.  Opened from 2t + 1 senders there is no OEC round:
    both forms count exactly those elements as failed, open them to zero, run the last step on that zero and leave the same bytes;
    a checked run raises with the decode's error.  Opened from all n senders (three launches) they are corrected."""
    pkg, eng = pkg_eng
    n, t, N, k, m = 7, 2, 37, 32, 8
    ins = random_inputs(n, t, N, m, 4242, with_w)
    honest = expected(ins, n, t, N, k, m, 2 * t + 1)
    bad_el = (6, 36)                                                                # 36: the last element, alone in its workgroup
    for i in bad_el:
        ins["a"][3, i] = ins["a"][4, i]
    want = expected(ins, n, t, N, k, m, 2 * t + 1)                                  # the oracle's decode fails the same chunks, to zero
    assert want["rc"] == 8 and [i for i in range(N) if want["status"][i]] == list(bad_el) and not want["cop"][list(bad_el)].any()
    res = run_forms(pkg, eng, n, t, N, k, m, ins, check=True)
    for form, got in res.items():
        assert got["summary"].tolist() == [2, 2, bad_el[0], 8], form
        assert_equals_oracle(got, want, with_w, form)                               # status 8 at exactly those; the last step ran on zero
    assert_same_bytes(res, "2t+1 senders")
    want = expected(ins, n, t, N, k, m, n)                                          # OEC rounds available: never the one-launch form
    assert want["rc"] == 0 and GU.eq(want["cop"], honest["cop"])
    res = run_forms(pkg, eng, n, t, N, k, m, ins, open_senders=n)
    for form, got in res.items():
        assert got["summary"].tolist()[:2] == [2, 0], form                          # n_fallback, n_failed
        assert_equals_oracle(got, want, with_w, form)
    assert_same_bytes(res, "n senders")


@pytest.mark.parametrize("with_w", [False, True], ids=["truncpr", "fpdivconst"])
def test_pipeline_as_hip_graph(pkg_eng, with_w):
    """on a non-default stream: capture, zero `out`, replay -- the eager run's bytes, for both forms"""
    pkg, eng = pkg_eng
    n, t, N, k, m = 7, 2, 50, 32, 8
    ins = random_inputs(n, t, N, m, 777, with_w)
    want = expected(ins, n, t, N, k, m, 2 * t + 1)
    st = eng.stream_create()
    try:
        res = run_forms(pkg, eng, n, t, N, k, m, ins, stream=st, graph=True)
    finally:
        eng.sync(st)
        eng.stream_destroy(st)
    for form, got in res.items():
        assert GU.eq(got["out"], want["out"]), form
    assert_same_bytes(res, "graph")


def test_rejects_bad_calls(pkg_eng):
    """k = 0, m = 4097, m = 257, a multiplier without c_out, null required buffers, too few / duplicate / out-of-range senders:
    InvalidInput (4); a Goldilocks context: TypeMismatch (5).  Each is refused before the first launch: nothing is written."""
    pkg, eng = pkg_eng
    n, t, N, k, m = 7, 2, 20, 32, 4
    ins = random_inputs(n, t, N, m, 99, True)
    tp = make_pipe(pkg, eng, n, t, N, k, m, ins)
    b = {nm: tp.buffer(nm)[0] for nm in ("a", "w", "rbits", "rint", "c", "rdash", "osh", "cop", "out", "status", "summary")}
    outs = {"c": (n, N), "rdash": (n, N), "osh": (n, N), "out": (n, N), "cop": (N,)}
    marker = {nm: O.fill_random(300 + j, int(np.prod(sh))).reshape(sh + (4,)) for j, (nm, sh) in enumerate(outs.items())}
    for nm in outs:
        tp.upload_named(nm, marker[nm])
    st_marker, sm_marker = np.full(N, 0x5A, dtype=np.uint8), np.full(4, 0x5A5A5A5A, dtype=np.uint32)
    eng.h2d(b["status"], st_marker)
    eng.h2d(b["summary"], sm_marker)
    eng.sync()

    def call(ids=tuple(range(2 * t + 1)), eng_=eng, **kw):
        a = dict(b)
        shape = dict(k=k, m=m, N=N, n=n, t=t)
        for key, val in kw.items():
            (shape if key in shape else a)[key] = val
        return eng_.dev_truncpr_parties(list(ids), a["a"], a["w"], a["rbits"], a["rint"], shape["k"], shape["m"], shape["N"], shape["n"], shape["t"],
                                        a["c"], a["rdash"], a["osh"], a["cop"], a["out"], a["status"], a["summary"])

    try:
        for fused in (1 << 20, 0):
            eng.set_fused_truncpr(fused)
            assert call(k=0) == 4 and call(m=4097) == 4 and call(m=257) == 4
            assert call(c=0) == 4                                                   # w_dev without c_out
            for nm in ("a", "rint", "rbits", "rdash", "osh", "cop", "out"):
                assert call(**{nm: 0}) == 4, nm
            assert call(N=0) == 4 and call(n=0) == 4 and call(n=256) == 4 and call(t=3) == 4
            assert call(ids=range(2 * t)) == 4                                      # S < 2t + 1
            assert call(ids=(0, 1, 2, 3, 3)) == 4 and call(ids=(0, 1, 2, 3, n)) == 4
            gl = pkg.Engine(0, field="goldilocks")
            try:
                assert call(eng_=gl) == 5
            finally:
                gl.close()
        eng.sync()
        for nm, sh in outs.items():
            assert GU.eq(tp.download_named(nm, sh), marker[nm]), nm
        st_now, sm_now = np.zeros(N, dtype=np.uint8), np.zeros(4, dtype=np.uint32)
        eng.d2h(st_now, b["status"])
        eng.d2h(sm_now, b["summary"])
        eng.sync()
        assert np.array_equal(st_now, st_marker) and np.array_equal(sm_now, sm_marker)
        for fused in (1 << 20, 0):                                                  # and the good calls: without a multiplier c_out may be null,
            eng.set_fused_truncpr(fused)                                            # status and summary are optional
            assert call() == 0 and call(w=0, c=0) == 0 and call(status=0, summary=0) == 0
        eng.sync()
    finally:
        eng.set_fused_truncpr(pkg.hbmpc.FUSED_TRUNCPR_DEFAULT)
        tp.close()


def test_sender_rows_follow_the_decode_call(pkg_eng):
    """sender_ids that are not 0 .. S - 1: row s of the [party][N] arrays is read as sender_ids[s]'s share, as
    hbmpc_dev_batch_recover_p0 reads its sender rows -- in both forms.  The shares of parties (2, 0, 1) are laid out in that order."""
    pkg, eng = pkg_eng
    n, t, N, k, m = 4, 1, 9, 32, 4
    ids = (2, 0, 1)
    ins = random_inputs(n, t, N, m, 31337, False)
    perm = list(ids) + [3]
    laid = {nm: (np.ascontiguousarray(v[perm]) if nm != "w" else v) for nm, v in ins.items()}    # row s holds party perm[s]'s shares
    want = expected(ins, n, t, N, k, m, 2 * t + 1)                                  # the honest open: every sender set opens the same value
    tp = make_pipe(pkg, eng, n, t, N, k, m, laid)
    b = {nm: tp.buffer(nm)[0] for nm in ("a", "rbits", "rint", "rdash", "osh", "cop", "out", "status", "summary")}
    got = {}
    try:
        for form, fused in FORMS:
            eng.set_fused_truncpr(fused)
            eng.h2d(b["cop"], np.zeros((N, 4), dtype=np.uint64))
            assert eng.dev_truncpr_parties(list(ids), b["a"], 0, b["rbits"], b["rint"], k, m, N, n, t, 0, b["rdash"], b["osh"], b["cop"], b["out"],
                                           b["status"], b["summary"]) == 0
            got[form] = collect(eng, tp, False)
            assert GU.eq(got[form]["cop"], want["cop"]) and got[form]["summary"].tolist() == [0, 0, 0xffffffff, 0], form
            assert GU.eq(got[form]["out"], want["out"][perm]), form
        assert_same_bytes(got, "permuted senders")
    finally:
        eng.set_fused_truncpr(pkg.hbmpc.FUSED_TRUNCPR_DEFAULT)
        tp.close()


@pytest.mark.parametrize("with_w", [False, True], ids=["truncpr", "fpdivconst"])
@pytest.mark.parametrize("n,t,S", [(7, 2, 5), (7, 2, 6), (16, 5, 11)])
def test_sender_sets(pkg_eng, n, t, S, with_w):
    """the sets of tests/sender_sets.py -- unsorted, with party n - 1 and an id >= S, a low party left out -- so that a kernel with the
    prefix's table, or one that ignores the ids, opens something else at every element (tests/test_sender_sets.py).  Row s of the
    arrays holds the share of sender_ids[s]; the rows behind them hold the parties outside the set, whose shares of a and r_int
    are wrong throughout.  Honest senders, then one lying behind a verify row and one behind the P(0) row: from 2t + 1 senders
    exactly their elements fail in both forms, from 2t + 2 (three launches) they are repaired."""
    pkg, eng = pkg_eng
    N, k, m = 20, 32, 8
    ids = SS.sender_set(n, t, S)
    perm = list(ids) + SS.outsiders(n, ids)
    ins = SS.with_wrong_outsider(random_inputs(n, t, N, m, 9000 + n + S, with_w), n, ids, ("a", "rint"), every=True)
    honest = expected(ins, n, t, N, k, m, ids)
    lied, bad = SS.truncpr_with_liars(ins, ids, t)
    names = (("c",) if with_w else ()) + ("rdash", "osh", "out")
    try:
        for case, case_ins in (("honest", ins), ("liars", lied)):
            want = expected(case_ins, n, t, N, k, m, ids)
            assert np.flatnonzero(want["status"]).tolist() == ([] if case == "honest" else bad)
            if case == "honest" or S > 2 * t + 1:
                assert want["rc"] == 0 and GU.eq(want["cop"], honest["cop"])
                summary = [0 if case == "honest" else 2, 0, 0xffffffff, 0]          # n_fallback, n_failed, first_failed, first_error
            else:
                assert want["rc"] == 8 and not want["cop"][bad].any()
                summary = [2, 2, bad[0], 8]
            laid = {nm: (np.ascontiguousarray(v[perm]) if nm != "w" else v) for nm, v in case_ins.items()}    # row s holds party perm[s]'s shares
            tp = make_pipe(pkg, eng, n, t, N, k, m, laid, open_senders=S)
            b = {nm: tp.buffer(nm)[0] for nm in (("w", "c") if with_w else ()) + ("a", "rbits", "rint", "rdash", "osh", "cop", "out", "status", "summary")}
            got = {}
            try:
                for form, fused in (FORMS if S == 2 * t + 1 else FORMS[1:]):
                    eng.set_fused_truncpr(fused)
                    eng.h2d(b["cop"], np.zeros((N, 4), dtype=np.uint64))
                    eng.h2d(b["out"], np.zeros((n, N, 4), dtype=np.uint64))
                    assert eng.dev_truncpr_parties(list(ids), b["a"], b.get("w", 0), b["rbits"], b["rint"], k, m, N, n, t, b.get("c", 0), b["rdash"],
                                                   b["osh"], b["cop"], b["out"], b["status"], b["summary"]) == 0
                    got[form] = collect(eng, tp, with_w)
                    tag = (case, form, n, t, S)
                    assert GU.eq(got[form]["cop"], want["cop"]) and np.array_equal(got[form]["status"], want["status"]), tag
                    assert got[form]["summary"].tolist() == summary, tag
                    for nm in names:
                        assert GU.eq(got[form][nm], want[nm][perm]), tag + (nm,)
                if len(got) == 2:
                    assert_same_bytes(got, (case, n, t, S))
            finally:
                tp.close()
    finally:
        eng.set_fused_truncpr(pkg.hbmpc.FUSED_TRUNCPR_DEFAULT)


@pytest.mark.parametrize("seed", range(8))
def test_forms_random(pkg_eng, seed):
    """random shapes (t, n = 3t + 1 or 3t + 2, batch < 130, m in 0 .. 24, with or without a multiplier) with zero to two replaced
    shares among the senders: the two forms agree byte for byte in every buffer, status and summary"""
    pkg, eng = pkg_eng
    rng = np.random.default_rng(0x7C0 + seed)
    t = int(rng.integers(1, 6))
    n = 3 * t + 1 + int(rng.integers(0, 2))
    N, m = int(rng.integers(1, 130)), int(rng.integers(0, 25))
    with_w = bool(seed & 1)
    k = int(rng.integers(max(m, 2), 65)) & ~(1 if with_w else 0)                    # FpDivConst runs TruncPr with an even number of bits
    ins = random_inputs(n, t, N, m, 20000 + 100 * seed, with_w)
    tampered = set()
    for _ in range(int(rng.integers(0, 3))):
        nm, p, i = str(rng.choice(["a", "rint", "rbits"])), int(rng.integers(0, 2 * t + 1)), int(rng.integers(0, N))
        if nm == "rbits" and m == 0:
            continue
        ins[nm][p, ..., i, :] = ins[nm][(p + 1) % n, ..., i, :]
        tampered.add(i)
    res = run_forms(pkg, eng, n, t, N, k, m, ins)
    assert_same_bytes(res, (seed, n, t, N, k, m, with_w))
    assert res["three"]["summary"][1] == len(tampered) and {i for i in range(N) if res["three"]["status"][i]} == tampered
