"""Input and Output for all parties on one GPU (hbmpc_[gl_]dev_input_parties, hbmpc_[gl_]dev_output_parties, hbmpc_pipe_input_create,
hbmpc_pipe_output_create): the one-launch form of Input (a wave per element, csrc/kernels_input_wave.hpp) and the two-launch form
(the P(0) decode of the masks, k_input_finish) against the big-integer model of tests/clientio_ref.py -- never against the library
itself -- and against each other, byte for byte.  The rule that matters most: an element whose mask does not open is REFUSED --
zeros in mask, masked and every share, never x + 0."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from __graft_entry__ import ROOT, load_package
from tests import clientio_ref as R
from tests import edge_inputs as X
from tests import randbit_ref as RB
from tests import sender_sets as SS

pytestmark = pytest.mark.gpu
FORMS = (("one", None), ("multi", 0))          # hbmpc_set_fused_input: the default threshold / never one launch
FIELD_OF = {"fr": X.FR, "goldilocks": X.GL}
OK_SUMMARY = [0, 0xffffffff, 0]                # n_failed, first_failed, first_error


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


_cases = {}


def random_case(field, n, t, N, seed):
    """x (never zero) and a degree-t sharing of N uniform masks, as ints; computed once per shape and never modified"""
    key = (field, n, t, N, seed)
    if key not in _cases:
        x = [v or 1 for v in R.to_ints(RB.fill_random(field, seed, N), field)]
        r_sh = R.rows_to_ints(RB.share_all(field, RB.fill_random(field, seed + 1, N), n, t, seed + 2), field)
        _cases[key] = (x, r_sh)
    return _cases[key]


def set_form(pkg, eng, fused):
    eng.set_fused_input(pkg.hbmpc.FUSED_INPUT_DEFAULT if fused is None else fused)


def collect(eng, ip, stream=0):
    got = {nm: ip.download(nm).copy() for nm in ("mask", "masked", "out")}
    for nm, arr in (("status", np.zeros(ip.N, dtype=np.uint8)), ("summary", np.zeros(4, dtype=np.uint32))):
        eng.d2h(arr, ip.buffer(nm)[0], stream)
        got[nm] = arr
    eng.sync(stream)
    return got


def raw_input(eng, ip, ids, n, t, N, **kw):
    b = {nm: ip.buffer(nm)[0] for nm in ("x", "r", "mask", "masked", "out", "status", "summary")}
    b.update(kw)
    return eng.input_parties(list(ids), b["x"], b["r"], N, n, t, b["mask"], b["masked"], b["out"], b["status"], b["summary"])


def scribble(eng, ip, F, stream=0):
    """every output buffer holds a marker before the call: what the call leaves there is what it wrote"""
    n, N = ip.n, ip.N
    junk = F.arr([[(7 * p + g + 3) % F.mod for g in range(N)] for p in range(n)])
    ip.upload_named("out", junk)
    ip.upload_named("mask", junk[0])
    ip.upload_named("masked", junk[0])
    eng.h2d(ip.buffer("status")[0], np.full(N, 0x5A, dtype=np.uint8), stream)
    eng.h2d(ip.buffer("summary")[0], np.full(4, 0x5A5A5A5A, dtype=np.uint32), stream)


def run_both(pkg, eng, field, n, t, x, r_sh, ids):
    """the same inputs through both forms by the raw call (any sender set); returns {form: buffers}.  The default is put back."""
    F = FIELD_OF[field]
    N = len(x)
    ip = pkg.pipelines.Input(eng, n, t, N)
    res = {}
    try:
        ip.upload(F.arr(x), F.arr(r_sh))
        for form, fused in FORMS:
            set_form(pkg, eng, fused)
            scribble(eng, ip, F)
            assert raw_input(eng, ip, ids, n, t, N) == 0, eng.last_error()
            res[form] = collect(eng, ip)
    finally:
        eng.set_fused_input(pkg.hbmpc.FUSED_INPUT_DEFAULT)
        ip.close()
    return res


def assert_equals_model(F, got, want, tag):
    assert F.ints(got["mask"]) == want["mask"], (tag, "mask")
    assert F.ints(got["masked"]) == want["masked"], (tag, "masked")
    assert F.ints(got["out"]) == want["in_sh"], (tag, "in_sh")
    assert got["status"].tolist() == want["status"], (tag, "status")
    sm = got["summary"].tolist()
    assert sm[1] == want["summary"][0] and (sm[1] == 0 or sm[2:] == want["summary"][1:]), (tag, "summary")   # first_failed: valid when n_failed > 0


def assert_same_bytes(res, tag):
    for nm in res["multi"]:
        assert np.array_equal(res["one"][nm], res["multi"][nm]), (tag, nm)


def sender_sets_of(n, t):
    sets = [tuple(range(2 * t + 1))]
    if (n, t) in SS.SETS:
        sets.append(SS.sender_set(n, t))
    return sets


# (4, 1): two lanes to a table row; (5, 1): n > 3t + 1; (7, 2): a non-prefix sender set; (16, 5): four lanes to a row; (31, 10): two,
# another non-prefix set; (64, 21): every lane is a party.  N = 1: a lone wave; 3: idle waves; 4: a full workgroup; 5, 9: a second
# and a third workgroup with idle waves
@pytest.mark.parametrize("N", [1, 3, 4, 5, 9])
@pytest.mark.parametrize("n,t", [(4, 1), (5, 1), (7, 2), (16, 5), (31, 10), (64, 21)])
def test_forms_agree_and_agree_with_the_model(pkg_eng, n, t, N):
    pkg, eng = pkg_eng
    x, r_sh = random_case("fr", n, t, N, 1000 * n + N)
    for ids in sender_sets_of(n, t):
        want = R.input_model("fr", ids, x, r_sh, n, t)
        assert want["rc"] == 0 and want["summary"] == OK_SUMMARY
        res = run_both(pkg, eng, "fr", n, t, x, r_sh, ids)
        for form, got in res.items():
            assert_equals_model(X.FR, got, want, (form, ids))
            assert got["summary"].tolist() == [0] + OK_SUMMARY, form
        assert_same_bytes(res, (n, t, N, ids))
        out = R.output_model("fr", tuple(range(n)), X.FR.ints(res["one"]["out"]), n, t)
        assert out["rc"] == 0 and out["out"] == x                               # the shares open to the client's values


def edge_columns(F, n, t, ids):
    """columns (x, r_sh[n]) built from the edge values: for every edge value i a general column (x, mask, one party's r all edge
    values) and the four special ones -- x + mask wraps to 0, x + mask = r_p - 1 (share r - 1), mask = 0 (must open with status 0),
    masked == r_p (share 0).  The party whose r is forced rotates through the senders and a non-sender."""
    q = F.mod
    pool = list(dict.fromkeys(X.forced_parties(n, t, ids) + sorted(ids)))       # verify-row senders, a non-sender, P(0)-row senders
    cols, seen = [], {"x": set(), "mask": set(), "r": set()}

    def column(x, mask, rp, j):
        p = pool[j % len(pool)]
        forced = {-1: mask, p: rp}                                              # P(0) and t parties: a degree-t sharing
        for k, o in enumerate([o for o in pool if o != p][:t - 1]):
            forced[o] = X.pick(F, j + 3 * k + 1)
        sh = X.forced_sharing(F, n, t, forced)
        assert sh[p] == rp % q
        cols.append((x % q, sh, p))
        seen["x"].add(x % q), seen["mask"].add(mask % q), seen["r"].add(rp % q)

    for i in range(len(F.edge)):
        x, mask, rp = X.pick(F, i), X.pick(F, i + 4), X.pick(F, i + 7)
        column(x, mask, rp, i)                                                  # every edge value in each of the three places
        column(q - mask, mask, rp, i + 1)                                       # x + mask wraps to 0 (mask = 0: 0 + 0)
        column(rp - 1 - mask, mask, rp, i + 2)                                  # masked = r_p - 1: the share is r - 1
        column(x, 0, rp, i + 3)                                                 # mask = 0, opened: not a failure
        column(rp - mask, mask, rp, i + 4)                                      # masked == r_p: the share is 0
    for nm in seen:
        assert seen[nm] >= set(F.edge), nm
    return cols


@pytest.mark.parametrize("field,n,t", [("fr", 4, 1), ("fr", 16, 5), ("fr", 7, 2), ("goldilocks", 4, 1)])
def test_edge_values(pkg_eng, pkg_gl, field, n, t):
    pkg, eng = pkg_gl if field == "goldilocks" else pkg_eng
    F = FIELD_OF[field]
    ids = sender_sets_of(n, t)[-1]
    cols = edge_columns(F, n, t, ids)
    x = [c[0] for c in cols]
    r_sh = [[c[1][p] for c in cols] for p in range(n)]
    want = R.input_model(field, ids, x, r_sh, n, t)
    assert want["rc"] == 0 and want["status"] == [0] * len(cols)
    zero_masks = [g for g, m in enumerate(want["mask"]) if m == 0]
    assert len(zero_masks) >= len(F.edge)
    assert any(want["masked"][g] == 0 and x[g] != 0 for g in range(len(cols)))               # a wrap to zero of two nonzero values
    assert any(want["in_sh"][c[2]][g] == F.mod - 1 for g, c in enumerate(cols))
    assert any(want["in_sh"][c[2]][g] == 0 and want["masked"][g] != 0 for g, c in enumerate(cols))
    res = run_both(pkg, eng, field, n, t, x, r_sh, ids)
    for form, got in res.items():
        assert_equals_model(F, got, want, form)
        assert not got["status"][zero_masks].any(), form                       # mask = 0 with status 0 is an opened element
        for g in zero_masks:
            assert F.ints(got["masked"])[g] == x[g], (form, g)                 # ... so masked = x + 0 IS written there
    assert_same_bytes(res, (field, n, t))


def lie_case(field, n, t, ids_small, bit_index):
    """N = 6 elements; at element g one sender's share of the mask carries TAMPER_BITS[bit_index] set (Fr) or is off by one
    (Goldilocks).  The liar alternates between a sender behind the P(0) row and one behind a verify row."""
    F = FIELD_OF[field]
    N, g = 6, 1 + bit_index % 4
    x, r_sh = random_case(field, n, t, N, 4242 + n)
    low, ver = X.split_senders(ids_small, t)
    liar = low[1] if bit_index % 2 == 0 else ver[0]
    honest = [list(row) for row in r_sh]
    if field == "fr":
        base, bad = X.tamper_value(X.TAMPER_BITS[bit_index])
        forced = {p: X.pick(F, bit_index + 2 * k) for k, p in enumerate(X._other_forced(n, t, ids_small, liar))}
        forced[liar] = base
        col = X.forced_sharing(F, n, t, forced)
        for p in range(n):
            honest[p][g] = col[p]
        assert base ^ bad == 1 << X.TAMPER_BITS[bit_index]
    else:
        bad = (honest[liar][g] + 1) % F.mod
    lied = [list(row) for row in honest]
    lied[liar][g] = bad
    return x, honest, lied, g, liar


@pytest.mark.parametrize("n,t,small,big", [(4, 1, (0, 1, 2), (0, 1, 2, 3)), (7, 2, SS.SETS[(7, 2)][5], SS.SETS[(7, 2)][6])])
def test_failure_rule(pkg_eng, n, t, small, big):
    """one lying sender in one element.  At S = 2t + 1 there is no OEC round: that element is refused -- mask, masked and all n shares
    zero, status DecodingError, one failure in the summary -- and every other element is untouched.  At S = 2t + 2 the lie is
    corrected (status 1).  A lie by a party outside the sender set changes nothing."""
    pkg, eng = pkg_eng
    F = X.FR
    for bi in range(len(X.TAMPER_BITS)):
        x, honest, lied, g, liar = lie_case("fr", n, t, small, bi)
        clean = R.input_model("fr", small, x, honest, n, t)
        want = R.input_model("fr", small, x, lied, n, t)
        assert clean["rc"] == 0 and want["rc"] == 8 and want["status"] == [8 if h == g else 0 for h in range(len(x))]
        res = run_both(pkg, eng, "fr", n, t, x, lied, small)
        for form, got in res.items():
            assert_equals_model(F, got, want, (form, bi))
            assert got["status"][g] == 8 and got["summary"].tolist()[1:] == [1, g, 8], form
            assert not got["mask"][g].any() and not got["masked"][g].any() and not got["out"][:, g].any(), form
            assert x[g] != 0 and F.ints(got["masked"])[g] != x[g], form          # never x + 0: the client's value in the clear
            for h in range(len(x)):
                if h != g:
                    assert F.ints(got["masked"])[h] == clean["masked"][h] and F.ints(got["out"][:, h]) == [clean["in_sh"][p][h] for p in range(n)], form
        assert_same_bytes(res, ("2t+1", bi))
        if bi not in (0, 5):                                                     # the other sender counts: a P(0)-row liar and a verify-row liar
            continue
        want = R.input_model("fr", big, x, lied, n, t)
        assert want["rc"] == 0 and want["status"] == [1 if h == g else 0 for h in range(len(x))] and want["masked"] == clean["masked"]
        res = run_both(pkg, eng, "fr", n, t, x, lied, big)
        for form, got in res.items():
            assert_equals_model(F, got, want, (form, bi, "2t+2"))
            assert got["status"][g] == 1 and got["summary"].tolist()[1] == 0, form
        assert_same_bytes(res, ("2t+2", bi))
        outsider = SS.outsiders(n, small)[0]
        out_lie = [list(row) for row in honest]
        out_lie[outsider][g] = (out_lie[outsider][g] + 1) % F.mod
        want = R.input_model("fr", small, x, out_lie, n, t)
        assert want["rc"] == 0 and want["masked"] == clean["masked"] and want["mask"] == clean["mask"]
        res = run_both(pkg, eng, "fr", n, t, x, out_lie, small)
        for form, got in res.items():
            assert_equals_model(F, got, want, (form, bi, "outsider"))
        assert_same_bytes(res, ("outsider", bi))


@pytest.mark.parametrize("N", [1, 5])
@pytest.mark.parametrize("n,t", [(4, 1), (16, 5)])
def test_goldilocks(pkg_gl, n, t, N):
    """the two hbmpc_gl_* launches under both threshold settings against the model: honest, a refused element, a corrected one"""
    pkg, eng = pkg_gl
    F = X.GL
    x, r_sh = random_case("goldilocks", n, t, N, 77 * n + N)
    small, big = tuple(range(2 * t + 1)), tuple(range(2 * t + 2))
    lied = [list(row) for row in r_sh]
    lied[1][N - 1] = (lied[1][N - 1] + 1) % F.mod
    for ids, shares, rc in ((small, r_sh, 0), (small, lied, 8), (big, lied, 0)):
        want = R.input_model("goldilocks", ids, x, shares, n, t)
        assert want["rc"] == rc
        res = run_both(pkg, eng, "goldilocks", n, t, x, shares, ids)
        for form, got in res.items():
            assert_equals_model(F, got, want, (form, len(ids), rc))
        assert_same_bytes(res, (n, t, N, len(ids), rc))
        if rc == 8:
            got = res["one"]
            assert got["masked"][N - 1] == 0 and not got["out"][:, N - 1].any() and F.ints(got["masked"])[N - 1] != x[N - 1]


@pytest.mark.parametrize("N", [1, 5])
@pytest.mark.parametrize("n,t", [(4, 1), (16, 5)])
def test_output(pkg_eng, n, t, N):
    """honest, the liar refused at 2t + 1, the liar corrected at 2t + 2 -- against the model, and the bytes hbmpc_dev_batch_recover_p0
    leaves for the same senders' rows laid out one after the other"""
    pkg, eng = pkg_eng
    F = X.FR
    _, sh = random_case("fr", n, t, N, 31 * n + N)
    lied = [list(row) for row in sh]
    lied[1][N - 1] = (lied[1][N - 1] + 1) % F.mod
    small, big = tuple(range(2 * t, -1, -1)), tuple(range(2 * t + 2))                        # the small set in descending order
    op = pkg.pipelines.Output(eng, n, t, N)
    rows_d = eng.dev_alloc((2 * t + 2) * N * 32)
    ref = {nm: eng.dev_alloc(sz) for nm, sz in (("out", N * 32), ("status", N), ("summary", 64))}
    try:
        for ids, shares, rc in ((small, sh, 0), (small, lied, 8), (big, lied, 0)):
            want = R.output_model("fr", ids, shares, n, t)
            assert want["rc"] == rc
            arr = F.arr(shares)
            op.upload(arr)
            op.upload_named("out", F.arr([5] * N))
            assert eng.output_parties(list(ids), op.sh, N, n, t, op.out, op.buffer("status")[0], op.buffer("summary")[0]) == 0, eng.last_error()
            eng.h2d(rows_d, np.ascontiguousarray(arr[list(ids)]))
            assert eng.dev_batch_recover(list(ids), rows_d, N, n, t, t, ref["out"], status_d=ref["status"], summary_d=ref["summary"], p0=True) == 0
            got, same = {}, {}
            for nm, proto in (("out", F.arr([0] * N)), ("status", np.zeros(N, dtype=np.uint8)), ("summary", np.zeros(4, dtype=np.uint32))):
                got[nm], same[nm] = proto.copy(), proto.copy()
                eng.d2h(got[nm], op.buffer(nm)[0])
                eng.d2h(same[nm], ref[nm])
            eng.sync()
            assert F.ints(got["out"]) == want["out"] and got["status"].tolist() == want["status"] and got["summary"][1] == want["summary"][0]
            for nm in got:
                assert np.array_equal(got[nm], same[nm]), (nm, len(ids), rc)
        assert eng.output_parties(list(small), op.sh, N, n, t, op.out) == 0        # status and summary are optional here
        assert eng.output_parties(list(small), 0, N, n, t, op.out) == 4 and eng.output_parties(list(small[:-1]), op.sh, N, n, t, op.out) == 4
        eng.sync()
    finally:
        op.close()
        eng.dev_free(rows_d)
        for p in ref.values():
            eng.dev_free(p)


def test_refused_calls_write_nothing(pkg_eng, pkg_gl):
    """too few senders, a repeated id, an id >= n, a null buffer (status among them), N or n out of range: refused, and every output
    buffer keeps its marker in both threshold settings; the other field's context is TypeMismatch"""
    pkg, eng = pkg_eng
    n, t, N = 7, 2, 5
    x, r_sh = random_case("fr", n, t, N, 99)
    ip = pkg.pipelines.Input(eng, n, t, N)
    try:
        ip.upload(X.FR.arr(x), X.FR.arr(r_sh))
        scribble(eng, ip, X.FR)
        eng.sync()
        before = collect(eng, ip)
        for _, fused in FORMS:
            set_form(pkg, eng, fused)
            for ids in (tuple(range(2 * t)), (0, 1, 2, 3, 3), (0, 1, 2, 3, n)):
                assert raw_input(eng, ip, ids, n, t, N) == 4, ids
            for nm in ("x", "r", "mask", "masked", "out", "status"):
                assert raw_input(eng, ip, range(2 * t + 1), n, t, N, **{nm: 0}) == 4, nm
            assert raw_input(eng, ip, range(2 * t + 1), n, t, 0) == 4 and raw_input(eng, ip, range(2 * t + 1), 0, t, N) == 4
            assert raw_input(eng, ip, range(2 * t + 1), 256, t, N) == 4
        after = collect(eng, ip)
        for nm in before:
            assert np.array_equal(before[nm], after[nm]), nm
        assert raw_input(eng, ip, range(2 * t + 1), n, t, N, summary=0) == 0      # the summary is optional
        eng.sync()
        for bad in (2 * t, n + 1):
            for cls in (pkg.pipelines.Input, pkg.pipelines.Output):
                with pytest.raises(RuntimeError, match="ShareErrorCode 4"):
                    cls(eng, n, t, N, open_senders=bad)
        _, gl = pkg_gl
        ids = (C.c_size_t * (2 * t + 1))(*range(2 * t + 1))
        z = C.c_size_t
        ptr = {nm: C.c_void_p(ip.buffer(nm)[0]) for nm in ("x", "r", "mask", "masked", "out", "status")}
        inp = [ids, z(2 * t + 1), ptr["x"], ptr["r"], z(N), z(n), z(t), ptr["mask"], ptr["masked"], ptr["out"], ptr["status"], None, None]
        out = [ids, z(2 * t + 1), ptr["r"], z(N), z(n), z(t), ptr["mask"], ptr["status"], None, None]
        assert eng.L.hbmpc_dev_input_parties(gl.ctx, *inp) == 5 and eng.L.hbmpc_gl_dev_input_parties(eng.ctx, *inp) == 5
        assert eng.L.hbmpc_dev_output_parties(gl.ctx, *out) == 5 and eng.L.hbmpc_gl_dev_output_parties(eng.ctx, *out) == 5
    finally:
        eng.set_fused_input(pkg.hbmpc.FUSED_INPUT_DEFAULT)
        ip.close()


def test_handles(pkg_eng):
    """the Input handle eager, captured and replayed twice with other inputs uploaded between the replays, in both forms; a checked
    run() raises on a refused element; an unknown buffer name is refused"""
    pkg, eng = pkg_eng
    F = X.FR
    n, t, N = 16, 5, 9
    ids = tuple(range(2 * t + 1))
    sets = [random_case("fr", n, t, N, s) for s in (501, 502, 503)]
    wants = [R.input_model("fr", ids, x, r, n, t) for x, r in sets]
    st = eng.stream_create()
    try:
        for form, fused in FORMS:
            set_form(pkg, eng, fused)
            ip = pkg.pipelines.Input(eng, n, t, N, stream=st)
            try:
                ip.upload(F.arr(sets[0][0]), F.arr(sets[0][1]))
                ip.run(check=True)
                assert_equals_model(F, collect(eng, ip, st), wants[0], (form, "eager"))
                ip.capture()
                for k in (1, 2):
                    ip.upload(F.arr(sets[k][0]), F.arr(sets[k][1]))
                    scribble(eng, ip, F, st)
                    ip.replay()
                    assert_equals_model(F, collect(eng, ip, st), wants[k], (form, "replay", k))
                with pytest.raises(AttributeError):
                    ip.nosuchbuffer
                with pytest.raises(RuntimeError, match="ShareErrorCode"):
                    ip.buffer("nosuchbuffer")
            finally:
                ip.close()
            x, honest, lied, g, _ = lie_case("fr", n, t, ids, 3)
            ip = pkg.pipelines.Input(eng, n, t, len(x), stream=st)
            op = pkg.pipelines.Output(eng, n, t, len(x), stream=st)
            try:
                ip.upload(F.arr(x), F.arr(lied))
                with pytest.raises(RuntimeError, match="ShareErrorCode 8"):        # where the reference's `?` returns DecodingError
                    ip.run(check=True)
                ip.run(check=False)
                got = collect(eng, ip, st)
                assert got["status"][g] == 8 and not got["masked"][g].any() and not got["out"][:, g].any()
                op.upload(F.arr(lied))
                with pytest.raises(RuntimeError, match="ShareErrorCode 8"):
                    op.run(check=True)
                op.upload(F.arr(honest))
                op.run(check=True)
                assert F.ints(op.download()) == R.output_model("fr", ids, honest, n, t)["out"]
            finally:
                ip.close()
                op.close()
    finally:
        eng.set_fused_input(pkg.hbmpc.FUSED_INPUT_DEFAULT)
        eng.sync(st)
        eng.stream_destroy(st)


def test_client_to_client(pkg_eng):
    """config C1's shape from client values to client values through library handles only: n = 4, t = 1, N = 5; two Input handles
    (x and y), their `out` buffers into a Mul handle's x and y, its `out` into an Output handle's sh; what comes out is x y mod r"""
    pkg, eng = pkg_eng
    F = X.FR
    n, t, N = 4, 1, 5
    x, rx = random_case("fr", n, t, N, 9001)
    y, ry = random_case("fr", n, t, N, 9002)
    ta, tb = R.to_ints(RB.fill_random("fr", 9003, N), "fr"), R.to_ints(RB.fill_random("fr", 9004, N), "fr")
    tc = [a * b % F.mod for a, b in zip(ta, tb)]
    triple = [RB.share_all("fr", R.from_ints(v, "fr"), n, t, 9010 + j) for j, v in enumerate((ta, tb, tc))]
    pl = pkg.pipelines
    ix, iy, mp, op = pl.Input(eng, n, t, N), pl.Input(eng, n, t, N), pl.Mul(eng, n, t, N), pl.Output(eng, n, t, N)
    try:
        ix.upload(F.arr(x), F.arr(rx))
        iy.upload(F.arr(y), F.arr(ry))
        for nm, arr in zip(("ta", "tb", "tc"), triple):
            mp.upload_named(nm, arr)
        ix.run(check=True)
        iy.run(check=True)
        eng.d2d(mp.x, ix.out, n * N * 32)
        eng.d2d(mp.y, iy.out, n * N * 32)
        mp.run(check=True)
        eng.d2d(op.sh, mp.out, n * N * 32)
        op.run(check=True)
        assert F.ints(op.download()) == [a * b % F.mod for a, b in zip(x, y)]
    finally:
        for h in (ix, iy, mp, op):
            h.close()


def test_cpp_wrapper():
    """tests/cpp/test_input_pipeline (include/hbmpc_pipelines.hpp's Input and Output at n = 4, t = 1, N = 5: a round trip) in a child process"""
    exe = os.path.join(ROOT, "tests", "cpp", "test_input_pipeline")
    assert os.path.exists(exe), "built by make -C tests/cpp -f input.mk (build())"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
