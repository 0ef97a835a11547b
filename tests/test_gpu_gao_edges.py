"""The Byzantine fallback (k_gao in its five launch shapes, with and without INLINE, and k_unscale) on the structured words of
tests/gao_inputs.py: boundary error counts, the zero polynomial under errors, words on a polynomial of higher degree, error values solved
so that the remainder sequence of the EEA is degenerate, `dg < dv`, a second codeword, partial sender sets -- at both edge values of n of
every launch shape.  tests/test_gao_inputs.py proves without a GPU that these words reach every branch of the decode in every launch
shape, and pins the kernels each call below takes.

Every chunk of every call is compared with the C oracle (oracle.cref, oracle.cref_gl; tests/test_gao_inputs.py holds it to the Python
one on these very words), never with another route alone: coefficients zero padded, ncoeffs, the status byte, the return code and all
four words of hbmpc_recover_summary; then the routes with each other, byte for byte.  No sampling.

Oracle time, measured on the CPU of a build machine: this file's oracle calls (one batch_recover per batch of cases and field, the
stand-alone decodes; the layout tests reuse those results chunk by chunk) take 48.1 s in all (38.6 s of it over Fr), the oracle calls
of tests/test_gpu_random_shapes.py::test_random_encode_decode (replayed with the same seeds, run right after) 65.5 s."""
import numpy as np
import pytest

from __graft_entry__ import load_package
from tests import gao_inputs as X
from tests.test_gpu_mfma_edges import agree, dev_decode, summary_of

pytestmark = pytest.mark.gpu
NOTHING = [0, 0, 0xFFFFFFFF, 0]
SHAPES = X.MAIN_SHAPES + X.D0_SHAPES


def configure(eng, knobs="default"):
    """the knob strings of tests/cpp/recover_routes_dump applied to a context ("default" restores every one of them)"""
    mode, mn, small, generic, second = 1, 65536, 8192, False, True
    for tok in knobs.split(","):
        if tok.startswith("mc"):
            mode = int(tok[2:])
        elif tok.startswith("min"):
            mn = int(tok[3:])
        elif tok == "small0":
            small = 0
        elif tok == "generic":
            generic = True
        elif tok == "second0":
            second = False
        else:
            assert tok == "default", tok
    eng.set_small_batch_chunks(small)
    eng.set_matrix_cores(mode, mn)                               # 65 536: every threshold back at its default (each is capped there)
    eng.set_force_generic(generic)
    eng.set_second_chance(second)


@pytest.fixture(scope="module", params=list(X.IMPLS))
def env(request):
    impl = request.param
    pkg = load_package()
    eng = pkg.Engine(0, field="goldilocks") if impl == "gl" else pkg.Engine(0, impl=impl)
    yield impl, eng
    configure(eng)
    eng.close()


_oracle = {}


def oracle(b):
    """(sender rows [S][G], coefficients, ncoeffs, status) of a batch of cases, by the C oracle, once per field"""
    key = (b.F.name, b.n, b.t, b.d, b.set_name)
    if key not in _oracle:
        ev = b.array()
        rc, co, nco, st = b.F.O.batch_recover(b.ids, ev, b.n, b.d, b.t)
        assert rc == (8 if (st > 1).any() else 0)
        assert [int(s) != 0 for s in st] == [c.flagged for c in b.cases]
        for g, c in enumerate(b.cases):                          # the oracle's answer is the one known by construction, where there is one
            if c.expect is not None and c.expect[0] == "err":
                assert st[g] == c.expect[1], (key, c.name)
            elif c.expect is not None:
                assert st[g] <= 1 and b.F.ints(co[g]) == c.expect[1] + [0] * (b.d + 1 - len(c.expect[1])), (key, c.name)
                assert st[g] == 0 or nco[g] == len(c.expect[1]), (key, c.name)
        _oracle[key] = (ev, co, nco, st)
    return _oracle[key]


def run_call(eng, call):
    """the device-pointer call, full and P(0), against the oracle chunk by chunk -> what it left, for the comparison between routes"""
    b = call.batch()
    ev, co0, nco0, st0 = [np.ascontiguousarray(a[:, call.picks] if i == 0 else a[call.picks]) for i, a in enumerate(oracle(b))]
    eb = 8 if call.impl == "gl" else 32
    where = (call.impl, call.knobs, call.shape, call.set_name, call.G)
    configure(eng, call.knobs)
    co, st, nco, su = dev_decode(eng, b.ids, ev, b.n, b.d, b.t, False, eb)
    bad = [(g, b.cases[call.picks[g]].name, int(st[g]), int(st0[g])) for g in np.flatnonzero((st != st0) | (nco != nco0))[:8]]
    assert not bad, (where, bad)
    bad = [(g, b.cases[call.picks[g]].name) for g in range(call.G) if not np.array_equal(co[g], co0[g])][:8]
    assert not bad, (where, bad)
    assert su.tolist() == summary_of(st0), (where, su.tolist())
    p0v, st1, _, su1 = dev_decode(eng, b.ids, ev, b.n, b.d, b.t, True, eb)
    assert np.array_equal(st1, st0) and np.array_equal(p0v[:, 0], co0[:, 0]) and su1.tolist() == summary_of(st0), where
    return co, st, nco, su, p0v, st1, su1


def clean_call(eng, call):
    """all senders honest, on the same context and stream, behind a call that used the fallback: all-optimistic status and a zero
    summary (the last block of the call before reset its counters)"""
    b = call.batch()
    clean = [i for i, c in enumerate(b.cases) if not c.flagged]
    ev, co0, nco0, st0 = [np.ascontiguousarray(a[:, clean * 7] if i == 0 else a[clean * 7]) for i, a in enumerate(oracle(b))]
    assert not st0.any()
    co, st, nco, su = dev_decode(eng, b.ids, ev, b.n, b.d, b.t, False, 8 if call.impl == "gl" else 32)
    assert not st.any() and np.array_equal(co, co0) and np.array_equal(nco, nco0) and su.tolist() == NOTHING, (call.impl, call.knobs, call.shape)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "n%d_t%d_d%d" % s)
def test_named_cases_through_every_route(env, shape):
    """every batch of named cases of the shape (all senders; S = d + t + 1 + r for r = 1, 2): the wave-per-chunk kernel with k_gao
    un-scaling inline, the lane kernels and k_unscale, the runtime-shaped kernels, for Fr the matrix cores from one chunk on -- each with
    the second chance on and off; then the host-pointer forms (the fallback tables built lazily behind the first kernel): the full
    decode with its return code, and P(0) of the decodable chunks alone"""
    impl, eng = env
    res = {}
    for call in X.named_calls(impl):
        if call.shape == shape:
            res.setdefault(call.set_name, {})[call.knobs] = run_call(eng, call)
    assert res
    for by_route in res.values():
        assert len(by_route) >= 6
        agree(by_route)
    configure(eng)
    for set_name in res:
        b = X.batch(X.IMPLS[impl], *shape, set_name)
        ev, co0, nco0, st0 = oracle(b)
        rc, co, nco, st = eng.batch_recover(b.ids, ev, b.n, b.d, b.t)
        assert rc == (8 if (st0 > 1).any() else 0) and np.array_equal(co, co0) and np.array_equal(nco, nco0) and np.array_equal(st, st0), (shape, set_name)
        good = np.flatnonzero(st0 <= 1)
        rc, p0v, st = eng.batch_recover_p0(b.ids, np.ascontiguousarray(ev[:, good]), b.n, b.d, b.t)
        assert rc == 0 and np.array_equal(p0v, co0[good, 0]) and np.array_equal(st, st0[good]), (shape, set_name)


@pytest.mark.parametrize("shape", X.MAIN_SHAPES, ids=lambda s: "n%d_t%d_d%d" % s)
def test_one_polynomial_and_standalone_decode(env, shape):
    """recover_secret on every named case of the shape (one chunk per call: trimmed coefficients, P(0), the error code), and the
    stand-alone gao_rs_decode (no acceptance count): the all-zero word, k = n, k = 0, one known point, a clean word, errors at and one
    past the capacity behind erasures"""
    impl, eng = env
    F = X.IMPLS[impl]
    n, t, d = shape
    configure(eng)
    b = X.batch(F, n, t, d)
    _, co0, nco0, st0 = oracle(b)
    for g, c in enumerate(b.cases):
        rc, co, sec = eng.recover_secret(c.ids, [d] * b.S, F.arr(c.vals), n, t)
        if st0[g] > 1:
            assert rc == st0[g], (shape, c.name, rc)
            continue
        want = F.ints(co0[g])[:nco0[g] if st0[g] == 1 else d + 1]
        while want and want[-1] == 0:
            want.pop()
        assert rc == 0 and (F.ints(co) if len(co) else []) == want and np.array_equal(sec, co0[g, 0]), (shape, c.name, rc)
    for c in X.gao_cases(F, n, d + 1):
        rec = F.arr(c.received)
        rc0, want = F.O.gao_rs_decode(rec, c.k, n, c.erasures)
        rc, co = eng.gao_rs_decode(rec, c.k, n, c.erasures)
        assert rc == rc0, (shape, c.name, rc, rc0)
        if rc0 == 0:
            assert len(co) == len(want) and np.array_equal(co, want), (shape, c.name)
        assert c.expect is None or (("ok", F.ints(co) if len(co) else []) if rc == 0 else ("err", rc)) == c.expect, (shape, c.name)


def test_groups_sharing_a_wave(env):
    """n <= 15: four chunks per wave, 16 <= n <= 31: two.  Every chunk of the call is flagged and the call has exactly that many chunks
    (block 0 takes list entries 0 .. NSUB - 1, so they share one wave in whatever order the list was appended), then one more (a second,
    partly empty block).  The longest word -- t + 1 errors: the EEA and the division in every round, then failure -- next to the
    shortest: the degree-(d + 1) word (no EEA step in any round) and the zero polynomial with one error (one exact step, round 1)."""
    impl, eng = env
    res = {}
    for call in X.wave_calls(impl):
        assert all(call.batch().cases[i].flagged for i in call.picks)
        res.setdefault((call.shape, call.G), {})[call.knobs] = run_call(eng, call)
        clean_call(eng, call)
    for by_route in res.values():
        agree(by_route)


def test_second_trip_through_the_flagged_list(env):
    """G = 2048 NSUB + 3 chunks, all flagged (about 30 distinct words, tiled; the second chance off so that each reaches k_gao): the
    first groups of the grid take a second list entry with the LDS polynomials and the scratch of the first still in place.  NSUB = 4
    (n = 15; 8 195 chunks are beyond the wave-per-chunk kernel, so the lane kernel and k_unscale, as pinned), 2 (n = 16), 1 (n = 32)"""
    impl, eng = env
    for call in X.second_trip_calls(impl):
        assert all(call.batch().cases[i].flagged for i in call.picks) and len(set(call.picks)) >= 25
        run_call(eng, call)
        clean_call(eng, call)


def test_unscale_lanes(env):
    """k_unscale, one lane per eight consecutive entries of the flagged list: scaled, unscaled (the zero polynomial: nothing to divide
    out) and failed chunks interleaved, 22 of them; a call where every flagged chunk fails (no lane has anything pending); one scaled chunk
    among failures.  The order of the flagged list is not deterministic (the first kernel appends with an atomic), so which entries
    share a lane is not either: these tests assert results only."""
    impl, eng = env
    for call in X.unscale_calls(impl):
        assert call.claim()[3] == "unscale"
        run_call(eng, call)
        clean_call(eng, call)
