"""The wave-, lane- and runtime-shaped decode kernels (k_batch_recover_wide with dot_shared, k_batch_recover<F, M, P0>,
k_batch_recover_generic, k_second_chance, k_second_chance_m<U29, M>, second_chance_wave) on the targeted chunks of tests/decode_inputs.py:
results at both edges of canon_loose's subtraction and of reduce_top's quotient at every verify row and output row, all-ones sharings,
one bit of one sender's share set at the limb boundaries, liars placed so that a named second-chance window accepts, flagged counts on
both sides of the switch between the second chance's wave and lane forms, and a flagged list longer than one trip of its grid.
tests/test_decode_inputs.py proves without a GPU that the inputs reach all of that and pins the kernels each call below takes.

Every call is the device-pointer decode with sentinel-filled outputs, full and P(0); every chunk of every call is compared with the C
oracle (oracle.cref, oracle.cref_gl) -- coefficients zero padded, ncoeffs, the status byte, the return code and all four summary words --
never with another route alone; then the routes with each other, byte for byte.  No sampling.  After every call that flagged or failed a
chunk an all-honest call on the same context and stream must leave status zero and the summary [0, 0, 0xFFFFFFFF, 0].

Measured on an MI355X: 97 tests in 11.91 s of wall time; no test above 2.0 s (n = 196 over Fr, most of it the C oracle's answer for that
batch: 3.2 s on a build machine's CPU), the second trip of 262 444 flagged chunks below 0.4 s.  One batch_recover of the oracle per batch of
chunks and field; the calls pick their chunks from its answer (profiles/decode_edges.txt)."""
import numpy as np
import pytest

from __graft_entry__ import load_package
from tests import decode_inputs as D
from tests.test_gpu_gao_edges import NOTHING, configure
from tests.test_gpu_mfma_edges import agree, dev_decode, summary_of

pytestmark = pytest.mark.gpu
ALL_SHAPES = D.SHAPES + tuple(s for s in D.SWEEP_SHAPES if s not in D.SHAPES)


def _env(impls):
    @pytest.fixture(scope="module", params=impls)
    def fixture(request):
        pkg = load_package()
        eng = pkg.Engine(0, field="goldilocks") if request.param == "gl" else pkg.Engine(0, impl=request.param)
        yield request.param, eng
        configure(eng)
        eng.close()
    return fixture


env = _env(list(D.IMPLS))                                         # u29, sat32 (a comparison route), gl
env2 = _env(["u29", "gl"])                                        # the calls that are about the second chance's own kernels


_oracle = {}


def oracle(b):
    """(sender rows [S][G], coefficients, ncoeffs, status) of a batch by the C oracle, once per field"""
    key = (b.F.name, b.n, b.t, b.d, b.set_name)
    if key not in _oracle:
        ev = b.array()
        rc, co, nco, st = b.F.O.batch_recover(b.ids, ev, b.n, b.d, b.t)
        assert rc == (8 if (st > 1).any() else 0)
        for g, c in enumerate(b.chunks):                             # the oracle's answer is the one known by construction
            if c.kind == "honest" or c.window is not None:
                assert st[g] == (0 if c.kind == "honest" else 1) and b.F.ints(co[g]) == [x % b.F.mod for x in c.poly], (key, c.name)
        _oracle[key] = (ev, co, nco, st)
    return _oracle[key]


def run_call(eng, call):
    """the device-pointer call, full and P(0), against the oracle chunk by chunk -> what it left, for the comparison between routes"""
    b = call.batch()
    picks = np.array(call.picks)
    ev, co0, nco0, st0 = [np.ascontiguousarray(a[:, picks] if i == 0 else a[picks]) for i, a in enumerate(oracle(b))]
    eb = 8 if call.impl == "gl" else 32
    where = (call.impl, call.knobs, call.shape, call.set_name, call.name, call.G)
    configure(eng, call.knobs)
    co, st, nco, su = dev_decode(eng, b.ids, ev, b.n, b.d, b.t, False, eb)          # asserts the return code (0: failures are in the summary)
    bad = [(int(g), b.chunks[call.picks[g]].name, int(st[g]), int(st0[g]), int(nco[g]), int(nco0[g])) for g in np.flatnonzero((st != st0) | (nco != nco0))[:8]]
    assert not bad, (where, bad)
    bad = [(g, b.chunks[call.picks[g]].name) for g in np.flatnonzero((co != co0).reshape(call.G, -1).any(axis=1))[:8]]
    assert not bad, (where, bad)
    assert su.tolist() == summary_of(st0), (where, su.tolist(), summary_of(st0))
    p0v, st1, _, su1 = dev_decode(eng, b.ids, ev, b.n, b.d, b.t, True, eb)
    assert np.array_equal(st1, st0) and np.array_equal(p0v[:, 0], co0[:, 0]) and su1.tolist() == summary_of(st0), where
    if st0.any():
        clean_call(eng, call)
    return co, st, nco, su, p0v, st1, su1


def clean_call(eng, call):
    """all senders honest, on the same context and stream, behind a call that flagged or failed chunks: status zero, an empty summary"""
    b = call.batch()
    clean = np.array([i for i, c in enumerate(b.chunks) if c.kind == "honest"] * 3)
    ev, co0, nco0, st0 = [np.ascontiguousarray(a[:, clean] if i == 0 else a[clean]) for i, a in enumerate(oracle(b))]
    assert not st0.any()
    co, st, nco, su = dev_decode(eng, b.ids, ev, b.n, b.d, b.t, False, 8 if call.impl == "gl" else 32)
    assert not st.any() and np.array_equal(co, co0) and np.array_equal(nco, nco0) and su.tolist() == NOTHING, (call.impl, call.knobs, call.shape, call.name)


@pytest.mark.parametrize("shape", ALL_SHAPES, ids=lambda s: "n%d_t%d_d%d" % s)
def test_targeted_chunks_through_every_route(env, shape):
    """every chunk of the shape with S = d + t + 1 (no OEC round: one launch) and S = n (the second chance fused into Wide, or in the
    tail), through Wide, the lane kernels and the runtime-shaped kernel, the second chance on and off; a whole block of rare chunks with a
    rare chunk last in the ragged final block (G = 300), and one rare chunk last among fast ones (G = 133); then the host-pointer forms
    (the fallback tables built lazily behind the first kernel)"""
    impl, eng = env
    res = {}
    for call in D.calls_for(impl, shape):
        res.setdefault((call.set_name, call.name), {})[call.knobs] = run_call(eng, call)
    assert res
    for by_route in res.values():
        agree(by_route)
    configure(eng)
    F = D.IMPLS[impl]
    for set_name in D.set_names(shape):
        b = D.batch(F, shape, set_name)
        ev, co0, nco0, st0 = oracle(b)
        rc, co, nco, st = eng.batch_recover(b.ids, ev, b.n, b.d, b.t)
        assert rc == (8 if (st0 > 1).any() else 0) and np.array_equal(co, co0) and np.array_equal(nco, nco0) and np.array_equal(st, st0), (impl, shape, set_name)
        good = np.flatnonzero(st0 <= 1)
        rc, p0v, st = eng.batch_recover_p0(b.ids, np.ascontiguousarray(ev[:, good]), b.n, b.d, b.t)
        assert rc == 0 and np.array_equal(p0v, co0[good, 0]) and np.array_equal(st, st0[good]), (impl, shape, set_name)


def test_flagged_counts_at_the_form_switches(env2):
    """G = 512, so the second chance runs 2 blocks of 4 waves: 8 and 9 flagged chunks around `count <= nwaves` of k_second_chance_m,
    40 and 41 around `count <= nwaves * spread` of k_second_chance"""
    impl, eng = env2
    for call in D.switch_calls(impl):
        run_call(eng, call)


def test_second_trip_through_the_flagged_list(env2):
    """262 144 + 300 chunks, every one flagged: the first blocks of the second chance's grid make a second trip, runs of 256 chunks that
    window 0 resolves alternate with runs that window 1 resolves, and the alternation turns over at chunk 262 144 so that a block meets
    the other window on its second trip; the oracle decodes the distinct words"""
    impl, eng = env2
    res = {}
    for call in D.second_trip_calls(impl):
        b = call.batch()
        assert call.G == D.SECOND_TRIP_G and all(b.chunks[g].window in (0, 1) for g in set(call.picks))
        res[call.knobs] = run_call(eng, call)
    agree(res)
