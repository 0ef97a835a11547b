"""Seeded RISS dealing on the device (contract "hbmpc-riss-chacha20-v1"; csrc/kernels_riss_sample.hpp, csrc/capi_riss_seeded.inc) against
the model of tests/riss_seeded_model.py, value for value: one sender's contributions (hbmpc_dev_riss_sample and its host form), the
fold of all senders in registers (hbmpc_dev_riss_sample_fold) against the model's sums and against hbmpc_dev_riss_fold over the
materialised contributions, the two seeded protocol calls against the existing calls fed those contributions, byte for byte in every
output buffer, and the refusals -- each on sentinel-filled outputs, which a refused call leaves as they were."""
import math

import numpy as np
import pytest

from __graft_entry__ import load_package
from tests import prandbit_ref as PR
from tests import riss_seeded_model as M

pytestmark = pytest.mark.gpu
INVALID_INPUT, TYPE_MISMATCH, FIELD_CAPACITY = 4, 5, 104
SENTINEL = 0xC3
# (n, t), B, first_index, lk -- and what the model says of each: elements that need a second block, hits of the bound itself
SAMPLE_SHAPES = [((7, 2), 300, 0, 20, 17, 0), ((4, 1), 300, 2**32 - 3, 1, 0, 414), ((4, 1), 300, 5, 59, 4, 0)]
OUTPUTS = ("sums", "bad", "r_p", "r_2", "r_q", "rb", "opened", "b_p", "b_2", "rstatus", "summary_first", "summary")
INT_OUTPUTS = ("sums", "bad", "r_p")


@pytest.fixture(scope="module")
def pkg():
    return load_package()


@pytest.fixture(scope="module")
def engines(pkg):
    fr, gl = pkg.Engine(0, field="fr"), pkg.Engine(0, field="goldilocks")
    yield fr, gl
    fr.close()
    gl.close()


@pytest.fixture(scope="module")
def stream(engines):
    st = engines[0].stream_create()
    yield st
    engines[0].sync(st)
    engines[0].stream_destroy(st)


class Dev:
    """named device buffers of one test, sentinel-filled; freed by close()"""

    def __init__(self, eng, stream, sizes):
        self.eng, self.s, self.size = eng, stream, dict(sizes)
        self.ptr = {k: eng.dev_alloc(max(v, 1)) for k, v in self.size.items()}
        self.fill(self.size)

    def fill(self, names, byte=SENTINEL):
        for k in names:
            self.eng.h2d(self.ptr[k], np.full(max(self.size[k], 1), byte, dtype=np.uint8), self.s)

    def put(self, name, arr):
        arr = np.ascontiguousarray(arr)
        assert arr.nbytes <= self.size[name]
        self.eng.h2d(self.ptr[name], arr, self.s)

    def get(self, name, dtype=np.uint8):
        out = np.zeros(self.size[name], dtype=np.uint8)
        self.eng.d2h(out, self.ptr[name], self.s)
        self.eng.sync(self.s)
        return out.view(dtype)

    def untouched(self, names=None):
        return all(bool((self.get(k) == SENTINEL).all()) for k in (names or self.size))

    def close(self):
        self.eng.sync(self.s)
        for p in self.ptr.values():
            self.eng.dev_free(p)


def seeds_of(n):
    return [M.sender_seed(s) for s in range(n)]


def seed_bytes(n):
    return np.frombuffer(b"".join(seeds_of(n)), dtype=np.uint8)


@pytest.mark.parametrize("shape", SAMPLE_SHAPES, ids=lambda s: "n%d_t%d_B%d_lk%d" % (s[0] + (s[1], s[3])))
def test_sample_equals_the_model(engines, stream, shape):
    """hbmpc_dev_riss_sample over either kind of context, and the host form, against the model -- at shapes where the model says the
    second block of a chain is needed (so a kernel without the retry path cannot pass) or the bound itself is hit"""
    (n, t), B, first, lk, want_retries, want_bound = shape
    Tn = math.comb(n, t)
    want, att = M.rows(M.SEED, 0, Tn, first, B, lk)
    assert int((att > 0).sum()) == want_retries and int((want == (1 << lk)).sum()) == want_bound     # the model's side of the condition
    assert want_retries > 0 or want_bound > 0
    for eng in engines:
        d = Dev(eng, stream, {"out": Tn * B * 8 + 256})
        try:
            assert eng.dev_riss_sample(M.SEED, n, t, 0, B, first, lk, d.ptr["out"], stream) == 0, eng.last_error()
            got = d.get("out", np.uint64)
            assert np.array_equal(got[:Tn * B].reshape(Tn, B), want), np.argwhere(got[:Tn * B].reshape(Tn, B) != want)[:4].tolist()
            assert (got[Tn * B:].view(np.uint8) == SENTINEL).all()                                 # nothing past [Tn][B]
        finally:
            d.close()
    rc, host = engines[0].riss_sample(M.SEED, n, t, 0, B, first, lk)
    assert rc == 0 and np.array_equal(host, want)


@pytest.mark.parametrize("B", [1, 257])
def test_sample_short_and_ragged_batches(engines, stream, B):
    """one lane of one block, and one lane past a full block; domain 1 and another sender's seed"""
    fr = engines[0]
    n, t, first, lk = 4, 1, 5, 59
    seed = M.sender_seed(2)
    want = M.rows(seed, 1, 4, first, B, lk)[0]
    d = Dev(fr, stream, {"out": 4 * B * 8 + 256})
    try:
        assert fr.dev_riss_sample(seed, n, t, 1, B, first, lk, d.ptr["out"], stream) == 0, fr.last_error()
        got = d.get("out", np.uint64)
        assert np.array_equal(got[:4 * B].reshape(4, B), want) and (got[4 * B:].view(np.uint8) == SENTINEL).all()
        assert not np.array_equal(want, M.rows(seed, 0, 4, first, B, lk)[0])                       # the domain is part of the position
    finally:
        d.close()


def test_capacity_rule_at_its_edge(engines, stream):
    """lk = 59 is the largest the capacity rule admits at n = 4 (59 + 2 + 2 < 64): it runs (above); lk = 60 is HBMPC_FIELD_CAPACITY"""
    fr = engines[0]
    d = Dev(fr, stream, {"out": 4 * 8 * 8, "seeds": 4 * 32})
    try:
        d.put("seeds", seed_bytes(4))
        assert fr.dev_riss_sample(M.SEED, 4, 1, 0, 8, 0, 60, d.ptr["out"], stream) == FIELD_CAPACITY
        assert fr.riss_sample_fold(d.ptr["seeds"], 4, 1, 0, 8, 0, 60, d.ptr["out"], stream) == FIELD_CAPACITY
        assert fr.riss_sample(M.SEED, 4, 1, 0, 8, 0, 60)[0] == FIELD_CAPACITY
        assert d.untouched(["out"])
        assert fr.dev_riss_sample(M.SEED, 4, 1, 0, 8, 0, 59, d.ptr["out"], stream) == 0
    finally:
        d.close()


def materialise(eng, stream, d, name, n, t, domain, B, first, lk):
    """contrib [n][Tn][B] in d.ptr[name]: every sender's hbmpc_dev_riss_sample output"""
    Tn = math.comb(n, t)
    for s, seed in enumerate(seeds_of(n)):
        assert eng.dev_riss_sample(seed, n, t, domain, B, first, lk, d.ptr[name] + s * Tn * B * 8, stream) == 0, eng.last_error()


@pytest.mark.parametrize("shape", [((4, 1), 300, 2**32 - 3, 1), ((7, 2), 300, 0, 20)], ids=["n4_t1", "n7_t2"])
def test_sample_fold_equals_the_sum_of_the_streams(engines, stream, shape):
    """a different seed per sender: sums = the sum of the n model streams, and = hbmpc_dev_riss_fold over the n materialised
    hbmpc_dev_riss_sample outputs byte for byte, whose verdict bytes are all zero"""
    fr = engines[0]
    (n, t), B, first, lk = shape
    Tn = math.comb(n, t)
    want = M.folded(seeds_of(n), 0, Tn, first, B, lk)
    d = Dev(fr, stream, {"seeds": n * 32, "sums": Tn * B * 8 + 256, "contrib": n * Tn * B * 8, "sums2": Tn * B * 8, "bad": n * Tn})
    try:
        d.put("seeds", seed_bytes(n))
        assert fr.riss_sample_fold(d.ptr["seeds"], n, t, 0, B, first, lk, d.ptr["sums"], stream) == 0, fr.last_error()
        got = d.get("sums", np.uint64)
        assert np.array_equal(got[:Tn * B].reshape(Tn, B), want) and (got[Tn * B:].view(np.uint8) == SENTINEL).all()
        materialise(fr, stream, d, "contrib", n, t, 0, B, first, lk)
        contrib = d.get("contrib", np.uint64).reshape(n, Tn, B)
        for s, seed in enumerate(seeds_of(n)):
            assert np.array_equal(contrib[s], M.rows(seed, 0, Tn, first, B, lk)[0]), s
        assert fr.dev_riss_fold(d.ptr["contrib"], n, Tn, B, lk, d.ptr["sums2"], d.ptr["bad"], stream) == 0
        assert np.array_equal(d.get("sums2"), d.get("sums")[:Tn * B * 8]) and not d.get("bad").any()
    finally:
        d.close()


def protocol_sizes(n, t, B):
    Tn, G = math.comb(n, t), B // (t + 1)
    return {"seeds": n * 32, "contrib": n * Tn * B * 8, "b_q": n * B * 8, "sums": Tn * B * 8, "bad": n * Tn, "r_p": n * B * 32, "r_2": n * B,
            "r_q": n * B * 8, "rb": n * B * 8, "Y": n * n * G * 8, "Z": n * G * 8, "opened": B * 8, "b_p": n * B * 32, "b_2": n * B, "rstatus": n * G,
            "summary_first": 16, "summary": 16}


def call_bit(fr, gl, d, stream, n, t, B, lk, first=None, **over):
    p = dict(d.ptr)
    p.update(over)
    tail = (n, t, B, lk, p["sums"], p["bad"], p["r_p"], p["r_2"], p["r_q"], p["rb"], p["Y"], p["Z"], p["opened"], p["b_p"], p["b_2"], p["rstatus"],
            p["summary_first"], p["summary"])
    if first is None:
        return fr.prandbit_parties(gl, p["contrib"], p["b_q"], *tail, stream=stream)
    return fr.prandbit_parties_seeded(gl, p["seeds"], first, p["b_q"], *tail, stream=stream)


@pytest.mark.parametrize("shape", [((4, 1), 8), ((7, 2), 300)], ids=["n4_t1_B8", "n7_t2_B300"])
def test_seeded_protocol_calls_equal_the_existing_calls(pkg, engines, stream, shape):
    """hbmpc_dev_prandbit_parties_seeded / _prandint_parties_seeded against hbmpc_dev_prandbit_parties / _prandint_parties fed the
    materialised contrib: every output buffer byte-equal, the existing call once as separate launches (hbmpc_set_fused_prandbit(0)) and
    once at the default threshold (it promises the same bytes either way)"""
    fr, gl = engines
    (n, t), B = shape
    lk, first = 40, 2**32 - 5
    _, _, b_q = PR.make_inputs(n, t, B, lk, seed=5 + n, with_bits=True)
    d = Dev(fr, stream, protocol_sizes(n, t, B))
    try:
        d.put("seeds", seed_bytes(n))
        d.put("b_q", np.array(b_q, dtype=np.uint64))
        got = {}
        for form, threshold in (("separate", 0), ("default", pkg.hbmpc.FUSED_PRANDBIT_DEFAULT), ("seeded", None)):
            d.fill(OUTPUTS + ("Y", "Z", "contrib"))
            if threshold is None:
                assert call_bit(fr, gl, d, stream, n, t, B, lk, first=first) == 0, fr.last_error()
            else:
                fr.set_fused_prandbit(threshold)
                materialise(fr, stream, d, "contrib", n, t, 0, B, first, lk)
                assert call_bit(fr, gl, d, stream, n, t, B, lk) == 0, fr.last_error()
            got[form] = {k: d.get(k).copy() for k in OUTPUTS}
        for form in ("separate", "default"):
            for k in OUTPUTS:
                assert np.array_equal(got["seeded"][k], got[form][k]), (form, k)
        Tn = math.comb(n, t)
        assert np.array_equal(got["seeded"]["sums"].view(np.uint64).reshape(Tn, B), M.folded(seeds_of(n), 0, Tn, first, B, lk))
        assert not got["seeded"]["bad"].any() and not got["seeded"]["rstatus"].any()
        # PRandInt: domain 1
        for form, threshold in (("separate", 0), ("default", pkg.hbmpc.FUSED_PRANDBIT_DEFAULT), ("seeded", None)):
            d.fill(INT_OUTPUTS + ("contrib",))
            if threshold is None:
                assert fr.prandint_parties_seeded(d.ptr["seeds"], first, n, t, B, lk, d.ptr["sums"], d.ptr["bad"], d.ptr["r_p"], stream=stream) == 0
            else:
                fr.set_fused_prandbit(threshold)
                materialise(fr, stream, d, "contrib", n, t, 1, B, first, lk)
                assert fr.prandint_parties(d.ptr["contrib"], n, t, B, lk, d.ptr["sums"], d.ptr["bad"], d.ptr["r_p"], stream=stream) == 0
            got[form] = {k: d.get(k).copy() for k in INT_OUTPUTS}
        for form in ("separate", "default"):
            for k in INT_OUTPUTS:
                assert np.array_equal(got["seeded"][k], got[form][k]), (form, k)
        assert np.array_equal(got["seeded"]["sums"].view(np.uint64).reshape(Tn, B), M.folded(seeds_of(n), 1, Tn, first, B, lk))
    finally:
        fr.set_fused_prandbit(pkg.hbmpc.FUSED_PRANDBIT_DEFAULT)
        d.close()


def test_refusals_write_nothing(engines, stream):
    """every check comes before the first launch or memset: after each refused call all outputs still hold the sentinel"""
    fr, gl = engines
    n, t, B, lk = 4, 1, 8, 40
    d = Dev(fr, stream, protocol_sizes(n, t, B))
    outs = OUTPUTS + ("Y", "Z")
    try:
        seeds = d.ptr["seeds"]
        d.put("seeds", seed_bytes(n))
        d.put("b_q", np.zeros(n * B, dtype=np.uint64))
        o = d.ptr["sums"]
        top = 2**64 - 1
        refused = [
            # one sender
            (fr.dev_riss_sample(M.SEED, n, t, 65536, B, 0, lk, o, stream), INVALID_INPUT, "domain beyond 16 bits"),
            (fr.dev_riss_sample(M.SEED, n, t, 0, B, 0, lk, 0, stream), INVALID_INPUT, "null out"),
            (fr.dev_riss_sample(None, n, t, 0, B, 0, lk, o, stream), INVALID_INPUT, "null seed"),
            (fr.dev_riss_sample(M.SEED, n, t, 0, B, top - 3, lk, o, stream), INVALID_INPUT, "first_index + B passes 2^64"),
            (fr.dev_riss_sample(M.SEED, n, 2, 0, B, 0, lk, o, stream), INVALID_INPUT, "n < 3t + 1"),
            (fr.dev_riss_sample(M.SEED, n, t, 0, B, 0, 60, o, stream), FIELD_CAPACITY, "capacity"),
            (fr.dev_riss_sample(M.SEED, n, t, 0, B, 0, 64, o, stream), FIELD_CAPACITY, "capacity, lk = 64"),
            (fr.dev_riss_sample(M.SEED, n, t, 0, 2**32 + 1, 0, lk, o, stream), INVALID_INPUT, "B beyond the range"),
            (fr.riss_sample(M.SEED, n, t, 65536, B, 0, lk)[0], INVALID_INPUT, "host form: domain"),
            # the fold
            (fr.riss_sample_fold(seeds, n, t, 65536, B, 0, lk, o, stream), INVALID_INPUT, "fold: domain"),
            (fr.riss_sample_fold(0, n, t, 0, B, 0, lk, o, stream), INVALID_INPUT, "fold: null seeds"),
            (fr.riss_sample_fold(seeds, n, t, 0, B, 0, lk, 0, stream), INVALID_INPUT, "fold: null sums"),
            (fr.riss_sample_fold(seeds, n, t, 0, B, top, lk, o, stream), INVALID_INPUT, "fold: index range"),
            (fr.riss_sample_fold(seeds, 6, 2, 0, B, 0, lk, o, stream), INVALID_INPUT, "fold: shape"),
            (fr.riss_sample_fold(seeds, n, t, 0, B, 0, 60, o, stream), FIELD_CAPACITY, "fold: capacity"),
            # PRandBit, seeded
            (call_bit(fr, gl, d, stream, n, t, B, lk, first=0, seeds=0), INVALID_INPUT, "bit: null seeds"),
            (call_bit(fr, gl, d, stream, n, t, B, lk, first=0, b_p=0), INVALID_INPUT, "bit: null b_p"),
            (call_bit(fr, gl, d, stream, n, t, B, lk, first=top - 2), INVALID_INPUT, "bit: index range"),
            (call_bit(fr, gl, d, stream, n, t, 7, lk, first=0), INVALID_INPUT, "bit: B not a multiple of t + 1"),
            (call_bit(fr, gl, d, stream, n, t, B, 60, first=0), FIELD_CAPACITY, "bit: capacity"),
            (call_bit(fr, gl, d, stream, n, 2, 6, lk, first=0), INVALID_INPUT, "bit: shape"),
            (call_bit(gl, gl, d, stream, n, t, B, lk, first=0), TYPE_MISMATCH, "bit: a Goldilocks context for Fr"),
            (call_bit(fr, fr, d, stream, n, t, B, lk, first=0), TYPE_MISMATCH, "bit: an Fr context for Goldilocks"),
            (fr.L.hbmpc_dev_prandbit_parties_seeded(None, None, *([None] * 23)), INVALID_INPUT, "bit: null contexts"),
            # PRandInt, seeded
            (fr.prandint_parties_seeded(0, 0, n, t, B, lk, d.ptr["sums"], d.ptr["bad"], d.ptr["r_p"], stream=stream), INVALID_INPUT, "int: null seeds"),
            (fr.prandint_parties_seeded(seeds, 0, n, t, B, lk, d.ptr["sums"], 0, d.ptr["r_p"], stream=stream), INVALID_INPUT, "int: null bad"),
            (fr.prandint_parties_seeded(seeds, top, n, t, B, lk, d.ptr["sums"], d.ptr["bad"], d.ptr["r_p"], stream=stream), INVALID_INPUT, "int: range"),
            (fr.prandint_parties_seeded(seeds, 0, n, t, B, 60, d.ptr["sums"], d.ptr["bad"], d.ptr["r_p"], stream=stream), FIELD_CAPACITY, "int: capacity"),
            (gl.prandint_parties_seeded(seeds, 0, n, t, B, lk, d.ptr["sums"], d.ptr["bad"], d.ptr["r_p"], stream=stream), TYPE_MISMATCH, "int: field"),
        ]
        for rc, want, what in refused:
            assert rc == want, (what, rc)
        # B = 0: ShareSuccess, nothing enqueued -- also with null buffers; validation still runs first
        assert fr.dev_riss_sample(M.SEED, n, t, 0, 0, 0, lk, 0, stream) == 0 and fr.riss_sample_fold(0, n, t, 0, 0, top, lk, 0, stream) == 0
        assert fr.dev_riss_sample(M.SEED, n, t, 65536, 0, 0, lk, 0, stream) == INVALID_INPUT
        assert call_bit(fr, gl, d, stream, n, t, 0, lk, first=0) == 0
        assert fr.prandint_parties_seeded(seeds, 0, n, t, 0, lk, 0, 0, 0, stream=stream) == 0
        assert d.untouched(outs)
        # and the same buffers do get written by a call that is accepted
        assert call_bit(fr, gl, d, stream, n, t, B, lk, first=0) == 0, fr.last_error()
        assert not d.untouched(["sums"]) and not d.get("bad").any()
    finally:
        d.close()
