"""The seeded handles (hbmpc_pipe_prandint_create_seeded, hbmpc_pipe_prandbit_create_seeded, hbmpc_pipe_fixedprep_create_seeded): the
stream index that run() uses and advances, hbmpc_pipe_set_stream_index, `seeds` in place of `contrib`, the refused capture(), and a
seeded FixedPrep against an unseeded one whose RISS parts were given the materialised contributions and the same polynomials."""
import ctypes as C
import math

import numpy as np
import pytest

from __graft_entry__ import load_package
from tests import fixedprep_ref as FR
from tests import riss_seeded_model as M

pytestmark = pytest.mark.gpu
INVALID_INPUT = 4


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
    st = engines[1].stream_create()
    yield st
    engines[1].sync(st)
    engines[1].stream_destroy(st)


def seeds_of(n):
    return [M.sender_seed(s) for s in range(n)]


def test_prandint_handle_draws_at_its_index_and_advances(pkg, engines, stream):
    """two run()s give the model's sums at indices [0, B) and then [B, 2B); set_stream_index moves it (here across 2^32); contrib is an
    unknown name and nothing of its size is allocated; capture() is refused with a message; an unseeded handle has no index"""
    fr, _ = engines
    n, t, B, lk = 7, 2, 37, 40
    Tn = math.comb(n, t)
    pipe = pkg.pipelines.PRandIntPipe(fr, n, t, B, lk, stream=stream, seeded=True)
    plain = pkg.pipelines.PRandIntPipe(fr, n, t, B, lk, stream=stream)
    try:
        pipe.upload_seeds(seeds_of(n))
        for first in (0, B):
            pipe.run()
            assert np.array_equal(pipe.download_named("sums", (Tn, B)), M.folded(seeds_of(n), 1, Tn, first, B, lk)), first
            assert not pipe.download_named("bad").any()
        first = 2**32 - 5
        pipe.set_stream_index(first)
        for k in range(2):
            pipe.run()
            assert np.array_equal(pipe.download_named("sums", (Tn, B)), M.folded(seeds_of(n), 1, Tn, first + k * B, B, lk)), k
        # r_p is the conversion of those sums: the unseeded handle, fed the same contributions, gives the same bytes
        contrib = np.stack([M.rows(s, 1, Tn, first + B, B, lk)[0] for s in seeds_of(n)])
        plain.upload_named("contrib", contrib)
        plain.run()
        for name in ("sums", "bad", "r_p"):
            assert np.array_equal(pipe.download_named(name), plain.download_named(name)), name
        L = fr.L
        assert L.hbmpc_pipe_buffer(pipe.h, b"contrib", None, None) == INVALID_INPUT
        assert pipe.buffer("seeds")[1] == n * 32
        assert L.hbmpc_pipe_capture(pipe.h) == INVALID_INPUT and "seeded" in fr.last_error()
        pipe.run()                                                   # the refusal left the handle and its index alone
        assert np.array_equal(pipe.download_named("sums", (Tn, B)), M.folded(seeds_of(n), 1, Tn, first + 2 * B, B, lk))
        assert L.hbmpc_pipe_set_stream_index(plain.h, C.c_uint64(3)) == INVALID_INPUT
        assert L.hbmpc_pipe_set_stream_index(None, C.c_uint64(3)) == INVALID_INPUT
        # a run() that is refused leaves the index where it was: the last B positions before 2^64 are accepted, one further is not
        pipe.set_stream_index(2**64 - B + 1)
        with pytest.raises(RuntimeError, match="ShareErrorCode %d" % INVALID_INPUT):
            pipe.run()
        pipe.set_stream_index(2**64 - 1 - B)
        pipe.run()
        assert np.array_equal(pipe.download_named("sums", (Tn, B)), M.folded(seeds_of(n), 1, Tn, 2**64 - 1 - B, B, lk))
    finally:
        pipe.close()
        plain.close()


def test_prandbit_handle_is_seeded_too(pkg, engines, stream):
    """the PRandBit handle: seeds and no contrib, domain 0, the index advances by B, capture() refused"""
    fr, gl = engines
    n, t, B, lk = 4, 1, 8, 40
    pipe = pkg.pipelines.PRandBitPipe(gl, fr, n, t, B, lk, stream=stream, seeded=True)
    try:
        pipe.upload_seeds(seeds_of(n))
        pipe.upload_named("b_q", np.zeros(n * B, dtype=np.uint64))     # shares of zero bits
        for first in (0, B):
            pipe.run(check=True)
            assert np.array_equal(pipe.download_named("sums", (4, B)), M.folded(seeds_of(n), 0, 4, first, B, lk)), first
        assert fr.L.hbmpc_pipe_buffer(pipe.h, b"contrib", None, None) == INVALID_INPUT
        assert fr.L.hbmpc_pipe_capture(pipe.h) == INVALID_INPUT and "seeded" in fr.last_error()
    finally:
        pipe.close()


def test_seeded_fixedprep_equals_the_unseeded_one(pkg, engines, stream):
    """(4, 1), 20 bits and 5 integers: the seeded handle against an unseeded one whose prandbit / prandint parts were given the
    materialised contributions (domain 0 over [0, R), domain 1 over [0, 5)) and the same polynomials -- r_bits, r_bits2 and r_int
    byte-equal; a take from each gives the same rbits / rint; the second run draws at the advanced index"""
    fr, gl = engines
    n, t, nb, ni = 4, 1, 20, 5
    inp = FR.inputs(n, t, nb, ni)
    lk, Tn = inp["lk"], math.comb(n, t)
    R = FR.sizes(n, t, nb)[0]
    arr = lambda rows: np.array(rows, dtype=np.uint64)  # noqa: E731
    preps = {k: pkg.pipelines.FixedPrep(gl, fr, n, t, nb, ni, lk, stream=stream, seeded=(k == "seeded")) for k in ("seeded", "plain")}
    k_fp, m_fp, N_fp = 16, 4, 3
    fps = {k: pkg.pipelines.FpMul(fr, n, t, N_fp, k_fp, m_fp, stream=stream) for k in preps}
    try:
        for prep in preps.values():
            prep.rs.upload(arr(inp["coeffs"]))
            prep.rd.upload(arr(inp["coeffs_t"]), arr(inp["coeffs_2t"]))
        seeded, plain = preps["seeded"], preps["plain"]
        seeded.upload_seeds(seeds_of(n))
        L = fr.L
        for h in (seeded, seeded.pb, seeded.pi):
            assert L.hbmpc_pipe_buffer(h.h, b"contrib", None, None) == INVALID_INPUT
        assert L.hbmpc_pipe_capture(seeded.h) == INVALID_INPUT and "seeded" in fr.last_error()
        for first in (0, max(R, ni)):
            plain.pb.upload_named("contrib", np.stack([M.rows(s, 0, Tn, first, R, lk)[0] for s in seeds_of(n)]))
            plain.pi.upload_named("contrib", np.stack([M.rows(s, 1, Tn, first, ni, lk)[0] for s in seeds_of(n)]))
            got = {}
            for k, prep in preps.items():
                prep.run(check=True)
                got[k] = {name: prep.download_named(name).copy() for name in ("r_bits", "r_bits2", "r_int")}
                assert prep.available() == (R, ni)
            for name in ("r_bits", "r_bits2", "r_int"):
                assert np.array_equal(got["seeded"][name], got["plain"][name]), (first, name)
            assert np.array_equal(seeded.pb.download_named("sums"), plain.pb.download_named("sums"))
        taken = {}
        for k, prep in preps.items():
            prep.take(fps[k])
            taken[k] = (fps[k].download_named("rbits", (n, m_fp, N_fp)).copy(), fps[k].download_named("rint", (n, N_fp)).copy())
            assert prep.available() == (R - m_fp * N_fp, ni - N_fp)
        assert np.array_equal(taken["seeded"][0], taken["plain"][0]) and np.array_equal(taken["seeded"][1], taken["plain"][1])
        assert np.array_equal(taken["seeded"][1].reshape(n, N_fp, 4), got["seeded"]["r_int"].reshape(n, ni, 4)[:, :N_fp])
    finally:
        for h in list(fps.values()) + list(preps.values()):
            h.close()
