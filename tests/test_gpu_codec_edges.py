"""The wire codec kernels (csrc/kernels_codec.hpp) at their edges: the canonical test decided in EVERY limb (is_canonical_u64x4 compares
four limbs against r; k_validate_fvec_gl one word against p), each offending value alone at the first and last element of a wave, of a
block and of the call, in one row of three; the precedence of k_unpack_shares' codes; and the pack kernels at padded strides with a
sentinel in the padding.  Bytes are compared with the numpy restatement of the ark layout of tests/test_gpu_codec.py."""
import numpy as np
import pytest

from __graft_entry__ import load_package
from oracle import cref as O
from oracle import spec as S
from tests.test_gpu_codec import ark_vec_f, ark_vec_shares

pytestmark = pytest.mark.gpu
R = S.R_MOD
P = (1 << 64) - (1 << 32) + 1
M64 = (1 << 64) - 1
SENTINEL = 0xEE


def limbs(v):
    return [(v >> (64 * k)) & M64 for k in range(4)]


def from_limbs(l):
    return sum(x << (64 * k) for k, x in enumerate(l))


def _fr_boundaries():
    """values decided in each limb of the comparison with r: limb k lower by one under all-ones (below r), limb k higher by one over
    zeros (above r); the limbs above k are r's, so the comparison reaches limb k and stops there"""
    r = limbs(R)
    ok, bad = [R - 1], [R, R + 1, (1 << 256) - 1]
    for k in (1, 2, 3):
        ok.append(from_limbs([M64] * k + [r[k] - 1] + r[k + 1:]))
        bad.append(from_limbs([0] * k + [r[k] + 1] + r[k + 1:]))
    assert all(v < R for v in ok) and all(R <= v < 1 << 256 for v in bad) and len(set(ok + bad)) == 10
    return ok, bad


FR_OK, FR_BAD = _fr_boundaries()
GL_OK, GL_BAD = [P - 1], [P, P + 1, M64]
SIZES = [1, 256, 257, 600]


def places(G):  # the first and last lane of a wave, of a block, and of the call
    return sorted({e for e in (0, 63, 64, 255, 256, G - 1) if e < G})


@pytest.fixture(scope="module")
def fr():
    e = load_package().Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def gold():
    e = load_package().Engine(0, field="goldilocks")
    yield e
    e.close()


def pack(vals, gl):
    if gl:
        return np.array(vals, dtype=np.uint64)
    return np.array([limbs(v) for v in vals], dtype=np.uint64).reshape(len(vals), 4)


def passing_elements(count, gl, seed):
    """canonical elements with every passing boundary value among them"""
    rng = np.random.default_rng(seed)
    edge = GL_OK if gl else FR_OK
    if gl:
        a = rng.integers(0, P, size=count, dtype=np.uint64)
    else:
        a = O.fill_random(seed, count)
    for i in range(count):
        if i % 5 == 0:
            a[i] = pack([edge[(i // 5) % len(edge)]], gl)[0]
    return a


class Dev:
    def __init__(self, eng):
        self.eng, self.ptrs = eng, []

    def put(self, arr):
        p = self.eng.dev_alloc(max(arr.nbytes, 64))
        self.ptrs.append(p)
        self.eng.h2d(p, np.ascontiguousarray(arr))
        return p

    def get(self, ptr, arr):
        self.eng.d2h(arr, ptr)
        self.eng.sync()
        return arr

    def free(self):
        self.eng.sync()
        for p in self.ptrs:
            self.eng.dev_free(p)


def fvec_payloads(rows_elems, gl, pad_words):
    """[n_rows][G] elements -> u64 words [n_rows][1 + G W + pad_words]: length prefix, elements, padding"""
    n_rows, G = rows_elems.shape[:2]
    W = 1 if gl else 4
    w = np.full((n_rows, 1 + G * W + pad_words), 0xEEEEEEEEEEEEEEEE, dtype=np.uint64)
    w[:, 0] = G
    w[:, 1: 1 + G * W] = rows_elems.reshape(n_rows, G * W)
    return w


@pytest.mark.parametrize("field", ["fr", "goldilocks"])
@pytest.mark.parametrize("G", SIZES)
def test_validate_fvec_boundaries(request, field, G):
    gl = field != "fr"
    eng = request.getfixturevalue("gold" if gl else "fr")
    n_rows, W, eb = 3, (1 if gl else 4), (8 if gl else 32)
    base = passing_elements(n_rows * G, gl, 100 + G).reshape((n_rows, G) + (() if gl else (4,)))
    words = fvec_payloads(base, gl, 3)
    stride = words.shape[1] * 8
    dev = Dev(eng)
    try:
        pd, sd = dev.put(words), dev.put(np.full(n_rows, 77, dtype=np.uint32))
        st = np.zeros(n_rows, dtype=np.uint32)
        assert eng.dev_validate_fvec(pd, stride, 8 + eb * G, G, n_rows, sd) == 0
        assert dev.get(sd, st).tolist() == [0, 0, 0]                    # every passing boundary value is among them
        case = 0
        for v in (GL_BAD if gl else FR_BAD):
            for e in places(G):
                row = case % n_rows
                case += 1
                w = words.copy()
                w[row, 1 + e * W: 1 + (e + 1) * W] = pack([v], gl).reshape(-1)
                eng.h2d(pd, w)
                assert eng.dev_validate_fvec(pd, stride, 8 + eb * G, G, n_rows, sd) == 0
                assert dev.get(sd, st).tolist() == [4 if j == row else 0 for j in range(n_rows)], (field, G, hex(v), e, row)
    finally:
        dev.free()


@pytest.mark.parametrize("G", SIZES)
def test_unpack_fvec_boundaries(fr, G):
    eng, n_rows, row_stride = fr, 3, G + 2
    base = passing_elements(n_rows * G, False, 200 + G).reshape(n_rows, G, 4)
    words = fvec_payloads(base, False, 3)
    stride = words.shape[1] * 8
    dev = Dev(eng)
    try:
        pd, sd = dev.put(words), dev.put(np.full(n_rows, 77, dtype=np.uint32))
        blank = np.full((n_rows, row_stride, 4), 0xEEEEEEEEEEEEEEEE, dtype=np.uint64)
        rd = dev.put(blank)
        st, out = np.zeros(n_rows, dtype=np.uint32), np.zeros_like(blank)
        assert eng.dev_unpack_fvec(pd, stride, 8 + 32 * G, G, n_rows, rd, row_stride, sd) == 0
        assert dev.get(sd, st).tolist() == [0, 0, 0]
        dev.get(rd, out)
        assert np.array_equal(out[:, :G], base) and np.array_equal(out[:, G:], blank[:, G:])   # the rows, and nothing between them
        case = 0
        for v in FR_BAD:
            for e in places(G):
                row = (case + 1) % n_rows
                case += 1
                w = words.copy()
                w[row, 1 + e * 4: 5 + e * 4] = limbs(v)
                eng.h2d(pd, w)
                assert eng.dev_unpack_fvec(pd, stride, 8 + 32 * G, G, n_rows, rd, row_stride, sd) == 0
                assert dev.get(sd, st).tolist() == [4 if j == row else 0 for j in range(n_rows)], (G, hex(v), e, row)
    finally:
        dev.free()


@pytest.mark.parametrize("N", SIZES)
def test_unpack_shares_and_validate_canonical_boundaries(fr, N):
    eng, sid, deg = fr, 3, 5
    vals = passing_elements(N, False, 300 + N)
    payload = np.frombuffer(ark_vec_shares(vals, sid, deg), dtype=np.uint64).copy()
    dev = Dev(eng)
    try:
        pd, vd, od, sd = dev.put(payload), dev.put(vals), dev.put(np.zeros((N, 4), dtype=np.uint64)), dev.put(np.full(1, 77, dtype=np.uint32))
        st, out = np.zeros(1, dtype=np.uint32), np.zeros((N, 4), dtype=np.uint64)
        assert eng.dev_unpack_shares(pd, payload.nbytes, N, sid, deg, od, sd) == 0
        assert dev.get(sd, st)[0] == 0 and np.array_equal(dev.get(od, out), vals)
        assert eng.dev_validate_canonical(vd, N, sd) == 0
        assert dev.get(sd, st)[0] == 0
        for v in FR_BAD:
            for e in places(N):
                w = payload.copy()
                w[1 + 6 * e: 5 + 6 * e] = limbs(v)
                eng.h2d(pd, w)
                assert eng.dev_unpack_shares(pd, payload.nbytes, N, sid, deg, od, sd) == 0
                assert dev.get(sd, st)[0] == 4, ("unpack_shares", N, hex(v), e)
                a = vals.copy()
                a[e] = limbs(v)
                eng.h2d(vd, a)
                assert eng.dev_validate_canonical(vd, N, sd) == 0
                assert dev.get(sd, st)[0] == 4, ("validate_canonical", N, hex(v), e)
    finally:
        dev.free()


def test_unpack_shares_code_precedence(fr):
    """status = the highest code seen: 2 (another degree) < 3 (another id) < 4 (not canonical), whichever records they are in"""
    eng, N, sid, deg = fr, 257, 3, 5
    vals = passing_elements(N, False, 400)
    payload = np.frombuffer(ark_vec_shares(vals, sid, deg), dtype=np.uint64).copy()
    dev = Dev(eng)
    try:
        pd, od, sd = dev.put(payload), dev.put(np.zeros((N, 4), dtype=np.uint64)), dev.put(np.zeros(1, dtype=np.uint32))
        st = np.zeros(1, dtype=np.uint32)

        def code(w):
            eng.h2d(pd, w)
            assert eng.dev_unpack_shares(pd, payload.nbytes, N, sid, deg, od, sd) == 0
            return int(dev.get(sd, st)[0])

        assert code(payload) == 0
        w = payload.copy()
        w[1 + 6 * 200 + 5] = deg + 1                       # a wrong degree in one record ...
        assert code(w) == 2
        w[1 + 6 * 10 + 4] = sid + 1                        # ... and a wrong id in another (an earlier one, in another wave)
        assert code(w) == 3
        w2 = w.copy()
        w2[1 + 6 * 100: 5 + 6 * 100] = limbs(R)            # ... and a value that is not canonical in a third
        assert code(w2) == 4
        w3 = payload.copy()                               # all three in ONE record
        w3[1 + 6 * 64: 7 + 6 * 64] = limbs(R) + [sid + 1, deg + 1]
        assert code(w3) == 4
        w3[1 + 6 * 64: 5 + 6 * 64] = limbs(R - 1)
        assert code(w3) == 3
        for field, want in ((4, 3), (5, 2)):               # a mismatch in the last record alone is seen
            w4 = payload.copy()
            w4[1 + 6 * (N - 1) + field] += 1
            assert code(w4) == want
        w5 = payload.copy()                               # a wrong length prefix
        w5[0] = N - 1
        assert code(w5) == 4
    finally:
        dev.free()


@pytest.mark.parametrize("G", [1, 256, 257])
def test_pack_fvec_padded(fr, G):
    eng, n_rows, row_stride = fr, 3, G + 3
    rows = O.fill_random(500 + G, n_rows * row_stride).reshape(n_rows, row_stride, 4)
    stride = 8 + 32 * G + 24
    dev = Dev(eng)
    try:
        rd, pd = dev.put(rows), dev.put(np.full(n_rows * stride, SENTINEL, dtype=np.uint8))
        assert eng.dev_pack_fvec(rd, row_stride, G, n_rows, pd, stride) == 0
        raw = dev.get(pd, np.zeros(n_rows * stride, dtype=np.uint8)).reshape(n_rows, stride)
        for j in range(n_rows):
            assert raw[j, : 8 + 32 * G].tobytes() == ark_vec_f(rows[j, :G]), j
        assert (raw[:, 8 + 32 * G:] == SENTINEL).all()      # the padding keeps its bytes
        assert eng.dev_pack_fvec(rd, G - 1, G, n_rows, pd, stride) == 4          # a row stride below the row length
        assert eng.dev_pack_fvec(rd, row_stride, G, n_rows, pd, 8 + 32 * G - 8) == 4  # a payload stride below the payload
    finally:
        dev.free()


@pytest.mark.parametrize("N", [1, 256, 257])
def test_pack_shares_padded(fr, N):
    eng, sid, deg = fr, 0xFFFFFFFF12345678, 7
    vals = O.fill_random(600 + N, N)
    nbytes = 8 + 48 * N
    dev = Dev(eng)
    try:
        vd, pd = dev.put(vals), dev.put(np.full(nbytes + 40, SENTINEL, dtype=np.uint8))
        assert eng.dev_pack_shares(vd, N, sid, deg, pd) == 0
        raw = dev.get(pd, np.zeros(nbytes + 40, dtype=np.uint8))
        assert raw[:nbytes].tobytes() == ark_vec_shares(vals, sid, deg)
        assert (raw[nbytes:] == SENTINEL).all()
    finally:
        dev.free()
