"""The integer-point Shamir scheme on the GPU against its model (tests/shamir_ref.py, common/share/shamir.rs:44-125): exact equality.
The encode on each route forced (the small-weight kernel, the wave-per-secret and the lane-per-secret Horner kernels), both fields;
each refusal by return code; the batched open behind every decode kernel family; encode -> element-wise calls -> open (the field
halves of feldman.rs:311-427); the table cache with domain ids and integer points alternating; host and dev_ forms."""
import ctypes as C
import random

import numpy as np
import pytest

from __graft_entry__ import load_package
from tests import shamir_ref as M
from tests.gpu_util import dev_buf, fetch
from tests.shamir_ref import FR, GL

pytestmark = pytest.mark.gpu

U64 = 1 << 64
P_GL = GL.R_MOD
SPEC = {"fr": FR, "goldilocks": GL}
FIELDS = ["fr", "goldilocks"]
SMALL, WIDE, LANE = 1, 2, 3
PTS16 = [7, 1, 3, 20, 2, 9, 33, 4, 100, 5, 6, 8, 11, 12, 13, 14]  # unsorted, not contiguous


@pytest.fixture(scope="module")
def engines():
    pkg = load_package()
    e = {f: pkg.Engine(0, field=f) for f in FIELDS}
    yield e
    for x in e.values():
        x.close()


@pytest.fixture(params=FIELDS)
def fe(request, engines):
    eng = engines[request.param]
    yield request.param, eng
    eng.set_shamir_route(0)
    eng.set_small_batch_chunks(8192)
    eng.set_force_generic(False)
    eng.set_matrix_cores(True, 65536)


def arr(field, ints, shape):
    """python integers -> the field's numpy layout"""
    ints = list(ints)
    if field == "fr":
        a = np.array([[(v >> (64 * i)) & (U64 - 1) for i in range(4)] for v in ints], dtype=np.uint64)
        return a.reshape(tuple(shape) + (4,))
    return np.array(ints, dtype=np.uint64).reshape(shape)


def ints(field, a):
    a = np.asarray(a)
    if field == "fr":
        flat = a.reshape(-1, 4)
        return [sum(int(x) << (64 * i) for i, x in enumerate(row)) for row in flat]
    return [int(x) for x in a.reshape(-1)]


def boundary(d):
    x = int(round(U64 ** (1.0 / d)))
    while x ** d >= U64:
        x -= 1
    while (x + 1) ** d < U64:
        x += 1
    return x


def set_route(eng, route):
    """force a route and say which kernel the planner then reports for a call the small-weight kernel covers"""
    eng.set_small_batch_chunks(0 if route == LANE else 8192)
    eng.set_shamir_route(1 if route == SMALL else 2)


def model_shares(spec, coeffs, d, pts):
    cols = [M.compute_shares(spec, c, d, pts) for c in coeffs]      # [B][m]
    return [cols[b][i] for i in range(len(pts)) for b in range(len(coeffs))]  # [m][B]


def check_encode(field, eng, coeffs, d, pts, want_kernel=None):
    spec = SPEC[field]
    B = len(coeffs)
    if want_kernel is not None:
        assert eng.shamir_route(pts, d, B) == (0, want_kernel)
    rc, got = eng.shamir_compute_shares(arr(field, [x for c in coeffs for x in c], (B, d + 1)), pts, d)
    assert rc == 0, eng.last_error()
    assert ints(field, got) == model_shares(spec, coeffs, d, pts)


@pytest.mark.parametrize("route", [SMALL, WIDE, LANE])
@pytest.mark.parametrize("m,d", [(1, 0), (4, 1), (6, 5), (16, 5), (8, 7)])
def test_encode(fe, route, m, d):
    field, eng = fe
    p = SPEC[field].R_MOD
    rng = random.Random(1000 * m + d)
    set_route(eng, route)
    for B in (1, 63, 64, 65, 257):
        coeffs = [[rng.randrange(p) for _ in range(d + 1)] for _ in range(B)]
        check_encode(field, eng, coeffs, d, PTS16[:m], route)


@pytest.mark.parametrize("route", [SMALL, WIDE, LANE])
def test_encode_extreme_coefficients(fe, route):
    field, eng = fe
    p = SPEC[field].R_MOD
    rng = random.Random(7)
    set_route(eng, route)
    B, m, d = 65, 16, 5
    for coeffs in ([[p - 1] * (d + 1)] * B, [[0] * (d + 1)] * B, [[rng.randrange(p) for _ in range(d)] + [0] for _ in range(B)],
                   [[0] * d + [p - 1]] * B):
        check_encode(field, eng, coeffs, d, PTS16[:m], route)


@pytest.mark.parametrize("d", [1, 2, 5, 10])
def test_encode_either_side_of_the_route_switch(fe, d):
    """the largest id with id^d < 2^64 runs the small-weight kernel with its largest weights; the next id leaves it although forced"""
    field, eng = fe
    p = SPEC[field].R_MOD
    rng = random.Random(d)
    b = boundary(d)
    rest = [x for x in (1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11) if x != b][:d]
    for B in (65, 257):
        coeffs = [[rng.randrange(p) for _ in range(d + 1)] for _ in range(B - 1)] + [[p - 1] * (d + 1)]
        set_route(eng, SMALL)
        check_encode(field, eng, coeffs, d, [b] + rest, SMALL)
        if b + 1 < U64 and (b + 1) % p != 0:
            check_encode(field, eng, coeffs, d, rest + [b + 1], WIDE)
        set_route(eng, WIDE)
        check_encode(field, eng, coeffs, d, [b] + rest, WIDE)
    eng.set_shamir_route(0)   # the planner's own choice at a large batch: 4 099 secrets, beyond the wave-per-secret range
    coeffs = [[rng.randrange(p) for _ in range(d + 1)] for _ in range(4099)]
    check_encode(field, eng, coeffs, d, [b] + rest, SMALL)
    if b + 1 < U64 and (b + 1) % p != 0:
        check_encode(field, eng, coeffs[:2100], d, rest + [b + 1], LANE)


def test_encode_goldilocks_ids_beyond_p(engines):
    eng = engines["goldilocks"]
    rng = random.Random(3)
    try:
        for route in (SMALL, WIDE, LANE):
            set_route(eng, route)
            coeffs = [[rng.randrange(P_GL) for _ in range(2)] for _ in range(65)]
            check_encode("goldilocks", eng, coeffs, 1, [1, P_GL + 1], route)          # two equal rows
            rc, got = eng.shamir_compute_shares(arr("goldilocks", [x for c in coeffs for x in c], (65, 2)), [1, P_GL + 1], 1)
            assert rc == 0 and np.array_equal(got[0], got[1])
            check_encode("goldilocks", eng, coeffs, 1, [U64 - 1, 2, P_GL - 1], route)
            # d = 2: an id beyond 2^32 leaves the small-weight kernel
            coeffs = [[rng.randrange(P_GL) for _ in range(3)] for _ in range(65)]
            check_encode("goldilocks", eng, coeffs, 2, [U64 - 1, P_GL + 1, 5], WIDE if route == SMALL else route)
    finally:
        eng.set_shamir_route(0)
        eng.set_small_batch_chunks(8192)


def test_encode_refusals(fe):
    field, eng = fe
    c = arr(field, [1, 2, 3] * 4, (4, 3))
    codes = lambda pts, d=2: eng.shamir_compute_shares(c[:, :d + 1].copy(), pts, d)[0]
    assert codes(None) == 4                                  # 1. no ids
    assert codes([1, 2]) == 1 and codes([0, 0]) == 1         # 2. too few, before the zero and the duplicate
    assert codes([1, 0, 2]) == 4                             # 3. a zero id
    assert codes([1, 2, 2]) == 4                             # 4. duplicates
    assert codes([3, 1, 2]) == 0
    if field == "goldilocks":
        assert codes([1, P_GL, 2]) == 4 and codes([1, P_GL + 1, 2]) == 0
    d_c = dev_buf(eng, c)
    d_o = eng.dev_alloc(4 * 3 * 32)
    try:
        assert eng.dev_shamir_compute_shares(d_c, 4, None, 2, d_o) == 4
        assert eng.dev_shamir_compute_shares(d_c, 4, [1, 2], 2, d_o) == 1
        assert eng.dev_shamir_compute_shares(d_c, 4, [1, 2, 0], 2, d_o) == 4
        assert eng.dev_shamir_compute_shares(d_c, 4, [2, 1, 2], 2, d_o) == 4
        assert eng.dev_shamir_compute_shares(0, 4, [1, 2, 3], 2, d_o) == 4      # a null buffer
        assert eng.dev_shamir_compute_shares(d_c, 0, [1, 2, 3], 2, d_o) == 0    # an empty batch
    finally:
        eng.dev_free(d_c)
        eng.dev_free(d_o)
    # the other field's entry point on this context
    other = eng.L.hbmpc_gl_shamir_compute_shares if field == "fr" else eng.L.hbmpc_shamir_compute_shares
    pts = (C.c_uint64 * 3)(1, 2, 3)
    assert other(eng.ctx, c.ctypes.data_as(C.c_void_p), C.c_size_t(4), pts, C.c_size_t(3), C.c_size_t(2), c.ctypes.data_as(C.c_void_p)) == 5


def test_host_and_dev_forms_agree(fe):
    field, eng = fe
    p = SPEC[field].R_MOD
    rng = random.Random(11)
    B, m, d = 257, 6, 5
    coeffs = [[rng.randrange(p) for _ in range(d + 1)] for _ in range(B)]
    c = arr(field, [x for r in coeffs for x in r], (B, d + 1))
    pts = PTS16[:m]
    eb = eng.ebytes
    d_c, d_o, d_co, d_deg, d_c0, d_deg2 = dev_buf(eng, c), eng.dev_alloc(m * B * eb), eng.dev_alloc(m * B * eb), eng.dev_alloc(B * 4), \
        eng.dev_alloc(B * eb), eng.dev_alloc(B * 4)
    try:
        for route in (SMALL, WIDE, LANE):
            set_route(eng, route)
            rc, host = eng.shamir_compute_shares(c, pts, d)
            assert rc == 0 and eng.dev_shamir_compute_shares(d_c, B, pts, d, d_o) == 0
            eng.sync()
            assert np.array_equal(fetch(eng, d_o, host.shape), host)
        rc, hco, hdeg = eng.shamir_batch_interpolate(pts, host)
        assert rc == 0 and eng.dev_shamir_batch_interpolate(pts, d_o, B, B, d_co, d_deg) == 0
        assert eng.dev_shamir_batch_interpolate_c0(pts, d_o, B, B, d_co, d_c0, d_deg2) == 0
        eng.sync()
        assert np.array_equal(fetch(eng, d_co, hco.shape), hco) and np.array_equal(fetch(eng, d_deg, (B,), np.uint32), hdeg)
        assert np.array_equal(fetch(eng, d_c0, hco[:, 0].shape), hco[:, 0]) and np.array_equal(fetch(eng, d_deg2, (B,), np.uint32), hdeg)
        assert ints(field, hco) == [x for r in coeffs for x in r]          # S = d + 1: the coefficient rows themselves
        assert [int(x) for x in hdeg] == [max((k for k in range(d + 1) if r[k]), default=0) for r in coeffs]
    finally:
        for q in (d_c, d_o, d_co, d_deg, d_c0, d_deg2):
            eng.dev_free(q)


DECODES = {"fast": (8192, True, 65536, False), "lane": (0, False, 0, False), "mfma": (0, True, 1, False), "generic": (8192, True, 65536, True)}


@pytest.mark.parametrize("mode", list(DECODES))
@pytest.mark.parametrize("m,d", [(6, 5), (16, 5)])
def test_batch_interpolate(fe, mode, m, d):
    """S in {d + 1, d + 2, m}, G in {1, 65, 257} (and 2 100 columns once: the matrix cores' own range), row_stride > G, one column
    lifted off its polynomial: degree_out exceeds d there and nowhere else; the c0 form against the full form"""
    field, eng = fe
    spec = SPEC[field]
    p = spec.R_MOD
    small, mc, mn, fg = DECODES[mode]
    eng.set_small_batch_chunks(small)
    eng.set_matrix_cores(mc, mn)
    eng.set_force_generic(fg)
    rng = random.Random(31 * m + d)
    pts = PTS16[:m]
    eb = eng.ebytes
    for S in sorted(x for x in {d + 1, d + 2, m} if x <= m):   # at (6, 5) there is no seventh point
        for G in (1, 65, 257) + ((2100,) if S == d + 1 and m == 6 else ()):
            sub = pts[m - S:]                                  # not a prefix either
            polys = [[rng.randrange(p) for _ in range(d)] + [rng.randrange(1, p)] for _ in range(G)]
            evals = [[spec.p_eval(c, x) for c in polys] for x in sub]   # [S][G]
            lifted = G // 2
            evals[S - 1][lifted] = (evals[S - 1][lifted] + 1) % p
            stride = G + 3
            buf = np.zeros((S, stride) + ((4,) if field == "fr" else ()), dtype=np.uint64)
            buf[:, :G] = arr(field, [v for row in evals for v in row], (S, G))
            want_co, want_deg = M.batch_interpolate(spec, sub, evals)
            d_e, d_co, d_deg, d_c0, d_deg2 = dev_buf(eng, buf), eng.dev_alloc(G * S * eb), eng.dev_alloc(G * 4), eng.dev_alloc(G * eb), eng.dev_alloc(G * 4)
            try:
                assert eng.dev_shamir_batch_interpolate(sub, d_e, stride, G, d_co, d_deg) == 0, eng.last_error()
                eng.sync()
                co, deg = fetch(eng, d_co, (G, S) + ((4,) if field == "fr" else ())), fetch(eng, d_deg, (G,), np.uint32)
                assert ints(field, co) == [x for r in want_co for x in r], (S, G)
                assert [int(x) for x in deg] == want_deg
                if S > d + 1:
                    assert [g for g in range(G) if deg[g] > d] == [lifted] and deg[lifted] == S - 1
                else:
                    assert all(x <= d for x in deg)
                assert eng.dev_shamir_batch_interpolate_c0(sub, d_e, stride, G, d_co, d_c0, d_deg2) == 0
                eng.sync()
                assert np.array_equal(fetch(eng, d_c0, co[:, 0].shape), co[:, 0]) and np.array_equal(fetch(eng, d_deg2, (G,), np.uint32), deg)
            finally:
                for q in (d_e, d_co, d_deg, d_c0, d_deg2):
                    eng.dev_free(q)


def test_interpolate_and_recover_refusals(fe):
    field, eng = fe
    spec = SPEC[field]
    c = [5, 6, 7]
    ids = [1, 2, 3, 4]
    vals = M.compute_shares(spec, c, 2, ids)
    ev = lambda n: arr(field, vals[:n], (n, 1))
    bi = lambda pts: eng.shamir_batch_interpolate(pts, ev(len(pts)))[0]
    assert bi([1, 2, 3]) == 0 and bi([1, 1, 2]) == 4 and bi([0, 1, 2]) == 4
    rs = lambda i, dg, v: eng.shamir_recover_secret(i, dg, arr(field, v, (len(v),)))
    assert rs([], [], [])[0] == 4                                             # 1. no shares
    assert rs([1, 1, 2], [2, 3, 2], vals[:3])[0] == 4                         # 2. duplicate ids, before 3
    assert rs([1, 2], [5, 2], vals[:2])[0] == 2                               # 3. unequal degrees, before 4
    assert rs([0, 2], [2, 2], vals[:2])[0] == 1                               # 4. too few, before 5
    assert rs([0, 2, 3], [2, 2, 2], vals[:3])[0] == 4                         # 5. a zero id
    bad = list(vals)
    bad[3] = (bad[3] + 1) % spec.R_MOD
    assert rs(ids, [2] * 4, bad)[0] == 2                                      # 7. interpolated degree beyond the shares'
    rc, co, sec = rs(ids, [2] * 4, vals)
    assert rc == 0 and ints(field, co) == c and ints(field, sec) == [5]
    rc, co, sec = rs([1, 2, 3], [2] * 3, [0, 0, 0])                           # the zero polynomial: length 0, secret 0
    assert rc == 0 and len(co) == 0 and ints(field, sec) == [0]
    if field == "goldilocks":
        assert bi([1, P_GL + 1]) == 4 and bi([P_GL, 2]) == 4
        assert rs([1, P_GL + 1], [1, 1], [7, 7])[0] == 4                      # 6. one field element twice
        assert rs([1, P_GL + 1], [1, 2], [7, 7])[0] == 2                      # ... after 3
        assert rs([1, P_GL + 1, P_GL], [1, 1, 1], [7, 7, 7])[0] == 4
    # the model agrees on every code
    for i, dg, v in (([1, 1, 2], [2, 3, 2], vals[:3]), ([1, 2], [5, 2], vals[:2]), ([0, 2], [2, 2], vals[:2]), (ids, [2] * 4, bad)):
        with pytest.raises(spec.ShareErr) as e:
            M.recover_secret(spec, i, dg, v)
        assert e.value.code == rs(i, dg, v)[0]


@pytest.mark.parametrize("ids", [[1, 2, 3, 4, 5, 6], [1, 2, 3, 4, 5, 6, 7, 20]])
def test_add_and_scalar_multiply_then_open(fe, ids):
    """the field halves of feldman.rs:311-427: shares of a and b at the reference's own points, a + b and 3 a share by share with the
    element-wise calls, each opened by the batched interpolation"""
    field, eng = fe
    spec = SPEC[field]
    p = spec.R_MOD
    rng = random.Random(len(ids))
    B, d = 65, 2
    A = [[rng.randrange(p) for _ in range(d + 1)] for _ in range(B)]
    Bc = [[rng.randrange(p) for _ in range(d + 1)] for _ in range(B)]
    rc, sa = eng.shamir_compute_shares(arr(field, [x for r in A for x in r], (B, d + 1)), ids, d)
    rc2, sb = eng.shamir_compute_shares(arr(field, [x for r in Bc for x in r], (B, d + 1)), ids, d)
    assert rc == 0 and rc2 == 0
    flat = lambda a: a.reshape((-1,) + a.shape[2:])
    rc, ssum = eng.fr_op("add", flat(sa), flat(sb))
    assert rc == 0
    rc, s3 = eng.fr_op_scalar("mul", flat(sa), arr(field, [3], (1,))[0])
    assert rc == 0
    for got, want in ((ssum, [[(x + y) % p for x, y in zip(r, q)] for r, q in zip(A, Bc)]), (s3, [[3 * x % p for x in r] for r in A])):
        rc, co, deg = eng.shamir_batch_interpolate(ids, got.reshape(sa.shape))
        assert rc == 0
        co = ints(field, co)
        S = len(ids)
        for b in range(B):
            assert co[b * S:b * S + d + 1] == want[b] and not any(co[b * S + d + 1:(b + 1) * S]) and deg[b] <= d


def test_cache_keeps_domain_ids_and_integer_points_apart(fe):
    """the integer points [1, 2, 3] and the domain ids [1, 2, 3] on one context, alternating, twice each: each against its own model"""
    field, eng = fe
    spec = SPEC[field]
    p = spec.R_MOD
    rng = random.Random(5)
    G, n = 65, 4
    polys = [[rng.randrange(p) for _ in range(3)] for _ in range(G)]
    at_points = [[spec.p_eval(c, x) for c in polys] for x in (1, 2, 3)]
    at_domain = [[spec.p_eval(c, spec.domain_element(n, j)) for c in polys] for j in (1, 2, 3)]
    want = [x for c in polys for x in c]
    e_pts, e_dom = dev_buf(eng, arr(field, [v for r in at_points for v in r], (3, G))), dev_buf(eng, arr(field, [v for r in at_domain for v in r], (3, G)))
    d_co, d_deg = eng.dev_alloc(G * 3 * eng.ebytes), eng.dev_alloc(G * 4)
    shape = (G, 3) + ((4,) if field == "fr" else ())
    try:
        for _ in range(2):
            assert eng.dev_batch_interpolate([1, 2, 3], e_dom, G, G, n, d_co, d_deg) == 0
            eng.sync()
            assert ints(field, fetch(eng, d_co, shape)) == want
            assert eng.dev_shamir_batch_interpolate([1, 2, 3], e_pts, G, G, d_co, d_deg) == 0
            eng.sync()
            assert ints(field, fetch(eng, d_co, shape)) == want
        # and the wrong pairing is a different polynomial: the two point sets are not the same numbers
        assert eng.dev_shamir_batch_interpolate([1, 2, 3], e_dom, G, G, d_co, d_deg) == 0
        eng.sync()
        assert ints(field, fetch(eng, d_co, shape)) != want
    finally:
        for q in (e_pts, e_dom, d_co, d_deg):
            eng.dev_free(q)
