"""hbmpc_dev_take_rows (csrc/kernels_take.hpp: a contiguous run of tile * group elements through LDS, `group` runs out; a group beyond
64 through k_transpose) called directly on both fields against numpy, bit for bit: group sizes on both routes, element counts below, at
and above one tile, one and sixteen rows, sources that start 1 and 3 elements into their buffer (no 128-byte alignment), padded strides
with a sentinel in every cell of the destination that is not written, eight slices of different shapes in one call, and refused calls,
which leave a sentinel-filled destination untouched."""
import numpy as np
import pytest

from __graft_entry__ import load_package
from tests import fixedprep_ref as FR

pytestmark = pytest.mark.gpu
SENTINEL = np.uint64(0xC3C3C3C3C3C3C3C3)
TRANSPOSE_GROUP = 100                                     # beyond the tile's 64: the transpose route


@pytest.fixture(scope="module", params=["fr", "goldilocks"])
def eng(request):
    e = load_package().Engine(0, field=request.param)
    yield e
    e.close()


def tail(eng):
    return (4,) if eng.field == "fr" else ()


def tile(eng, group):
    """the take kernel's i per workgroup (csrc/take_plan.hpp, pinned by tests/test_take_routes.py); the transpose's 16 beyond it"""
    return 512 // eng.ebytes * min(8, 64 // group) if group <= 64 else 16


def run(eng, specs, rows, seed, spoil=None):
    """specs: [(elements, group, source offset, source pad, destination pad)].  One call for all of them -> (rc, [(got, want)]), every
    destination prefilled with the sentinel.  spoil(slices): edits the slice list before the call (the refusals)."""
    rng = np.random.default_rng(seed)
    bufs, slices, pairs = [], [], []
    try:
        for elements, group, off, spad, dpad in specs:
            srs, drs = elements + spad, elements + dpad
            src = rng.integers(0, 1 << 64, size=(off + rows * srs,) + tail(eng), dtype=np.uint64)
            dst = np.full((rows * drs + 5,) + tail(eng), SENTINEL, dtype=np.uint64)
            sd, dd = eng.dev_alloc(max(src.nbytes, 64)), eng.dev_alloc(max(dst.nbytes, 64))
            bufs += [sd, dd]
            eng.h2d(sd, src)
            eng.h2d(dd, dst)
            slices.append([sd + off * eng.ebytes, srs, dd, drs, elements, group])
            pairs.append((dst, FR.take_rows_np(src[off:], rows, srs, dst.copy(), drs, elements, group), dd))
        if spoil:
            spoil(slices)
        rc = eng.take_rows(slices, rows)
        for dst, _, dd in pairs:
            eng.d2h(dst, dd)
        eng.sync()
    finally:
        for b in bufs:
            eng.dev_free(b)
    return rc, [(got, want) for got, want, _ in pairs]


@pytest.mark.parametrize("group", [1, 2, 3, 16, 17, 64, TRANSPOSE_GROUP])
def test_take_against_numpy(eng, group):
    T = tile(eng, group)
    for C in (1, T - 1, T, T + 1):
        if C < 1:
            continue
        for rows in (1, 16):
            for off, spad, dpad in ((0, 0, 0), (1, 3, 1), (3, 0, 2)):
                rc, res = run(eng, [(C * group, group, off, spad, dpad)], rows, group * 1000 + C)
                assert rc == 0, eng.last_error()
                got, want = res[0]
                assert np.array_equal(got, want), (eng.field, group, C, rows, off, spad, dpad, np.argwhere(got != want)[:4].tolist())


def test_eight_slices_of_different_shapes_in_one_call(eng):
    specs = [(1, 1, 0, 0, 0), (7 * 3, 3, 1, 2, 0), (130 * 16, 16, 3, 0, 1), (600, 1, 1, 1, 1), (17 * 17, 17, 0, 5, 0), (64 * 33, 64, 1, 0, 3),
             (TRANSPOSE_GROUP * 19, TRANSPOSE_GROUP, 3, 1, 0), (2 * 1025, 2, 0, 0, 0)]
    rc, res = run(eng, specs, 5, 8)
    assert rc == 0, eng.last_error()
    for spec, (got, want) in zip(specs, res):
        assert np.array_equal(got, want), (eng.field, spec)


def test_refused_calls_write_nothing(eng):
    """every refusal of the header's list: InvalidInput (4) and sentinel-filled destinations -- also the first slice's, when it is the
    second that is wrong (all checks come before the launch)"""
    specs = [(48, 4, 0, 2, 2), (30, 3, 1, 0, 0)]

    def setter(i, field, value):
        def spoil(slices):
            slices[i][field] = value
        return spoil
    SRC, SRS, DST, DRS, EL, GR = range(6)
    bad = [setter(1, SRC, None), setter(1, DST, None), setter(0, SRC, None), setter(1, EL, 0), setter(1, GR, 0), setter(1, GR, 4),   # 30 % 4 != 0
           setter(1, SRS, 29), setter(1, DRS, 29), setter(0, DRS, 47)]
    for k, spoil in enumerate(bad):
        rc, res = run(eng, specs, 3, 100 + k, spoil)
        assert rc == 4, (k, rc)
        for got, _ in res:
            assert (got == SENTINEL).all(), k
    rc, res = run(eng, [(4, 1, 0, 0, 0)] * 9, 1, 300)                                              # nine slices; none
    assert rc == 4 and all((got == SENTINEL).all() for got, _ in res)
    assert eng.take_rows([], 1) == 4
    # rows = 0 (and past the grid): refused with the buffers of a valid one-row call
    for rows in (0, 65536):
        dst = np.full((48,) + tail(eng), SENTINEL, dtype=np.uint64)
        src = np.zeros((48,) + tail(eng), dtype=np.uint64)
        sd, dd = eng.dev_alloc(src.nbytes), eng.dev_alloc(dst.nbytes)
        try:
            eng.h2d(sd, src)
            eng.h2d(dd, dst)
            assert eng.take_rows([[sd, 48, dd, 48, 48, 4]], rows) == 4
            eng.d2h(dst, dd)
            eng.sync()
        finally:
            eng.dev_free(sd)
            eng.dev_free(dd)
        assert (dst == SENTINEL).all(), rows
    rc, res = run(eng, specs, 3, 400)                                                              # and the same specs do run
    assert rc == 0 and all(np.array_equal(got, want) for got, want in res)
