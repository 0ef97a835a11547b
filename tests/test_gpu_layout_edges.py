"""hbmpc_dev_transpose (csrc/kernels_codec.hpp: k_transpose<W>, a 16 x 64 tile through LDS) called directly on both fields against
numpy.swapaxes: shapes below, at and above one tile in either direction, padded row strides, batches at strides larger than one matrix,
one source broadcast to every batch, a sentinel in every cell of the destination that is not written, and the argument checks."""
import numpy as np
import pytest

from __graft_entry__ import load_package

pytestmark = pytest.mark.gpu
SENTINEL = np.uint64(0xC3C3C3C3C3C3C3C3)


@pytest.fixture(scope="module", params=["fr", "goldilocks"])
def eng(request):
    e = load_package().Engine(0, field=request.param)
    yield e
    e.close()


def tail(eng):
    return (4,) if eng.field == "fr" else ()


def transpose(eng, src, rows, cols, srs, drs, batch, sbs, dbs, dst_len):
    """-> (rc, the whole destination buffer of dst_len elements, prefilled with the sentinel)"""
    dst = np.full((dst_len,) + tail(eng), SENTINEL, dtype=np.uint64)
    sd, dd = eng.dev_alloc(max(src.nbytes, 64)), eng.dev_alloc(max(dst.nbytes, 64))
    try:
        eng.h2d(sd, src)
        eng.h2d(dd, dst)
        rc = eng.dev_transpose(sd, rows, cols, srs, dd, drs, batch, sbs, dbs)
        eng.d2h(dst, dd)
        eng.sync()
    finally:
        eng.dev_free(sd)
        eng.dev_free(dd)
    return rc, dst


def expected(eng, src, rows, cols, srs, drs, batch, sbs, dbs, dst_len):
    want = np.full((dst_len,) + tail(eng), SENTINEL, dtype=np.uint64)
    for b in range(batch):
        m = src[b * sbs: b * sbs + rows * srs].reshape((rows, srs) + tail(eng))[:, :cols]
        view = want[b * dbs: b * dbs + cols * drs].reshape((cols, drs) + tail(eng))
        view[:, :rows] = np.swapaxes(m, 0, 1)
    return want


@pytest.mark.parametrize("rows,cols", [(1, 1), (15, 63), (16, 64), (17, 65), (33, 130), (7, 300), (300, 7)])
def test_transpose_against_numpy(eng, rows, cols):
    rng = np.random.default_rng(rows * 1000 + cols)
    for pad in (0, 3):
        srs, drs = cols + pad, rows + pad
        for batch, broadcast in ((1, False), (3, False), (3, True)):
            sbs = 0 if broadcast else rows * srs + 5          # batch strides larger than one matrix (or one source for every batch)
            dbs = cols * drs + 7
            src_len = (0 if broadcast else (batch - 1) * sbs) + rows * srs
            dst_len = (batch - 1) * dbs + cols * drs + 9
            src = rng.integers(0, 1 << 64, size=(src_len,) + tail(eng), dtype=np.uint64)
            rc, got = transpose(eng, src, rows, cols, srs, drs, batch, sbs, dbs, dst_len)
            assert rc == 0, eng.last_error()
            want = expected(eng, src, rows, cols, srs, drs, batch, sbs, dbs, dst_len)
            assert np.array_equal(got, want), (eng.field, rows, cols, pad, batch, broadcast, np.argwhere(got != want)[:4].tolist())


def test_transpose_argument_checks(eng):
    rows, cols = 17, 65
    src = np.arange(rows * cols * (4 if eng.field == "fr" else 1), dtype=np.uint64).reshape((rows * cols,) + tail(eng))
    n = rows * cols
    untouched = np.full((n,) + tail(eng), SENTINEL, dtype=np.uint64)
    for srs, drs, batch in ((cols - 1, rows, 1), (cols, rows - 1, 1), (cols, rows, 65536)):   # a row stride below the row length; a batch past the grid
        rc, got = transpose(eng, src, rows, cols, srs, drs, batch, 0, 0, n)
        assert rc == 4 and np.array_equal(got, untouched), (srs, drs, batch, rc)
    for r, c, b in ((0, cols, 1), (rows, 0, 1), (rows, cols, 0)):                            # nothing to do: success, nothing written
        rc, got = transpose(eng, src, r, c, cols, rows, b, 0, 0, n)
        assert rc == 0 and np.array_equal(got, untouched), (r, c, b, rc)
    rc, got = transpose(eng, src, rows, cols, cols, rows, 1, 0, 0, n)                        # and the same buffers do transpose
    assert rc == 0 and np.array_equal(got, expected(eng, src, rows, cols, cols, rows, 1, 0, 0, n))
