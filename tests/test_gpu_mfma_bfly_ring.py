"""The ring form of the plain chunk-major point-pair encode (csrc/kernels_mfma_bfly_ring.hpp: a loader wave per workgroup fills an LDS
ring with whole lines, the other waves compute), bit for bit against the oracle.  Eight workgroups -- the smallest grid, where the
route hands this executor every batch of 17 tiles or more -- so that few tiles reach every state of the ring: compute waves with no
tile, with exactly one, one slot round per workgroup and one more or less, two rounds and more.  By default the library takes the
ring form only from four tiles per compute wave on (bfly_ring_min_tiles: below that it is slower), which with 8 workgroups is 384
tiles, so these tests switch it on at every size (hbmpc_set_matrix_cores mode 5); the default rule is run on both sides of its
threshold as well.  One seeded input of the largest G per shape and its oracle result, computed once; the cases are prefixes of it
(an output column does not depend on G).  Outputs go through the strided call into rows G + 8 apart prefilled with -1: the guards
must stay.  Also: modes 1, 4 (the same pairs with every wave gathering its own inputs) and 5 give the same bytes, and three calls
back to back on one stream with no sync between them are each right (no flag or slot state survives a launch)."""
import numpy as np
import pytest

from __graft_entry__ import load_package
from oracle import cref as O

pytestmark = pytest.mark.gpu

O_R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
CW = S = 12   # BFLY_RING_LIB of csrc/bfly_ring_plan.hpp: compute waves and slots per workgroup
WGS = 8
RING_ALWAYS, RING_BY_SIZE, RING_NEVER = 5, 1, 4   # hbmpc_set_matrix_cores modes
MIN_TILES_PER_WAVE = 4   # bfly_ring_min_tiles


@pytest.fixture(scope="module")
def eng():
    e = load_package().Engine(0)
    e.set_small_batch_chunks(0)
    e.set_matrix_cores(RING_ALWAYS, 1)
    yield e
    e.close()


def polys(seed, G, d):
    x = O.fill_random(seed, G * (d + 1)).reshape(G, d + 1, 4)
    x[0] = 0
    x[1] = O.ints_to_u256([O_R - 1] * (d + 1))
    x[2, :, :] = 0
    x[2, d, 0] = 1
    x[3] = O.ints_to_u256([(O_R - 1) if i & 1 else 0 for i in range(d + 1)])   # the odd half alone at its maximum
    x[4] = O.ints_to_u256([0 if i & 1 else (O_R - 1) for i in range(d + 1)])   # the even half alone
    return x


class Case:
    """one seeded input of gmax chunks on the device with the oracle's result; check(G) encodes the first G chunks"""

    def __init__(self, eng, seed, n, d, gmax):
        import torch
        self.eng, self.n, self.d, self.gmax = eng, n, d, gmax
        self.dev = torch.device("cuda", 0)
        x = polys(seed, gmax, d)
        rc0, y0 = O.vandermonde_apply(x, n, d)
        assert rc0 == 0
        self.x = torch.as_tensor(x.view(np.int64), device=self.dev).contiguous()
        self.want = torch.as_tensor(np.ascontiguousarray(y0).view(np.int64), device=self.dev)   # [n][gmax][4]
        torch.cuda.synchronize()

    def alloc(self, G):
        import torch
        y = torch.full((self.n, G + 8, 4), -1, dtype=torch.int64, device=self.dev)
        torch.cuda.synchronize()
        return y

    def launch(self, G, y=None):
        y = self.alloc(G) if y is None else y
        assert self.eng.dev_vandermonde_apply_strided(self.x.data_ptr(), G, self.n, self.d, y.data_ptr(), G + 8, 0) == 0
        return y

    def verify(self, y, G):
        import torch
        assert torch.equal(y[:, :G], self.want[:, :G]), (self.n, self.d, G)
        assert bool((y[:, G:] == -1).all()), (self.n, self.d, G)

    def check(self, G):
        y = self.launch(G)
        self.eng.sync()
        self.verify(y, G)


def sizes(tile_counts):
    """G = 32 T - r with r cycling through 0, 1, 31: the last tile whole, one chunk short, one chunk long"""
    return [32 * T - (0, 1, 31)[i % 3] for i, T in enumerate(tile_counts)]


@pytest.fixture()
def few_workgroups(eng):
    eng.set_matrix_core_workgroups(WGS)
    yield eng
    eng.set_matrix_core_workgroups(0)


def test_every_tile_count_of_the_headline_shape(few_workgroups):
    """(n, d) = (16, 5), 8 pairs: every tile count from 17 (the first this kernel gets) to 8 (2 S + CW) + 1"""
    counts = list(range(17, WGS * (2 * S + CW) + 2))
    # what the range is there for: waves without a tile and with exactly one, S - 1, S and S + 1 tiles in a workgroup, beyond 2 S
    assert 17 < WGS * CW and WGS * S - 1 in counts and WGS * S + 1 in counts and WGS * 2 * S + 1 in counts
    case = Case(few_workgroups, 0x52494E47, 16, 5, 32 * counts[-1])
    for G in sizes(counts):
        case.check(G)


@pytest.mark.parametrize("n,d", [(9, 1), (12, 7), (8, 3)])
def test_other_shapes(few_workgroups, n, d):
    """two and eight coefficients on 16 points (d + 1 = 8: table and ring do not fit the LDS together, the gathering kernel runs) and
    a domain of 8 points, whose role has 4 pairs"""
    counts = [17, WGS * CW - 1, WGS * CW + 1, WGS * S - 1, WGS * S + 1, WGS * 2 * S + 5]
    case = Case(few_workgroups, 0x52494E47 + 64 * n + d, n, d, 32 * max(counts))
    for G in sizes(counts):
        case.check(G)


@pytest.mark.parametrize("G,wgs", [(40017, WGS), (16613, 0)])
def test_same_bytes_in_every_mode(eng, G, wgs):
    """by size (40 017 chunks on 8 workgroups: the ring form; 16 613 on the default grid: not), never and always"""
    import torch
    case = Case(eng, 0x52494E47 + G, 16, 5, G)
    eng.set_matrix_core_workgroups(wgs)
    try:
        ys = []
        for mode in (RING_BY_SIZE, RING_NEVER, RING_ALWAYS):
            eng.set_matrix_cores(mode, 1)
            y = case.launch(G)
            eng.sync()
            case.verify(y, G)
            ys.append(y)
        assert torch.equal(ys[0], ys[1]) and torch.equal(ys[0], ys[2])
    finally:
        eng.set_matrix_cores(RING_ALWAYS, 1)
        eng.set_matrix_core_workgroups(0)


def test_default_rule_on_both_sides_of_its_threshold(few_workgroups):
    """the tile counts around four per compute wave, where the default switches forms"""
    edge = MIN_TILES_PER_WAVE * WGS * CW
    counts = [edge - 1, edge, edge + 1]
    case = Case(few_workgroups, 0x52494E47 + edge, 16, 5, 32 * max(counts))
    few_workgroups.set_matrix_cores(RING_BY_SIZE, 1)
    try:
        for G in sizes(counts):
            case.check(G)
    finally:
        few_workgroups.set_matrix_cores(RING_ALWAYS, 1)


def test_three_calls_back_to_back(few_workgroups):
    """different inputs and sizes on one stream, no sync between the launches: each result is right"""
    cases = [Case(few_workgroups, 0x52494E47 + 7 * k, 16, 5, G) for k, G in enumerate((32 * 150 - 1, 32 * 97, 32 * 290 - 31))]
    ys = [c.alloc(c.gmax) for c in cases]
    for c, y in zip(cases, ys):
        c.launch(c.gmax, y)
    few_workgroups.sync()
    for c, y in zip(cases, ys):
        c.verify(y, c.gmax)
