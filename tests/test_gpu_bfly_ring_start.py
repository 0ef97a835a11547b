"""The start of the ring encode (csrc/kernels_mfma_bfly_ring.hpp): the loader wave requests its first D = 4 tiles BEFORE the barrier
and takes no part in the table copy; the compute waves copy the table with all of a thread's loads ahead of its first LDS write.
What can go wrong there is a matter of how many items a workgroup has -- none (it must still reach the barrier), fewer than D (nothing
is published before the final wait), exactly D, D + 1, S = 12 and S + 1 (the first wait for a freed slot) -- and of the clamped last
tile.  hbmpc_set_matrix_cores mode 5 asks for the ring form at every size, mode 4 for the same pairs with every wave gathering its own
inputs: the two must agree byte for byte, and the first <= 4096 secrets must be what oracle.cref.compute_shares gives.

Which sizes reach the kernel.  The route (csrc/encode_route.hpp) hands a batch to the point-pair executor from 2 tiles per workgroup
on, and a grid has at least 8 workgroups, so through the library the ring kernel sees G >= 513 (17 tiles) and nothing below: at
G = 1, 31, 32, 33, 383 and 385 both modes run the small-batch kernels, and these cases check only that mode 5 changes nothing
there.  The kernel itself runs G = 1, 31, 32, 33, 95, 97, 129, 383, 385 and 543 in tools/ubench_bfly_ring (`edges`), compared with the
gathering kernel.  On 8 workgroups, workgroup w owns tiles 12 w .. 12 w + 11 of the first 96, so the sizes below beyond the issue's
list put the states above into a workgroup that the library does launch: 17 tiles (G = 543): 12, 5 and six times no item; 27, 28 and
29 tiles: 3, 4 and 5 items in workgroup 2; 97 tiles: 13 in workgroup 0.  Likewise M = 9 on 4 pairs is instantiated but cannot be
asked for: 4 pairs mean n <= 8, and n > d is required, so (8, 7), M = 8, is the largest 4-pair table a call can reach.

One seeded input per shape with the oracle's result for its first 4096 chunks, computed once; the sizes are prefixes of it (an output
column does not depend on G).  The visibility cases: batch_recover of the shares right behind compute_shares, on the same stream
with no host sync between them and on a second stream behind an event, must return the coefficients with status 0 -- the row stores'
cache policy must leave them visible to the next kernel."""
import numpy as np
import pytest

from __graft_entry__ import load_package
from oracle import cref as O

pytestmark = pytest.mark.gpu

RING_ALWAYS, RING_NEVER = 5, 4   # hbmpc_set_matrix_cores modes
WGS = 8
ORACLE_MAX = 4096
ISSUE_SIZES = [1, 31, 32, 33, 383, 385, 543, 16613, 40017]
STATE_SIZES = [32 * 27 - 1, 32 * 28, 32 * 28 + 1, 32 * 96 + 1]   # on 8 workgroups: 3, 4, 5 items in workgroup 2; 13 in workgroup 0
SHAPES = [(16, 5), (8, 3), (16, 6), (8, 7)]   # M = 6 on 8 pairs; 4 pairs; M = 7, the largest 8-pair table; M = 8, the largest reachable 4-pair one
GMAX = max(ISSUE_SIZES + STATE_SIZES)


@pytest.fixture(scope="module")
def eng():
    e = load_package().Engine(0)
    e.set_small_batch_chunks(0)
    yield e
    e.set_matrix_cores(1, 65536)
    e.set_matrix_core_workgroups(0)
    e.close()


_inputs = {}


def shape_input(n, d):
    """(coefficients on the device, the oracle's shares of the first ORACLE_MAX chunks on the device); never modified"""
    import torch
    if (n, d) not in _inputs:
        dev = torch.device("cuda", 0)
        x = O.fill_random(0x57A27 + 64 * n + d, GMAX * (d + 1)).reshape(GMAX, d + 1, 4)
        x[0] = 0
        rc, want = O.compute_shares(x[:ORACLE_MAX], n, d)
        assert rc == 0
        _inputs[(n, d)] = (torch.as_tensor(x.view(np.int64), device=dev).contiguous(),
                           torch.as_tensor(np.ascontiguousarray(want).view(np.int64), device=dev))
        torch.cuda.synchronize()
    return _inputs[(n, d)]


def encode(eng, mode, x, G, n, d):
    """[n][G + 8][4] with the guard columns left at -1"""
    import torch
    y = torch.full((n, G + 8, 4), -1, dtype=torch.int64, device=x.device)
    torch.cuda.synchronize()
    eng.set_matrix_cores(mode, 1)
    assert eng.dev_vandermonde_apply_strided(x.data_ptr(), G, n, d, y.data_ptr(), G + 8, 0) == 0
    eng.sync()
    return y


def check(eng, n, d, G):
    import torch
    x, want = shape_input(n, d)
    ring = encode(eng, RING_ALWAYS, x, G, n, d)
    gather = encode(eng, RING_NEVER, x, G, n, d)
    assert torch.equal(ring, gather), (n, d, G)
    k = min(G, ORACLE_MAX)
    assert torch.equal(ring[:, :k], want[:, :k]), (n, d, G)
    assert bool((ring[:, G:] == -1).all()), (n, d, G)


@pytest.mark.parametrize("n,d", SHAPES)
def test_ring_start_on_the_default_grid(eng, n, d):
    """one workgroup per CU: at 16 613 and 40 017 chunks most workgroups have two or three items, fewer than D"""
    eng.set_matrix_core_workgroups(0)
    for G in ISSUE_SIZES:
        check(eng, n, d, G)


@pytest.mark.parametrize("n,d", SHAPES)
def test_ring_start_on_eight_workgroups(eng, n, d):
    """the smallest grid: 0, 3, 4, 5, 12 and 13 items in a workgroup, and 13 rounds of the ring at 40 017 chunks"""
    eng.set_matrix_core_workgroups(WGS)
    try:
        for G in ISSUE_SIZES + STATE_SIZES:
            check(eng, n, d, G)
    finally:
        eng.set_matrix_core_workgroups(0)


@pytest.mark.parametrize("second_stream", [False, True])
def test_shares_are_visible_to_the_next_kernel(eng, second_stream):
    """dev_compute_shares by the ring kernel, then dev_batch_recover of those shares with no host sync in between"""
    import torch
    n, d, t, G = 16, 5, 5, 40017
    dev = torch.device("cuda", 0)
    x, _ = shape_input(n, d)
    eng.set_matrix_core_workgroups(WGS)
    eng.set_matrix_cores(RING_ALWAYS, 1)
    try:
        sh = torch.full((n, G, 4), -1, dtype=torch.int64, device=dev)
        co = torch.full((G, d + 1, 4), -1, dtype=torch.int64, device=dev)
        st = torch.full((G,), 255, dtype=torch.uint8, device=dev)
        producer = torch.cuda.Stream(device=dev)
        consumer = torch.cuda.Stream(device=dev) if second_stream else producer
        torch.cuda.synchronize()
        assert eng.dev_compute_shares(x.data_ptr(), G, n, d, sh.data_ptr(), stream=producer.cuda_stream) == 0
        if second_stream:
            done = torch.cuda.Event()
            done.record(producer)
            consumer.wait_event(done)
        assert eng.dev_batch_recover(list(range(n)), sh.data_ptr(), G, n, d, t, co.data_ptr(), 0, st.data_ptr(),
                                     stream=consumer.cuda_stream) == 0
        eng.sync(consumer.cuda_stream)
        torch.cuda.synchronize()
        assert bool((st == 0).all())
        assert torch.equal(co, x[:G])
    finally:
        eng.set_matrix_cores(1, 65536)
        eng.set_matrix_core_workgroups(0)
