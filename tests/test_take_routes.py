"""Which route a slice of hbmpc_dev_take_rows takes and the tile the take kernel moves: the rule (mpc-protocols_amd/csrc/take_plan.hpp)
compiled for the CPU under ASan + UBSan (tests/cpp/take_routes_dump.cpp).  The GPU test compares both routes with numpy, so a slip that
sends every slice through the transpose passes it; this pins the rule.  Runs without a GPU.

The rule, from the kernel's LDS budget: a tile is a contiguous source run of tile * group elements; the LDS holds 512 bytes x 64 of them,
a full tile writes `group` runs of at least 512 bytes, a small group gets up to eight such runs per workgroup, and a group beyond 64 does
not fit and takes the transpose."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "take_routes_dump")


@pytest.fixture(scope="module")
def plan():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "cpp"), "-f", "take.mk"], stdout=subprocess.DEVNULL)

    def run(queries):
        text = "".join("%d %d\n" % q for q in queries)
        p = subprocess.run([BIN], input=text, capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, p.stderr[-2000:]          # ASan / UBSan findings abort with a non-zero code
        lines = p.stdout.splitlines()
        assert len(lines) == len(queries)
        return dict(zip(queries, lines))
    return run


def rule(eb, group):
    if group > 64:
        return "transpose"
    return "take tile=%d" % (512 // eb * min(8, 64 // group))


# derived by hand from the rule above
ANCHORS = [((32, 1), "take tile=128"), ((32, 8), "take tile=128"), ((32, 9), "take tile=112"), ((32, 16), "take tile=64"),
           ((32, 17), "take tile=48"), ((32, 32), "take tile=32"), ((32, 33), "take tile=16"), ((32, 64), "take tile=16"),
           ((32, 65), "transpose"), ((32, 4096), "transpose"),
           ((8, 1), "take tile=512"), ((8, 3), "take tile=512"), ((8, 16), "take tile=256"), ((8, 64), "take tile=64"), ((8, 65), "transpose")]


def test_anchors(plan):
    got = plan([q for q, _ in ANCHORS])
    for q, want in ANCHORS:
        assert got[q] == want and rule(*q) == want, (q, got[q])


def test_grid(plan):
    queries = [(eb, g) for eb in (8, 32) for g in list(range(1, 200)) + [4095, 4096, 4097, 1 << 20]]
    for q, line in plan(queries).items():
        assert line == rule(*q), (q, line)


def test_limits_fit_the_kernel():
    """8 slices (the kernel's argument array), groups up to 64, rows in the grid's y, and no tile beyond the kernel's LDS array"""
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "cpp"), "-f", "take.mk"], stdout=subprocess.DEVNULL)
    out = subprocess.run([BIN, "limits"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr[-2000:]
    slices, group, rows, lds = map(int, out.stdout.split())
    assert (slices, group, rows) == (8, 64, 65535)
    assert lds == 512 * 64 + 512 * 8 and lds <= 64 * 1024     # elements + a padding word per i of the longest tile; static LDS
