"""Which kernel an encode takes: the route planner (mpc-protocols_amd/csrc/encode_route.hpp) compiled for the CPU under ASan + UBSan
(tests/cpp/encode_routes_dump.cpp) over a grid of shapes and knob settings.  The GPU tests compare bytes, and every route gives the
same bytes; this pins the routes themselves -- the headline shape on the point-pair kernel, the producers' dealers in one launch, the
lists written by the kernel.  Runs without a GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "encode_routes_dump")
KNOBS = ["default", "mc0", "mc1,min1", "mc2", "mc3", "generic", "fusion0", "small0", "wgs8"]
NS = list(range(3, 18)) + [20, 31, 32, 40, 64, 100]


def ds(n):
    t = (n - 1) // 3
    return sorted({1, t, 2 * t, n - 1} & set(range(1, n)))


def gs(parties):
    """batch sizes at every threshold: the wave-per-chunk range (2 048 chunks over all parties), 512 tiles, 2^14, 2^20"""
    return sorted({g for g in (2048 // parties, 2048 // parties + 1, 2049, 16384, 16385, (1 << 14) // parties, 1 << 20) if g >= 1})


@pytest.fixture(scope="module")
def plan():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "cpp"), "encode_routes_dump"], stdout=subprocess.DEVNULL)

    def run(queries):
        text = "".join(" ".join(map(str, q)) + "\n" for q in queries)
        p = subprocess.run([BIN], input=text, capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stderr[-2000:]          # ASan / UBSan findings abort with a non-zero code
        lines = p.stdout.splitlines()
        assert len(lines) == len(queries)
        return dict(zip(queries, lines))
    return run


# (call, knobs, field, G, n, d, parties) -> the first route (kernel, M, pairs or rows per role, roles, one launch or one per party)
ANCHORS = [
    (("shares", "default", "fr", 1 << 20, 16, 5, 1), "Bfly M=6 rows=8 roles=1 one"),  # the headline: k_mfma_bfly<6,12,8>
    (("shares", "default", "fr", 1000, 16, 5, 1), "WideDot M=6"),
    (("shares", "default", "fr", 4096, 16, 5, 1), "MfmaRowsTeam M=6 rows=16 roles=1 one"),
    (("shares", "default", "fr", 15019, 16, 5, 16), "BflyParties M=6 rows=8 roles=1 one"),
    (("shares", "default", "fr", 1 << 20, 31, 10, 1), "Bfly M=11 rows=8 roles=2 one"),
    (("shares", "default", "gl", 1 << 20, 16, 5, 1), "Fft1 M=6"),
    (("shares", "default", "sat32", 1 << 20, 16, 5, 1), "Generic M=6"),
    (("shares", "mc3", "fr", 1 << 20, 16, 5, 1), "Fft1 M=6"),
    (("split", "default", "fr", 16 * 1500, 16, 15, 1), "BflyLists M=16 rows=8 roles=1 one lists_in_kernel=1"),
    (("split", "default", "fr", 7 * 367, 7, 6, 1), "Fft1Mix M=7 rows=0 roles=0 one lists_in_kernel=1"),
    (("triple", "default", "fr", 381300, 16, 10, 16), "BflyTriple M=11 rows=8 roles=1 one"),
    (("triple_ws", "default", "fr", 100, 16, 10, 16), "LocalProduct M=11 rows=0 roles=0 one>WideDot M=11"),
]


def test_anchor_routes(plan):
    queries = [tuple("lists" if c == "split" else c for c in q[:1]) + q[1:] for q, _ in ANCHORS]
    got = plan(queries)
    for (q, want), qq in zip(ANCHORS, queries):
        assert got[qq].startswith(want), (q, got[qq])


def test_grid_plans(plan):
    """every shape of the grid gets a plan that ends in a route that cannot decline, under every knob setting (a small batch: the
    wave-per-chunk kernel alone)"""
    queries = []
    for knobs in KNOBS:
        for field in ("fr", "gl", "sat32"):
            for n in NS:
                for d in ds(n):
                    for parties in (1, 2, 16, 65):
                        for G in gs(parties):
                            queries.append(("shares", knobs, field, G, n, d, parties))
                            if parties == 1:
                                queries.append(("strided", knobs, field, G, n, d, 1))
                                queries.append(("rows", knobs, field, G, n, d, 1))
                            if parties == 16:
                                queries.append(("triple", knobs, field, G, n, d, 16))
                                queries.append(("triple_ws", knobs, field, G, n, d, 16))
    got = plan(queries)
    ends = {"shares": "Generic", "strided": "Generic", "rows": "Transpose", "triple": "LocalProduct", "triple_ws": "LocalProduct"}
    for q, line in got.items():
        routes = line.split(" all=")[1].split(",")
        assert routes[-1] == ends[q[0]] or (q[0] in ("shares", "strided") and routes in (["WideDot"], ["Wide"])), (q, line)
        head = line.split(" all=")[0]
        first = head.split()[0]
        if q[1] == "generic":                               # force_generic: the generic kernel, after the workspace step where there is one
            assert first == "Generic" or (first in ("Transpose", "LocalProduct") and ">Generic" in head), (q, line)
        if q[2] == "sat32" and q[0] in ("shares", "strided"):
            assert first in ("Generic", "Wide"), (q, line)
        if q[1] == "mc0":                                   # matrix cores off: no matrix-core kernel
            assert not first.startswith(("Mfma", "Bfly")), (q, line)


def test_lists_in_kernel_agrees_with_the_route(plan):
    """hbmpc_dev_apply_rows_lists_in_kernel is the planner's answer: a list-writing kernel first (k_mfma_bfly<.., LISTS> or
    k_eval_fft1_mix) -- and for the mixing step (d = n - 1) it is the condition include/hbmpc_hip.h documents"""
    queries = []
    for knobs in KNOBS:
        for field in ("fr", "gl", "sat32"):
            for n in NS:
                for G in sorted({n * k for k in (1, 64, 367, 1024, 1500)} | {16384, 16385, 1 << 20}):
                    queries.append(("lists", knobs, field, G, n, n - 1, 1))
    got = plan(queries)
    for q, line in got.items():
        knobs, field, G, n = q[1].split(","), q[2], q[3], q[4]
        first = line.split()[0]
        yes = line.split("lists_in_kernel=")[1].split()[0] == "1"
        assert yes == (first in ("BflyLists", "Fft1Mix")), (q, line)
        size = 1 << (n - 1).bit_length()
        nwg = 8 if "wgs8" in knobs else 256
        fused = "fusion0" not in knobs and "generic" not in knobs
        if field == "gl":
            want = fused and n >= 3 and size <= 16
        elif field == "sat32":
            want = False
        else:
            mfma = "mc0" not in knobs and "mc3" not in knobs and 5 <= n and 8 <= size <= 16 and (G + 31) // 32 > 2 * nwg
            want = fused and ((3 <= n and size <= 8) or mfma)
        assert yes == want, (q, line)
