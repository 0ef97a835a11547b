"""Which form hbmpc_[gl_]dev_input_parties takes -- one launch (a wave per element) or the two separate launches: the planner
(mpc-protocols_amd/csrc/protocol_route.hpp, ProtocolCall::Input) compiled for the CPU under ASan + UBSan
(tests/cpp/input_routes_dump.cpp).  The GPU tests compare the two forms byte for byte, so a slip that sends every call down the
separate launches passes all of them; this pins the form itself.  Runs without a GPU.

The rule, restated here from the call's documentation (include/hbmpc_hip.h): one launch iff the context is Fr in 29-bit limbs,
nothing forces the generic kernels, a decode without an OEC round is one launch (hbmpc_set_single_launch_decode), there are
exactly 2t + 1 senders, n <= 64, t <= 30 and N <= the threshold; the lanes that share a table row are TruncPr's."""
import os
import re
import subprocess

import pytest

from __graft_entry__ import PKG_DIR, load_package

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "input_routes_dump")
FIELDS = ("fr", "sat32", "gl")
NS = (4, 5, 7, 10, 16, 17, 31, 64, 65, 255)
KNOBS = ("default", "generic", "single0", "inputmax100", "inputmax0")


def default_threshold():
    src = open(os.path.join(PKG_DIR, "csrc", "hbmpc_capi.hip")).read()
    return int(re.search(r"\bfused_input_max\s*=\s*(\d+)\s*;", src).group(1))


D = default_threshold()
# the default threshold and the knob settings' (100, 0), each +- 1
SIZES = sorted({1} | {x + dx for x in (100, D) for dx in (-1, 0, 1) if x + dx >= 1})


@pytest.fixture(scope="module")
def plan():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "cpp"), "-f", "input.mk", "input_routes_dump"], stdout=subprocess.DEVNULL)

    def run(queries):
        text = "".join(" ".join(map(str, q)) + "\n" for q in queries)
        p = subprocess.run([BIN, str(D)], input=text, capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stderr[-2000:]          # ASan / UBSan findings abort with a non-zero code
        lines = p.stdout.splitlines()
        assert len(lines) == len(queries)
        return dict(zip(queries, lines))
    return run


def lane_share(rows, lanes, t):
    lk = 0
    while lk < 2 and (rows << (lk + 1)) <= lanes and (2 << lk) <= t + 1:
        lk += 1
    return lk


def rule(knobs, field, N, n, t, S):
    kn = knobs.split(",")
    mx = D
    for tok in kn:
        if tok.startswith("inputmax"):
            mx = int(tok[8:])
    one = (field == "fr" and "generic" not in kn and "single0" not in kn and S == 2 * t + 1 and n <= 64 and t <= 30 and N <= mx)
    return "one lk=%d" % lane_share(t + 1, 64, t) if one else "launches"


# derived by hand: t + 1 = 6 rows, 6 << 2 = 24 <= 64 and 4 <= 6: four lanes to a row (lk = 2)
ANCHORS = [
    (("default", "fr", D, 16, 5, 11), "one lk=2"),
    (("default", "fr", D + 1, 16, 5, 11), "launches"),
    (("default", "fr", D, 16, 5, 12), "launches"),           # an OEC round exists
    (("default", "gl", D, 16, 5, 11), "launches"),
    (("default", "gl", 1, 16, 5, 11), "launches"),
    (("default", "sat32", 1, 16, 5, 11), "launches"),
    (("default", "fr", 1, 65, 21, 43), "launches"),          # n = 65: a lane per party no longer fits the wave
    (("default", "fr", 1, 64, 21, 43), "one lk=1"),          # 22 rows: 44 <= 64, 88 > 64
    (("default", "fr", 1, 4, 1, 3), "one lk=1"),             # 2 rows, 2 <= t + 1 = 2 < 4
    (("default", "fr", 1, 64, 31, 63), "launches"),          # t = 31 > 30
    (("inputmax100", "fr", 100, 16, 5, 11), "one lk=2"),
    (("inputmax100", "fr", 101, 16, 5, 11), "launches"),
    (("inputmax0", "fr", 1, 16, 5, 11), "launches"),
    (("generic", "fr", 1, 16, 5, 11), "launches"),
    (("single0", "fr", 1, 16, 5, 11), "launches"),
]


def test_anchors(plan):
    got = plan([query for query, _ in ANCHORS])
    for query, want in ANCHORS:
        assert got[query] == want, (query, got[query])
        assert rule(*query) == want, query


def test_grid(plan):
    queries = []
    for knobs in KNOBS:
        for field in FIELDS:
            for n in NS:
                for t in sorted({t for t in (0, 1, (n - 1) // 3, (n - 1) // 2) if 2 * t + 1 <= n}):
                    for S in sorted({2 * t + 1, 2 * t + 2, n} & set(range(2 * t + 1, n + 1))):
                        queries += [(knobs, field, size, n, t, S) for size in SIZES]
    assert len(queries) > 5000
    got = plan(queries)
    seen = set()
    for query, line in got.items():
        assert line == rule(*query), (query, line)
        seen.add(line.split()[0])
    assert seen == {"one", "launches"}                       # the grid reaches both forms


def test_the_other_calls_answer_as_before(plan):
    """ProtocolCall::Input and fused_input_max come last: tests/cpp/protocol_routes_dump.cpp, which lists the first nine knobs and
    casts 0 .. 4 to the enum, builds unchanged (tests/test_protocol_routes.py holds its answers)"""
    src = open(os.path.join(PKG_DIR, "csrc", "protocol_route.hpp")).read()
    assert re.search(r"enum class ProtocolCall \{ TripleGen, FpMul, TruncPr, Mul, RandBit, Input \}", src)
    fields = re.search(r"struct ProtocolKnobs \{(.*?)\};", src, re.S).group(1)
    assert fields.rstrip().splitlines()[-1].strip().startswith("size_t fused_input_max")
    assert load_package().hbmpc.FUSED_INPUT_DEFAULT == D
