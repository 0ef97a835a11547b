"""Which form hbmpc_[gl_]dev_batchrecon_parties takes -- one launch (a workgroup per chunk) or the three separate launches: the planner
(mpc-protocols_amd/csrc/protocol_route.hpp, plan_batchrecon) compiled for the CPU under ASan + UBSan
(tests/cpp/batchrecon_routes_dump.cpp).  The GPU tests compare the forms byte for byte, so a slip that sends every call down the
separate launches passes all of them; this pins the form itself.  Runs without a GPU.

The rule, restated here from the call's documentation (include/hbmpc_hip.h): one launch iff the context is Fr in 29-bit limbs or
Goldilocks, nothing forces the generic kernels, a decode without an OEC round is one launch (hbmpc_set_single_launch_decode),
n <= 16, both sender sets have exactly d + t + 1 parties and there are at most `threshold` chunks of d + 1 elements.  The EvalBatch
arm's lane share is 1 over Fr in 29-bit limbs while 2 n (t + 1) <= 256, else 0."""
import os
import re
import subprocess

import pytest

from __graft_entry__ import PKG_DIR, load_package
from tests import test_protocol_routes as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "batchrecon_routes_dump")
FIELDS = ("fr", "sat32", "gl")
KNOBS = ("default", "generic", "single0", "batchreconmax100", "batchreconmax0")


def default_thresholds():
    src = open(os.path.join(PKG_DIR, "csrc", "hbmpc_capi.hip")).read()
    m = re.search(r"\bFUSED_BATCHRECON_FR\s*=\s*(\d+)\s*,\s*FUSED_BATCHRECON_GL\s*=\s*(\d+)\s*;", src)
    return {"fr": int(m.group(1)), "sat32": int(m.group(1)), "gl": int(m.group(2))}


D = default_thresholds()
SIZES = sorted({1} | {x + dx for x in (100, D["fr"], D["gl"]) for dx in (-1, 0, 1) if x + dx >= 1})


@pytest.fixture(scope="module")
def plan():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "cpp"), "-f", "batchrecon.mk", "batchrecon_routes_dump"], stdout=subprocess.DEVNULL)

    def run(queries):
        text = "".join(" ".join(map(str, q)) + "\n" for q in queries)
        p = subprocess.run([BIN, "%d,%d" % (D["fr"], D["gl"])], input=text, capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stderr[-2000:]          # ASan / UBSan findings abort with a non-zero code
        lines = p.stdout.splitlines()
        assert len(lines) == len(queries)
        return dict(zip(queries, lines))
    return run


def rule(call, knobs, field, N, n, t, d, S1, S2):
    kn = knobs.split(",")
    mx = D[field]
    for tok in kn:
        if tok.startswith("batchreconmax"):
            mx = int(tok[13:])
    one = (field in ("fr", "gl") and "generic" not in kn and "single0" not in kn and n <= 16 and S1 == d + t + 1 and S2 == d + t + 1
           and N // (d + 1) <= mx)
    lk = 1 if field == "fr" and 2 * n * (t + 1) <= 256 else 0
    return "%s lk=%d" % ("one" if one else "launches", lk)


def q(knobs, field, G, n, t, d, S1=None, S2=None):
    S = d + t + 1
    return ("batchrecon", knobs, field, G * (d + 1), n, t, d, S if S1 is None else S1, S if S2 is None else S2)


# derived by hand; the thresholds are forced so that the anchors hold whatever the measured defaults are
ANCHORS = [
    (q("batchreconmax100", "fr", 100, 16, 5, 5), "one lk=1"),               # 2 * 16 * 6 = 192 <= 256: lane pairs
    (q("batchreconmax100", "fr", 101, 16, 5, 5), "launches lk=1"),
    (q("batchreconmax100", "fr", 100, 16, 5, 10), "one lk=1"),              # S = 16 = n
    (q("batchreconmax100", "fr", 1, 17, 5, 5), "launches lk=1"),            # n = 17: the (party, recipient) pairs no longer fit
    (q("batchreconmax100", "fr", 1, 16, 5, 5, S1=12), "launches lk=1"),     # S1 = d + t + 2: an OEC round exists
    (q("batchreconmax100", "fr", 1, 16, 5, 5, S2=12), "launches lk=1"),     # S2 = d + t + 2
    (q("batchreconmax100", "fr", 1, 16, 5, 4, S1=11, S2=10), "launches lk=1"),   # S1 != S2 (S2 exact, S1 not)
    (q("batchreconmax100", "fr", 1, 16, 5, 4, S1=10, S2=11), "launches lk=1"),
    (q("batchreconmax100", "fr", 1, 16, 5, 4, S1=10, S2=10), "one lk=1"),
    (q("batchreconmax100", "sat32", 1, 16, 5, 5), "launches lk=0"),         # no kernel over Sat32
    (q("batchreconmax100", "gl", 100, 16, 5, 5), "one lk=0"),               # Goldilocks: a lane per row
    (q("batchreconmax100", "gl", 101, 16, 5, 5), "launches lk=0"),
    (q("batchreconmax100,generic", "fr", 1, 16, 5, 5), "launches lk=1"),
    (q("batchreconmax100,single0", "fr", 1, 16, 5, 5), "launches lk=1"),
    (q("batchreconmax0", "fr", 1, 4, 1, 1), "launches lk=1"),               # 0: never one launch
    (q("batchreconmax100", "fr", 1, 16, 1, 1), "one lk=1"),                 # (16, 1): 2 * 16 * 2 = 64 lanes
    (q("batchreconmax100", "fr", 1, 16, 0, 15), "one lk=1"),                # t = 0: 32 lanes
    (q("batchreconmax100", "fr", 1, 31, 10, 10), "launches lk=0"),          # 2 * 31 * 11 = 682 > 256: no sharing (and n > 16)
    (q("batchreconmax100", "fr", 100, 4, 1, 1), "one lk=1"),
]


def test_anchors(plan):
    got = plan([query for query, _ in ANCHORS])
    for query, want in ANCHORS:
        assert got[query] == want, (query, got[query])
        assert rule(*query) == want, query


def test_defaults_match_the_wrapper(plan):
    dflt = load_package().hbmpc.FUSED_BATCHRECON_DEFAULT
    assert dflt == {"fr": D["fr"], "goldilocks": D["gl"]}
    for field in ("fr", "gl"):
        if D[field]:
            got = plan([q("default", field, D[field], 16, 5, 5), q("default", field, D[field] + 1, 16, 5, 5)])
            assert [v.split()[0] for v in got.values()] == ["one", "launches"]
        else:
            assert list(plan([q("default", field, 1, 16, 5, 5)]).values())[0].startswith("launches")


def test_grid(plan):
    queries = []
    for knobs in KNOBS:
        for field in FIELDS:
            for n in (4, 5, 7, 10, 16, 17, 31):
                for t in sorted({0, 1, (n - 1) // 3}):
                    for d in sorted({1, t, 2 * t, n - t - 1} & set(range(1, n - t))):
                        S = d + t + 1
                        for S1, S2 in {(S, S), (min(S + 1, n), S), (S, min(S + 1, n)), (n, n)}:
                            queries += [q(knobs, field, G, n, t, d, S1, S2) for G in SIZES]
    assert len(queries) > 5000
    got = plan(queries)
    seen = set()
    for query, line in got.items():
        assert line == rule(*query), (query, line)
        seen.add(line.split()[0])
    assert seen == {"one", "launches"}                       # the grid reaches both forms


def test_the_other_calls_answer_as_before(plan):
    """plan_batchrecon sits beside plan_protocol: a few hundred of tests/test_protocol_routes.py's queries through this binary get that
    file's parent_rule answers"""
    queries = [query for query, _ in PR.ANCHORS]
    for call in PR.CALLS:
        for field in FIELDS:
            for n, t in ((4, 1), (16, 5), (31, 10)):
                for size in (1, 256, 257, 1024, 1025, 8192):
                    queries.append(PR.q(call, "default", field, size, n, t, 2 * t + 1, 16))
    queries = list(dict.fromkeys(queries))
    assert len(queries) > 300
    got = plan(queries)
    for query, line in got.items():
        assert line == PR.parent_rule(*query), (query, line)
