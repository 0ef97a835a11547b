"""Which form hbmpc_[gl_]dev_ransha_parties and hbmpc_[gl_]dev_randousha_parties take -- one launch (a workgroup per column) or the
separate launches: the planner (mpc-protocols_amd/csrc/protocol_route.hpp, plan_producers) compiled for the CPU under ASan + UBSan as a
stand-alone program (tests/cpp/producers_routes_dump.cpp).  The GPU tests compare the forms byte for byte, so a slip that sends every
call down the separate launches passes all of them; this pins the form itself.  Runs without a GPU.

The rule, restated here from the calls' documentation (include/hbmpc_hip.h): one launch iff the context is Fr in 29-bit limbs or
Goldilocks, nothing forces the generic kernels or the OEC kernels (hbmpc_set_force_generic, hbmpc_set_single_launch_decode), 1 <= t,
2t < n <= 16, for RanSha verify_senders == 2t + 1 and n >= 3t + 1, the tables fit a workgroup's 160 KB of LDS, and there are at most
`threshold` columns per dealer."""
import os
import re
import subprocess

import pytest

from __graft_entry__ import PKG_DIR, load_package

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "producers_routes_dump")
FIELDS = ("fr", "sat32", "gl")
KNOBS = ("default", "generic", "single0", "producersmax0", "producersmax100")
CALLS = ("ransha", "randousha")
NS = (1, 2, 3, 4, 5, 7, 13, 16, 17)


def default_thresholds():
    src = open(os.path.join(PKG_DIR, "csrc", "hbmpc_capi.hip")).read()
    m = re.search(r"\bFUSED_PRODUCERS_FR\s*=\s*(\d+)\s*,\s*FUSED_PRODUCERS_GL\s*=\s*(\d+)\s*;", src)
    return {"fr": int(m.group(1)), "sat32": int(m.group(1)), "gl": int(m.group(2))}


D = default_thresholds()
SIZES = sorted({1} | {x + dx for x in (100, D["fr"], D["gl"]) for dx in (-1, 0, 1) if x + dx >= 1})


@pytest.fixture(scope="module")
def plan():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "cpp"), "-f", "producers.mk", "producers_routes_dump"], stdout=subprocess.DEVNULL)

    def run(queries):
        text = "".join(" ".join(map(str, q)) + "\n" for q in queries)
        p = subprocess.run([BIN, "%d,%d" % (D["fr"], D["gl"])], input=text, capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stderr[-2000:]          # ASan / UBSan findings abort with a non-zero code
        lines = p.stdout.splitlines()
        assert len(lines) == len(queries)
        return dict(zip(queries, lines))
    return run


def lds_bytes(call, field, n, t):
    """the workgroup's LDS as csrc/kernels_producers_wg.hpp lays it out: per sharing the dealt and the mixed block (n n elements each) and
    the verifiers' table, the n x n Vandermonde table, the kept coefficients (4 per verifier), 64 flag words; elements of 12 words and
    constants of 9 over Fr, 2 and 2 over Goldilocks"""
    ls, nl = (2, 2) if field == "gl" else (12, 9)
    dou = call == "randousha"
    nver = n - t - 1 if dou else 2 * t
    tabs = (2 * t + 1) * (t + 1) if not dou else 2 * n * n if field == "gl" else n * (3 * t + 2)
    return 4 * ((4 if dou else 2) * n * n * ls + n * n * nl + tabs * nl + 4 * nver * ls + 64 + 16)


def rule(call, knobs, field, K, n, t, S):
    kn = knobs.split(",")
    mx = D[field]
    for tok in kn:
        if tok.startswith("producersmax"):
            mx = int(tok[12:])
    one = (field in ("fr", "gl") and "generic" not in kn and "single0" not in kn and 1 <= t and 2 * t < n <= 16
           and (call == "randousha" or (S == 2 * t + 1 and n >= 3 * t + 1)) and lds_bytes(call, field, n, t) <= 160 * 1024 and K <= mx)
    return "one" if one else "launches"


# derived by hand; the thresholds are forced so that the anchors hold whatever the measured defaults are
ANCHORS = [
    (("ransha", "producersmax100", "fr", 100, 16, 5, 11), "one"),
    (("ransha", "producersmax100", "fr", 101, 16, 5, 11), "launches"),
    (("ransha", "producersmax100", "fr", 1, 16, 5, 12), "launches"),          # an OEC round exists
    (("ransha", "producersmax100", "fr", 1, 16, 5, 16), "launches"),
    (("ransha", "producersmax100", "fr", 1, 17, 5, 11), "launches"),          # the (row, party) pairs no longer fit
    (("ransha", "producersmax100", "fr", 1, 5, 2, 5), "launches"),            # n < 3t + 1: recover_secret refuses every column
    (("randousha", "producersmax100", "fr", 1, 5, 2, 5), "one"),              # RanDouSha needs n > 2t alone
    (("ransha", "producersmax100", "fr", 1, 2, 0, 1), "launches"),            # t = 0: no verifier
    (("randousha", "producersmax100", "fr", 1, 2, 0, 2), "launches"),
    (("ransha", "producersmax100", "sat32", 1, 4, 1, 3), "launches"),         # no kernel over Sat32
    (("randousha", "producersmax100", "sat32", 1, 4, 1, 4), "launches"),
    (("ransha", "producersmax100", "gl", 100, 16, 5, 11), "one"),
    (("randousha", "producersmax100", "gl", 101, 16, 5, 16), "launches"),
    (("randousha", "producersmax100", "gl", 100, 16, 5, 16), "one"),
    (("randousha", "producersmax100", "fr", 100, 16, 5, 16), "one"),
    (("randousha", "producersmax100,generic", "fr", 1, 16, 5, 16), "launches"),
    (("ransha", "producersmax100,single0", "fr", 1, 4, 1, 3), "launches"),
    (("ransha", "producersmax0", "fr", 1, 4, 1, 3), "launches"),              # 0: never one launch
    (("ransha", "producersmax100", "fr", 1, 4, 1, 3), "one"),
    (("randousha", "producersmax100", "fr", 1, 16, 1, 16), "one"),
]


def test_anchors(plan):
    got = plan([query for query, _ in ANCHORS])
    for query, want in ANCHORS:
        assert got[query] == want, (query, got[query])
        assert rule(*query) == want, query


def test_defaults_match_the_wrapper(plan):
    dflt = load_package().hbmpc.FUSED_PRODUCERS_DEFAULT
    assert dflt == {"fr": D["fr"], "goldilocks": D["gl"]}
    for field in ("fr", "gl"):
        for call, S in (("ransha", 11), ("randousha", 16)):
            if D[field]:
                got = plan([(call, "default", field, D[field], 16, 5, S), (call, "default", field, D[field] + 1, 16, 5, S)])
                assert list(got.values()) == ["one", "launches"]
            else:
                assert list(plan([(call, "default", field, 1, 16, 5, S)]).values()) == ["launches"]


def test_grid(plan):
    queries = []
    for call in CALLS:
        for knobs in KNOBS:
            for field in FIELDS:
                for n in NS:
                    for t in sorted({0, 1, (n - 1) // 3, (n - 1) // 2}):
                        if n <= 2 * t:
                            continue
                        for S in sorted({2 * t + 1, n}):
                            queries += [(call, knobs, field, K, n, t, S) for K in SIZES]
    assert len(queries) > 5000
    got = plan(queries)
    seen = set()
    for query, line in got.items():
        assert line == rule(*query), (query, line)
        seen.add((query[0], line))
    assert seen == {(c, f) for c in CALLS for f in ("one", "launches")}   # the grid reaches both forms of both calls
    # the tables of every covered shape fit: the LDS clause never decides below n = 17
    assert all(lds_bytes(c, f, n, t) <= 160 * 1024 for c in CALLS for f in ("fr", "gl") for n in NS if n <= 16 for t in range(1, (n + 1) // 2))
