"""Which form hbmpc_dev_prandbit_parties / hbmpc_dev_prandint_parties take -- one launch (csrc/kernels_prandbit_wg.hpp) or the separate
launches: the planner (mpc-protocols_amd/csrc/prandbit_route.hpp) compiled for the CPU under ASan + UBSan
(tests/cpp/prandbit_routes_dump.cpp).  The GPU tests compare the two forms byte for byte, so a slip that sends every call down the
separate launches passes all of them; this pins the form itself, and the LDS layout the eligibility is derived from.  Runs without a GPU.

The rule, restated here independently of the header (include/hbmpc_hip.h states it for callers): one launch exactly when the Fr context runs U29, is not forced
generic, single-launch decodes are on (PRandBit), 1 <= t, 3t + 1 <= n <= 16, open_senders == 2t + 1 (PRandBit; 0 means that), the
layout fits 160 KB, and the number of chunks is <= the threshold."""
import math
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "prandbit_routes_dump")
NS = (4, 5, 7, 10, 12, 13, 16, 17)
THRESHOLD = 100
LDS_LIMIT = 160 * 1024


@pytest.fixture(scope="module")
def plan():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "cpp"), "-f", "prandbit_routes.mk", "prandbit_routes_dump"], stdout=subprocess.DEVNULL)

    def run(queries):
        text = "".join(" ".join(map(str, q)) + "\n" for q in queries)
        p = subprocess.run([BIN], input=text, capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stderr[-2000:]          # ASan / UBSan findings abort with a non-zero code
        lines = p.stdout.splitlines()
        assert len(lines) == len(queries)
        return dict(zip(queries, lines))
    return run


def layout(n, t):
    """(bytes, slices) of the kernel's LDS: the tables C(n,t) n 11 words (8 Fr, 2 Goldilocks, 1 GF(2^8)), vmat and the decode table, the
    chunk's sums, r + b, messages, revealed and opened values, flags, and the conversion's merge area of 37 words per (slice > 0, output)"""
    Tn, M = math.comb(n, t), t + 1
    outs = n * M
    ks = max(1, min(256 // outs, Tn, 8))
    words = Tn * n * 11 + n * M * 2 + (t + M) * M * 2 + Tn * M * 2 + n * M * 2 + n * n * 2 + n * 2 + M * 2 + n + 1
    words = (words + 3) & ~3
    return 4 * (words + (ks - 1) * outs * 37), ks


def rule(call, knobs, field, chunks, n, t, S):
    kn = knobs.split(",")
    mx = 256
    for tok in kn:
        if tok.startswith("max"):
            mx = int(tok[3:])
    senders = S if S else 2 * t + 1
    shape = 1 <= t and 3 * t + 1 <= n <= 16
    lds, ks = layout(n, t) if shape else (0, 0)
    one = shape and field == "fr" and "generic" not in kn and lds <= LDS_LIMIT and 1 <= chunks <= mx
    if call == "prandbit":
        one = one and "single0" not in kn and senders == 2 * t + 1
    return "%s chunks=%d senders=%d lds=%d ks=%d" % ("one" if one else "launches", chunks, senders, lds, ks)


def q(call, knobs, field, chunks, n, t, S=0):
    return (call, knobs, field, chunks, n, t, S)


def test_anchors(plan):
    """the shapes the reference runs are eligible up to (12,3); (13,4) and (16,5) are not: their tables do not fit"""
    th = "max%d" % THRESHOLD
    anchors = [(q("prandbit", th, "fr", 1, n, t), "one") for n, t in ((4, 1), (5, 1), (7, 2), (10, 3), (12, 3))]
    anchors += [(q("prandbit", th, "fr", 1, n, t), "launches") for n, t in ((13, 4), (16, 5), (17, 5), (4, 0))]
    anchors += [(q("prandbit", th, "fr", THRESHOLD, 7, 2), "one"), (q("prandbit", th, "fr", THRESHOLD + 1, 7, 2), "launches"),
                (q("prandbit", "max0", "fr", 1, 7, 2), "launches"), (q("prandbit", th, "sat32", 1, 7, 2), "launches"),
                (q("prandbit", th + ",generic", "fr", 1, 7, 2), "launches"), (q("prandbit", th + ",single0", "fr", 1, 7, 2), "launches"),
                (q("prandint", th + ",single0", "fr", 1, 7, 2), "one"),          # PRandInt has no open
                (q("prandbit", th, "fr", 1, 7, 2, 5), "one"), (q("prandbit", th, "fr", 1, 7, 2, 6), "launches"),
                (q("prandbit", th, "fr", 1, 7, 2, 7), "launches"), (q("prandint", th, "fr", 1, 7, 2, 7), "one"),
                (q("prandint", th, "fr", 1, 10, 3), "one"), (q("prandint", th, "fr", 1, 13, 4), "launches")]
    got = plan([query for query, _ in anchors])
    for query, want in anchors:
        assert got[query].split()[0] == want, (query, got[query])
        assert rule(*query) == got[query], (query, got[query], rule(*query))
    # the layout's sizes: (4,1) a few KB (mostly the merge area), (10,3) above the 64 KB that need the LDS attribute, (12,3) within
    # 160 KB, (13,4) far outside
    lds = {(n, t): layout(n, t)[0] for n, t in ((4, 1), (10, 3), (12, 3), (13, 4), (16, 5))}
    assert lds[(4, 1)] < 8 * 1024 and 64 * 1024 < lds[(10, 3)] < LDS_LIMIT and lds[(12, 3)] <= LDS_LIMIT
    assert lds[(13, 4)] > 2 * LDS_LIMIT and lds[(16, 5)] > 16 * LDS_LIMIT
    # the tables alone: C(n,t) n 11 words -- 0.7 KB at (4,1), 113 KB at (12,3), 399 KB at (13,4), 3 MB at (16,5)
    tables = lambda n, t: math.comb(n, t) * n * 11 * 4  # noqa: E731
    assert tables(4, 1) == 704 and tables(12, 3) // 1024 == 113 and tables(13, 4) // 1024 == 399 and tables(16, 5) > 3 * 10**6


def test_grid_against_the_restated_rule(plan):
    queries = []
    for call in ("prandbit", "prandint"):
        for field in ("fr", "sat32"):
            for extra in ("", ",generic", ",single0"):
                for n in NS:
                    for t in range(0, (n - 1) // 3 + 1):
                        for S in sorted({0, 2 * t + 1, 2 * t + 2, n}):
                            for chunks in (1, THRESHOLD - 1, THRESHOLD, THRESHOLD + 1):
                                queries.append(q(call, "max%d%s" % (THRESHOLD, extra), field, chunks, n, t, S))
                    queries.append(q(call, "max0" + extra, field, 1, n, (n - 1) // 3))
    assert len(queries) > 3000
    got = plan(queries)
    seen = set()
    for query, line in got.items():
        assert line == rule(*query), (query, line, rule(*query))
        seen.add((query[0], line.split()[0]))
    assert seen == {(c, form) for c in ("prandbit", "prandint") for form in ("one", "launches")}
