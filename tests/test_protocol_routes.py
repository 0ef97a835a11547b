"""Which form a "whole protocol step for all parties" call takes -- one launch, or the separate launches (and whether those offer the
first open to the decode's pair form): the planner (mpc-protocols_amd/csrc/protocol_route.hpp) compiled for the CPU under ASan + UBSan
(tests/cpp/protocol_routes_dump.cpp).  The GPU tests compare the two forms byte for byte, so a slip that sends every call down the
separate launches passes all of them; this pins the form itself.  Runs without a GPU.

The rule is restated below from the five hand-written predicates the planner replaced, as they stood in commit 6794365 ("Matrix-core
kernels: digit-sum extremes and slow-path inputs, proved"); every `file:line` is of that commit."""
import ctypes as C
import os
import subprocess

import pytest

from __graft_entry__ import load_package

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "protocol_routes_dump")
CALLS = ("triplegen", "fpmul", "truncpr", "mul", "randbit")
FIELDS = ("fr", "sat32", "gl")
NS = (4, 5, 7, 10, 16, 17, 31, 64, 65, 255)
MS = (0, 16, 252, 253, 256)
# every threshold of a context's defaults and the knob settings below, each +- 1 (elements, or chunks for triplegen and randbit)
SIZES = sorted({1} | {x + dx for x in (100, 256, 512, 768, 1024, 2048, 8192) for dx in (-1, 0, 1)})


@pytest.fixture(scope="module")
def plan():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "cpp"), "protocol_routes_dump"], stdout=subprocess.DEVNULL)

    def run(queries):
        text = "".join(" ".join(map(str, q)) + "\n" for q in queries)
        p = subprocess.run([BIN], input=text, capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stderr[-2000:]          # ASan / UBSan findings abort with a non-zero code
        lines = p.stdout.splitlines()
        assert len(lines) == len(queries)
        return dict(zip(queries, lines))
    return run


def lane_share(rows, lanes, t):
    """while (lk < 2 && (rows << (lk + 1)) <= lanes && (2 << lk) <= t + 1) ++lk"""
    lk = 0
    while lk < 2 and (rows << (lk + 1)) <= lanes and (2 << lk) <= t + 1:
        lk += 1
    return lk


def parent_rule(call, knobs, field, N, n, t, S, m):
    """the answer of commit 6794365 to the call, as the dump tool prints it"""
    kn = knobs.split(",")
    # hbmpc_capi.hip:77-82 (the struct's defaults), :42 and :356 (RandBit's threshold per field)
    mx = {"triplegen": 1024, "fpmul": 2048, "truncpr": 768, "mul": 1024, "randbit": 1024 if field == "gl" else 256}
    pair_decode_min = 8192
    for tok in kn:
        for c in CALLS:
            if tok.startswith(c + "max"):
                mx[c] = int(tok[len(c) + 3:])
    force_generic, direct_fail = "generic" in kn, "single0" not in kn       # hbmpc_set_force_generic, hbmpc_set_single_launch_decode
    gold, u29 = field == "gl", field == "fr"
    if call == "triplegen":
        # hbmpc_capi.hip:2104-2105: G <= (gold ? fused_triplegen_max / 2 : fused_triplegen_max) && n == 3 * t + 1 && n <= 16 &&
        #                           (gold || impl == IMPL_U29) && !force_generic && direct_fail
        G = N // (2 * t + 1)
        one = G <= (mx[call] // 2 if gold else mx[call]) and n == 3 * t + 1 and n <= 16 and (gold or u29) and not force_generic and direct_fail
        return "one" if one else "launches pair=0"
    if call == "randbit":
        # capi_randbit.inc:66: G <= fused_randbit_max && n <= 16 && t >= 1 && (gold || impl == IMPL_U29) && !force_generic && direct_fail
        G = N // (t + 1)
        one = G <= mx[call] and n <= 16 and t >= 1 and (gold or u29) and not force_generic and direct_fail
        return "one" if one else "launches pair=0"
    # hbmpc_capi.hip:2197 (FPMul), capi_truncpr.inc:52, capi_mul.inc:67:
    #   N <= fused_X_max && S == 2 * t + 1 && impl == IMPL_U29 && !force_generic && direct_fail && n <= 64 && t <= 30
    one = N <= mx[call] and S == 2 * t + 1 and u29 and not force_generic and direct_fail and n <= 64 and t <= 30
    if call == "fpmul":
        one = one and (4 + m) * n <= 4096                                   # hbmpc_capi.hip:2198
    lk_row = lane_share(t + 2, 32, t)                                       # hbmpc_capi.hip:2209 (lk1), capi_mul.inc:74
    lk_wave = lane_share(t + 1, 64, t)                                      # hbmpc_capi.hip:2210 (lk3), capi_truncpr.inc:58
    if one:
        return {"fpmul": "one lk=%d lk3=%d" % (lk_row, lk_wave), "truncpr": "one lk=%d" % lk_wave, "mul": "one lk=%d" % lk_row}[call]
    # hbmpc_capi.hip:2241, capi_mul.inc:20: N >= pair_decode_min.  Over Goldilocks hbmpc_gl_dev_mul_parties has no pair form
    # (capi_mul.inc:34-43) and hbmpc_dev_fpmul_parties refuses the context (:2187); TruncPr opens one share, not a pair.
    pair = call in ("fpmul", "mul") and not gold and N >= pair_decode_min
    return "launches pair=%d" % pair


def chunks(call, t):
    """elements per unit of N: a chunk of 2t + 1 triples (hbmpc_capi.hip:2095-2098), of t + 1 elements (capi_randbit.inc:61-63)"""
    return {"triplegen": 2 * t + 1, "randbit": t + 1}.get(call, 1)


def q(call, knobs, field, size, n, t, S=0, m=0):
    return (call, knobs, field, size * chunks(call, t), n, t, S, m)


# query -> answer, each derived by hand from the line of that commit it cites
ANCHORS = [
    # TripleGen, hbmpc_capi.hip:2104-2105
    (q("triplegen", "default", "fr", 1024, 4, 1), "one"),                   # N = 3072
    (q("triplegen", "default", "fr", 1025, 4, 1), "launches pair=0"),
    (q("triplegen", "default", "gl", 512, 4, 1), "one"),                    # fused_triplegen_max / 2
    (q("triplegen", "default", "gl", 513, 4, 1), "launches pair=0"),
    (q("triplegen", "default", "fr", 16, 5, 1), "launches pair=0"),         # n != 3t + 1
    (q("triplegen", "default", "fr", 16, 19, 6), "launches pair=0"),        # n > 16
    (q("triplegen", "default", "fr", 16, 16, 5), "one"),
    (q("triplegen", "default", "sat32", 16, 4, 1), "launches pair=0"),
    # FPMul, hbmpc_capi.hip:2197-2198, the widths :2209-2210, the pair form :2241
    (q("fpmul", "default", "fr", 2048, 16, 5, 11, 16), "one lk=2 lk3=2"),
    (q("fpmul", "default", "fr", 2049, 16, 5, 11, 16), "launches pair=0"),
    (q("fpmul", "default", "fr", 8192, 16, 5, 11, 16), "launches pair=1"),
    (q("fpmul", "default", "fr", 8191, 16, 5, 11, 16), "launches pair=0"),
    (q("fpmul", "default", "fr", 2048, 16, 5, 12, 16), "launches pair=0"),  # an OEC round exists
    (q("fpmul", "default", "fr", 2048, 16, 5, 11, 252), "one lk=2 lk3=2"),  # (4 + 252) * 16 = 4096
    (q("fpmul", "default", "fr", 2048, 16, 5, 11, 253), "launches pair=0"),
    (q("fpmul", "default", "fr", 2048, 4, 1, 3, 16), "one lk=1 lk3=1"),
    (q("fpmul", "default", "fr", 2048, 31, 10, 21, 16), "one lk=1 lk3=2"),
    (q("fpmul", "default", "fr", 2048, 64, 21, 43, 16), "one lk=0 lk3=1"),
    (q("fpmul", "default", "fr", 2048, 65, 21, 43, 16), "launches pair=0"),
    (q("fpmul", "default", "gl", 2048, 16, 5, 11, 16), "launches pair=0"),
    (q("fpmul", "default", "sat32", 2048, 16, 5, 11, 16), "launches pair=0"),
    # TruncPr, capi_truncpr.inc:52, the width :58 (the wave rule)
    (q("truncpr", "default", "fr", 768, 16, 5, 11), "one lk=2"),
    (q("truncpr", "default", "fr", 769, 16, 5, 11), "launches pair=0"),
    (q("truncpr", "default", "fr", 768, 64, 21, 43), "one lk=1"),
    (q("truncpr", "default", "fr", 768, 4, 1, 3), "one lk=1"),
    (q("truncpr", "default", "fr", 8192, 16, 5, 11), "launches pair=0"),
    # Mul, capi_mul.inc:67, the width :74 (the row rule), the pair form :20, Goldilocks :34-43
    (q("mul", "default", "fr", 1024, 16, 5, 11), "one lk=2"),
    (q("mul", "default", "fr", 1025, 16, 5, 11), "launches pair=0"),
    (q("mul", "default", "fr", 1024, 31, 10, 21), "one lk=1"),
    (q("mul", "default", "fr", 1024, 64, 21, 43), "one lk=0"),
    (q("mul", "default", "fr", 8192, 16, 5, 11), "launches pair=1"),
    (q("mul", "default", "gl", 1, 16, 5, 11), "launches pair=0"),
    (q("mul", "default", "gl", 8192, 16, 5, 11), "launches pair=0"),
    # RandBit, capi_randbit.inc:66; the thresholds hbmpc_capi.hip:42
    (q("randbit", "default", "fr", 256, 4, 1), "one"),
    (q("randbit", "default", "fr", 257, 4, 1), "launches pair=0"),
    (q("randbit", "default", "gl", 1024, 4, 1), "one"),
    (q("randbit", "default", "gl", 1025, 4, 1), "launches pair=0"),
    (q("randbit", "default", "fr", 256, 4, 0), "launches pair=0"),          # t = 0
    (q("randbit", "default", "fr", 16, 17, 5), "launches pair=0"),          # n > 16
    (q("randbit", "default", "fr", 16, 16, 7), "one"),                      # n = 2t + 2: no n == 3t + 1 here
]
# test aids: everything takes the separate launches
for _knobs in ("generic", "single0"):
    ANCHORS += [(q("triplegen", _knobs, "fr", 16, 4, 1), "launches pair=0"), (q("fpmul", _knobs, "fr", 16, 16, 5, 11, 16), "launches pair=0"),
                (q("truncpr", _knobs, "fr", 16, 16, 5, 11), "launches pair=0"), (q("mul", _knobs, "fr", 16, 16, 5, 11), "launches pair=0"),
                (q("randbit", _knobs, "gl", 16, 4, 1), "launches pair=0")]


def test_anchors(plan):
    got = plan([query for query, _ in ANCHORS])
    for query, want in ANCHORS:
        assert got[query] == want, (query, got[query])
        assert parent_rule(*query) == want, query           # the restatement below the grid agrees with the hand derivation


def test_grid_against_the_replaced_predicates(plan):
    queries = []
    for call in CALLS:
        for knobs in ("default", "generic", "single0", call + "max100", call + "max0"):
            for field in FIELDS:
                for n in NS:
                    for t in sorted({t for t in (0, 1, (n - 1) // 3, (n - 1) // 2) if 2 * t + 1 <= n}):
                        senders = sorted({2 * t + 1, 2 * t + 2, n} & set(range(2 * t + 1, n + 1))) if call in ("fpmul", "truncpr", "mul") else [0]
                        for S in senders:
                            for m in (MS if call == "fpmul" else (0,)):
                                queries += [q(call, knobs, field, size, n, t, S, m) for size in SIZES]
    assert len(queries) > 50000
    got = plan(queries)
    seen = set()
    for query, line in got.items():
        assert line == parent_rule(*query), (query, line)
        seen.add((query[0], line.split()[0]))
    assert seen == {(c, form) for c in CALLS for form in ("one", "launches")}  # the grid reaches both forms of every call


def test_null_context_is_invalid_input():
    """no context, so no device: InvalidInput (4) before anything is read -- non-null buffers, so the null-buffer check is not the one
    that answers"""
    L = load_package().lib()
    p, z = C.c_void_p(64), C.c_size_t
    fpmul = [None, p, z(3)] + [p] * 7 + [z(16), z(8), z(5), z(4), z(1)] + [p] * 8 + [None] * 3
    assert L.hbmpc_dev_fpmul_parties(*fpmul) == 4
    triplegen = [None] + [p] * 4 + [z(3), z(4), z(1)] + [p] * 5 + [None] * 3
    assert L.hbmpc_dev_triplegen_parties(*triplegen) == 4
    assert L.hbmpc_gl_dev_triplegen_parties(*triplegen) == 4
    check = [None, p, z(3), p, z(8), z(8), z(4), z(1), z(2), z(8), p, p, None, p, None]
    assert L.hbmpc_dev_recover_check_degree_strided(*check) == 4
    assert L.hbmpc_gl_dev_recover_check_degree_strided(*check) == 4
