"""What the inputs of tests/mfma_inputs.py reach inside the matrix-core kernels, proved without a GPU with the integer model of
tests/mfma_model.py -- and the model itself checked first: its tables byte for byte against the product's (tests/cpp/host_tables_dump),
its epilogues' values against big-int dot products.  tests/test_gpu_mfma_edges.py runs exactly these inputs, through the routes pinned
here with the planners' dump tools.

Reached, per case (digit sums over every row and chunk of the case; the permitted interval is [0, 0xff0000), over Goldilocks [0, 2^23)).
In every (row, digit) the inputs attain the widest value any input chosen byte by byte from the table's signs can, with the top byte of
an element capped so that it stays canonical (asserted below):

  case                         chunks   digit sums reached        largest slow-path k
  pairs (7, 2)                    613   0x0c40aa .. 0x236a73      1
  pairs (16, 5)                  1221   0x189ca7 .. 0x471759      1
  pairs (13, 4)                  1029   0x14dee7 .. 0x3af17a      1
  pairs (16, 15)  (m = 16)       1221   0x40d0a0 .. 0xbe5c8c      1
  pairs (31, 10)                 2277   0x2c2f2d .. 0x83d0f5      1
  triple (16, 5), rows 2^261     1221   0x142c5e .. 0x4bd67f      1
  inverse transform, n = 16      1221   0x4076fe .. 0xbeb422      1
  rows (31, 10)                  2149   0x2bd377 .. 0x83f0c8      1
  rows (20, 6)                   1445   0x1cc85c .. 0x532427      1
  rows (16, 5)                   1157   0x18381d .. 0x477505      1
  decode (4, 1, 1)                293   0x06eb1c .. 0x1924ad      1
  decode (16, 5, 5)               837   0x15fac4 .. 0x49f59e      1
  decode (16, 10, 5)             1157   0x285981 .. 0x871860      1
  decode (31, 10, 10)            1477   0x29ae52 .. 0x86ddb9      1
  decode (43, 14, 13)            1957   0x393458 .. 0xb6d4c4      1
  decode (31, 14, 10)            1765   0x37e300 .. 0xb7a785      1
  Goldilocks (31, 10, 10) encode  677   0x153794 .. 0x16c83d      w2 up to 0x16c6
  Goldilocks (31, 10, 10) decode  485   0x08e83d .. 0x2312d5      w2 up to 0x2328
  Goldilocks (64, 21, 21) encode 1285   0x29c4c6 .. 0x2e3ea0      w2 up to 0x2e62  (22 inputs: beyond the kernel's 16, the model alone)
  Goldilocks (64, 21, 21) decode  901   0x1333a6 .. 0x44d3a8      w2 up to 0x43fa  (the same)

The largest k is 1 in every case, and no search can do better: the quotient estimate q' of reduce_words falls short of S / r by
less than 3 10^-4 (truncating S to its top word: < 2^-14; dividing by R_TOP + 1 instead of r / 2^224: < q / 2^31 with q < 2^18; the
two floors of the reciprocal multiply: < 2^-13), so q' >= floor(S / r) - 1 and one subtraction always suffices; it is NEEDED exactly
when the residue S mod r is below that shortfall times r -- results 0, 1, 2 and 2^200 here.  The other way into the slow path is a
residue whose top word equals r's (r - 1, r - 2, R_TOP 2^224 + x): no subtraction.  The E accumulator of a point pair alone cannot be
negative (its bias is about 32 m 16384 and the even inputs move it by at most half of that: min_E of the table, asserted below); T can.
"""
import os
import random
import subprocess

import numpy as np
import pytest

from tests import mfma_inputs as X
from tests import mfma_model as MM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
R, P = MM.R, MM.P


# ---- the model against the product's tables ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dump():
    subprocess.check_call(["make", "-C", CPP, "host_tables_dump"], stdout=subprocess.DEVNULL)

    def run(field, n, d, t):
        p = subprocess.run([os.path.join(CPP, "host_tables_dump"), field, str(n), str(d), str(t), ",".join(map(str, range(n))), "full"],
                           capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, p.stderr[-2000:]
        out = {}
        for line in p.stdout.splitlines():
            k, _, v = line.partition(" ")
            out[k] = v
        return {k: b"".join(int(w, 16).to_bytes(4, "little") for w in v.split()) for k, v in out.items() if k in ("mfma", "enc", "bfly", "bflyR", "bflyinv")}
    return run


TABLE_SHAPES = sorted(set(X.DECODE_SHAPES) | set(X.TEAM_SHAPES) | {(n, d, 0) for n, d in X.PAIR_SHAPES + X.ROW_ENCODE_SHAPES})


@pytest.mark.parametrize("n,d,t", TABLE_SHAPES)
def test_model_tables_are_the_products_fr(dump, n, d, t):
    """byte for byte: the decode rows, the encode's rows (one per point), the point pairs, the pairs times 2^261 (triple generation) and
    the pairs of the inverse transform"""
    o = dump("fr", n, d, t)
    m = d + 1
    V = X.vandermonde("fr", n, m)
    half = X.domain_size(n) // 2
    if m <= 15:
        assert o["mfma"] == MM.plain_table_bytes(X.decode_rows("fr", n, d, t, tuple(range(n))))
        assert o["enc"] == MM.plain_table_bytes(V)
    assert len(o["bfly"]) == min(half, n) * (m * 1024 + 256) and o["bfly"] == MM.pair_table_bytes(V, half)
    if m <= 15:
        assert len(o["bflyR"]) > 0 and o["bflyR"] == MM.pair_table_bytes(X.vandermonde("fr", n, m, MM.RADIX % R), half)
    if n == X.DEG_N:
        assert len(o["bflyinv"]) == 8 * (16 * 1024 + 256) and o["bflyinv"] == MM.pair_table_bytes(X.inverse_transform(n), n // 2)


def test_model_tables_are_the_products_goldilocks(dump):
    n, d, t = X.GL_SHAPES[0]
    o = dump("gl", n, d, t)
    assert o["mfma"] == MM.gl_table_bytes(X.decode_rows("gl", n, d, t, tuple(range(n))))
    assert o["enc"] == MM.gl_table_bytes(X.vandermonde("gl", n, d + 1))


# ---- the model's values against big-int arithmetic ---------------------------------------------------------------------------------
def test_epilogue_values_are_dot_products():
    rng = random.Random(5)
    C = X.decode_rows("fr", 16, 5, 5, tuple(range(16)))
    rows = MM.plain_table(C)
    pairs = MM.pair_table(X.vandermonde("fr", 13, 5), 8)
    V = X.vandermonde("fr", 13, 5)
    chunks = [[rng.randrange(R) for _ in range(6)] for _ in range(40)] + [[0] * 6, [R - 1] * 6, [1] + [0] * 5]
    Xb = MM.chunk_bytes(chunks)
    for j, row in enumerate(rows):
        for g, L in enumerate(row.sums(Xb)):
            want = MM.dot(C[j], chunks[g], R)
            res = MM.reduce_words(MM.halves(L))
            assert res["value"] == want and res["k"] == res["k_needed"] <= 1
            ok = MM.verify_tile(MM.halves(L), want)
            assert not ok["bad"] and ok["top_eq_q"] and ok["words_equal"]
            for bit in X.TAMPER_BITS:
                if want ^ (1 << bit) < R:
                    assert MM.verify_tile(MM.halves(L), want ^ (1 << bit))["bad"], (j, g, bit)
    chunks5 = [c[:5] for c in chunks]
    Xb = MM.chunk_bytes(chunks5)
    for p, pr in enumerate(pairs):
        E, T, plus, minus = pr.sums(Xb)
        for g in range(len(chunks5)):
            assert MM.reduce_words(MM.halves(None, (E[g], T[g], 1)))["value"] == MM.dot(V[p], chunks5[g], R) == MM.reduce_words(MM.halves(plus[g]))["value"]
            if pr.partner:
                assert MM.reduce_words(MM.halves(None, (E[g], T[g], -1)))["value"] == MM.dot(V[p + 8], chunks5[g], R)
    Cg = X.decode_rows("gl", 31, 10, 10, tuple(range(31)))
    chunks = [[rng.randrange(P) for _ in range(11)] for _ in range(40)] + [[0] * 11, [P - 1] * 11]
    Xb = MM.chunk_bytes(chunks, 8)
    for j, row in enumerate(MM.gl_table(Cg)):
        for g, L in enumerate(row.sums(Xb)):
            assert MM.gl_finish(L)["value"] == MM.dot(Cg[j], chunks[g], P)
    for a, x in list(X.SUB_PAIRS.values()) + [(rng.randrange(R), rng.randrange(R)) for _ in range(200)]:
        assert MM.sub_mod_r(a, x)[0] == (a - x) % R


def test_sub_pairs_borrow_where_they_say():
    """sub_mod_r: the low 128 bits alone, the high half alone, both ends with equal high halves, not at all, a == x, and the low half's
    '+ r' with and without a carry"""
    info = {k: MM.sub_mod_r(a, x)[1] for k, (a, x) in X.SUB_PAIRS.items()}
    assert all(a < R and x < R for a, x in X.SUB_PAIRS.values())
    key = lambda i: (i["b_lo"], i["b_hi"], i["b2"], i["neg"])   # noqa: E731
    assert key(info["low_only"]) == key(info["low_only_high_words"]) == (1, 0, 0, False)
    assert key(info["high_only_no_carry"]) == key(info["high_only_carry"]) == (0, 1, 0, True)
    assert (info["high_only_no_carry"]["c"], info["high_only_carry"]["c"]) == (0, 1)
    assert key(info["both_ends_equal_high_carry"]) == key(info["both_ends_equal_high_no_carry"]) == (1, 0, 1, True)
    assert (info["both_ends_equal_high_carry"]["c"], info["both_ends_equal_high_no_carry"]["c"]) == (1, 0)
    assert key(info["both_borrow"]) == (1, 1, 0, True)
    assert key(info["none"]) == key(info["none_top"]) == (0, 0, 0, False)
    for k in ("equal_zero", "equal_top", "equal_mid"):
        assert key(info[k]) == (0, 0, 0, False) and MM.sub_mod_r(*X.SUB_PAIRS[k])[0] == 0
    assert MM.sub_mod_r(*X.SUB_PAIRS["zero_minus_top"])[0] == 1 and MM.sub_mod_r(*X.SUB_PAIRS["one_minus_two"])[0] == R - 1


# ---- the coverage proof --------------------------------------------------------------------------------------------------------------
def capped_extremes(dig, bias, width, cap, sign=None):
    """per digit, the extremes of the digit sum over inputs whose top byte per element is at most `cap`"""
    top = (np.arange(dig.shape[0]) % width) == width - 1
    hi_s = np.where(top, cap - 128, 127)[:, None]
    d = dig if sign is None else dig * sign[:, None]
    b = np.array(bias, dtype=np.int64)
    return b + (np.minimum(d, 0) * hi_s).sum(0) - 128 * np.maximum(d, 0).sum(0), b + (np.maximum(d, 0) * hi_s).sum(0) - 128 * np.minimum(d, 0).sum(0)


def replay(case, sums, g, j):
    return MM.reduce_words(MM.halves(sums[j][g]))


FR_CASES = ([("pairs", s) for s in X.PAIR_SHAPES] + [("triple", X.TRIPLE_SHAPE[:2]), ("inverse", (X.DEG_N,))] +
            [("rows", s) for s in X.ROW_ENCODE_SHAPES + [X.TEAM_SHAPES[0][:2]]] + [("decode", s) for s in X.DECODE_SHAPES])
BUILD = {"pairs": X.pair_case, "triple": X.triple_case, "inverse": X.inverse_case, "rows": X.row_encode_case, "decode": X.decode_case}
PAIR_CLASSES = {"plus_max", "plus_min", "minus_max", "minus_min", "T_negative", "E_lowest"}
COMMON_CLASSES = {"value_max", "value_min", "slow_solved", "search_best", "slow_alone", "slow_tile", "slow_ragged", "filler"}


@pytest.mark.parametrize("kind,shape", FR_CASES, ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else v)
def test_fr_coverage(kind, shape):
    case = BUILD[kind](*shape)
    m = case.m
    assert all(0 <= v < R for ch in case.x for v in ch) and all(len(ch) == m for ch in case.x), "canonical inputs only"
    assert set(case.classes) == COMMON_CLASSES | (PAIR_CLASSES if case.pairs else {"digit_max", "digit_min"}) | {"inverse": {"low_degree"}, "pairs": {"constant"}, "rows": {"constant"}}.get(kind, set())
    sums = X.sums_by_row(case, case.x)
    lo, hi = min(int(v.min()) for v in sums.values()), max(int(v.max()) for v in sums.values())
    assert 0 <= lo and hi < MM.LIMIT, "a digit sum outside the interval the carry pass assumes: a product bug"
    # at least as wide as the per-digit extremes from the table's signs, in every (row, digit)
    if case.pairs is None:
        for j, row in enumerate(case.rows):
            want_lo, want_hi = capped_extremes(row.dig, row.bias, 32, 0x72)
            assert (sums[j].min(0) <= want_lo).all() and (sums[j].max(0) >= want_hi).all(), j
    else:
        Xb = MM.chunk_bytes(case.x)
        odd = np.array([-1 if (k // 32) & 1 else 1 for k in range(32 * m)])
        min_E = min_T = 1 << 60
        for p, pr in enumerate(case.pairs):
            want_lo, want_hi = capped_extremes(pr.dig, pr.row.bias, 32, 0x72)
            assert (sums[p].min(0) <= want_lo).all() and (sums[p].max(0) >= want_hi).all(), p
            if pr.partner:
                want_lo, want_hi = capped_extremes(pr.dig, pr.b2, 32, 0x72, odd)
                assert (sums[p + case.half].min(0) <= want_lo).all() and (sums[p + case.half].max(0) >= want_hi).all(), p
            E, T, _, _ = pr.sums(Xb)
            min_E, min_T = min(min_E, int(E.min())), min(min_T, int(T.min()))
            # E alone cannot be negative whatever the input (the table's own extreme), T alone can and does
            floor_E = np.array(pr.bE) + 127 * np.minimum(pr.dig_even, 0).sum(0) - 128 * np.maximum(pr.dig_even, 0).sum(0)
            assert (floor_E > 0).all(), p
            neg = [g for g in case.classes["T_negative"] if (T[g] < 0).any()]
            assert len(neg) >= 1 or not pr.dig_odd.any(), p
        assert min_E > 0 and min_T < 0
        for g in case.classes["T_negative"]:              # the pair-level add of a negative T wraps 32 bits and still gives the sum
            for p, pr in enumerate(case.pairs):
                E, T, plus, minus = (v[0] for v in pr.sums(Xb[g:g + 1]))
                if (T < 0).any():
                    assert MM.halves(None, (E, T, 1)) == MM.halves(plus) and (not pr.partner or MM.halves(None, (E, T, -1)) == MM.halves(minus))
    # the slow path: every solved target replayed
    seen = {}
    kmax = 0
    for g, (j, y) in case.targets.items():
        res = replay(case, sums, g, j)
        assert res["value"] == MM.dot(case.C[j], case.x[g], R) and (y is None or res["value"] == y), (g, j)
        assert res["k"] == res["k_needed"] <= MM.SLOW_ITERATIONS, "more subtractions needed than the slow path makes: a product bug"
        kmax = max(kmax, res["k"])
        if y is not None:
            seen.setdefault(y, []).append(res)
    for y in (0, 1, 2, 1 << 200):
        assert all(not r["fast"] and r["k"] == 1 for r in seen[y]), y
    for y in (R - 1, R - 2, X.TOP, X.TOP + 0x1234567):
        assert all(not r["fast"] and r["k"] == 0 and r["top_is_rtop"] for r in seen[y]), y
    assert all(r["fast"] for r in seen[X.TOP - 1])
    for g in case.classes.get("constant", []):           # every row of a constant polynomial is its value
        want = case.x[g][0]
        for j in case.reduce_rows:
            res = replay(case, sums, g, j)
            assert res["value"] == want and res["fast"] == all(r["fast"] for r in seen[want]) and res["k"] == res["k_needed"], (g, j)
    assert {b for rs in seen.values() for r in rs for b in r["borrows"]} == {0, 1}, "the low half's borrow: handed up and not"
    assert all(r["cin"] != 0 for rs in seen.values() for r in rs)
    # a bounded search over uniform inputs on one row finds nothing deeper (the module docstring says why)
    rng = random.Random(case.G)
    rand = [[rng.randrange(R) for _ in range(m)] for _ in range(256)]
    rs = X.sums_by_row(case, rand)[case.search_row]
    for L in rs:
        q, res = X.fr_quick(L)
        assert 0 <= res < 2 * R
        kmax = max(kmax, res // R)
    assert kmax == 1
    # the layout: a slow chunk alone among fast ones, a whole slow tile, a slow chunk last in the ragged tile
    def slow_rows(g):
        return [j for j in case.reduce_rows if not replay(case, sums, g, j)["fast"]]
    a, f, rg = case.layout["alone"], case.layout["full_tile"], case.layout["ragged"]
    assert a % 32 == 17 and f % 32 == 0 and rg == case.G - 1 and case.G % 32 == 5
    tile = range(a - 17, a + 15)
    assert [g for g in tile if slow_rows(g)] == [a]
    assert all(slow_rows(g) for g in range(f, f + 32))
    assert slow_rows(rg) and not any(slow_rows(g) for g in range(rg - 4, rg))
    print("%s %s: G = %d, digit sums 0x%06x .. 0x%06x, largest k = %d" % (kind, shape, case.G, lo, hi, kmax))


@pytest.mark.parametrize("n,d,t", X.DECODE_SHAPES)
def test_decode_chunks_verify_and_tampered_ones_do_not(n, d, t):
    """the other senders' values come from the oracle: every verify row of every chunk passes verify_tile; a claimed value with one bit
    flipped (bits 0, 31, 32, 127, 128, 253) fails it, through the word comparison and, for bit 0 .. 31, through another q"""
    case = X.decode_case(n, d, t)
    y = X.evals_of(case)
    claimed = X.fr_ints(y[d + 1:d + t + 1])
    sums = X.sums_by_row(case, case.x)
    step = max(1, case.G // 150)
    for r in range(t):
        for g in list(range(0, case.G, step)) + list(range(case.layout["alone"] - 17, case.G)):
            v = MM.verify_tile(MM.halves(sums[r][g]), claimed[r][g])
            assert not v["bad"] and v["top_eq_q"], (r, g)
    ev, info = X.tampered(case, y)
    assert ev.shape[1] == 32 and {bit for _, s, bit in info if s is not None} == set(X.TAMPER_BITS)
    vals = X.fr_ints(ev)
    for k, (src, sender, bit) in enumerate(info):
        assert all(vals[s][k] < R for s in range(n))
        if sender is not None:
            r = sender - (d + 1)
            assert vals[sender][k] == claimed[r][src] ^ (1 << bit)
            v = MM.verify_tile(MM.halves(sums[r][src]), vals[sender][k])
            assert v["bad"] and not v["words_equal"] and (v["q"] != MM.verify_tile(MM.halves(sums[r][src]), claimed[r][src])["q"]) == (bit < 32)


@pytest.mark.parametrize("n,d,t", X.GL_SHAPES)
def test_goldilocks_coverage(n, d, t):
    for case in (X.gl_encode_case(n, d), X.gl_decode_case(n, d, t)):
        assert all(0 <= v < P for ch in case.x for v in ch)
        sums = X.sums_by_row(case, case.x, 8)
        lo, hi = min(int(v.min()) for v in sums.values()), max(int(v.max()) for v in sums.values())
        assert 0 <= lo and hi < MM.LIMIT_GL
        w2max, seen = 0, {}
        for j, row in enumerate(case.rows):
            want_lo, want_hi = capped_extremes(row.dig, row.bias, 8, 0xfe)
            assert (sums[j].min(0) <= want_lo).all() and (sums[j].max(0) >= want_hi).all(), j
            for g in case.classes["value_max"] + case.classes["digit_max"][::7]:
                res = MM.gl_finish(sums[j][g])
                assert res["value"] == MM.dot(case.C[j], case.x[g], P)
                w2max = max(w2max, res["w2"])
        assert w2max < 1 << 17
        for g, (j, y) in case.targets.items():
            res = MM.gl_finish(sums[j][g])
            assert res["value"] == y == MM.dot(case.C[j], case.x[g], P)
            seen.setdefault(y, []).append((res["wrap"], res["ge_p"]))
        # results below 2^32 - 1 land on V + p after the fold (one subtraction), from 2^32 - 1 on the 64-bit sum wraps, large ones do neither
        for y in (0, 1, (1 << 32) - 2):
            assert set(seen[y]) == {(False, True)}, y
        for y in ((1 << 32) - 1, 1 << 32, (1 << 40) + 3):
            assert set(seen[y]) == {(True, False)}, y
        for y in (P - (1 << 32), P - 2, P - 1):
            assert set(seen[y]) == {(False, False)}, y
        print("goldilocks %s: G = %d, digit sums 0x%06x .. 0x%06x, w2 up to 0x%x" % ((n, d, t), case.G, lo, hi, w2max))


# ---- which kernel each case takes ----------------------------------------------------------------------------------------------------
def _plan(tool, queries):
    subprocess.check_call(["make", "-C", CPP, tool], stdout=subprocess.DEVNULL)
    text = "".join(" ".join(map(str, q)) + "\n" for q in queries)
    p = subprocess.run([os.path.join(CPP, tool)], input=text, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = p.stdout.splitlines()
    assert len(lines) == len(queries)
    return lines


def test_routes_are_pinned():
    """every (call, knobs, G, shape) tests/test_gpu_mfma_edges.py runs, through the planners: a later threshold change cannot quietly send
    these inputs to another kernel"""
    enc = X.encode_routes()
    for (q, want), line in zip(enc, _plan("encode_routes_dump", [q for q, _ in enc])):
        assert line.startswith(want), (q, line)
    dec = X.decode_routes()
    for (q, want), line in zip(dec, _plan("recover_routes_dump", [q for q, _ in dec])):
        assert line.startswith(want), (q, line)


def test_sub_case_reaches_every_pair_behind_both_kinds_of_row():
    """the FpMul inputs of the SUB decode: every pair of SUB_PAIRS is (a_p, x_p) for a sender behind an interpolation row (the B operand
    of the MFMAs) and for a sender behind a verify row (the claimed value), in the first half (a - x) and in the second (b - y)"""
    n, t = X.SUB_SHAPE
    case = X.sub_case(n, t)
    assert case["N"] % 32 == 0 and X.mfma_sub_covers(t + 1)
    for minuend, subtrahend in (("ta", "x"), ("tb", "y")):
        for who in (case["low"], case["ver"]):
            seen = {(col[minuend][p], col[subtrahend][p]) for col in case["cols"] for p in who}
            assert set(X.SUB_PAIRS.values()) <= seen, (minuend, [k for k, v in X.SUB_PAIRS.items() if v not in seen])
    assert all(0 <= v < R for col in case["cols"] for nm in ("x", "y", "ta", "tb", "tc", "rint") for v in col[nm])
