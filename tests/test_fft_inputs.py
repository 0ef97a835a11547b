"""tests/fft_inputs.py without a GPU and without the library: the site table of the lane-per-chunk FFT encode kernels' edge tests.

Fr: every assertion of tests/fft_model.py (limb and value bounds from fft_bd, the preconditions of sub<K>, mulc_u, normalize and
canon_loose) holds on every row of every case, the model's outputs equal the oracle's, and the targeted outputs take both rare cases of
canon_loose -- the top limb reaches r's and cond_sub_r subtracts ("sub"), and it reaches r's and it does not ("nosub").

  "sub" needs a lazy value of r or more before the store.  Where fft_bd bounds an output by 1 r (it is a copy of a canonical input: a
  single coefficient in pass 0, or an index no butterfly adds to) the case cannot occur, by the bound itself.  With d = 0 it cannot occur
  in the twisted passes either: the output is mulc_u(c_0, 2^261 mod r), congruent to c_0 and below c_0 (2^261 mod r) / 2^261 + r < c_0 + r,
  so it IS c_0.  Those are the only outputs excused (sub_reachable below), and for them the test asserts that the case did NOT occur.

  Domains of up to 16 points: every output row j < n of every instantiation.  Beyond: the targeted points of each case (j = 0, n - 1, one
  per pass), and over the cases of one P every 16-point output index.

Goldilocks: per instantiation 4 096 random rows go through the model first; every branch of addm / subm / mulm they fire must fire in
the generated case, the model's outputs equal the oracle's, and r < t0, r >= P and lo < hh of mulm fire in every kernel family (random
rows fire neither of the last two).  The triple kernel's staging step and the mixing step's rows are held to the same.

Routes: tests/cpp/encode_routes_dump names Fft1, FftP, Fft1Triple or Fft1Mix first for every call of tests/test_gpu_fft_edges.py."""
import os
import subprocess

import numpy as np
import pytest

from tests import fft_inputs as X
from tests import fft_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FFT1 = X.fft1_shapes()
FFTP = X.fftP_shapes()
_reports = {}


def ids(shapes):
    return ["-".join(map(str, s)) for s in shapes]


def fr_report(family, shape):
    """the model over every row of one Fr case: outputs against the oracle, the cases of canon_loose per output row, the maxima"""
    key = (family, shape)
    if key in _reports:
        return _reports[key]
    if family == "fft1":
        LOG, CNT, n = shape
        c = X.chunk_case("fr", "fft1", n, CNT - 1)
    else:
        Pn, dp1, n = shape
        c = X.fftP_case("fr", Pn, dp1, n)
    rc, want = X.FR.O.vandermonde_apply(c.array(), c.n, c.d)
    assert rc == 0
    want = X.FR.ints(want)
    stats, seen = M.Stats(), {}
    for g, row in enumerate(c.rows):
        out, cases = M.fr_fft1(row, c.LOG, c.d + 1, c.n, stats) if family == "fft1" else M.fr_fftP(row, c.P, c.n, stats)
        assert out == [want[j][g] for j in range(c.n)], (shape, g)
        for j, case in cases.items():
            seen.setdefault(j, set()).add(case)
    _reports[key] = (c, seen, stats)
    return _reports[key]


def out_vb(c, j):
    """fft_bd's value bound of output row j"""
    if c.family == "fft1":
        return M.bounds(c.LOG, c.d + 1, 1, 1)[(c.LOG, j)][1]
    Q = 2 if c.fold else 1
    return M.bounds(4, min(c.d + 1, 16), Q, Q if j % c.P == 0 else 2 * Q)[(4, j // c.P)][1]


def sub_reachable(c, j):
    return out_vb(c, j) > 1 and c.d >= 1


def test_constants_and_case_structure():
    k = M.consts()
    assert M.value(k["U_MOD"]) == M.R and all(M.value(k["U_SUBC%d" % K]) == K * M.R for K in (2, 4, 8, 16, 32, 64))
    assert len(FFT1) == 31 + 6 and len({s[:2] for s in FFT1}) == 31
    assert len(FFTP) == 2 * 19 + 2 * 7 and {n for Pn, dp1, n in FFTP if Pn == 16} >= {256, 129}
    # the shapes that get the small batches and the strided / party-batched calls are generated shapes (a tuple that is none never matches)
    assert set(X.SMALL_G_FFT1) | set(X.STRIDED_FFT1) <= set(FFT1) and set(X.SMALL_G_FFTP) | set(X.STRIDED_FFTP) <= set(FFTP)
    assert len(set(X.SMALL_G_FFT1)) == len(set(X.SMALL_G_FFTP)) == 4 and len(set(X.STRIDED_FFT1)) == len(set(X.STRIDED_FFTP)) == 3
    assert any(dp1 > 16 for _, dp1, _ in X.SMALL_G_FFTP) and any(n == 256 for _, _, n in X.SMALL_G_FFTP)
    small = [q for q, _ in X.route_queries() if q[0] == "shares" and q[6] == 1 and q[3] in X.SMALL_G]
    assert len(small) == 2 * 8 * len(X.SMALL_G)                            # 4 fft1 + 4 fftP shapes per field, each at G = 1, 63, 64, 65
    for field in ("fr", "goldilocks"):
        F = X.FIELDS[field]
        for c in X.fft1_cases(field) + X.fftP_cases(field):
            dp1 = c.d + 1
            assert c.G % 64 == 1 and c.G >= 129 and all(len(r) == dp1 and all(0 <= v < F.mod for v in r) for r in c.rows)
            assert [0] * dp1 in c.rows and [F.mod - 1] * dp1 in c.rows and [X.ALL_ONES[field]] * dp1 in c.rows
            assert all([v] + [0] * c.d in c.rows for v in F.edge)
            assert all([(F.mod - 1) * int(i == k) for i in range(dp1)] in c.rows for k in range(dp1))
            if c.fold:
                assert [X.ALL_ONES[field] if i in (0, 16) else 0 for i in range(dp1)] in c.rows
            for g, j, v in c.targets:                                     # the targeted outputs are what they claim
                assert X.evaluate(F, c.rows[g], c.n, j) == v and all(c.rows[g][1:])
            want = set(range(c.n)) if X.domain_size(c.n) <= 16 else {0, c.n - 1}
            assert {j for _, j, _ in c.targets} >= want and {v for _, _, v in c.targets} == set(X.TARGETS[field])
            if c.family == "fftP":
                assert {j % c.P for _, j, _ in c.targets} == set(range(c.P))


@pytest.mark.parametrize("shape", FFT1, ids=ids(FFT1))
def test_fr_fft1_model_and_sites(shape):
    c, seen, stats = fr_report("fft1", shape)
    for j in range(c.n):
        assert "nosub" in seen[j], (shape, j, seen[j])
        if sub_reachable(c, j):
            assert "sub" in seen[j], (shape, j, seen[j])
        else:
            assert "sub" not in seen[j] and out_vb(c, j) == 1


@pytest.mark.parametrize("shape", FFTP, ids=ids(FFTP))
def test_fr_fftP_model_and_sites(shape):
    c, seen, stats = fr_report("fftP", shape)
    for j in sorted({j for _, j, _ in c.targets}):
        assert "nosub" in seen[j], (shape, j, seen[j])
        if sub_reachable(c, j):
            assert "sub" in seen[j], (shape, j, seen[j])
        else:
            assert "sub" not in seen[j] and c.d == 0


def test_fr_fftP_every_16_point_index_per_P():
    """over the cases of one P, every index of the 16-point transform stores an output in both rare cases"""
    for Pn in (2, 4, 8, 16):
        both = set()
        for shape in FFTP:
            if shape[0] == Pn:
                c, seen, _ = fr_report("fftP", shape)
                both |= {j // Pn for j, s in seen.items() if {"sub", "nosub"} <= s}
        assert both == set(range(16)), (Pn, both)


def fr_triple_report(shape):
    """the triple kernel's model over every element of the one-party case: the staged coefficients, the outputs, the staging step's cases"""
    key = ("triple", shape)
    if key not in _reports:
        LOG, cnt, n = shape
        t = X.triple_case("fr", LOG, cnt, n, 1)
        rows = t["c"][0]
        rc, want = X.FR.O.vandermonde_apply(X.FR.arr(rows), n, cnt - 1)
        assert rc == 0
        want = X.FR.ints(want)
        stats, staged_cases = M.Stats(), set()
        for g, row in enumerate(rows):
            e = slice(g * cnt, (g + 1) * cnt)
            out, _, staged, sc = M.fr_fft1_triple(t["a"][0][e], t["b"][0][e], t["r2t"][0][e], LOG, cnt, n, stats)
            assert staged == row and out == [want[j][g] for j in range(n)], (g,)
            staged_cases |= set(sc)
        _reports[key] = (t, staged_cases, stats)
    return _reports[key]


def fr_mix_report(n):
    key = ("mix", n)
    if key not in _reports:
        c = X.chunk_case("fr", "fft1", n, n - 1)
        rows = X.mix_rows("fr", n)
        rc, want = X.FR.O.vandermonde_apply(X.FR.arr(rows), n, n - 1)
        assert rc == 0
        want = X.FR.ints(want)
        stats, seen = M.Stats(), {}
        for g, row in enumerate(rows):
            out, cases = M.fr_fft1(row, c.LOG, n, n, stats)
            assert out == [want[j][g] for j in range(n)]
            for j, case in cases.items():
                seen.setdefault(j, set()).add(case)
        _reports[key] = (c, seen, stats)
    return _reports[key]


def test_fr_model_maxima_stay_below_the_bounds():
    """the largest limb and value any butterfly produced, as fractions of fft_bd's bound, per kernel family (printed for the record; no
    threshold but 1)"""
    total = M.Stats()
    families = (("fft1", [fr_report("fft1", sh)[2] for sh in FFT1]), ("fftP", [fr_report("fftP", sh)[2] for sh in FFTP]),
                ("fft1_triple", [fr_triple_report(sh)[2] for sh in X.triple_shapes()]), ("fft1_mix", [fr_mix_report(n)[2] for n in X.MIX_N["fr"]]))
    for family, all_stats in families:
        fam = M.Stats()
        for st in all_stats:
            fam.merge(st)
        print("%s: %d butterflies, largest limb %.6f of its bound at %s, largest value %.6f of its bound at %s" %
              (family, fam.butterflies, fam.limb, fam.limb_at, fam.val, fam.val_at))
        print("  largest limb / bound, by limb bound: " + ", ".join("%d: %.4f" % kv for kv in sorted(fam.by_lbu.items())))
        print("  largest value / bound, by value bound: " + ", ".join("%d: %.4f" % kv for kv in sorted(fam.by_vb.items())))
        assert fam.butterflies > 0
        total.merge(fam)
    assert 0 < total.limb <= 1 and 0 < total.val <= 1       # (as floats; the model asserts the strict bounds on the integers)


@pytest.mark.parametrize("LOG,cnt,n", X.triple_shapes())
def test_fr_triple_model(LOG, cnt, n):
    """the staging step gives the chunk-major row (so the transform's sites are the fft1 case's), on every element, under the model's
    assertions; both parties' forms are valid inputs"""
    for parties in (1, 3):
        t = X.triple_case("fr", LOG, cnt, n, parties)
        assert all(len(t[k]) == parties and len(t[k][0]) == t["G"] * cnt for k in ("a", "b", "r2t"))
    t, staged_cases, _ = fr_triple_report((LOG, cnt, n))
    assert staged_cases == {"below", "sub", "nosub"}                       # the staging step's own store takes every case
    assert set(t["a"][0]) >= set(X.FR.edge) and set(t["b"][0]) >= set(X.FR.edge)


@pytest.mark.parametrize("n", X.MIX_N["fr"])
def test_fr_mix_model(n):
    """k_eval_fft1_mix is the fft1 transform of <LOG, n> reading rows: its n K chunks are the (n, n - 1) case, taken round again"""
    c, seen, _ = fr_mix_report(n)
    K, rows = X.mix_K("fr", n), X.mix_rows("fr", n)
    assert K % 64 and len(rows) == n * K >= 129 and rows[:min(c.G, n * K)] == c.rows[:n * K]
    assert all({"sub", "nosub"} <= seen[j] for j in range(n)), seen


# ---- Goldilocks --------------------------------------------------------------------------------------------------------------------------
_gl_traces = {}


def gl_run(c, rows):
    x = np.array(rows, dtype=np.uint64).reshape(len(rows), c.d + 1)
    return M.gl_fft1(x, c.LOG, c.d + 1, c.n) if c.family == "fft1" else M.gl_fftP(x, c.P, c.n)


def gl_check(c):
    key = (c.family, c.n, c.d)
    if key in _gl_traces:
        return _gl_traces[key]
    rng = np.random.default_rng(c.n * 1000 + c.d)
    rnd = rng.integers(0, X.P, size=(4096, c.d + 1), dtype=np.uint64)
    _, base = gl_run(c, rnd)
    out, tr = gl_run(c, c.rows)
    rc, want = X.GL.O.vandermonde_apply(c.array(), c.n, c.d)
    assert rc == 0 and np.array_equal(out, want), (c.family, c.n, c.d)
    missing = [b for b in M.BRANCHES if base.fired[b] and not tr.fired[b]]
    assert not missing, (c.family, c.n, c.d, missing)
    _gl_traces[key] = tr
    return tr


@pytest.mark.parametrize("shape", FFT1, ids=ids(FFT1))
def test_gl_fft1_model_and_branches(shape):
    LOG, CNT, n = shape
    c = X.chunk_case("goldilocks", "fft1", n, CNT - 1)
    tr = gl_check(c)
    first = [(op, k) for op, k in tr.muls if k != 1]
    if first:                                                             # the first multiplied value takes every edge value
        ops = {int(v) for v in first[0][0]}
        assert ops >= set(X.EDGE_GL), (shape, sorted(set(X.EDGE_GL) - ops))
        assert len(c.extra) >= len(X.EDGE_GL)
    else:
        assert c.extra == []


@pytest.mark.parametrize("shape", FFTP, ids=ids(FFTP))
def test_gl_fftP_model_and_branches(shape):
    Pn, dp1, n = shape
    c = X.fftP_case("goldilocks", Pn, dp1, n)
    tr = gl_check(c)
    w = X.GL.S.domain_omega(16 * Pn)
    for _, r, k, v in c.extra:                                            # operand v under twist (r, k), and product v
        tw = pow(w, r * k, X.P)
        assert any(row[k] == v for row in c.rows) and any(row[k] * tw % X.P == v for row in c.rows)
    assert len(c.extra) == len(X.EDGE_GL)


def test_gl_rare_mulm_branches_per_family():
    """r < t0 and r >= P fire in each of fft1, fftP plain and fftP fold: the search of fft_inputs.gl_rare_operand found an operand for
    every family, none is recorded as unreachable.  So does lo < hh, which random operands do not fire either (the edge values do)"""
    fired = {}
    for c in X.fft1_cases("goldilocks") + X.fftP_cases("goldilocks"):
        fam = fired.setdefault(c.family + ("_fold" if c.fold else ""), {"mulm_r_lt_t0": 0, "mulm_r_ge_p": 0, "mulm_lo_lt_hh": 0})
        tr = gl_check(c)
        for b in fam:
            fam[b] += tr.fired[b]
    assert set(fired) == {"fft1", "fftP", "fftP_fold"}
    for fam, f in fired.items():
        assert f["mulm_r_lt_t0"] > 0 and f["mulm_r_ge_p"] > 0 and f["mulm_lo_lt_hh"] > 0, (fam, f)


@pytest.mark.parametrize("n", X.MIX_N["goldilocks"])
def test_gl_mix_model(n):
    """the mixing step's rows over Goldilocks: the (n, n - 1) case under the same branch table as every fft1 case, and the model on the
    n K chunks the GPU test feeds against the oracle"""
    c = X.chunk_case("goldilocks", "fft1", n, n - 1)
    gl_check(c)
    K, rows = X.mix_K("goldilocks", n), X.mix_rows("goldilocks", n)
    assert K % 64 and len(rows) == n * K >= 129 and rows[:min(c.G, n * K)] == c.rows[:n * K]
    out, _ = gl_run(c, rows)
    rc, want = X.GL.O.vandermonde_apply(X.GL.arr(rows), n, n - 1)
    assert rc == 0 and np.array_equal(out, want)


@pytest.mark.parametrize("LOG,cnt,n", X.triple_shapes())
def test_gl_triple_model(LOG, cnt, n):
    """the staging step over Goldilocks gives the chunk-major row, fires every branch that 4 096 random (a, b, r2t) fire and, by the
    operands solved for it, mulm's final subtraction; the transform behind it is the (n, d) case under the fft1 branch table"""
    t = X.triple_case("goldilocks", LOG, cnt, n, 1)
    rng = np.random.default_rng(LOG * 100 + cnt)
    base = M.GlTrace()
    M.gl_triple_stage(*(rng.integers(0, X.P, size=4096, dtype=np.uint64) for _ in range(3)), base)
    tr = M.GlTrace()
    a, b, r = (np.array(t[k][0], dtype=np.uint64) for k in ("a", "b", "r2t"))
    staged = M.gl_triple_stage(a, b, r, tr)
    assert np.array_equal(staged.reshape(-1, cnt), np.array(t["c"][0], dtype=np.uint64))
    missing = [br for br in M.BRANCHES if base.fired[br] and not tr.fired[br]]
    assert not missing and base.fired["subm_borrow"] and base.fired["mulm_r_lt_t0"], missing
    assert tr.fired["mulm_r_ge_p"] > 0 and tr.fired["mulm_lo_lt_hh"] > 0  # random operands fire neither: lo < hh needs a product whose low word is below 2^32
    assert not tr.fired["addm_wrap"] and not tr.fired["addm_ge_p"]       # the staging step does not add
    assert set(t["a"][0]) >= set(X.EDGE_GL) and set(t["b"][0]) >= set(X.EDGE_GL)
    gl_check(X.chunk_case("goldilocks", "fft1", n, cnt - 1))


# ---- routes -------------------------------------------------------------------------------------------------------------------------------
def test_every_case_takes_its_fft_kernel_first():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "cpp"), "encode_routes_dump"], stdout=subprocess.DEVNULL)
    queries = X.route_queries()
    text = "".join(" ".join(map(str, q)) + "\n" for q, _ in queries)
    p = subprocess.run([os.path.join(ROOT, "tests", "cpp", "encode_routes_dump")], input=text, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = p.stdout.splitlines()
    assert len(lines) == len(queries)
    for (q, want), line in zip(queries, lines):
        assert line.split()[0] == want, (q, line)
        if q[0] == "lists":
            assert "lists_in_kernel=1" in line, (q, line)
    assert {w for _, w in queries} == {"Fft1", "FftP", "Fft1Triple", "Fft1Mix"}
