"""tests/gao_inputs.py does what it says, without a GPU: the instrumented restatement returns what oracle.spec / oracle.spec_gl return,
every named case reaches the branch events it is named for and the result known by construction, every event is reached in every launch
shape of k_gao (the coverage table; the constructions the generator declared impossible are listed here), the C oracle agrees with the
Python one, and the kernels each call of tests/test_gpu_gao_edges.py takes are pinned through the route planner.

The Python oracle pays O(n^3) big-integer operations per OEC round (3.5 s at n = 255 over Fr, and a word takes up to t rounds), the
restatement O(n^2).  Compared with the Python oracle: every case with n <= 32, every case of the d = 0 shapes (few known points) at every
n, a sample of the cases (one per kind of word) at n = 63, 64 and 127, every stand-alone case with n <= 64, and a few hundred random words.
Compared with the C oracle, which tests/test_oracle_c.py and tests/test_oracle_gl_c.py hold to the Python one: every case with n <= 64,
every case of the d = 0 shapes, the Goldilocks cases at n = 127 and every stand-alone case.  The C oracle needs 0.1 - 2 s per word at the
large n; there tests/test_gpu_gao_edges.py, which computes those answers anyway, checks them against the results known by construction
before it uses them."""
import os
import random
import subprocess

import pytest

from tests import gao_inputs as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
FIELDS = ("fr", "goldilocks")
EVENTS = ("no_eea", "g1_deficient", "later_quotient_deg>=2", "remainder_drop>1", "eea_exact", "dg<dv", "remainder_nonzero", "quotient_deg>=k",
          "dv=0", "quotient_short", "accept_fail", "success", "oec_fail")
# (bucket, event) NOT reached by any case: none.  The constructions that do not exist, by shape (the generator says why): the top three
# coefficients of g1 cannot vanish with the EEA still entered unless t - 3 >= (t + 1) // 2, i.e. t >= 6 -- g1_deficient is reached through
# s = 1 and s = 2 there, and the s = 3 word is kept as `degenerate_s3_below_threshold` (round 1 without an EEA step).
HOLES = set()
IMPOSSIBLE = {shape: ["degenerate_s3"] for shape in X.MAIN_SHAPES if shape[1] < 6}
SPEC_GAO_MAX_N = 64
SPEC_SAMPLE = {63: ("boundary_r8_emax+1_pm1", "zero_polynomial_2_errors", "degree_mid_word", "degenerate_s2", "second_codeword", "late_errors"),
               127: ("zero_polynomial_2_errors", "degenerate_s2", "subset_one_error_too_many")}
SPEC_SAMPLE[64] = SPEC_SAMPLE[63]


def spec_checked(b, c):
    return b.n <= 32 or b.d == 0 or c.name in SPEC_SAMPLE.get(b.n, ())


def spec_recover(F, c):
    try:
        return "ok", F.S.recover_secret([F.S.Share(v, i, c.d) for i, v in zip(c.ids, c.vals)], c.n, c.t)[0]
    except F.S.ShareErr as e:
        return "err", e.code


def spec_gao(F, c):
    try:
        return "ok", F.S.gao_rs_decode(c.received, c.k, c.n, c.erasures)
    except F.S.ShareErr as e:
        return "err", e.code


_traced = {}


def traced(F):
    """[(batch, [(case, Trace, result)])] of every batch of the field, computed once"""
    if F.name not in _traced:
        _traced[F.name] = [(b, [(c,) + c.trace() for c in b.cases]) for b in X.all_batches(F)]
    return _traced[F.name]


@pytest.mark.parametrize("field", FIELDS)
def test_restatement_returns_what_the_spec_returns_on_the_cases(field):
    F = X.FIELDS[field]
    compared = 0
    for b, rows in traced(F):
        for c, tr, res in rows:
            if spec_checked(b, c):
                assert res == spec_recover(F, c), (b.n, b.t, b.d, b.set_name, c.name)
                compared += 1
    assert compared > 150
    for n, t, d in X.MAIN_SHAPES:
        for c in X.gao_cases(F, n, d + 1):
            if n <= SPEC_GAO_MAX_N:
                assert c.trace()[1] == spec_gao(F, c), (n, c.name)


@pytest.mark.parametrize("field", FIELDS)
def test_restatement_returns_what_the_spec_returns_on_random_words(field):
    """300 random words as tests/test_gpu_random_shapes.py draws them (n <= 20, a fifth of the polynomials of low degree, up to t + 1
    errors, senders missing), and 100 random stand-alone decodes"""
    F = X.FIELDS[field]
    p, rng = F.mod, random.Random(field)
    outcomes = set()
    for _ in range(300):
        n = rng.randint(4, 20)
        t = rng.randint(1, (n - 1) // 3)
        d = rng.randint(0, n - 2 * t - 1)
        poly = [rng.randrange(p) for _ in range(d + 1)]
        if rng.randrange(5) == 0:
            cut = rng.randrange(d + 1)
            poly[cut:] = [0] * (d + 1 - cut)
        ids = rng.sample(range(n), rng.randint(d + t + 1, n))
        bad = rng.sample(ids, rng.randint(0, min(len(ids), t + 1)))
        vals = X.word(F, n, ids, poly, {i: rng.randrange(1, p) for i in bad})
        c = X.Case("random", F, n, t, d, ids, [vals[i] for i in ids])
        tr, res = c.trace()
        assert res == spec_recover(F, c), (n, t, d, ids, bad)
        outcomes.add((res[0], tr.optimistic))
    assert outcomes == {("ok", True), ("ok", False), ("err", False)}
    for _ in range(100):
        n = rng.randint(2, 20)
        k = rng.randint(0, n)
        erasures = rng.sample(range(n), rng.randint(0, n - 1))
        msg = [rng.randrange(p) for _ in range(k)]
        vals = X.word(F, n, range(n), msg, {i: rng.randrange(1, p) for i in rng.sample(range(n), rng.randint(0, min(3, n)))})
        c = X.GaoCase("random", F, n, k, [vals[i] for i in range(n)], erasures)
        if (n - len(set(erasures)) + k) // 2 == 0:
            continue                                              # the reference divides by the zero polynomial there
        assert c.trace()[1] == spec_gao(F, c), (n, k, erasures)


@pytest.mark.parametrize("field", FIELDS)
def test_every_case_reaches_its_events_and_its_known_result(field):
    F = X.FIELDS[field]
    for b, rows in traced(F):
        for c, tr, res in rows:
            where = (b.n, b.t, b.d, b.set_name, c.name)
            assert all(0 <= v < F.mod for v in c.vals) and sorted(c.ids) == X.sender_sets(b.n, b.t, b.d)[b.set_name], where
            assert tr.optimistic == (not c.flagged), where       # every case but the honest word fails the optimistic verification
            for event, rnd in c.wants:
                assert tr.has(event, rnd), (where, event, rnd, [sorted(e) for e in tr.rounds])
            for event, rnd in c.wants_not:
                assert not tr.has(event, rnd), (where, event, rnd)
            if c.expect is not None:
                assert res == c.expect, where
    for n, t, d in X.MAIN_SHAPES:
        # wrong values ONLY beyond round 1's known set: accepted optimistically, the kernel never sees the word
        c = X.errors_beyond_round_one(F, n, t, d)
        tr, res = c.trace()
        assert tr.optimistic and res == c.expect, (n, t, d)
        for c in X.gao_cases(F, n, d + 1):
            ev, res = c.trace()
            assert all(e in ev for e, _ in c.wants), (n, c.name, sorted(ev))
            assert c.expect is None or res == c.expect, (n, c.name)


@pytest.mark.parametrize("field", FIELDS)
def test_named_cases_by_name(field):
    """the claims of the generator's docstring, on the smallest shape, spelled out"""
    F = X.FIELDS[field]
    n, t, d = 15, 4, 6
    by_name = {c.name: (tr, res) for b, rows in traced(F) if (b.n, b.d, b.set_name) == (n, d, "all") for c, tr, res in rows}
    tr, res = by_name["degree_d+1_word"]                         # no EEA step at all, remainder zero, quotient degree >= k: every round
    assert res == ("err", 8) and len(tr.rounds) == t and all({"no_eea", "quotient_deg>=k"} <= ev and "remainder_nonzero" not in ev for ev in tr.rounds)
    tr, res = by_name["zero_polynomial_2_errors"]                # the correct division fails the acceptance count in round 1, passes in 2
    assert res == ("ok", []) and tr.success == 2 and {"accept_fail", "eea_exact"} <= tr.rounds[0]
    tr, res = by_name["boundary_r%d_emax+1_pm1" % t]             # t + 1 errors: the EEA and the division in every round
    assert res == ("err", 8) and all(ev == {"remainder_nonzero"} for ev in tr.rounds)
    tr, res = by_name["degenerate_s2"]
    assert {"g1_deficient(2)"} <= tr.rounds[0] and tr.has("later_quotient_deg>=2") and tr.has("remainder_drop>1") and res[0] == "ok"
    assert len(by_name["constant_t_errors"][1][1]) == 1 and len(by_name["degree_one_t_errors"][1][1]) == 2     # trimmed, last round
    assert by_name["constant_t_errors"][0].success == t


def test_coverage_table():
    """every event in every launch shape (lanes per chunk: 16, 32, 64, 128, 256), per field"""
    for field in FIELDS:
        F = X.FIELDS[field]
        pairs = [(b.n, tr) for b, rows in traced(F) for _, tr, _ in rows]
        pairs += [(n, c.trace()[0]) for n, t, d in X.MAIN_SHAPES for c in X.gao_cases(F, n, d + 1)]
        reached = X.bucket_table(pairs)
        missing = {(sub, e) for _, sub in X.BUCKETS for e in EVENTS if (sub, e) not in reached}
        assert missing == HOLES, (field, sorted(missing ^ HOLES))
        for n, t, d in X.MAIN_SHAPES:
            for set_name in X.sender_sets(n, t, d):
                _, impossible = X.build_cases(F, n, t, d, set_name)
                assert [nm for nm, _ in impossible] == (IMPOSSIBLE.get((n, t, d), []) if set_name == "all" else []), (n, t, d, set_name, impossible)
    # both edge values of every launch shape carry cases, one shape each with d + 2 t + 1 = n (the top lane of the group is used)
    assert sorted(n for n, _, _ in X.MAIN_SHAPES) == [15, 16, 31, 32, 63, 64, 127, 128, 255]
    assert all(d + 2 * t + 1 == n for n, t, d in X.MAIN_SHAPES)


def test_the_frozen_dg_lt_dv_seeds_are_what_the_search_finds():
    for field in FIELDS:
        for shape in X.D0_SHAPES:
            assert X.find_dg_lt_dv(X.FIELDS[field], *shape) == X.DG_LT_DV_SEED[(field, shape)], (field, shape)


def _rows_of(F, b, res):
    """(coefficients zero padded, ncoeffs, status) per chunk as batch_recover_secret reports them, from recover_secret's results"""
    out = []
    for c, tr, r in res:
        if r[0] == "err":
            out.append(([0] * (b.d + 1), 0, r[1]))
        else:
            out.append((list(r[1]) + [0] * (b.d + 1 - len(r[1])), b.d + 1 if tr.optimistic else len(r[1]), 0 if tr.optimistic else 1))
    return out


@pytest.mark.parametrize("field", FIELDS)
def test_c_oracle_agrees(field):
    """oracle.cref / oracle.cref_gl, coefficient for coefficient and error code for error code: with the Python oracle on every case with
    n <= 40 and on the stand-alone cases with n <= 64, with the restatement on the others (module docstring)"""
    F = X.FIELDS[field]
    for b, rows in traced(F):
        if b.n > 64 and b.d and (field, b.n) != ("goldilocks", 127):
            continue
        rc, co, nco, st = F.O.batch_recover(b.ids, b.array(), b.n, b.d, b.t)
        want = _rows_of(F, b, rows)
        assert F.ints(co) == [w[0] for w in want] and nco.tolist() == [w[1] for w in want] and st.tolist() == [w[2] for w in want], (b.n, b.t, b.d, b.set_name)
        assert rc == (8 if any(w[2] > 1 for w in want) else 0)
        for c, tr, res in rows:
            if b.n <= 40 and not spec_checked(b, c):             # (the others: test_restatement_returns_what_the_spec_returns_on_the_cases)
                assert res == spec_recover(F, c)
    for n, t, d in X.MAIN_SHAPES:
        for c in X.gao_cases(F, n, d + 1):
            rc, co = F.O.gao_rs_decode(F.arr(c.received), c.k, c.n, c.erasures)
            want = spec_gao(F, c) if n <= SPEC_GAO_MAX_N else c.trace()[1]
            assert (("ok", F.ints(co) if len(co) else []) if rc == 0 else ("err", rc)) == want, (n, c.name)


def test_routes_are_pinned():
    """every call of tests/test_gpu_gao_edges.py, full and P(0), through the route planner: the first kernel, rmax, where the second
    chance runs and whether k_gao un-scales inline or k_unscale follows -- as the generator claims them"""
    subprocess.check_call(["make", "-C", CPP, "recover_routes_dump"], stdout=subprocess.DEVNULL)
    for impl in X.IMPLS:
        calls = X.gpu_calls(impl)
        queries = [c.query(form) for c in calls for form in ("dev", "p0")]
        text = "".join(" ".join(map(str, q)) + "\n" for q in queries)
        p = subprocess.run([os.path.join(CPP, "recover_routes_dump")], input=text, capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, p.stderr[-2000:]
        lines = p.stdout.splitlines()
        assert len(lines) == len(queries)
        for q, line, c in zip(queries, lines, [c for c in calls for _ in range(2)]):
            head = line.split(" all=")[0]
            fields = dict(kv.split("=") for kv in head.split()[1:] if "=" in kv)
            assert head.split()[4] == "tail", (q, line)
            assert (head.split()[0], int(fields["rmax"]), fields["second"], fields["gao"]) == c.claim(), (q, line)
    # the layouts the GPU file relies on: one wave / a second, partly empty block; a second trip; both un-scaling routes
    assert {c.G for c in X.wave_calls("u29")} == {2, 3, 4, 5}
    assert [c.G for c in X.second_trip_calls("gl")] == [8195, 4099, 2051]
    assert [c.claim()[3] for c in X.second_trip_calls("u29")] == ["unscale", "inline", "inline"]
    assert all(c.claim()[3] == "unscale" and c.G % 8 for c in X.unscale_calls("u29"))
