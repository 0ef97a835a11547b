"""tests/decode_inputs.py does what it says, without a GPU.

  - tests/decode_model.py is held to plain big-integer arithmetic (unit tests) and, on every chunk of every batch, to the C oracle
    (status, coefficients, trimmed length; oracle.spec on a sample): the model cannot drift from what tests/test_gpu_decode_edges.py
    compares with.  No precondition assert of the model fires on any generated row.
  - the site table: per (kernel family, shape, form) every verify row and every output row takes each canon_loose case in some honest
    chunk (or the shape has a recorded excuse), every second-chance window that a chunk claims accepts it and takes each case on its check rows and
    on its coefficient rows, Goldilocks fires the branches
    listed -- the final `lo < hh` through a word solved for it -- and none of those recorded as unreached or impossible.
  - the Wide kernel's parameters (tests/cpp/wide_plan_dump) put every shape on the path it is there for, and the route planner
    (tests/cpp/recover_routes_dump) gives every call of the GPU file the first kernel, rmax, second-chance form and tail claimed.
  - each deliberate mistake of decode_model.MUTATIONS changes the model's answer on at least one committed input, per kernel family to
    which it applies: the evidence that the GPU file would notice a kernel that was wrong in that way.

Measured on the CPU of a build machine: 84 tests, 65 s (790 000 modelled rows, identical ones computed once; profiles/decode_edges.txt
has the closest approach to each accumulator bound and what the inputs do not reach)."""
import random
import subprocess

import pytest

from tests import decode_inputs as D
from tests import decode_model as DM
from tests import fft_model as FM

FIELDS = {"fr": (D.FR, "u29"), "goldilocks": (D.GL, "gl")}
ALL_SHAPES = D.SHAPES + tuple(s for s in D.SWEEP_SHAPES if s not in D.SHAPES)
R, P = D.R, D.P
CANON = {"slow_keep", "slow_sub", "q1"}
# Goldilocks: every branch the inputs fire -- what random rows fire (the three columns' carries, the wrap of the final fold) and the rare
# ones, the final `lo < hh` among them -- is required of every family over the shapes together; GL_REQUIRED, D.GL_UNREACHED and
# GL_IMPOSSIBLE together are all of decode_model.GL_BRANCHES; reductions 0 .. 2 reduce a column of at most 96 bits, so their hh is zero and `lo < hh` cannot be taken (asserted per row)
GL_REQUIRED = {("carry", 0), ("carry", 1), ("carry", 2), (0, "r>=P"), (1, "r<t0"), (1, "r>=P"), (3, "lo<hh"), (3, "r<t0"), (3, "r>=P")}
GL_IMPOSSIBLE = {(k, "lo<hh") for k in range(3)}
STATS = {}


# ---- the model against plain arithmetic -----------------------------------------------------------------------------------------------
def test_fr_dot_products_are_the_montgomery_sum():
    rng = random.Random(1)
    A = DM.FrModel()
    rinv = pow(FM.RADIX, -1, R)
    for m in (1, 2, 5, 6, 7, 12, 13, 25, 43):
        ys = [rng.choice((rng.randrange(R), R - 1, D.E.MAXLIMB, 0)) for _ in range(m)]
        row = [FM.const_form(rng.choice((rng.randrange(R), R - 1, 1))) for _ in range(m)]
        want = sum(y * c for y, c in zip(ys, row)) * rinv % R
        got = [A.dot_plain(ys, row), A.dot_row(ys, row)] + [A.dot_shared(ys, row, lk) for lk in (1, 2) if (1 << lk) <= m]
        assert all(g == got[0] for g in got)                         # folding and sharing move carries, never the value
        assert got[0][1] % R == want and got[0][1] < 2 * R
        assert A.canon_loose(got[0])[0][1] == want and A.cond_sub_r(got[0])[0][1] == want


def test_fr_canon_loose_cases():
    A = DM.FrModel()
    case = lambda v: A.canon_loose((FM.limbs_of(v), v))[1]                                                    # noqa: E731
    assert [case(v) for v in (0, D.E.B - 1, D.E.B, R - 1)] == ["fast", "fast", "slow_keep", "slow_keep"]
    assert [case(R + v) for v in (0, 1, D.Q1 - 1, D.Q1, D.F1 - 1, D.F1, D.F1 + 1)] == ["slow_sub"] * 5 + ["q1", "q1"]
    assert D.Q1 < D.F1 < D.Q1 + (3 << 232)                        # the estimate stays at 0 for at most two more steps of the top limb
    assert case(2 * R - 1) == "slow_keep" or case(2 * R - 1) == "q1"
    loose = ([(1 << 32) - 1] * 8 + [3 << 24], sum(((1 << 32) - 1) << 29 * i for i in range(8)) + (3 << 24 << 232))
    z, _ = A.canon_loose(loose)
    assert z[1] == loose[1] % R
    with pytest.raises(AssertionError):
        A.cond_sub_r((FM.limbs_of(2 * R), 2 * R))
    with pytest.raises(AssertionError):
        A.canon_loose((FM.limbs_of(FM.RADIX), FM.RADIX))


def test_fr_column_overflow_is_noticed():
    """seven all-ones terms without a fold stay below 2^64 (9 * 7 + 9 bits: MAX_DOT_TERMS is 6 with room to spare), 71 do not"""
    A = DM.FrModel()
    big = (1 << 261) - 1
    cols = [0] * 18
    with pytest.raises(AssertionError):
        for _ in range(71):
            prod = DM.packed(R - 1) * DM._pack(big)
            for k in range(17):
                cols[k] += (prod >> 128 * k) & DM.M128
            A._check(cols)


def test_gl_dot_products_and_branches():
    rng = random.Random(2)
    A = DM.GlModel()
    for m in (1, 2, 3, 17, 64):
        ys = [rng.choice((rng.randrange(P), P - 1, 0xFFFFFFFF, 1 << 32)) for _ in range(m)]
        row = [rng.choice((rng.randrange(P), P - 1, 1)) for _ in range(m)]
        assert A.dot_plain(ys, row)[1] == sum(y * c for y, c in zip(ys, row)) % P
    for x, want in ((0, set()), (P, {"r>=P"}), ((1 << 96) + 0, {"lo<hh"}), ((1 << 64) - 1 + (1 << 64), {"r<t0"})):
        A.last = set()
        assert A.reduce128(x, 9) == x % P and {b for _, b in A.last} == want, (hex(x), A.last)


# ---- every chunk through the model, once ---------------------------------------------------------------------------------------------
class Run:
    """one (family, form) over a batch: verdicts[g], and the model with its statistics"""


_analysis = {}


def families_of(F, b):
    out = [("wide", False), ("wide", True), ("generic", False)]
    if b.m <= 16:
        out.append(("lane", False))
    return out


def analyse(field, shape, set_name):
    key = (field, shape, set_name)
    if key in _analysis:
        return _analysis[key]
    F, impl = FIELDS[field]
    b = D.batch(F, shape, set_name)
    T = DM.tables(F.name, b.n, b.d, b.t, b.srt)
    rc, co, nco, st = F.O.batch_recover(b.ids, b.array(), b.n, b.d, b.t)
    assert rc == (8 if (st > 1).any() else 0)
    runs, memo = {}, {}
    for fam, p0 in families_of(F, b):
        lk = D.wide_facts("fr", b.n, b.t, b.d, p0)["lk"] if fam == "wide" and F is D.FR else 0
        if fam == "generic" and ("wide", False) in runs and runs[("wide", False)].lk == 0:
            runs[(fam, p0)] = runs[("wide", False)]                  # the same loop, the same arithmetic: the same figures
            if F is D.FR:
                STATS.setdefault((field, fam), DM.Stats()).merge(runs[(fam, p0)].A.stats)
            continue
        r = Run()
        r.lk = lk
        r.A = DM.FrModel(memo=memo) if F is D.FR else DM.GlModel()
        second_form = "m" if fam == "lane" and F is D.FR and 2 <= b.m <= 16 else "generic"
        r.verdicts = [DM.decode(r.A, T, fam, b.sorted_values(c), p0, lk, "on" if b.rmax else "none", second_form, direct=not b.rmax) for c in b.chunks]
        runs[(fam, p0)] = r
        if F is D.FR:
            STATS.setdefault((field, fam), DM.Stats()).merge(r.A.stats)
    _analysis[key] = (b, T, (co, nco, st), runs)
    return _analysis[key]


CASES = [(f, s) for f in FIELDS for s in ALL_SHAPES]


@pytest.mark.parametrize("field,shape", CASES, ids=lambda v: v if isinstance(v, str) else "n%d_t%d_d%d" % v)
def test_model_agrees_with_the_oracle_and_the_inputs_reach_their_sites(field, shape):
    F, impl = FIELDS[field]
    for set_name in D.set_names(shape):
        b, T, (co, nco, st), runs = analyse(field, shape, set_name)
        co = F.ints(co)
        where = (field, shape, set_name)
        m, nv = b.m, b.needed - b.m
        assert not b.rmax or (b.starts(), b.Pfx) == (T.starts, T.P), where
        assert all(0 <= v < F.mod for c in b.chunks for v in c.vals.values()) and all(sorted(c.vals) == b.srt for c in b.chunks), where
        for g, c in enumerate(b.chunks):                              # what each kind of chunk becomes, as the oracle says
            if c.kind == "honest" or "_beyond_" in c.name:
                assert st[g] == 0 and co[g] == [x % F.mod for x in c.poly], (where, c.name)
            elif c.kind == "tamper":
                assert st[g] == (1 if b.rmax else 8), (where, c.name)
                assert st[g] == 8 or co[g] == [x % F.mod for x in c.poly], (where, c.name)
            elif c.window is not None:
                assert st[g] == 1 and co[g] == [x % F.mod for x in c.poly], (where, c.name)
                want_len = max([k + 1 for k, x in enumerate(c.poly) if x % F.mod] or [0])
                assert nco[g] == want_len, (where, c.name)
            else:
                assert st[g] in (1, 8), (where, c.name)
        for (fam, p0), r in runs.items():
            tag = where + (fam, "p0" if p0 else "full")
            ow = 1 if p0 else m
            for g, (c, V) in enumerate(zip(b.chunks, r.verdicts)):
                if V.status is None:                                  # on to k_gao: the model stops, the oracle goes on
                    assert b.rmax and st[g] in (1, 8) and c.window is None, (tag, c.name)
                else:
                    assert (V.status, V.coeffs) == (st[g], co[g][:ow]) and (p0 or V.ncoeffs == nco[g]), (tag, c.name, V.status, st[g], V.ncoeffs, nco[g])
                assert c.window is None or V.window == c.window, (tag, c.name, V.window)
            honest = [V for c, V in zip(b.chunks, r.verdicts) if c.kind == "honest"]
            if F is D.GL:
                for V in r.verdicts:
                    for site, fired in V.gl.items():
                        assert not fired & (GL_IMPOSSIBLE | set(D.GL_UNREACHED)), (tag, site, fired)
                continue
            # -- the site table over Fr: every row of the first kernel on every case, in some honest chunk
            need = ({"lt2r_sub", "lt2r_keep"} if m > 1 else {"lt2r_keep"}) if fam == "lane" else CANON if m > 1 else {"slow_keep"}
            for site in [("v", i) for i in range(nv)] + [("o", k) for k in range(ow)]:
                seen = {V.cases[site] for V in honest}
                assert need <= seen, (tag, site, sorted(seen))
                if m == 1:                                            # EXCUSES["m1_no_quotient"]
                    assert not seen & {"slow_sub", "q1", "lt2r_sub"}, (tag, site, sorted(seen))
            # -- and of every second-chance window that a chunk claims
            for w in sorted({c.window for c in b.chunks if c.window is not None}):
                acc = [V for c, V in zip(b.chunks, r.verdicts) if c.window == w]
                outs = {V.cases[("so", w, k)] for V in acc for k in range(m)}
                checks = {v for V in acc for s, v in V.cases.items() if s[0] == "sv" and s[1] == w}
                if F is D.FR and fam == "lane" and 2 <= m <= 16:         # k_second_chance_m: cond_sub_r on every row
                    assert {"lt2r_sub", "lt2r_keep"} <= outs and {"lt2r_sub", "lt2r_keep"} <= checks, (tag, w, outs, checks)
                else:                                                # second_dot: canon_loose; m = 1: EXCUSES["m1_no_quotient"]
                    want = CANON if m > 1 else {"slow_keep"}
                    assert want <= outs, (tag, w, "coefficient rows", sorted(outs))
                    assert want <= checks, (tag, w, "check rows", sorted(checks))
                assert any(V.ncoeffs < m for V in acc) and any(V.ncoeffs == 0 for V in acc), (tag, w)      # trimmed lengths, the zero polynomial


def test_every_window_is_claimed_and_some_chunks_go_on_to_gao():
    for field, (F, impl) in FIELDS.items():
        for shape in D.SHAPES:
            if "all" not in D.set_names(shape):
                continue
            b = D.batch(F, shape, "all")
            claimed = {c.window for c in b.chunks if c.window is not None}
            starts = b.starts()
            possible = {w for w in range(len(starts)) if D.window_liars(starts, b.m, b.Pfx, w, b.rmax) is not None}
            assert claimed == possible and 0 in claimed, (field, shape, claimed, possible)
            assert len(starts) < 2 or 1 in claimed, (field, shape)
            everywhere = D.window_liars(starts, b.m, b.Pfx, len(starts), b.t)         # liars in every window, no more than t of them
            assert any(c.name.startswith("unresolved") for c in b.chunks) == (everywhere is not None), (field, shape)
    # all four windows somewhere, and the windows start at 0, m, P - m and ceil(m / 2)
    b = D.batch(D.FR, (40, 13, 12), "all")
    assert b.starts() == [0, b.m, b.Pfx - b.m, (b.m + 1) // 2] and {c.window for c in b.chunks if c.window is not None} == {0, 1, 2, 3}


def test_goldilocks_branches():
    """every family fires what random rows fire, over the shapes together; the branches never fired are the ones recorded"""
    for fam in ("wide", "generic", "lane"):
        fired = set()
        for shape in ALL_SHAPES:
            for set_name in D.set_names(shape):
                r = analyse("goldilocks", shape, set_name)[3].get((fam, False))
                if r is not None:
                    fired |= set(r.A.fired)
        assert GL_REQUIRED <= fired, (fam, sorted(GL_REQUIRED - fired, key=str))
        assert not fired & (GL_IMPOSSIBLE | set(D.GL_UNREACHED)), fam


def test_the_frozen_goldilocks_fold_word_is_what_the_search_finds():
    """output row 0 of (4, 1, 1), both sender sets: the search on the dumped constants gives the frozen word, and the chunk built from it
    takes `lo < hh` in the final reduce128 of that row in every family and form"""
    for set_name in D.set_names(D.GL_FOLD_SHAPE):
        b, T, _, runs = analyse("goldilocks", D.GL_FOLD_SHAPE, set_name)
        assert D.gl_fold_word(*T.bc[0]) == D.GL_FOLD_WORD, set_name
        g = b.index("gl_final_lo_lt_hh")
        assert b.sorted_values(b.chunks[g])[:2] == list(D.GL_FOLD_WORD)
        for key, r in runs.items():
            assert (3, "lo<hh") in r.verdicts[g].gl[("o", 0)], (set_name, key)
    assert set(DM.GL_BRANCHES) == GL_REQUIRED | GL_IMPOSSIBLE | set(D.GL_UNREACHED)


def test_oracle_spec_agrees_on_a_sample():
    """oracle.spec / oracle.spec_gl on every chunk of the two smallest shapes and on the tampered and liar chunks of (10, 3, 3)"""
    for field, (F, impl) in FIELDS.items():
        for shape, pick in (((4, 1, 1), None), ((7, 2, 2), None), ((10, 3, 3), ("tamper", "liar"))):
            for set_name in D.set_names(shape):
                b, T, (co, nco, st), runs = analyse(field, shape, set_name)
                co = F.ints(co)
                for g, c in enumerate(b.chunks):
                    if pick and c.kind not in pick:
                        continue
                    try:
                        poly = F.S.recover_secret([F.S.Share(c.vals[i], i, b.d) for i in b.ids], b.n, b.t)[0]
                        assert st[g] <= 1 and list(poly) + [0] * (b.m - len(poly)) == co[g], (field, shape, set_name, c.name)
                    except F.S.ShareErr as e:
                        assert st[g] == e.code, (field, shape, set_name, c.name)


# ---- the launch parameters and the routes -----------------------------------------------------------------------------------------------
def test_wide_parameters_put_every_shape_on_its_path():
    for shape, claims in D.WIDE_CLAIMS.items():
        for p0, claim in zip((False, True), claims):
            facts = D.wide_facts("fr", *shape, p0)
            assert {k: facts[k] for k in claim} == claim, (shape, p0, facts)
            gl = D.wide_facts("gl", *shape, p0)
            assert gl["lk"] == 0 and D.wide_facts("sat32", *shape, p0)["lk"] == 0
    lks = {D.wide_facts("fr", *s, p0)["lk"] for s in D.SHAPES for p0 in (False, True)}
    tails = {D.wide_facts("fr", *s, p0)["tail_words"] for s in D.SHAPES for p0 in (False, True)}
    assert lks == {0, 1, 2} and tails == {0, 1, 2, 3}
    # one step on from the largest staged table the table no longer fits
    assert D.wide_facts("fr", 124, 41, 23, False)["lds"] <= 65536 < 4 * 66 * 32 + (41 + 25) * 25 * 9 * 4
    # a table that is not contiguous is staged from both ranges only when there is one output row
    out = subprocess.run([DM.make("wide_plan_dump")], input="fr 11 6 1 0 0 1\nfr 11 6 0 0 0 1\nfr 11 6 0 0 1 0\n", capture_output=True, text=True)
    assert out.returncode == 0 and [ln.split()[1:3] for ln in out.stdout.splitlines()] == [["324", "1"], ["0", "0"], ["0", "0"]]


def test_routes_are_pinned():
    exe = DM.make("recover_routes_dump")
    firsts = set()
    for impl in D.IMPLS:
        calls = D.all_calls(impl) + (D.second_trip_calls(impl) if impl != "sat32" else [])
        queries = [c.query(form) for c in calls for form in ("dev", "p0")]
        p = subprocess.run([exe], input="".join(" ".join(map(str, q)) + "\n" for q in queries), capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stderr[-2000:]
        lines = p.stdout.splitlines()
        assert len(lines) == len(queries)
        for q, line, c in zip(queries, lines, [c for c in calls for _ in range(2)]):
            head = line.split(" all=")[0].split()
            fields = dict(kv.split("=") for kv in head[1:] if "=" in kv)
            assert (head[0], head[4], int(fields["rmax"]), fields["second"]) == c.claim(), (q, line, c.claim())
            firsts.add((impl, head[0]))
    assert firsts == {("u29", "Wide"), ("u29", "RecoverM"), ("u29", "Generic"), ("gl", "Wide"), ("gl", "GoldRecoverM"), ("gl", "Generic"), ("sat32", "Wide")}
    # M = 17 falls through to the runtime-shaped kernel; P - m = 66 leaves the second chance to the tail
    assert D.Call("u29", "mc0,small0", (21, 2, 16), "direct", range(3)).claim()[0] == "Generic"
    assert D.Call("u29", "mc0", (100, 33, 1), "all", range(3)).claim()[3] == "m"
    # the layouts: a whole block of rare chunks, a rare chunk last in a ragged block; counts on both sides of the form switches
    b = D.batch(D.FR, (10, 3, 3), "direct")
    blk, alone = D.layout_picks(b, "block"), D.layout_picks(b, "alone")
    assert len(blk) == 300 and len(alone) == 133 and all(b.chunks[g].rare for g in blk[:256] + blk[-1:] + alone[-1:]) and not any(b.chunks[g].rare for g in alone[:-1])
    for impl in ("u29", "gl"):
        sw = D.switch_calls(impl)
        flagged = [sum(1 for g in c.picks if c.batch().chunks[g].kind != "honest") for c in sw]
        assert flagged == [8, 9, 40, 41] and all(c.G == 512 for c in sw)
        b = sw[0].batch()
        assert (b.Pfx - b.m) // 2 * 8 == 40


# ---- the inputs tell a wrong kernel from a right one -------------------------------------------------------------------------------------
MUT_SHAPES = (((10, 3, 3), "all"), ((7, 2, 2), "all"), ((17, 5, 11), "direct"), ((40, 13, 12), "direct"))
APPLIES = {                                                           # mutation -> (fields, families, needs)
    "ge_strict": (("fr",), ("wide", "generic"), None), "no_sub": (("fr",), ("wide", "generic"), None), "q_plus1": (("fr",), ("wide", "generic"), None),
    "eq_no_limb8": (("fr", "goldilocks"), ("wide", "generic", "lane"), None), "eq_no_limb0": (("fr", "goldilocks"), ("wide", "generic", "lane"), None),
    "zero_before_canon": (("fr",), ("wide", "generic"), "second"),
    "bias_all": (("fr",), ("wide",), "lk1"), "no_dpp2": (("fr",), ("wide",), "lk2"), "row_not_divided": (("fr",), ("wide",), "lk1"),
    "expect_next_row": (("fr", "goldilocks"), ("wide", "generic", "lane"), None), "ws_off_by_one": (("fr", "goldilocks"), ("wide", "generic", "lane"), "second"),
}


@pytest.mark.parametrize("mut", DM.MUTATIONS)
def test_each_mistake_changes_an_answer(mut):
    fields, fams, needs = APPLIES[mut]
    for field in fields:
        F, impl = FIELDS[field]
        for fam in fams:
            changed, ran = 0, 0
            for shape, set_name in MUT_SHAPES:
                b, T, _, runs = analyse(field, shape, set_name)
                r = runs[(fam, False)]
                if (needs == "second" and not b.rmax) or (needs == "lk1" and r.lk < 1) or (needs == "lk2" and r.lk < 2):
                    continue
                ran += 1
                A = DM.FrModel(mut=(mut,)) if F is D.FR else DM.GlModel(mut=(mut,))
                second_form = "m" if fam == "lane" and F is D.FR and 2 <= b.m <= 16 else "generic"
                for c, V in zip(b.chunks, r.verdicts):
                    try:
                        W = DM.decode(A, T, fam, b.sorted_values(c), False, r.lk, "on" if b.rmax else "none", second_form, direct=not b.rmax)
                    except AssertionError:
                        continue                                      # the mistake breaks a precondition of the model: not counted
                    changed += (W.status, W.window, W.coeffs, W.ncoeffs) != (V.status, V.window, V.coeffs, V.ncoeffs)
            assert ran and changed, (mut, field, fam, ran, changed)


def test_bounds_report():
    """the closest approach to each accumulator bound per kernel family, over every Fr row above (profiles/decode_edges.txt)"""
    for shape in ALL_SHAPES:
        for set_name in D.set_names(shape):
            analyse("fr", shape, set_name)
    for fam in ("wide", "lane", "generic"):
        s = STATS[("fr", fam)]
        print(fam, s.line(), s.cases)
        assert 0.25 < s.col64 / 2.0 ** 64 < 1 and s.dots > 10000
    assert 0.25 < STATS[("fr", "wide")].dpp32 / 2.0 ** 32 < 1
    assert STATS[("fr", "lane")].lt2r < 2 * R and STATS[("fr", "wide")].loose < FM.RADIX
