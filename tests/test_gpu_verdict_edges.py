"""The verifiers' verdict kernels (csrc/kernels_codec.hpp: k_check_degree, k_check_top_coeff, k_check_double, k_check_double_sel,
k_check_double_c0) called directly, on both fields, against tests/verdict_model.py: every size around the wave and the block, every
cause of a failure on its own, accumulation into bad[], the columns forms with failures placed so that the lowest failing column is NOT
at the first failing lane of its wave, RanSha's fused verifier against its own loop, and hbmpc_dev_batch_interpolate_c0.
Everything is exact: integers and bytes."""
import ctypes as C
import random

import numpy as np
import pytest

from __graft_entry__ import load_package
from oracle import cref as O
from oracle import cref_gl as OG
from oracle import spec as SFR
from oracle.spec_gl import S as SGL
from tests import verdict_model as M

pytestmark = pytest.mark.gpu
M64 = (1 << 64) - 1
FRESH = list(M.FRESH)


class Field:
    """one context, its element format and a few named device buffers that are reused from launch to launch"""

    def __init__(self, name):
        self.name, self.gl = name, name != "fr"
        self.S = SGL if self.gl else SFR
        self.mod = self.S.R_MOD
        self.W = 1 if self.gl else 4
        self.tail = () if self.gl else (4,)
        self.eng = load_package().Engine(0, field=name)
        self._bufs = {}

    def pack(self, vals):  # Python ints (below 2^(64 W), not reduced) -> [len] elements
        if self.gl:
            return np.array(vals, dtype=np.uint64).reshape(len(vals))
        return np.array([[(v >> (64 * k)) & M64 for k in range(4)] for v in vals], dtype=np.uint64).reshape(len(vals), 4)

    def ints(self, a):
        a = np.ascontiguousarray(a)
        return [int(x) for x in a.reshape(-1)] if self.gl else O.u256_to_ints(a.reshape(-1, 4))

    def put(self, name, arr):
        arr = np.ascontiguousarray(arr)
        ptr, cap = self._bufs.get(name, (0, 0))
        if cap < arr.nbytes or not ptr:
            if ptr:
                self.eng.sync()
                self.eng.dev_free(ptr)
            cap = max(arr.nbytes, 4096)
            ptr = self.eng.dev_alloc(cap)
            self._bufs[name] = (ptr, cap)
        if arr.nbytes:
            self.eng.h2d(ptr, arr)
        return ptr

    def get(self, name, arr):
        self.eng.d2h(arr, self._bufs[name][0])
        self.eng.sync()
        return arr

    def close(self):
        self.eng.sync()
        for ptr, _ in self._bufs.values():
            self.eng.dev_free(ptr)
        self.eng.close()


@pytest.fixture(scope="module")
def fr():
    f = Field("fr")
    yield f
    f.close()


@pytest.fixture(scope="module")
def gold():
    f = Field("goldilocks")
    yield f
    f.close()


@pytest.fixture(scope="module", params=["fr", "goldilocks"])
def F(request):
    return request.getfixturevalue("fr" if request.param == "fr" else "gold")


class Tab:
    """[G][k] field elements as Python ints (what the model reads) and as the device's words, kept in step"""

    def __init__(self, F, rows):
        self.F, self.rows = F, [list(r) for r in rows]
        self.arr = F.pack([v for r in self.rows for v in r]).reshape((len(self.rows), len(self.rows[0])) + F.tail)

    def set(self, g, j, v):
        self.rows[g][j] = v
        self.arr[g, j] = self.F.pack([v])[0]

    def copy(self):
        t = Tab.__new__(Tab)
        t.F, t.rows, t.arr = self.F, [list(r) for r in self.rows], self.arr.copy()
        return t

    def column(self, j):
        return [r[j] for r in self.rows]


def rnd(F, rng):  # a non-zero element; over Fr all four words are set (the top one below r's)
    while True:
        v = rng.randrange(1, F.mod)
        if all((v >> (64 * k)) & M64 for k in range(F.W)):
            return v


def copy_data(d):
    return {k: (v.copy() if isinstance(v, Tab) else list(v) if isinstance(v, list) else v) for k, v in d.items()}


def u8(x):
    return np.array(x, dtype=np.uint8)


# ---- the five calls: honest inputs, one way per cause to spoil an entry, the launch and the model --------------------------------
class CheckDegree:
    name, has_columns = "check_degree", False

    def __init__(self, want=2, m=5):
        self.want, self.m, self.label = want, m, f"check_degree-want{want}-m{m}"
        self.causes = [("status", 2), ("status", 8), ("status", 255), ("top_zero",)] + ([("high", k) for k in range(want + 1, m)])

    def honest(self, F, rng, G):
        return {"co": Tab(F, [[rnd(F, rng) for _ in range(self.want + 1)] + [0] * (self.m - self.want - 1) for _ in range(G)]),
                "st": [rng.choice((0, 1)) for _ in range(G)]}

    def spoil(self, F, rng, d, g, cause):
        if cause[0] == "status":
            d["st"][g] = cause[1]
        elif cause[0] == "top_zero":
            d["co"].set(g, self.want, 0)
        else:
            d["co"].set(g, cause[1], rnd(F, rng))

    def launch(self, F, d, bad, columns):
        G = len(d["co"].rows)
        return F.eng.dev_check_degree(F.put("a", d["co"].arr), F.put("sa", u8(d["st"])) if d["st"] is not None else 0, G, self.m, self.want, bad)

    def model(self, d, bad, columns):
        return M.check_degree(d["co"].rows, d["st"], self.want, bad)


class CheckTopCoeff:
    name, has_columns = "check_top_coeff", True

    def __init__(self, want=2):
        self.want, self.label = want, f"check_top_coeff-want{want}"
        self.causes = [("status", 2), ("status", 8), ("status", 255)] + ([("top_zero",)] if want > 0 else [])

    def honest(self, F, rng, G):
        return {"top": Tab(F, [[rnd(F, rng)] for _ in range(G)]), "st": [rng.choice((0, 1)) for _ in range(G)]}

    def spoil(self, F, rng, d, g, cause):
        if cause[0] == "status":
            d["st"][g] = cause[1]
        else:
            d["top"].set(g, 0, 0)

    def launch(self, F, d, bad, columns):
        G = len(d["top"].rows)
        return F.eng.dev_check_top_coeff(F.put("a", d["top"].arr), F.put("sa", u8(d["st"])) if d["st"] is not None else 0, G, self.want, bad,
                                         columns=columns)

    def model(self, d, bad, columns):
        return M.check_top_coeff(d["top"].column(0), d["st"], self.want, bad, columns or 0)


class CheckDouble:
    name, has_columns = "check_double_share", False

    def __init__(self, t=1, m=4):
        self.t, self.m, self.label = t, m, f"check_double_share-t{t}-m{m}"
        self.causes = [("t_low",), ("2t_low",), ("c0",)] + [("t_high", k) for k in range(t + 1, m)] + [("2t_high", k) for k in range(2 * t + 1, m)]

    def honest(self, F, rng, G):
        t, m = self.t, self.m
        a = [[rnd(F, rng) for _ in range(t + 1)] + [0] * (m - t - 1) for _ in range(G)]
        b = [[a[g][0]] + [rnd(F, rng) for _ in range(2 * t)] + [0] * (m - 2 * t - 1) for g in range(G)]
        return {"ct": Tab(F, a), "c2t": Tab(F, b)}

    def spoil(self, F, rng, d, g, cause):
        if cause[0] == "t_low":
            d["ct"].set(g, self.t, 0)
        elif cause[0] == "2t_low":
            d["c2t"].set(g, 2 * self.t, 0)
        elif cause[0] == "c0":
            d["c2t"].set(g, 0, (d["c2t"].rows[g][0] + 1) % F.mod)
        elif cause[0] == "t_high":
            d["ct"].set(g, cause[1], rnd(F, rng))
        else:
            d["c2t"].set(g, cause[1], rnd(F, rng))

    def launch(self, F, d, bad, columns):
        return F.eng.dev_check_double_share(F.put("a", d["ct"].arr), F.put("b", d["c2t"].arr), len(d["ct"].rows), self.m, self.t, bad)

    def model(self, d, bad, columns):
        return M.check_double_share(d["ct"].rows, d["c2t"].rows, self.t, bad)


class CheckDoubleSel:
    name, has_columns = "check_double_share_sel", True

    def __init__(self, t=2):
        self.t, self.label = t, f"check_double_share_sel-t{t}"
        self.causes = [(which, code) for which in ("st_t", "st_2t") for code in (2, 8, 255)] + [("c0",)] + ([("top_t",), ("top_2t",)] if t > 0 else [])

    def honest(self, F, rng, G):
        a = [[rnd(F, rng), rnd(F, rng)] for _ in range(G)]
        return {"sel_t": Tab(F, a), "sel_2t": Tab(F, [[a[g][0], rnd(F, rng)] for g in range(G)]),
                "st_t": [rng.choice((0, 1)) for _ in range(G)], "st_2t": [rng.choice((0, 1)) for _ in range(G)]}

    def spoil(self, F, rng, d, g, cause):
        if cause[0] in ("st_t", "st_2t"):
            d[cause[0]][g] = cause[1]
        elif cause[0] == "c0":
            d["sel_t"].set(g, 0, (d["sel_t"].rows[g][0] + 1) % F.mod)
        else:
            d["sel_t" if cause[0] == "top_t" else "sel_2t"].set(g, 1, 0)

    def launch(self, F, d, bad, columns):
        return F.eng.dev_check_double_share_sel(F.put("a", d["sel_t"].arr), F.put("sa", u8(d["st_t"])), F.put("b", d["sel_2t"].arr),
                                                F.put("sb", u8(d["st_2t"])), len(d["st_t"]), columns or 0, self.t, bad)

    def model(self, d, bad, columns):
        return M.check_double_share_sel(d["sel_t"].rows, d["st_t"], d["sel_2t"].rows, d["st_2t"], self.t, bad, columns or 0)


class CheckDoubleC0:
    """columns=None: hbmpc_dev_check_double_share_c0; a number (0 too): hbmpc_dev_check_double_share_c0_columns"""
    name, has_columns = "check_double_share_c0", True

    def __init__(self, t=2):
        self.t, self.label = t, f"check_double_share_c0-t{t}"
        self.causes = [("deg_t", t - 1), ("deg_t", t + 1), ("deg_2t", 2 * t - 1), ("deg_2t", 2 * t + 1), ("deg_t", 0), ("c0",)]

    def honest(self, F, rng, G):
        a = [[rnd(F, rng)] for _ in range(G)]
        return {"c0_t": Tab(F, a), "c0_2t": Tab(F, a), "deg_t": [self.t] * G, "deg_2t": [2 * self.t] * G}

    def spoil(self, F, rng, d, g, cause):
        if cause[0] == "c0":
            d["c0_2t"].set(g, 0, (d["c0_2t"].rows[g][0] + 1) % F.mod)
        else:
            d[cause[0]][g] = cause[1]

    def launch(self, F, d, bad, columns):
        return F.eng.dev_check_double_share_c0(F.put("a", d["c0_t"].arr), F.put("da", np.array(d["deg_t"], dtype=np.uint32)),
                                               F.put("b", d["c0_2t"].arr), F.put("db", np.array(d["deg_2t"], dtype=np.uint32)),
                                               len(d["deg_t"]), self.t, bad, columns=columns)

    def model(self, d, bad, columns):
        return M.check_double_share_c0(d["c0_t"].column(0), d["deg_t"], d["c0_2t"].column(0), d["deg_2t"], self.t, bad, columns or 0)


CALLS = [CheckDegree(), CheckTopCoeff(), CheckDouble(), CheckDoubleSel(), CheckDoubleC0()]
COLUMN_CALLS = [c for c in CALLS if c.has_columns]


def verdict(F, call, d, bad=M.FRESH, columns=None, again=False):
    """-> (rc, [count, first]) of one launch on bad (again: on what the buffer holds from the launch before)"""
    ptr = F._bufs["bad"][0] if again else F.put("bad", np.array(bad, dtype=np.uint32))
    rc = call.launch(F, d, ptr, columns)
    out = F.get("bad", np.zeros(2, dtype=np.uint32))
    return rc, [int(out[0]), int(out[1])]


def spoiled(F, call, rng, base, entries):
    d = copy_data(base)
    for g in sorted(entries):
        call.spoil(F, rng, d, g, call.causes[g % len(call.causes)])
    return d


def check(F, call, d, failing, bad=M.FRESH, columns=None):
    """the kernel's pair is the model's; the model's count is the number of entries the test spoiled (the model itself is pinned by
    tests/test_verdict_model.py)"""
    want = call.model(d, bad, columns)
    assert want[0] == bad[0] + len(failing), (call.name, sorted(failing), want)
    rc, got = verdict(F, call, d, bad, columns)
    assert rc == 0, (call.name, F.eng.last_error())
    assert got == want, (call.name, F.name, "columns", columns, "failing", sorted(failing), "got", got, "want", want)
    return got


# ---- sizes, one verifier ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", [1, 63, 64, 65, 255, 256, 257, 700])
@pytest.mark.parametrize("call", CALLS, ids=lambda c: c.name)
def test_sizes_one_verifier(F, call, G):
    rng = random.Random(1000 + G)
    base = call.honest(F, rng, G)
    sets = [set(), {0}, {G - 1}, {g for g in (63, 64) if g < G}, set(range(G))]
    for failing in sets:
        d = spoiled(F, call, rng, base, failing)
        got = check(F, call, d, failing)
        assert got == ([len(failing), min(failing)] if failing else FRESH)
        if call.has_columns:  # the same through the columns entry point with columns = 0 (G is one verifier)
            assert check(F, call, d, failing, columns=0) == got


@pytest.mark.parametrize("call", CALLS, ids=lambda c: c.name)
def test_accumulation(F, call):
    G = 300
    rng = random.Random(77)
    failing = {70, 130, 299}
    d = spoiled(F, call, rng, call.honest(F, rng, G), failing)
    assert check(F, call, d, failing) == [3, 70]
    rc, twice = verdict(F, call, d, again=True)          # a second call on the same bad: the count doubles, the first index stays
    assert rc == 0 and twice == [6, 70] == call.model(d, [3, 70], None)
    assert check(F, call, d, failing, bad=(5, 12)) == [8, 12]     # a preset first index below every failing one stays
    assert check(F, call, d, failing, bad=(5, 100)) == [8, 70]
    assert check(F, call, call.honest(F, rng, G), set(), bad=(5, 12)) == [5, 12]    # and nothing is written without a failure


# ---- several verifiers' columns in one array ------------------------------------------------------------------------------------------
SHAPES = [(100, 2), (100, 3), (63, 5), (65, 4), (7, 40), (64, 3), (256, 2), (1, 130)]
# (higher column in an earlier verifier, lower column in a later verifier): in ONE wave where the columns are no multiple of 64 (and
# more than one), so that the lowest failing column is not at the wave's first failing lane; just two verifiers otherwise
HAND_MADE = {(100, 2): (70, 105), (100, 3): (195, 203), (63, 5): (100, 127), (65, 4): (128, 131), (7, 40): (131, 190),
             (64, 3): (10, 67), (256, 2): (200, 273), (1, 130): (5, 77)}


def test_hand_made_sets_are_what_they_claim():  # (no device work: the fixture is not requested)
    assert sorted(HAND_MADE) == sorted(SHAPES)
    for (columns, verifiers), (e1, e2) in HAND_MADE.items():
        assert e1 < e2 < columns * verifiers and e1 // columns < e2 // columns
        if columns % 64 != 0 and columns > 1:
            assert e1 // 64 == e2 // 64 and e2 % columns < e1 % columns
        elif columns > 1:
            assert e2 % columns < e1 % columns


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("call", COLUMN_CALLS, ids=lambda c: c.name)
def test_lowest_failing_column(F, call, shape):
    columns, verifiers = shape
    G = columns * verifiers
    rng = random.Random(columns * 1000 + verifiers)
    base = call.honest(F, rng, G)
    e1, e2 = HAND_MADE[shape]
    got = check(F, call, spoiled(F, call, rng, base, {e1, e2}), {e1, e2}, columns=columns)
    assert got == [2, e2 % columns]
    for _ in range(32):
        failing = set(rng.sample(range(G), rng.randint(1, min(6, G))))
        got = check(F, call, spoiled(F, call, rng, base, failing), failing, columns=columns)
        assert got == [len(failing), min(g % columns for g in failing)]
    check(F, call, base, set(), columns=columns)


@pytest.mark.parametrize("call", COLUMN_CALLS, ids=lambda c: c.name)
def test_columns_must_divide_the_entries(F, call):
    rng = random.Random(5)
    d = spoiled(F, call, rng, call.honest(F, rng, 200), {3, 150})
    for columns in (64, 199, 201, 400):
        rc, got = verdict(F, call, d, bad=(7, 9), columns=columns)
        assert rc == 4 and got == [7, 9], (call.name, columns, rc, got)
    assert check(F, call, d, {3, 150}, bad=(7, 9), columns=50) == [9, 0]


# ---- every cause on its own ------------------------------------------------------------------------------------------------------------
PLACES = (0, 127, 199)   # entry 0, lane 63 of the second wave, the last entry
G_CAUSES = 200


@pytest.mark.parametrize("call", CALLS + [CheckTopCoeff(want=1), CheckDegree(want=1, m=2), CheckDouble(t=2, m=7), CheckDoubleSel(t=1), CheckDoubleC0(t=1)],
                         ids=lambda c: c.label)
def test_every_cause_alone(F, call):
    rng = random.Random(11)
    base = call.honest(F, rng, G_CAUSES)
    assert verdict(F, call, base) == (0, FRESH)           # status bytes 0 and 1 (both drawn) pass
    for cause in call.causes:
        for g in PLACES:
            d = copy_data(base)
            call.spoil(F, rng, d, g, cause)
            want = call.model(d, M.FRESH, None)
            assert want == [1, g], (call.name, cause, g, want)
            assert verdict(F, call, d) == (0, want), (call.name, F.name, cause, g)


def test_null_status_is_accepted(F):
    rng = random.Random(13)
    for call in (CheckDegree(), CheckTopCoeff()):
        d = call.honest(F, rng, G_CAUSES)
        d["st"] = None
        assert verdict(F, call, d) == (0, FRESH)
        for g in PLACES:
            e = copy_data(d)
            call.spoil(F, rng, e, g, ("top_zero",))
            assert call.model(e, M.FRESH, None) == [1, g] and verdict(F, call, e) == (0, [1, g])


def test_check_degree_zero_polynomial_and_one_coefficient(F):
    rng = random.Random(17)
    for want, m, passes in ((0, 3, True), (1, 3, False), (2, 3, False), (0, 1, True)):
        call = CheckDegree(want=want, m=m)
        d = {"co": Tab(F, [[rnd(F, rng)] + [0] * (m - 1) if want == 0 else [rnd(F, rng) for _ in range(want + 1)] + [0] * (m - want - 1)
                           for _ in range(G_CAUSES)]), "st": [0] * G_CAUSES}
        assert verdict(F, call, d) == (0, FRESH)
        for g in PLACES:  # the zero polynomial: degree() is 0
            e = copy_data(d)
            for k in range(m):
                e["co"].set(g, k, 0)
            want_bad = call.model(e, M.FRESH, None)
            assert want_bad == (FRESH if passes else [1, g])
            assert verdict(F, call, e) == (0, want_bad), (want, m, g)
    # m = 1 with want = 1: no polynomial of one coefficient has degree 1 -- every entry fails, the zero ones too
    call = CheckDegree(want=1, m=1)
    d = {"co": Tab(F, [[rnd(F, rng) if g % 2 else 0] for g in range(70)]), "st": [0] * 70}
    assert call.model(d, M.FRESH, None) == [70, 0] and verdict(F, call, d) == (0, [70, 0])


def test_zero_degree_ignores_the_top_coefficient(F):
    rng = random.Random(19)
    top = CheckTopCoeff(want=0)                            # want = 0: only the status counts
    d = top.honest(F, rng, G_CAUSES)
    for g in range(G_CAUSES):
        if g % 3 == 0:
            d["top"].set(g, 0, 0)
    assert top.model(d, M.FRESH, None) == FRESH and verdict(F, top, d) == (0, FRESH)
    for g in PLACES:
        e = copy_data(d)
        e["st"][g] = 8
        assert verdict(F, top, e) == (0, [1, g]) and top.model(e, M.FRESH, None) == [1, g]
    sel = CheckDoubleSel(t=0)                              # t = 0: a zero "top" coefficient (it IS the constant term) is no failure
    d = sel.honest(F, rng, G_CAUSES)
    for g in range(0, G_CAUSES, 3):
        for k in ("sel_t", "sel_2t"):
            d[k].set(g, 0, 0), d[k].set(g, 1, 0)
    assert sel.model(d, M.FRESH, None) == FRESH and verdict(F, sel, d) == (0, FRESH)
    for cause in sel.causes:
        e = copy_data(d)
        sel.spoil(F, rng, e, 127, cause)
        assert sel.model(e, M.FRESH, None) == [1, 127] and verdict(F, sel, e) == (0, [1, 127]), cause


# ---- one 64-bit word decides (Fr: an element is four words) ---------------------------------------------------------------------------
@pytest.mark.parametrize("word", [0, 1, 2, 3])
def test_one_word_decides(fr, word):
    F = fr  # (a Goldilocks element is one word: the cases above are these)
    one = 1 << (64 * word)
    rng = random.Random(23 + word)
    G = G_CAUSES
    # "non-zero": every deciding coefficient is zero except for this one word -- nothing fails; made zero, the entry fails
    deg = CheckDegree()
    d = deg.honest(F, rng, G)
    for g in range(G):
        d["co"].set(g, deg.want, one)
    assert deg.model(d, M.FRESH, None) == FRESH and verdict(F, deg, d) == (0, FRESH)
    for g in PLACES:  # a coefficient above `want` that differs from zero in this word alone
        e = copy_data(d)
        e["co"].set(g, deg.m - 1, one)
        assert deg.model(e, M.FRESH, None) == [1, g] and verdict(F, deg, e) == (0, [1, g])
    top = CheckTopCoeff()
    d = top.honest(F, rng, G)
    for g in range(G):
        d["top"].set(g, 0, one)
    assert top.model(d, M.FRESH, None) == FRESH and verdict(F, top, d) == (0, FRESH)
    assert verdict(F, top, d, columns=50) == (0, FRESH)
    dbl = CheckDouble()
    d = dbl.honest(F, rng, G)
    for g in range(G):
        d["ct"].set(g, dbl.t, one), d["c2t"].set(g, 2 * dbl.t, one)
    assert dbl.model(d, M.FRESH, None) == FRESH and verdict(F, dbl, d) == (0, FRESH)
    for g in PLACES:
        for key, k in (("ct", dbl.t + 1), ("c2t", 2 * dbl.t + 1)):  # too high a degree by one word
            e = copy_data(d)
            e[key].set(g, k, one)
            assert dbl.model(e, M.FRESH, None) == [1, g] and verdict(F, dbl, e) == (0, [1, g]), (key, g)
        e = copy_data(d)                                             # constant terms that differ in this word alone
        e["c2t"].set(g, 0, e["ct"].rows[g][0] ^ one)
        assert dbl.model(e, M.FRESH, None) == [1, g] and verdict(F, dbl, e) == (0, [1, g])
    sel = CheckDoubleSel()
    d = sel.honest(F, rng, G)
    for g in range(G):
        d["sel_t"].set(g, 1, one), d["sel_2t"].set(g, 1, one)
    assert sel.model(d, M.FRESH, None) == FRESH and verdict(F, sel, d) == (0, FRESH)
    c0 = CheckDoubleC0()
    d0 = c0.honest(F, rng, G)
    for g in PLACES:
        e = copy_data(d)
        e["sel_2t"].set(g, 0, e["sel_t"].rows[g][0] ^ one)
        assert sel.model(e, M.FRESH, None) == [1, g] and verdict(F, sel, e) == (0, [1, g])
        assert verdict(F, sel, e, columns=100) == (0, [1, g % 100])
        e = copy_data(d0)
        e["c0_2t"].set(g, 0, e["c0_t"].rows[g][0] ^ one)
        assert c0.model(e, M.FRESH, None) == [1, g] and verdict(F, c0, e) == (0, [1, g])
        assert verdict(F, c0, e, columns=100) == (0, [1, g % 100])


# ---- RanSha's verifier: the fused form against its own loop --------------------------------------------------------------------------
@pytest.mark.parametrize("dense", [True, False], ids=["dense", "spaced"])
@pytest.mark.parametrize("n,t", [(7, 2), (16, 5)])
def test_recover_check_degree_fused_against_loop(F, n, t, dense):
    """three verifiers of 100 columns, 2t + 1 senders; verifier 0's column 70 and verifier 1's column 5 have degree t - 1 (honest shares:
    status 0).  Entries 70 and 105 share a wave of the fused form's verdict launch: bad = [2, 5] there as in the loop"""
    G, groups = 100, 3
    senders = list(range(2 * t + 1))
    group_stride = G if dense else 128
    row_stride = groups * group_stride + 7
    rng = random.Random(n * 100 + t + dense)
    polys = [[rnd(F, rng) for _ in range(t + 1)] for _ in range(groups * G)]
    polys[0 * G + 70][t] = 0
    polys[1 * G + 5][t] = 0
    x = F.pack([v for p in polys for v in p]).reshape((groups * G, t + 1) + F.tail)
    rc, y = (OG if F.gl else O).vandermonde_apply(x, n, t)      # y[party][chunk]: the oracle's encode
    assert rc == 0
    rows = F.pack([rnd(F, rng) for _ in range(len(senders) * row_stride)]).reshape((len(senders), row_stride) + F.tail)  # junk between the groups
    for s, party in enumerate(senders):
        for q in range(groups):
            rows[s, q * group_stride: q * group_stride + G] = y[party, q * G: (q + 1) * G]
    ev = F.put("rows", rows)
    ws = F.put("ws", np.zeros((max(groups * G, G * (t + 1)),) + F.tail, dtype=np.uint64))
    try:
        for fused in (1, 0):
            assert F.eng.L.hbmpc_set_producer_fusion(F.eng.ctx, C.c_int(fused)) == 0
            st = F.put("st", np.full(groups * G, 0xEE, dtype=np.uint8))
            bad = F.put("bad", np.array(M.FRESH, dtype=np.uint32))
            rc = F.eng.dev_recover_check_degree_strided(senders, ev, row_stride, G, n, t, ws, st, bad, groups=groups, group_stride=group_stride)
            assert rc == 0, F.eng.last_error()
            got = F.get("bad", np.zeros(2, dtype=np.uint32))
            status = F.get("st", np.zeros(groups * G, dtype=np.uint8))
            assert [int(got[0]), int(got[1])] == [2, 5], (F.name, n, t, dense, fused, got)
            # every verifier's decode is clean; the loop reuses the first G bytes for each verifier in turn
            assert not status[:G].any() and set(status[G:].tolist()) <= {0, 0xEE}, (fused, status)
    finally:
        F.eng.L.hbmpc_set_producer_fusion(F.eng.ctx, C.c_int(1))


# ---- hbmpc_dev_batch_interpolate_c0 -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [8, 16, 7, 13])
def test_batch_interpolate_c0(F, n):
    """c0 and DensePolynomial::degree() of the interpolation through ALL n shares, G = 130 columns of degree d, d - 1, 0 (non-zero
    constant) and the zero polynomial.  n = 8, 16 over Fr: the kernel that stores only these two (two workgroups, so that 130 columns
    reach it); n = 7, 13 and Goldilocks: the full interpolation into tmp_coeffs_dev and the extraction pass."""
    G, d = 130, n // 2
    rng = random.Random(n)
    polys = []
    for g in range(G):
        kind = g % 4
        p = [rnd(F, rng) for _ in range(d + 1)]
        if kind == 1:
            p[d] = 0
        elif kind == 2:
            p = [p[0]] + [0] * d
        elif kind == 3:
            p = [0] * (d + 1)
        polys.append(p)
    x = F.pack([v for p in polys for v in p]).reshape((G, d + 1) + F.tail)
    rc, y = (OG if F.gl else O).vandermonde_apply(x, n, d)
    assert rc == 0
    stride = G + 5
    rows = F.pack([rnd(F, rng) for _ in range(n * stride)]).reshape((n, stride) + F.tail)
    rows[:, :G] = y
    SENTINEL = 0xA5A5A5A5A5A5A5A5
    tmp = F.put("ws", np.full((G * n,) + F.tail, SENTINEL, dtype=np.uint64))
    c0_d = F.put("a", np.full((G + 1,) + F.tail, SENTINEL, dtype=np.uint64))
    deg_d = F.put("da", np.full(G + 1, 0xA5A5A5A5, dtype=np.uint32))
    ids = list(range(n))
    rng.shuffle(ids)                                        # the senders' rows in any order: row s is party ids[s]'s
    ev = F.put("rows", np.ascontiguousarray(rows[ids]))
    F.eng.set_matrix_core_workgroups(2)
    try:
        rc = F.eng.dev_batch_interpolate_c0(ids, ev, stride, G, n, tmp, c0_d, deg_d)
        assert rc == 0, F.eng.last_error()
        c0 = F.get("a", np.zeros((G + 1,) + F.tail, dtype=np.uint64))
        deg = F.get("da", np.zeros(G + 1, dtype=np.uint32))
        left = F.get("ws", np.zeros((G * n,) + F.tail, dtype=np.uint64))
    finally:
        F.eng.set_matrix_core_workgroups(0)
    assert F.ints(c0[:G]) == [p[0] for p in polys]
    assert deg[:G].tolist() == [M.degree(p + [0] * (n - d - 1)) for p in polys]
    assert deg[G] == 0xA5A5A5A5 and (c0[G] == np.uint64(SENTINEL)).all()     # nothing past the G columns
    if not F.gl and n in (8, 16):  # the form that writes only c0 and the degree ran: no coefficient row was stored
        assert (left == np.uint64(SENTINEL)).all()
