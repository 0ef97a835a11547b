"""One dot product of the decode kernels of csrc/kernels_recover.hpp (k_batch_recover_wide with dot_shared, k_batch_recover<F, M, P0>,
k_batch_recover_generic, second_dot / k_second_chance_m) in Python integers, and a chunk's verdict built from such dot products.

The table words are the ones the kernels read: tests/cpp/host_tables_dump prints build_recover_tables and build_second_tables in the
device-constant form, and nothing here recomputes them.  What is restated is the arithmetic of csrc/fr_u29.hpp -- acc_zero (the bias),
acc_mac, acc_fold every MAX_DOT_TERMS terms, acc_fold_needed<M>, the partial sums of dot_shared per `sidx` with the two DPP steps as
32-bit adds (column 17 as a 64-bit one), acc_reduce -- with reduce_top and cond_sub_r taken from tests/fft_model.py (FrLane), and of
csrc/fr_gold.hpp: the three columns with their carry counts, reduce96, reduce128 and the final fold of acc_reduce.

Every precondition is asserted where the kernel relies on it: each 64-bit column below 2^64, each 32-bit DPP operand and sum below 2^32,
the value below 2 r in front of cond_sub_r / store_lt2r and below 2^261 in front of canon_loose; acc_reduce's result is compared with
(T + (-T / r mod 2^261) r) / 2^261.  Stats keeps the closest approach to each of those bounds.

canon_loose reports the case it took: `fast`; `slow_keep` (the subtraction entered, nothing subtracted); `slow_sub` (entered, r
subtracted); `q1` (reduce_top subtracted r itself, the rest fast).  For Goldilocks a dot product reports the branches it fired, in the
manner of fft_model.GlTrace: ("carry", column), and (reduction, "lo<hh" | "r<t0" | "r>=P") for reductions 0 .. 2 (the columns' reduce96)
and 3 (the final reduce128).

`mut` switches on ONE deliberate mistake in the model (MUTATIONS); tests/test_decode_inputs.py shows with them that the committed inputs
tell a subtly wrong kernel from a right one.  No mutated kernel exists.
"""
import os
import subprocess

from tests import fft_model as FM
from tests.fft_model import MASK, R, RADIX, R_INV, limbs_of, value

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
P_GL = FM.P_GL
EPS = 0xFFFFFFFF
M64 = (1 << 64) - 1
M128 = (1 << 128) - 1
MAX_DOT_TERMS = 6
MUTATIONS = ("ge_strict", "no_sub", "q_plus1", "eq_no_limb8", "eq_no_limb0", "zero_before_canon", "bias_all", "no_dpp2", "row_not_divided",
             "expect_next_row", "ws_off_by_one")
_built = set()


def make(tool):
    if tool not in _built:
        subprocess.check_call(["make", "-C", CPP, tool], stdout=subprocess.DEVNULL)
        _built.add(tool)
    return os.path.join(CPP, tool)


# ---- the tables, as host_tables_dump prints them ------------------------------------------------------------------------------------------
class Tables:
    """vm[r][i], bc[k][i]: the optimistic decode's rows; with OEC rounds P, starts[w], ev[w][e][i], sbc[w][k][i] of the second chance.
    A constant is the integer its words spell (Fr: nine normalised 29-bit limbs of c 2^261 mod r; Goldilocks: the value)."""


_tables = {}


def tables(field, n, d, t, sorted_ids):
    key = (field, n, d, t, tuple(sorted_ids))
    if key in _tables:
        return _tables[key]
    p = subprocess.run([make("host_tables_dump"), {"fr": "fr", "goldilocks": "gl"}[field], str(n), str(d), str(t), ",".join(map(str, sorted_ids))],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = {}
    for line in p.stdout.splitlines():
        k, _, v = line.partition(" ")
        lines.setdefault(k, []).append(v)
    nl = 9 if field == "fr" else 2
    m, needed, S = d + 1, d + t + 1, len(sorted_ids)

    def consts(words):
        out = []
        for i in range(0, len(words), nl):
            w = words[i:i + nl]
            if nl == 9:
                assert max(w) <= MASK
                out.append(sum(x << 29 * j for j, x in enumerate(w)))
            else:
                out.append(w[0] | w[1] << 32)
        return out

    def rows(cs, count):
        assert len(cs) == count * m
        return [cs[r * m:(r + 1) * m] for r in range(count)]

    T = Tables()
    T.field, T.m, T.needed = field, m, needed
    T.vm = rows(consts([int(x, 16) for x in lines["recover_vm"][0].split()]), needed - m)
    T.bc = rows(consts([int(x, 16) for x in lines["recover_bc"][0].split()]), m)
    T.rmax = min(t, S - needed) if S > needed else 0
    T.P, T.starts, T.ev, T.sbc = needed + T.rmax, [], [], []
    if T.rmax:
        tok = lines["second"][0].split()
        assert int(tok[0]) == T.P
        nw = int(tok[1])
        T.starts = [int(x) for x in tok[2:2 + nw]]
        cs = consts([int(x, 16) for x in tok[2 + nw:]])
        per = T.P * m
        assert len(cs) == nw * per
        for w in range(nw):
            blk = rows(cs[w * per:(w + 1) * per], T.P)
            T.ev.append(blk[:T.P - m]), T.sbc.append(blk[T.P - m:])
    _tables[key] = T
    return T


# ---- Fr / U29 -----------------------------------------------------------------------------------------------------------------------------
class Stats:
    """the closest approach to each bound: the largest 64-bit column (as a fraction of 2^64), the largest 32-bit DPP sum (of 2^32), the
    largest value handed to cond_sub_r (of 2 r) and to canon_loose (of 2^261); the canon_loose cases seen"""

    def __init__(self):
        self.col64, self.dpp32, self.lt2r, self.loose, self.dots = 0, 0, 0, 0, 0
        self.cases = {}

    def merge(self, o):
        self.col64, self.dpp32, self.lt2r, self.loose, self.dots = max(self.col64, o.col64), max(self.dpp32, o.dpp32), max(self.lt2r, o.lt2r), max(self.loose, o.loose), self.dots + o.dots
        for k, v in o.cases.items():
            self.cases[k] = self.cases.get(k, 0) + v

    def line(self):
        return "column %.6f of 2^64, DPP sum %.6f of 2^32, cond_sub_r input %.6f of 2 r, canon_loose input %.6f of 2^261 (%d dot products)" % (
            self.col64 / 2.0 ** 64, self.dpp32 / 2.0 ** 32, self.lt2r / (2.0 * R), self.loose / float(RADIX), self.dots)


def _pack(v):
    """nine 29-bit limbs of v, 128 bits apart: the product of two packed values holds the 17 column sums of acc_mac"""
    return sum(((v >> 29 * i) & MASK if i < 8 else v >> 232) << 128 * i for i in range(9))


_packed = {}


def packed(v):
    if v not in _packed:
        if len(_packed) > 200000:
            _packed.clear()
        _packed[v] = _pack(v)
    return _packed[v]


class FrModel:
    def __init__(self, stats=None, mut=(), memo=None):
        """memo: a dict shared by the models of one batch -- the same row times the same values is computed once, whichever family or
        form asks (its figures are counted for each)"""
        self.memo = memo if memo is not None and not mut else None
        self.lane = FM.FrLane()
        self.mod = self.lane.mod
        self.stats = stats if stats is not None else Stats()
        self.mut = frozenset(mut)
        assert self.mut <= set(MUTATIONS)

    # -- the accumulator
    def _check(self, cols):
        top = max(cols)
        assert top <= M64, "a 64-bit column overflowed"
        self.stats.col64 = max(self.stats.col64, top)

    @staticmethod
    def _fold(cols, which=range(17)):
        for i in which:
            cols[i + 1] += cols[i] >> 29
            cols[i] &= MASK

    def partial(self, ys, row, idxs, bias, rule):
        """the columns after the terms `idxs` of sum ys[i] row[i]; rule: "pending" (acc_fold when 6 terms are pending, and once at the
        end: the Wide, Generic and second_dot loops, and each lane of dot_shared) or ("needed", M) (dot_row: acc_fold_needed<M> in
        front of every sixth term, nothing at the end)"""
        cols = [MASK] * 9 + [0] * 9 if bias else [0] * 18
        pending = 0
        for i in idxs:
            if rule == "pending" and pending == MAX_DOT_TERMS:
                self._check(cols)
                self._fold(cols)
                pending = 1
            if rule != "pending" and i > 0 and i % MAX_DOT_TERMS == 0:
                self._check(cols)
                M = rule[1]
                self._fold(cols, [k for k in range(17) if (min(k, 16 - k, 8) + 1) * M + 9 > 64])
            assert 0 <= ys[i] < R and row[i] < RADIX
            prod = packed(ys[i]) * packed(row[i])
            for k in range(17):
                cols[k] += (prod >> 128 * k) & M128
            pending += 1
        self._check(cols)
        if rule == "pending":
            self._fold(cols)
        return cols

    def reduce(self, cols):
        """acc_reduce -> (limbs, value)"""
        T = sum(c << 29 * k for k, c in enumerate(cols)) - sum(MASK << 29 * k for k in range(9))
        c = list(cols)
        for k in range(9):
            m = ~c[k] & MASK
            c[k + 1] += c[k] >> 29
            for j in range(1, 9):
                c[k + j] += m * self.mod[j]
            self._check(c)
        t = []
        for k in range(9, 17):
            c[k + 1] += c[k] >> 29
            t.append(c[k] & MASK)
        self._check(c)
        assert c[17] < 1 << 32, "acc_reduce's top limb"
        t.append(c[17])
        want = (T + (-T * R_INV % RADIX) * R) >> 261
        assert value(t) == want and (T + (-T * R_INV % RADIX) * R) & (RADIX - 1) == 0, "acc_reduce is not the Montgomery reduction of the sum"
        self.stats.dots += 1
        return (t, want)

    def _once(self, key, ys, row, fn):
        if self.memo is None:
            return fn(ys, row)
        key += (id(row), tuple(ys))
        hit = self.memo.get(key)
        if hit is None:
            st = self.stats
            keep, st.col64, st.dpp32 = (st.col64, st.dpp32), 0, 0
            hit = self.memo[key] = (fn(ys, row), st.col64, st.dpp32, row)      # the row is kept alive: its id is the key
            st.col64, st.dpp32, st.dots = keep[0], keep[1], st.dots - 1
        self.stats.col64, self.stats.dpp32, self.stats.dots = max(self.stats.col64, hit[1]), max(self.stats.dpp32, hit[2]), self.stats.dots + 1
        return hit[0]

    def dot_plain(self, ys, row):
        return self._once(("plain",), ys, row, lambda y, r: self.reduce(self.partial(y, r, range(len(r)), True, "pending")))

    def dot_row(self, ys, row):
        return self._once(("row",), ys, row, lambda y, r: self.reduce(self.partial(y, r, range(len(r)), True, ("needed", len(r)))))

    def dot_shared(self, ys, row, lk):
        return self._once(("shared", lk), ys, row, lambda y, r: self._dot_shared(y, r, lk))

    def _dot_shared(self, ys, row, lk):
        """the 2^lk lanes of a row; every lane ends with the same total (lane 0's is returned)"""
        lanes = 1 << lk
        parts = [self.partial(ys, row, range(s, len(row), lanes), s == 0 or "bias_all" in self.mut, "pending") for s in range(lanes)]
        for step in range(lk):
            if step == 1 and "no_dpp2" in self.mut:
                break
            nxt = []
            for s in range(lanes):
                a, b = parts[s], parts[s ^ (1 << step)]
                assert max(a[:17]) < 1 << 32 and max(b[:17]) < 1 << 32, "a folded column does not fit the 32-bit DPP operand"
                col = [x + y for x, y in zip(a[:17], b[:17])]
                assert max(col) < 1 << 32, "a 32-bit DPP sum overflowed"
                self.stats.dpp32 = max(self.stats.dpp32, max(col))
                assert a[17] + b[17] <= M64
                nxt.append(col + [a[17] + b[17]])
            parts = nxt
        assert all(p == parts[0] for p in parts) or "no_dpp2" in self.mut
        return self.reduce(parts[0])

    # -- canonicalisation
    def cond_sub_r(self, e):
        assert e[1] < 2 * R, "cond_sub_r beyond 2 r"
        self.stats.lt2r = max(self.stats.lt2r, e[1])
        z = self.lane.cond_sub_r(e)
        assert z[1] == e[1] % R
        case = "lt2r_sub" if z[1] != e[1] else "lt2r_keep"
        self.stats.cases[case] = self.stats.cases.get(case, 0) + 1
        return z, case

    def canon_loose(self, e):
        self.stats.loose = max(self.stats.loose, e[1])
        y = self.lane.reduce_top(e)                               # asserts value < 2^261 and the result below 2 r
        q1 = y[1] != e[1]
        if "q_plus1" in self.mut:
            v = (y[1] - R) % (1 << 264)
            y = (limbs_of(v), v)
        enter = y[0][8] > self.mod[8] if "ge_strict" in self.mut else y[0][8] >= self.mod[8]
        if not enter:
            case = "q1" if q1 else "fast"
            z = y
        else:
            z = y if "no_sub" in self.mut else self.lane.cond_sub_r(y)
            case = "slow_sub" if z[1] != y[1] else "slow_keep"
        if not self.mut:
            assert z[1] == e[1] % R and z[1] < R
        self.stats.cases[case] = self.stats.cases.get(case, 0) + 1
        return z, case

    def eq(self, a, v):
        """eq_canon of an element with a canonical input value"""
        b = limbs_of(v)
        skip = 8 if "eq_no_limb8" in self.mut else 0 if "eq_no_limb0" in self.mut else -1
        return all(x == y for i, (x, y) in enumerate(zip(a[0], b)) if i != skip)

    @staticmethod
    def is_zero(a):
        return not any(a[0])

    @staticmethod
    def stored(a):
        return value(a[0]) & ((1 << 256) - 1)


# ---- Goldilocks ---------------------------------------------------------------------------------------------------------------------------
GL_BRANCHES = tuple(("carry", c) for c in range(3)) + tuple((k, b) for k in range(4) for b in ("lo<hh", "r<t0", "r>=P"))


class GlModel:
    """canon_loose and cond_sub_r are the identity; `fired` collects the branches of every dot product, `last` those of the last one"""

    def __init__(self, stats=None, mut=()):
        self.fired, self.last, self.mut = {}, set(), frozenset(mut)
        self.stats = stats if stats is not None else Stats()

    def _note(self, b):
        self.last.add(b)
        self.fired[b] = self.fired.get(b, 0) + 1

    def reduce128(self, x, k):
        assert x < 1 << 128
        lo, hi = x & M64, x >> 64
        hh, hl = hi >> 32, hi & EPS
        t0 = (lo - hh) & M64
        if lo < hh:
            self._note((k, "lo<hh"))
            t0 = (t0 - EPS) & M64
        t1 = hl * EPS
        r = (t0 + t1) & M64
        if r < t0:
            self._note((k, "r<t0"))
            r = (r + EPS) & M64
        if r >= P_GL:
            self._note((k, "r>=P"))
            r -= P_GL
        assert r == x % P_GL, "reduce128"
        return r

    def dot_plain(self, ys, row):
        self.last = set()
        C = [0, 0, 0]
        for a, c in zip(ys, row):
            assert 0 <= a < P_GL and 0 <= c < P_GL
            a0, a1, c0, c1 = a & EPS, a >> 32, c & EPS, c >> 32
            C[0] += a0 * c0
            C[1] += a0 * c1 + a1 * c0
            C[2] += a1 * c1
        r = []
        for k in range(3):
            assert C[k] >> 64 < 1 << 32, "a carry count overflowed"
            if C[k] >> 64:
                self._note(("carry", k))
            r.append(self.reduce128(C[k], k))
        t = r[0] + (r[1] << 32) + r[2] * EPS
        assert t < 1 << 98
        out = self.reduce128(t, 3)
        assert out == sum(a * c for a, c in zip(ys, row)) % P_GL
        self.stats.dots += 1
        return ([out & EPS, out >> 32], out)

    dot_row = dot_plain

    def dot_shared(self, ys, row, lk):
        raise AssertionError("Goldilocks has no shared dot product")

    def cond_sub_r(self, e):
        return e, "gl"

    def canon_loose(self, e):
        return e, "gl"

    def eq(self, a, v):
        skip = 1 if "eq_no_limb8" in self.mut else 0 if "eq_no_limb0" in self.mut else -1
        return all(x == y for i, (x, y) in enumerate(zip(a[0], [v & EPS, v >> 32])) if i != skip)

    @staticmethod
    def is_zero(a):
        return not any(a[0])

    @staticmethod
    def stored(a):
        return a[0][0] | a[0][1] << 32


# ---- a chunk's verdict ----------------------------------------------------------------------------------------------------------------------
class Verdict:
    """status 0 / 1 / 8, or None: the chunk goes on to k_gao (the model stops there); window: the accepting second-chance window;
    coeffs: the m coefficients zero padded (ow of them stored); ncoeffs; cases: {("v", row) | ("o", row) | ("sv", w, e) | ("so", w, k):
    the canon_loose case}; gl: {site: the Goldilocks branches of that dot product}"""

    def __init__(self):
        self.status, self.window, self.coeffs, self.ncoeffs, self.cases, self.gl = None, None, None, None, {}, {}


def decode(A, T, family, ys, p0, lk=0, second="none", second_form="wave", direct=False):
    """One chunk through a first kernel and, where the call has one, the second chance.
    A: FrModel / GlModel; T: tables(); ys: the senders' values by sorted position (S of them);
    family: "wide" (dot_shared when lk > 0, canon_loose at the comparison, store_loose), "lane" (dot_row, cond_sub_r, store_lt2r),
    "generic" (the plain loop, canon_loose, store_loose); second: "none" or "on"; second_form: "wave" / "generic" (second_dot,
    canon_loose) or "m" (dot_row, cond_sub_r: k_second_chance_m's lane form)."""
    m, nv, mut = T.m, T.needed - T.m, A.mut
    V = Verdict()
    win = ys[:m]

    def one(row, site, fam):
        if fam == "lane":
            e, case = A.cond_sub_r(A.dot_row(win_now[0], row))
        elif fam == "wide" and lk > 0:
            e, case = A.canon_loose(A.dot_shared(win_now[0], row, lk))
        else:
            e, case = A.canon_loose(A.dot_plain(win_now[0], row))
        V.cases[site] = case
        if isinstance(A, GlModel):
            V.gl[site] = set(A.last)
        return e

    win_now = [win]
    allrows = T.vm + (T.bc[:1] if p0 else T.bc)
    ok = True
    for r in range(nv):
        row = T.vm[r]
        if "row_not_divided" in mut and family == "wide" and lk > 0:
            # lane l computes row l with the terms of sidx = l mod 2^lk; the quad's sums are added: row r is what lane r << lk of the
            # right kernel owns, here the lanes r 2^lk .. of the wrong one
            row = _mixed_row(allrows, r, lk, m)
        e = one(row, ("v", r), family)
        exp = ys[m + (r + 1 if "expect_next_row" in mut and r + 1 < nv else r)]
        ok = ok and A.eq(e, exp)
    if ok:
        V.status, V.ncoeffs = 0, m
        V.coeffs = [A.stored(one(T.bc[k], ("o", k), family)) for k in range(1 if p0 else m)]
        return V
    if direct:
        V.status, V.ncoeffs, V.coeffs = 8, 0, [0] * (1 if p0 else m)
        return V
    if second == "none":
        return V
    fam2 = "lane" if second_form == "m" else "generic"
    for w, ws in enumerate(T.starts):
        win_now[0] = ys[ws:ws + m]
        mism = 0
        for e_i in range(T.P - m):
            wse = ws + 1 if "ws_off_by_one" in mut else ws
            s = e_i if e_i < wse else e_i + m
            if s >= T.P:
                s = T.P - 1
            e = one(T.ev[w][e_i], ("sv", w, e_i), fam2)
            mism += 0 if A.eq(e, ys[s]) else 1
        if mism > T.rmax:
            continue
        V.status, V.window, V.coeffs, length = 1, w, [], 0
        for k in range(m):
            if fam2 == "lane":
                raw = A.dot_row(win_now[0], T.sbc[w][k])
                c, case = A.cond_sub_r(raw)
            else:
                raw = A.dot_plain(win_now[0], T.sbc[w][k])
                c, case = A.canon_loose(raw)
            V.cases[("so", w, k)] = case
            if isinstance(A, GlModel):
                V.gl[("so", w, k)] = set(A.last)
            if not A.is_zero(raw if "zero_before_canon" in mut else c):
                length = k + 1
            V.coeffs.append(A.stored(c))
        V.ncoeffs = length
        if p0:
            V.coeffs = V.coeffs[:1]
        return V
    return V


def _mixed_row(allrows, r, lk, m):
    lanes = 1 << lk
    out = [0] * m
    base = (r >> lk) << lk
    for s in range(lanes):
        src = allrows[base + s] if base + s < len(allrows) else [0] * m
        for i in range(s, m, lanes):
            out[i] = src[i]
    return out
