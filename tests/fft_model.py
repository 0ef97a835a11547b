"""One lane of the pruned-FFT encode kernels (csrc/kernels_eval.hpp: k_eval_fft1, k_eval_fftP and its fold form, k_eval_fft1_mix,
k_eval_fft1_triple) in Python integers, with every assumption the lazy radix-2^29 arithmetic of csrc/fr_u29.hpp makes checked where
it is made.

The decisions -- which inputs are zero, where u and v are normalised, where a lazy v is canonicalised, which K a subtraction adds --
are NOT restated here: they are read from tests/cpp/fft_bounds_dump, which prints csrc/fft_bounds.hpp's fft_bd, sub_k and bitrev_c and
the U_MOD / U_SUBC* limbs of csrc/fr_consts.h.  What is restated is the arithmetic: fft_bfly, the two load forms (plain, twisted) with
and without fold, the triple kernel's staging step, and add / sub<K> / normalize / mulc_u / reduce_top / cond_sub_r / canon_loose /
store_loose as fr_u29.hpp writes them.

FrLane asserts, at every butterfly: every limb below lbu 2^29 and below 2^32, the value below vb r; the operand of sub<K> normalised,
at most K r / 2, and no limb of U_SUBC_K - t negative; every limb of a mulc_u input below 2^31; every value handed to normalize or
canon_loose below 2^261.  It records per output which case of reduce_top occurred ("below": top limb below r's; "sub": it reaches r's
and cond_sub_r subtracts; "nosub": it reaches r's and it does not), and the largest limb and value seen against fft_bd's bound.

Goldilocks (csrc/fr_gold.hpp) has no lazy form: its model is the same butterflies over addm / subm / mulm as written, on numpy uint64
columns (a whole batch at once), recording which branch of each fired.
"""
import os
import subprocess

import numpy as np

from oracle import spec as S
from oracle import spec_gl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "fft_bounds_dump")
R = S.R_MOD
P_GL = spec_gl.P
MASK = (1 << 29) - 1
RADIX = 1 << 261
R_INV = pow(R, -1, RADIX)
SG = spec_gl.S


# ---- the dump ------------------------------------------------------------------------------------------------------------------------
class _Dump:
    consts, subk, bd, bitrev, built = {}, {}, {}, {}, False


def _run(queries):
    if not _Dump.built:
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "cpp"), "fft_bounds_dump"], stdout=subprocess.DEVNULL)
        _Dump.built = True
    text = "".join("%d %d %d %d\n" % q for q in queries)
    p = subprocess.run([BIN], input=text, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]          # ASan / UBSan findings abort with a non-zero code
    cur = None
    for line in p.stdout.splitlines():
        f = line.split()
        if f[0] == "const":
            _Dump.consts[f[1]] = [int(v, 16) for v in f[2:]]
        elif f[0] == "subk":
            _Dump.subk[int(f[1])] = int(f[2])
        elif f[0] == "query":
            cur = tuple(int(v) for v in f[1:])
            _Dump.bd[cur], _Dump.bitrev[cur[0]] = {}, {}
        elif f[0] == "bd":
            _Dump.bd[cur][(int(f[1]), int(f[2]))] = (int(f[3]), int(f[4]))
        elif f[0] == "bitrev":
            _Dump.bitrev[cur[0]][int(f[1])] = int(f[2])
    assert all(q in _Dump.bd for q in queries)


def preload(queries):
    """one run of the dump tool for many (LOG, CNT, LBU0, VB0)"""
    need = sorted({q for q in queries if q not in _Dump.bd})
    if need or not _Dump.consts:
        _run(need)


def bounds(LOG, CNT, LBU0, VB0):
    """fft_bd of that instantiation: {(stage, idx): (lbu, vb)}"""
    preload([(LOG, CNT, LBU0, VB0)])
    return _Dump.bd[(LOG, CNT, LBU0, VB0)]


def bitrev(LOG):
    if LOG not in _Dump.bitrev:
        preload([(LOG, 1, 1, 1)])
    return _Dump.bitrev[LOG]


def consts():
    preload([])
    return _Dump.consts


def sub_k(vb):
    preload([])
    return _Dump.subk[vb]


# ---- Fr / U29 ------------------------------------------------------------------------------------------------------------------------
def limbs_of(v):
    """a value as 9 normalised limbs (the top one takes what is left)"""
    return [(v >> 29 * i) & MASK for i in range(8)] + [v >> 232]


def value(e):
    return sum(l << 29 * i for i, l in enumerate(e))


def const_form(c):
    """the device-constant form of c: c 2^261 mod r"""
    return c * RADIX % R


class Stats:
    """the largest limb and value seen, as fractions of fft_bd's bound, and where"""

    def __init__(self):
        self.limb, self.val, self.limb_at, self.val_at, self.butterflies = 0.0, 0.0, None, None, 0
        self.by_lbu, self.by_vb = {}, {}
        self.in_limb, self.in_val = 0.0, 0.0          # the same over the transforms' inputs and their copies, which the loads alone decide

    def see(self, top, v, lbu, vb, where, lazy):
        lr, vr = top / (lbu << 29), v / (vb * R)
        if not lazy:
            self.in_limb, self.in_val = max(self.in_limb, lr), max(self.in_val, vr)
            return
        # per bound: a sum of two canonical values sits at its bound of 2 by construction; the larger bounds tell how much room is left
        self.by_lbu[lbu], self.by_vb[vb] = max(self.by_lbu.get(lbu, 0.0), lr), max(self.by_vb.get(vb, 0.0), vr)
        if lr > self.limb:
            self.limb, self.limb_at = lr, where + ((lbu, vb),)
        if vr > self.val:
            self.val, self.val_at = vr, where + ((lbu, vb),)

    def merge(self, o):
        if o.limb > self.limb:
            self.limb, self.limb_at = o.limb, o.limb_at
        if o.val > self.val:
            self.val, self.val_at = o.val, o.val_at
        for mine, theirs in ((self.by_lbu, o.by_lbu), (self.by_vb, o.by_vb)):
            for k, v in theirs.items():
                mine[k] = max(mine.get(k, 0.0), v)
        self.in_limb, self.in_val, self.butterflies = max(self.in_limb, o.in_limb), max(self.in_val, o.in_val), self.butterflies + o.butterflies


class FrLane:
    """the arithmetic of fr_u29.hpp, with its preconditions asserted.  An element is (its 9 limbs, the value they stand for): the value is
    carried along by the rules of each operation and compared with the limbs' own sum wherever the kernel reduces (reduce_top)."""

    def __init__(self, stats=None):
        self.c = consts()
        self.mod = self.c["U_MOD"]
        assert value(self.mod) == R and all(value(self.c["U_SUBC%d" % k]) == k * R for k in (2, 4, 8, 16, 32, 64))
        self.stats = stats if stats is not None else Stats()
        self.cases = {}                     # output index -> the reduce_top case of its store
        self.zero = ([0] * 9, 0)

    def check(self, e, bd, where, lazy=True):
        """lazy: e came out of a butterfly's arithmetic (an input, or a copy of one where the partner is zero, is what the load made it)"""
        lbu, vb = bd
        top = max(e[0])
        assert lbu > 0, where
        assert top < (lbu << 29) and top < 1 << 32 and min(e[0]) >= 0, ("limb", where, [hex(l) for l in e[0]], bd)
        assert e[1] < vb * R, ("value", where, e[1] / R, bd)
        self.stats.see(top, e[1], lbu, vb, where, lazy)

    @staticmethod
    def load(v):
        assert 0 <= v < 1 << 256
        return (limbs_of(v), v)

    @staticmethod
    def add(a, b):
        return ([x + y for x, y in zip(a[0], b[0])], a[1] + b[1])

    def sub(self, K, a, b, where=None):
        c = self.c["U_SUBC%d" % K]
        assert max(b[0][:8]) <= MASK, ("sub operand not normalised", where)
        assert 2 * b[1] <= K * R, ("sub operand beyond K r / 2", where, K, b[1] / R)
        d = [ci - bi for ci, bi in zip(c, b[0])]
        assert min(d) >= 0, ("U_SUBC - t has a negative limb", where, K)
        out = [x + y for x, y in zip(a[0], d)]
        assert max(out) < 1 << 32, ("sub overflows a limb", where)
        return (out, a[1] + K * R - b[1])

    @staticmethod
    def normalize(a, where=None):
        assert a[1] < RADIX, ("normalize beyond 2^261", where)
        r = list(a[0])
        for i in range(8):
            r[i + 1] += r[i] >> 29
            r[i] &= MASK
        assert r[8] < 1 << 32
        return (r, a[1])

    @staticmethod
    def mont(a, c, where=None):
        """(a c + m r) / 2^261 with m = -a c / r mod 2^261: a an element (each limb below 2^31), c an integer below 2^261 (normalised limbs)"""
        assert max(a[0]) < 1 << 31, ("mulc input limb beyond 2^31", where, [hex(l) for l in a[0]])
        t = a[1] * c
        m = -t * R_INV % RADIX
        s = t + m * R
        assert s & (RADIX - 1) == 0
        s >>= 261
        return (limbs_of(s), s)

    def reduce_top(self, e, where=None):
        x = e[0]
        assert value(x) == e[1], where                           # the carried value is the limbs' own
        assert e[1] < RADIX and max(x) < 1 << 32, ("canon_loose beyond 2^261", where)
        top = x[8] + (x[7] >> 29)
        assert top < 1 << 32
        recip = (1 << 45) // (self.mod[8] + 1)
        nq = -((top * recip) >> 45)
        y, acc = [], 0
        for i in range(9):
            acc += x[i] + nq * self.mod[i]
            if i < 8:
                y.append(acc & MASK)
                acc >>= 29                  # arithmetic, as on an int64
            else:
                assert 0 <= acc < 1 << 32, ("reduce_top's top limb", where, acc)
                y.append(acc)
        v = value(y)
        assert v == e[1] + nq * R and v < 2 * R, ("reduce_top's range", where)
        return (y, v)

    def cond_sub_r(self, e):
        x = e[0]
        d, c = [], 0
        for i in range(9):
            v = x[i] - self.mod[i] + c
            c = v >> 29
            d.append(v & MASK if i < 8 else v)
        return e if d[8] < 0 else (d, value(d))

    def canon_loose(self, x, where=None):
        """-> (canonical element, case)"""
        y = self.reduce_top(x, where)
        if y[0][8] < self.mod[8]:
            assert y[1] < R
            return y, "below"
        z = self.cond_sub_r(y)
        assert z[1] < R and z[1] == y[1] % R, where
        return z, ("sub" if z[1] != y[1] else "nosub")

    def store_loose(self, x, j, where=None):
        c, case = self.canon_loose(x, where)
        assert max(c[0][:8]) <= MASK and c[0][8] < 1 << 24
        self.cases[j] = case
        return c[1]

    # -- fft_bfly, stage by stage (the order within a stage and the kernels' interleaving of the last two do not change a value)
    def transform(self, X, LOG, bd, tw, tag):
        size = 1 << LOG
        for i in range(size):
            assert (X[i] is None) == (bd[(0, i)][0] == 0), (tag, i)
            if X[i] is not None:
                self.check(X[i], bd[(0, i)], (tag, 0, i), lazy=False)
        for s in range(LOG):
            B = 1 << s
            for idx in range(size // 2):
                blk, k = divmod(idx, B)
                iu = blk * 2 * B + k
                iv = iu + B
                bu, bv = bd[(s, iu)], bd[(s, iv)]
                where = (tag, s, idx)
                if bv[0] == 0:
                    if bu[0] != 0:
                        X[iv] = X[iu]
                else:
                    self.stats.butterflies += 1
                    tight = bv[0] == 1 and bv[1] <= 2
                    if k == 0:
                        t = X[iv] if tight else self.canon_loose(X[iv], where)[0]
                    else:
                        vin = self.normalize(X[iv], where) if bv[0] > 4 else X[iv]
                        t = self.mont(vin, tw[k * (size // (2 * B))], where)
                    tvb = (bv[1] if tight else 1) if k == 0 else 2
                    K = sub_k(tvb)
                    assert K <= 64
                    if bu[0] == 0:
                        X[iu] = t
                        X[iv] = self.sub(K, self.zero, t, where)
                    else:
                        u = self.normalize(X[iu], where) if bu[0] + 2 > 7 else X[iu]
                        X[iu] = self.add(u, t)
                        X[iv] = self.sub(K, u, t, where)
                for i in (iu, iv):
                    if bd[(s + 1, i)][0]:
                        self.check(X[i], bd[(s + 1, i)], (tag, s + 1, i), lazy=bv[0] != 0)
                    else:
                        assert X[i] is None
        return X


_tw_cache = {}


def fr_twiddles(size):
    """tw[q] = omega_size^q in device-constant form, q < size / 2"""
    if size not in _tw_cache:
        w = S.domain_omega(size)
        _tw_cache[size] = [const_form(pow(w, q, R)) for q in range(max(size // 2, 1))]
    return _tw_cache[size]


_twist_cache = {}


def fr_twist(size, dp1):
    """twist[r][k] = omega_size^(r k) in device-constant form, r < size / 16, k < dp1"""
    if (size, dp1) not in _twist_cache:
        w = S.domain_omega(size)
        _twist_cache[(size, dp1)] = [[const_form(pow(w, r * k, R)) for k in range(dp1)] for r in range(size // 16)]
    return _twist_cache[(size, dp1)]


def fr_fft1(row, LOG, CNT, n, stats=None):
    """k_eval_fft1 / k_eval_fft1_mix on one chunk: -> (the n stored outputs, {j: case})"""
    assert len(row) == CNT
    lane = FrLane(stats)
    bd, br = bounds(LOG, CNT, 1, 1), bitrev(LOG)
    X = [lane.load(row[br[p]]) if br[p] < CNT else None for p in range(1 << LOG)]
    lane.transform(X, LOG, bd, fr_twiddles(1 << LOG), "fft1")
    return [lane.store_loose(X[j], j, ("store", j)) for j in range(n)], lane.cases


def fr_fftP(row, P, n, stats=None):
    """k_eval_fftP on one chunk (the fold form when the row has more than 16 coefficients)"""
    dp1 = len(row)
    fold, cnt16 = dp1 > 16, min(dp1, 16)
    Q = 2 if fold else 1
    size = 16 * P
    lane = FrLane(stats)
    br, tw16, twist = bitrev(4), fr_twiddles(16), fr_twist(size, dp1)
    out = [None] * n
    for r in range(P):
        bd = bounds(4, cnt16, Q, Q if r == 0 else 2 * Q)
        X = [None] * 16
        for p in range(16):
            k = br[p]
            if k >= cnt16:
                continue
            if r == 0:
                X[p] = lane.load(row[k])
                if fold and k + 16 < dp1:
                    X[p] = lane.add(X[p], lane.load(row[k + 16]))
            else:
                X[p] = lane.mont(lane.load(row[k]), twist[r][k], ("twist", r, k))
                if fold and k + 16 < dp1:
                    X[p] = lane.add(X[p], lane.mont(lane.load(row[k + 16]), twist[r][k + 16], ("twist", r, k + 16)))
        lane.transform(X, 4, bd, tw16, ("pass", r))
        for idx in range(16):
            j = r + P * idx
            if j < n:
                out[j] = lane.store_loose(X[idx], j, ("store", j))
    return out, lane.cases


def fr_triple_stage(a, b, r2t, lane):
    """the staging step of k_eval_fft1_triple for one element: mulc by R^2, mont, sub<2>, store_loose -> the canonical a b - r2t"""
    am = lane.mont(lane.load(a), const_form(RADIX % R), "triple a R^2")          # U_R2: 2^522 mod r
    assert max(am[0][:8]) <= MASK and am[1] < 2 * R
    pr = lane.mont(lane.load(b), am[1], "triple a b")
    assert pr[1] < 2 * R
    c = lane.sub(2, pr, lane.load(r2t), "triple sub")
    return lane.canon_loose(c, "triple store")


def fr_fft1_triple(a, b, r2t, LOG, CNT, n, stats=None):
    """-> (outputs, cases, the staged coefficients, the staging step's cases)"""
    lane = FrLane(stats)
    staged = [fr_triple_stage(x, y, z, lane) for x, y, z in zip(a, b, r2t)]
    row = [c[1] for c, _ in staged]
    out, cases = fr_fft1(row, LOG, CNT, n, lane.stats)
    return out, cases, row, [case for _, case in staged]


# ---- Goldilocks: a batch of chunks at once, columns of numpy uint64 -----------------------------------------------------------------
EPS = np.uint64(0xFFFFFFFF)
PG = np.uint64(P_GL)
BRANCHES = ("addm_wrap", "addm_ge_p", "subm_borrow", "mulm_lo_lt_hh", "mulm_r_lt_t0", "mulm_r_ge_p")


class GlTrace:
    """which branches fired (counts over all rows), and the operands of every multiply in order"""

    def __init__(self):
        self.fired = {b: 0 for b in BRANCHES}
        self.muls, self.adds, self.subs = [], [], []

    def note(self, name, mask):
        self.fired[name] += int(np.count_nonzero(mask))


def gl_addm(a, b, tr):
    with np.errstate(over="ignore"):
        s = a + b
        wrap = s < a
        s = np.where(wrap, s + EPS, s)
        ge = s >= PG
        tr.note("addm_wrap", wrap), tr.note("addm_ge_p", ge)
        return np.where(ge, s - PG, s)


def gl_subm(a, b, tr):
    with np.errstate(over="ignore"):
        d = a - b
        borrow = a < b
        tr.note("subm_borrow", borrow)
        return np.where(borrow, d - EPS, d)


def gl_mulm(a, b, tr):
    """a: a column, b: a column or one constant"""
    b = np.broadcast_to(np.asarray(b, dtype=np.uint64), a.shape)
    with np.errstate(over="ignore"):
        lo = a * b
        a0, a1, b0, b1 = a & EPS, a >> np.uint64(32), b & EPS, b >> np.uint64(32)
        p00, p01, p10, p11 = a0 * b0, a0 * b1, a1 * b0, a1 * b1
        mid = (p00 >> np.uint64(32)) + (p01 & EPS) + (p10 & EPS)
        hi = p11 + (p01 >> np.uint64(32)) + (p10 >> np.uint64(32)) + (mid >> np.uint64(32))
        hh, hl = hi >> np.uint64(32), hi & EPS
        t0 = lo - hh
        m1 = lo < hh
        t0 = np.where(m1, t0 - EPS, t0)
        t1 = hl * EPS
        r = t0 + t1
        m2 = r < t0
        r = np.where(m2, r + EPS, r)
        m3 = r >= PG
        tr.note("mulm_lo_lt_hh", m1), tr.note("mulm_r_lt_t0", m2), tr.note("mulm_r_ge_p", m3)
        tr.last_mul = (m1, m2, m3)          # per row, for searches
        return np.where(m3, r - PG, r)


def gl_twiddles(size):
    w = SG.domain_omega(size)
    return [pow(w, q, P_GL) for q in range(max(size // 2, 1))]


def gl_transform(X, LOG, bd, tw, tr):
    """fft_bfly over Gold: canon_loose and normalize are the identity, sub<K> is subm"""
    size = 1 << LOG
    zero = None
    for s in range(LOG):
        B = 1 << s
        for idx in range(size // 2):
            blk, k = divmod(idx, B)
            iu = blk * 2 * B + k
            iv = iu + B
            bu, bv = bd[(s, iu)], bd[(s, iv)]
            if bv[0] == 0:
                if bu[0] != 0:
                    X[iv] = X[iu]
                continue
            if k == 0:
                t = X[iv]
            else:
                tr.muls.append((X[iv], tw[k * (size // (2 * B))]))
                t = gl_mulm(X[iv], np.uint64(tw[k * (size // (2 * B))]), tr)
            if bu[0] == 0:
                zero = np.zeros_like(t) if zero is None else zero
                X[iu] = t
                tr.subs.append((zero, t))
                X[iv] = gl_subm(zero, t, tr)
            else:
                u = X[iu]
                tr.adds.append((u, t)), tr.subs.append((u, t))
                X[iu] = gl_addm(u, t, tr)
                X[iv] = gl_subm(u, t, tr)
    return X


def gl_fft1(rows, LOG, CNT, n, tr=None):
    """rows: uint64 [G][CNT] -> ([n][G], trace)"""
    tr = tr if tr is not None else GlTrace()
    rows = np.ascontiguousarray(rows, dtype=np.uint64).reshape(-1, CNT)
    bd, br = bounds(LOG, CNT, 1, 1), bitrev(LOG)
    X = [rows[:, br[p]].copy() if br[p] < CNT else None for p in range(1 << LOG)]
    gl_transform(X, LOG, bd, gl_twiddles(1 << LOG), tr)
    return np.stack([X[j] for j in range(n)]), tr


def gl_fftP(rows, P, n, tr=None):
    tr = tr if tr is not None else GlTrace()
    rows = np.ascontiguousarray(rows, dtype=np.uint64)
    dp1 = rows.shape[1]
    fold, cnt16 = dp1 > 16, min(dp1, 16)
    Q = 2 if fold else 1
    size = 16 * P
    br, tw16, w = bitrev(4), gl_twiddles(16), SG.domain_omega(size)
    out = np.zeros((n, rows.shape[0]), dtype=np.uint64)
    for r in range(P):
        bd = bounds(4, cnt16, Q, Q if r == 0 else 2 * Q)
        X = [None] * 16
        for p in range(16):
            k = br[p]
            if k >= cnt16:
                continue
            if r == 0:
                X[p] = rows[:, k].copy()
                if fold and k + 16 < dp1:
                    tr.adds.append((X[p], rows[:, k + 16]))
                    X[p] = gl_addm(X[p], rows[:, k + 16], tr)
            else:
                tr.muls.append((rows[:, k], pow(w, r * k, P_GL)))
                X[p] = gl_mulm(rows[:, k], np.uint64(pow(w, r * k, P_GL)), tr)
                if fold and k + 16 < dp1:
                    tr.muls.append((rows[:, k + 16], pow(w, r * (k + 16), P_GL)))
                    hi = gl_mulm(rows[:, k + 16], np.uint64(pow(w, r * (k + 16), P_GL)), tr)
                    tr.adds.append((X[p], hi))
                    X[p] = gl_addm(X[p], hi, tr)
        gl_transform(X, 4, bd, tw16, tr)
        for idx in range(16):
            if r + P * idx < n:
                out[r + P * idx] = X[idx]
    return out, tr


def gl_triple_stage(a, b, r2t, tr):
    """the staging step over Gold: mulc(a, 1), mont(b, .), sub<2>"""
    am = gl_mulm(a, np.uint64(1), tr)
    pr = gl_mulm(b, am, tr)
    return gl_subm(pr, r2t, tr)
