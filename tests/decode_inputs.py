"""Deterministic targeted inputs for the decode kernels of csrc/kernels_recover.hpp: k_batch_recover_wide (with dot_shared),
k_batch_recover<F, M, P0>, k_batch_recover_generic, k_second_chance, k_second_chance_m<U29, M> and second_chance_wave.

Uniform values never reach what these kernels branch on: canon_loose's subtraction needs a result within 2^232 of a multiple of r, the
quotient estimate of reduce_top flips at 2^232 - (r mod 2^232), a coefficient is zero only in the all-zero word, and a random corruption
differs in every limb.  Here every chunk is a polynomial chosen so that a NAMED row of the tables produces a NAMED value:

  coef_*      the polynomial's coefficient k is the target: output row k of the first kernel, coefficient row k of a second-chance window
  verify_*    the polynomial through chosen values at a block of verify-row senders: verify rows of the first kernel, check rows of a window
  constant_*  degree 0: every term of every row carries the same all-ones value (the accumulator columns' headroom)
  tamper_*    an honest chunk with ONE bit of ONE sender's share set: a sender of the interpolation window, each verify-row sender, a sender
              beyond d + t + 1 (never read when the call has OEC rounds and the others are honest)
  window*_*   liars placed so that exactly one second-chance window is free of them and every window tried before it is not; per window the
              accepted polynomial has the targets as coefficients (coef_*) or as values at honest positions outside the window (check_*)
  unresolved* liars in every window: on to k_gao

Plain Python integers, numpy and oracle/ alone; every value canonical; tests/test_decode_inputs.py proves with tests/decode_model.py what
each chunk reaches and holds the model to the oracle.  The Wide kernel's launch parameters are asked from tests/cpp/wide_plan_dump and
restated nowhere: rows per sweep, terms per lane, which sweeps and staging loops run are arithmetic on the dumped numbers (wide_facts).
"""
import random
import subprocess

from tests import decode_model as DM
from tests import edge_inputs as E
from tests import gao_inputs as X

FR, GL = E.FR, E.GL
R, P = E.R, E.P
IMPLS = X.IMPLS                                                  # u29, sat32 -> Fr; gl -> Goldilocks
Q1 = (1 << 232) - (R % (1 << 232))                               # v + r reaches the next top limb from here on: reduce_top's quotient flips to 1
# reduce_top estimates the quotient as (top * RECIP) >> 45 with RECIP = floor(2^45 / (r's top limb + 1)): rounding the reciprocal down keeps
# the estimate at 0 a little beyond Q1 (such a value still takes the full subtraction), and it becomes 1 from the top limb TOP_FLIP on
TOP_FLIP = -(-(1 << 45) // ((1 << 45) // ((R >> 232) + 1)))
F1 = (TOP_FLIP << 232) - R                                       # the smallest v for which v + r is reduced by reduce_top itself
# value classes over Fr, by the canon_loose case a result with that true value takes when the dot product's Montgomery quotient leaves
# one r on top of a small value (tests/test_decode_inputs.py asserts the cases; m = 1 is the exception recorded in EXCUSES)
FR_GROUPS = {"sub": (0, 1, 2), "q1": (Q1 - 1, Q1, Q1 + 1), "flip": (F1 - 1, F1, F1 + 1), "keep": (E.B, E.B + 5, R - 2, R - 1), "other": (E.B - 1, E.MAXLIMB, (R - 1) // 2, (R + 1) // 2)}
GL_GROUPS = {"low": E.EDGE_GL[:3], "mid": E.EDGE_GL[3:6], "high": E.EDGE_GL[6:]}
RARE = {"sub": "slow_sub", "q1": "slow_sub", "flip": "q1", "keep": "slow_keep"}
GL_TAMPER_BITS = (0, 63)

# (n, t, d): the smallest shapes that reach each path of the Wide kernel (WIDE_CLAIMS says which), then the lane kernels' instantiations
SHAPES = ((16, 5, 0), (4, 1, 1), (7, 2, 2), (10, 3, 3), (16, 5, 10), (17, 5, 11), (40, 13, 12), (32, 10, 21), (33, 10, 22), (70, 3, 30),
          (64, 21, 42), (124, 41, 23), (125, 41, 24), (196, 65, 1), (100, 33, 1))
SWEEP_SHAPES = tuple((max(7, M + 4), 2, M - 1) for M in range(1, 18))
# what the shape is there for, per form (full, P(0)), as facts of wide_facts() over Fr: only the keys named are pinned
WIDE_CLAIMS = {
    (16, 5, 0): ({"lk": 0, "terms": 1}, {"lk": 0, "terms": 1}),
    (4, 1, 1): ({"lk": 1, "terms": 1, "tail_words": 2}, {"lk": 1}),
    (7, 2, 2): ({"lk": 1, "terms": 2, "tail_words": 3}, {"lk": 1, "tail_words": 1}),
    (10, 3, 3): ({"lk": 2, "terms": 1}, {}),
    (16, 5, 10): ({"lk": 2, "rows": 16, "lanes_used": 64}, {}),
    (17, 5, 11): ({"lk": 1, "rows": 17, "terms": 6, "fold_in_shared": False}, {"lk": 2}),
    (40, 13, 12): ({"lk": 1, "terms": 7, "fold_in_shared": True}, {}),
    (32, 10, 21): ({"lk": 1, "rows": 32, "lanes_used": 64, "terms": 11}, {"lk": 2, "terms": 6}),
    (33, 10, 22): ({"lk": 0, "rows": 33, "tail_words": 3, "second_pass": True}, {}),
    (70, 3, 30): ({}, {"lk": 2, "terms": 8}),
    (64, 21, 42): ({"tab": False, "rows": 64}, {"tab": True, "lk": 1, "terms": 22}),
    (124, 41, 23): ({"tab": True, "lds": 64480, "stage_loop": True, "second_output_sweep": True}, {}),
    (125, 41, 24): ({"tab": False}, {}),
    (196, 65, 1): ({"second_verify_sweep": True}, {"second_verify_sweep": True}),
    (100, 33, 1): ({}, {}),
}
# canon_loose cases a shape cannot reach, with the argument (tests/test_decode_inputs.py asserts that no generated row takes them)
EXCUSES = {
    "m1_no_quotient": "m = 1: the one table constant is 1 in Montgomery form (2^261 mod r), so T / 2^261 < y and the reduction returns y itself, "
                      "canonical: a small value never arrives with an r on top (no slow_sub, no q1)",
}
# `lo < hh` in the final reduce128 of a Goldilocks dot product needs the 98-bit fold t = r0 + 2^32 r1 + EPS r2 to reach 2^96 with its low
# 64 bits all zero: about 2^-66 per row.  gl_fold_word() solves for it at m = 2; the answer for output row 0 of (4, 1, 1) -- the same
# constants for both sender sets, whose two lowest senders are 0 and 1 -- is frozen here and tests/test_decode_inputs.py re-runs the search
# on the dumped table and the model on the chunk.
GL_FOLD_SHAPE = (4, 1, 1)
GL_FOLD_WORD = (11630625803857236898, 11631346293211253758)
# Goldilocks branches that no generated row fires although a canonical input could (a column residue in the top 2^32 values below 2^64, or a
# column within cnt * 2^32 of a multiple of 2^64: about 2^-32 per row each); tests/test_decode_inputs.py asserts them absent, so that an
# input that starts to fire one is noticed and the list shrinks
GL_UNREACHED = ((0, "r<t0"), (2, "r<t0"), (2, "r>=P"))


def _reduce2(u, v):
    """Lagrange-Gauss reduction of a basis of a plane lattice"""
    norm = lambda x: x[0] * x[0] + x[1] * x[1]                    # noqa: E731
    while True:
        if norm(u) < norm(v):
            u, v = v, u
        num, den = u[0] * v[0] + u[1] * v[1], norm(v)
        k = (2 * num + den) // (2 * den)
        if k == 0:
            return v, u
        u = (u[0] - k * v[0], u[1] - k * v[1])


def gl_fold_word(c, e, seed=0, tries=20000):
    """(a, b), canonical, such that the final fold of a c + b e takes `lo < hh` (c odd).  With the high halves a1, b1 chosen, r2 and the
    part of column 1 they give are known; for each guess of how often P is taken off columns 0 and 1 the fold is a0 c + b0 e + K, and
    a0, b0 < 2^32 with a0 c + b0 e = -K (mod 2^64) is a closest-vector problem in a plane lattice.  The model says whether a candidate
    really takes the branch."""
    N, EPS = 1 << 64, 0xFFFFFFFF
    rng, A = random.Random(seed), DM.GlModel()
    ci = pow(c, -1, N)
    s1, s2 = _reduce2((N, 0), (-e * ci % N, 1))
    det = s1[0] * s2[1] - s1[1] * s2[0]
    c0, c1, e0, e1 = c & EPS, c >> 32, e & EPS, e >> 32
    for _ in range(tries):
        a1, b1 = rng.randrange(1 << 31, EPS), rng.randrange(1 << 31, EPS)
        r2, K1 = (a1 * c1 + b1 * e1) % P, a1 * c0 + b1 * e0
        for j0 in range(3):
            for j1 in range(4):
                K = (K1 << 32) + EPS * r2 - j0 * P - (j1 * P << 32)
                x0 = (-K % N * ci % N, 0)
                tx, ty = x0[0] - (1 << 31), x0[1] - (1 << 31)
                ka = (2 * (tx * s2[1] - ty * s2[0]) + det) // (2 * det)
                kb = (2 * (-tx * s1[1] + ty * s1[0]) + det) // (2 * det)
                for da in (-1, 0, 1):
                    for db in (-1, 0, 1):
                        a0 = x0[0] - (ka + da) * s1[0] - (kb + db) * s2[0]
                        b0 = x0[1] - (ka + da) * s1[1] - (kb + db) * s2[1]
                        a, b = a1 << 32 | a0, b1 << 32 | b0
                        if 0 <= a0 <= EPS and 0 <= b0 <= EPS and a < P and b < P:
                            A.dot_plain([a, b], [c, e])
                            if (3, "lo<hh") in A.last:
                                return a, b
    return None


# ---- the Wide kernel's launch parameters ------------------------------------------------------------------------------------------------
_plans = {}


def wide_plan(field, needed, m, p0):
    """(lds bytes, tab_words, split, lk) of a decode call's Wide launch (the library's tables are contiguous and aligned)"""
    key = (field, needed, m, int(p0))
    if key not in _plans:
        p = subprocess.run([DM.make("wide_plan_dump")], input="%s %d %d %d 0 1 1\n" % key, capture_output=True, text=True, timeout=60)
        assert p.returncode == 0, p.stderr[-2000:]
        _plans[key] = tuple(int(x) for x in p.stdout.split())
    return _plans[key]


def wide_facts(field, n, t, d, p0):
    """what the kernel does with those parameters: plain arithmetic on the dumped numbers and the kernel's loop bounds"""
    m, needed = d + 1, d + t + 1
    lds, tab_words, split, lk = wide_plan(field, needed, m, p0)
    nv, ow = needed - m, 1 if p0 else m
    rows = nv + ow
    tq = tab_words >> 2
    return {"lds": lds, "tab": tab_words != 0, "split": split, "lk": lk, "rows": rows, "lanes_used": min(64, rows << lk) if lk else min(64, rows),
            "terms": -(-m // (1 << lk)), "fold_in_shared": lk > 0 and -(-m // (1 << lk)) > DM.MAX_DOT_TERMS,
            "tail_words": tab_words - (tq << 2) if tab_words and not split else 0, "second_pass": tab_words != 0 and tq > 256,
            "stage_loop": needed > 64, "second_verify_sweep": nv > 64, "second_output_sweep": rows > 64}


# ---- chunks -------------------------------------------------------------------------------------------------------------------------------
class Chunk:
    """one word: vals = {sender id: value}; kind: honest / tamper / liar; rare: the group its targets come from (or None);
    window: the second-chance window claimed to accept it (None: no claim); liars: the sorted positions that lie"""

    def __init__(self, name, vals, kind="honest", rare=None, window=None, liars=(), poly=None):
        self.name, self.vals, self.kind, self.rare, self.window, self.liars, self.poly = name, vals, kind, rare, window, tuple(liars), poly


def groups_of(F):
    return FR_GROUPS if F is FR else GL_GROUPS


def tamper_pair(F, bit):
    if F is FR:
        return E.tamper_value(bit)
    base = (P - 3) if bit == 0 else (1 << 32) + 5
    assert not base >> bit & 1 and base | 1 << bit < P
    return base, base | 1 << bit


def _poly_through(F, n, parties, values):
    """the coefficients (zero padded to len(parties)) of the polynomial through those senders' values"""
    co = X._interpolate(F, n, list(parties), [v % F.mod for v in values])
    return list(co) + [0] * (len(parties) - len(co))


def window_liars(starts, m, Pfx, w, limit):
    """the smallest set of positions below Pfx, at most `limit` of them, that meets every window tried before w and misses window w; None when
    there is none (w == len(starts): a set that meets every window)"""
    wins = [set(range(s, s + m)) for s in starts]
    free = wins[w] if w < len(wins) else set()
    need = wins[:w]
    best = None

    def rec(chosen, rest):
        nonlocal best
        if best is not None and len(chosen) >= len(best):
            return
        if not rest:
            best = list(chosen)
            return
        if len(chosen) == limit:
            return
        for pos in sorted(rest[0] - free):
            rec(chosen + [pos], [x for x in rest if pos not in x])

    rec([], need)
    return best


class Batch:
    """the chunks of one (field, shape, sender set): set_name "direct" (S = d + t + 1, no OEC round) or "all" (S = n)"""

    def __init__(self, F, n, t, d, set_name):
        self.F, self.n, self.t, self.d, self.set_name = F, n, t, d, set_name
        m, needed = d + 1, d + t + 1
        self.m, self.needed = m, needed
        rng = random.Random("decode/%s/%d/%d/%d/%s" % (F.name, n, t, d, set_name))
        self.srt = sorted(rng.sample(range(n), needed)) if set_name == "direct" else list(range(n))
        self.S = len(self.srt)
        self.ids = list(self.srt)
        rng.shuffle(self.ids)
        self.rmax = X.rmax_of(t, d, self.S)
        self.Pfx = needed + self.rmax
        self.chunks = []
        self._build(rng)
        self.G = len(self.chunks)

    # -- helpers
    def _word(self, poly, errors=None):
        return X.word(self.F, self.n, self.srt, poly, errors or {})

    def _add(self, name, poly, **kw):
        self.chunks.append(Chunk(name, self._word(poly), poly=list(poly), **kw))
        return self.chunks[-1]

    def _lie(self, base, name, positions, rng, **kw):
        """a copy of an honest chunk with wrong values at those sorted positions (+1, -1 alternating: every limb but the lowest agrees)"""
        vals = dict(base.vals)
        for j, pos in enumerate(positions):
            i = self.srt[pos]
            vals[i] = (vals[i] + (1, self.F.mod - 1, 1 << 40)[j % 3]) % self.F.mod
        self.chunks.append(Chunk(name, vals, kind="liar", rare=base.rare, liars=positions, poly=base.poly, **kw))

    def _build(self, rng):
        F, n, m, needed, srt, q = self.F, self.n, self.m, self.needed, self.srt, self.F.mod
        nv = needed - m
        win, ver = srt[:m], srt[m:needed]
        groups = groups_of(F)
        # honest, uniform: the fast path of everything
        for j in range(3):
            self._add("random_%d" % j, [rng.randrange(q) for _ in range(m)])
        # coefficient k is the target, for every k and every value of every group
        coef = {}
        for gname, vals in groups.items():
            for rot in range(len(vals)):
                c = self._add("coef_%s_%d" % (gname, rot), [vals[(k + rot) % len(vals)] for k in range(m)], rare=gname)
                coef.setdefault(gname, c)
        # the values at a block of verify-row senders are the target (the rest of the d + 1 free values: window senders, edge values)
        verify = {}
        blocks = [ver[i:i + m] for i in range(0, nv, m)]
        for gname, vals in groups.items():
            for rot in ((0, 1) if gname == "flip" else (0,)):      # two of the three values around the flip per row: one of them is beyond it
                for bi, blk in enumerate(blocks):
                    fill = [p for p in win if p not in blk][:m - len(blk)]
                    parties = list(blk) + fill
                    values = [vals[(bi + i + rot) % len(vals)] for i in range(len(blk))] + [E.pick(F, bi + 3 * i) for i in range(len(fill))]
                    c = self._add("verify_%s_%d_b%d" % (gname, rot, bi), _poly_through(F, n, parties, values), rare=gname)
                    assert all(c.vals[p] == v % q for p, v in zip(parties, values))
                    verify.setdefault(gname, c)
        # headroom: every sender holds the same all-ones value (so do the first m: the polynomial through them is the constant)
        for nm, v in (("maxlimb", E.MAXLIMB), ("rm1", R - 1)) if F is FR else (("pm1", P - 1), ("p_2_32", P - (1 << 32))):
            self._add("constant_" + nm, [v] + [0] * (m - 1))
        self._add("zero", [0] * m, rare="sub")
        if F is GL and (n, self.t, self.d) == GL_FOLD_SHAPE:        # output row 0 takes `lo < hh` in its final reduction
            self._add("gl_final_lo_lt_hh", _poly_through(F, n, win, GL_FOLD_WORD), rare="fold")
        # one bit of one sender's share: every bit at a window sender and at a sender beyond d + t + 1, every verify-row sender with the bits
        # in turn (from the top one down, so that the last senders of a long verify sweep carry the high limbs too)
        bits = E.TAMPER_BITS if F is FR else GL_TAMPER_BITS
        targets = [("win", win[bi % m], bit) for bi, bit in enumerate(bits)]
        targets += [("ver", ver[vi], bits[-1 - vi % len(bits)]) for vi in range(nv)]
        targets += [("beyond", srt[needed + bi % (self.S - needed)], bit) for bi, bit in enumerate(bits)] if self.rmax else []
        for kind, sender, bit in targets:
            base, hit = tamper_pair(F, bit)
            others = [p for p in (win + ver) if p != sender][:m - 1]
            poly = _poly_through(F, n, [sender] + others, [base] + [rng.randrange(q) for _ in others])
            vals = self._word(poly)
            assert vals[sender] == base
            vals[sender] = hit
            self.chunks.append(Chunk("tamper_%s_s%d_bit%d" % (kind, sender, bit), vals, kind="tamper", liars=(srt.index(sender),), poly=poly))
        # second chance: exactly window w accepts.  Per window and group: the accepted polynomial's coefficients are the targets (coef_*),
        # and its values at honest positions outside the window are (check_*: the check rows' results)
        if self.rmax:
            starts = self.starts()
            for w in range(len(starts) + 1):
                liars = window_liars(starts, m, self.Pfx, w, self.rmax if w < len(starts) else self.t)
                if liars is None or (w == 0 and not liars):
                    liars = [m] if w == 0 and nv else None      # window 0: the optimistic verification must fail, a liar in a verify row
                if not liars:
                    continue
                claimed = w if w < len(starts) else None
                tag = "window%d" % w if w < len(starts) else "unresolved"
                for g in groups:
                    self._lie(coef[g], "%s_%s" % (tag, coef[g].name), liars, rng, window=claimed)
                ws = starts[w] if w < len(starts) else 0
                outside = [pos for pos in range(self.Pfx) if not ws <= pos < ws + m and pos not in liars]
                for gname, vals in groups.items():
                    forced = outside[:m]
                    fill = [pos for pos in range(ws, ws + m)][:m - len(forced)]
                    first = 1 if gname == "flip" else 0           # the value beyond the flip comes first: some windows have one honest check row
                    values = [vals[(first + i) % len(vals)] for i in range(len(forced))] + [E.pick(F, w + 3 * i) for i in range(len(fill))]
                    poly = _poly_through(F, n, [srt[pos] for pos in forced + fill], values)
                    base = Chunk("check_%s" % gname, self._word(poly), rare=gname, poly=poly)
                    self._lie(base, "%s_check_%s" % (tag, gname), liars, rng, window=claimed)
                sp = ([1, q - 1] + [0] * m)[:m] if m > 1 else [0]
                short = Chunk("short_poly", self._word(sp), poly=sp)
                self._lie(short, tag + "_top_coefficients_zero", liars, rng, window=claimed)
                zero = Chunk("zero", self._word([0] * m), poly=[0] * m)
                self._lie(zero, tag + "_zero_polynomial", liars, rng, window=claimed)
            # exactly rmax mismatches, the first check row honest: the last count a window still accepts
            self._lie(coef["keep" if F is FR else "high"], "window0_rmax_liars", ([m + 1] if nv > 1 else [m]) + list(range(self.Pfx - self.rmax + 1, self.Pfx)), rng, window=0)
            if self.t + 1 <= self.Pfx - m:
                self._lie(coef[next(iter(groups))], "too_many_liars", list(range(m, m + self.t + 1)), rng)

    def starts(self):
        """where the second-chance windows start: the lowest m positions of the prefix, the next m, the last m and one straddling the first
        two, those that fit and are distinct (tests/test_decode_inputs.py holds this to the tables the library builds)"""
        out = []
        for o in (0, self.m, self.Pfx - self.m, (self.m + 1) // 2):
            if 0 <= o and o + self.m <= self.Pfx and o not in out:
                out.append(o)
        return out

    def sorted_values(self, c):
        return [c.vals[i] for i in self.srt]

    def array(self, picks=None):
        picks = range(self.G) if picks is None else picks
        return self.F.arr([[self.chunks[g].vals[i] for g in picks] for i in self.ids])

    def index(self, prefix, nth=0):
        return [i for i, c in enumerate(self.chunks) if c.name.startswith(prefix)][nth]


_batches = {}


def batch(F, shape, set_name):
    key = (F.name, shape, set_name)
    if key not in _batches:
        _batches[key] = Batch(F, *shape, set_name)
    return _batches[key]


def set_names(shape):
    n, t, d = shape
    return ("direct",) + (("all",) if n > d + t + 1 else ())


# ---- calls ----------------------------------------------------------------------------------------------------------------------------------
ROUTES = ("mc0", "mc0,small0", "mc0,generic")


def routes_for(impl, shape, set_name):
    """matrix cores off throughout, so that the first kernel is the one named: Wide, the lane kernels, the runtime-shaped one; each with the
    second chance off where the call has OEC rounds.  sat32 is a comparison route: the default only.  The instantiation sweep: the lane
    kernels only."""
    n, t, d = shape
    base = ("mc0",) if impl == "sat32" else ("mc0,small0",) if shape not in SHAPES else ROUTES
    return tuple(k for r in base for k in ((r, r + ",second0") if set_name == "all" else (r,)))


class Call:
    def __init__(self, impl, knobs, shape, set_name, picks, name="cases"):
        self.impl, self.knobs, self.shape, self.set_name, self.picks, self.name = impl, knobs, shape, set_name, list(picks), name
        self.F, self.G = IMPLS[impl], len(self.picks)

    def batch(self):
        return batch(self.F, self.shape, self.set_name)

    def query(self, form):
        n, t, d = self.shape
        return (form, self.knobs, {"u29": "fr"}.get(self.impl, self.impl), self.G, n, d, t, self.batch().S, "-")

    def claim(self):
        """(first kernel, one | tail, rmax, second) as tests/cpp/recover_routes_dump prints them"""
        n, t, d = self.shape
        kn, m, b = self.knobs.split(","), d + 1, self.batch()
        wide = "small0" not in kn and "generic" not in kn and self.G <= 8192
        if "generic" in kn or self.impl == "sat32" and not wide:
            first = "Generic"
        elif wide:
            first = "Wide"
        else:
            first = {"u29": "RecoverM", "gl": "GoldRecoverM"}[self.impl] if m <= 16 else "Generic"
        if not b.rmax:
            return first, "one", 0, "none"
        tail_second = "m" if self.impl == "u29" and "generic" not in kn else "generic"
        fused = first == "Wide" and m <= 64 and b.Pfx - m <= 64
        return first, "tail", b.rmax, "none" if "second0" in kn else "kernel" if fused else tail_second


def layout_picks(b, shape_kind):
    """canon_loose's subtraction is taken per wave.  "block": a whole block of rare chunks, fast ones, and a rare chunk last in the ragged
    final block (G = 300: G % 4 and G % 256 are not zero); "alone": one rare chunk among fast ones, last of a ragged block (G = 133)"""
    fast = [b.index("random_%d" % j) for j in range(3)]
    rare = [i for i, c in enumerate(b.chunks) if c.kind == "honest" and c.rare is not None and (b.F is GL or c.rare in RARE)]
    assert rare
    if shape_kind == "block":
        return [rare[g % len(rare)] for g in range(256)] + [fast[g % 3] for g in range(43)] + [rare[0]]
    return [fast[g % 3] for g in range(132)] + [rare[-1]]


def calls_for(impl, shape):
    out = []
    for set_name in set_names(shape):
        b = batch(IMPLS[impl], shape, set_name)
        for knobs in routes_for(impl, shape, set_name):
            out.append(Call(impl, knobs, shape, set_name, range(b.G)))
            if "second0" not in knobs and impl != "sat32":
                out.append(Call(impl, knobs, shape, set_name, layout_picks(b, "block"), "block"))
                out.append(Call(impl, knobs, shape, set_name, layout_picks(b, "alone"), "alone"))
    return out


SWITCH_SHAPE = (16, 5, 5)


def switch_calls(impl):
    """flagged counts at the switch between the wave form and the lane form of the second chance, G = 512: the kernels run
    min(ceil(G / 256), 1024) = 2 blocks of 4 waves, so nwaves = 8 (k_second_chance_m: 8 and 9 flagged) and, with P - m = 10 check rows,
    nwaves * spread = 40 (k_second_chance: 40 and 41)"""
    b = batch(IMPLS[impl], SWITCH_SHAPE, "all")
    fast = [b.index("random_%d" % j) for j in range(3)]
    liars = [i for i, c in enumerate(b.chunks) if c.window is not None or c.name.startswith("unresolved")]
    out = []
    for knobs, counts in (("mc0,small0", (8, 9)), ("mc0,generic", (40, 41))):
        for cnt in counts:
            picks = [fast[g % 3] for g in range(512)]
            for j in range(cnt):
                picks[(j * 12 + 5) % 512] = liars[j % len(liars)]
            out.append(Call(impl, knobs, SWITCH_SHAPE, "all", picks, "switch%d" % cnt))
    return out


SECOND_TRIP_SHAPE = (7, 2, 2)
SECOND_TRIP_G = 262144 + 300


def second_trip_calls(impl):
    """more flagged chunks than the second chance's grid takes in one trip (1024 blocks of 256): every chunk flagged, 24 distinct
    words over Fr and 16 over Goldilocks (every chunk of the shape that claims window 0 or 1).  Whole runs of 256 consecutive chunks that window 0 resolves alternate with runs that window 1 resolves, and the alternation
    turns over at chunk 262 144: with the list in chunk order block 0 meets window 0 and then window 1, block 1 window 1 and then window 0
    (its `first` has moved to 1, so the candidates wrap round past the last window)"""
    b = batch(IMPLS[impl], SECOND_TRIP_SHAPE, "all")
    wa = [i for i, c in enumerate(b.chunks) if c.window == 0][:12]
    wb = [i for i, c in enumerate(b.chunks) if c.window == 1][:12]
    k = min(len(wa), len(wb))
    assert k >= 8
    picks = [(wa, wb)[((g >> 8) + (g >> 18)) & 1][g % k] for g in range(SECOND_TRIP_G)]
    return [Call(impl, knobs, SECOND_TRIP_SHAPE, "all", picks, "second_trip") for knobs in ("mc0,small0", "mc0,generic")]


def all_calls(impl):
    out = []
    for shape in SHAPES + tuple(s for s in SWEEP_SHAPES if s not in SHAPES):
        out += calls_for(impl, shape)
    return out + (switch_calls(impl) if impl != "sat32" else [])
