"""Deterministic bound-edge inputs for the lane-per-chunk FFT encode kernels (csrc/kernels_eval.hpp: k_eval_fft1, k_eval_fftP and its
fold form, k_eval_fft1_triple, k_eval_fft1_mix), over Fr / U29 and Goldilocks, from plain integers and oracle/ alone.

The kernels add lazily and reduce where compile-time bookkeeping (csrc/fft_bounds.hpp) says they must; a wrong decision shows only on
all-ones limbs, on terms that add constructively, or on an output within 2^232 of r.  Every chunk-major case holds

  the rows all zero, all r - 1, all MAXLIMB (Goldilocks: all 2^32 - 1), for the fold form the pairs (k, k + 16) both MAXLIMB
  constant polynomials over every edge value, one impulse row of r - 1 per coefficient position
  targeted outputs        random non-zero coefficients with c_0 solved so that the evaluation at a chosen point j IS a chosen value
  targeted intermediates  (Goldilocks) coefficients solved in the model so that an operand of a multiply inside the transform is a chosen
                          edge value, or one that takes the multiply's rare final subtraction
  random rows             up to a batch of G = 1 (mod 64), G >= 129: two full tiles and a tile of one row

tests/test_fft_inputs.py proves on the CPU, with the model of tests/fft_model.py, that the inputs reach their sites and that every case
takes the FFT route; tests/test_gpu_fft_edges.py compares every byte with the oracle."""
import random

import numpy as np

from tests import fft_model as M
from tests.edge_inputs import B, EDGE_GL, FR, GL, MAXLIMB, P, R

K_FFT = "mc0,small0"                               # no matrix cores, no wave-per-chunk kernels: the lane-per-chunk FFTs
TARGETS = {"fr": (0, 1, B - 1, B, B + 5, R - 2, R - 1, MAXLIMB), "goldilocks": EDGE_GL}
ALL_ONES = {"fr": MAXLIMB, "goldilocks": (1 << 32) - 1}
SMALL_G = (1, 63, 64, 65)
FIELDS = {"fr": FR, "goldilocks": GL}


def domain_size(n):
    return 1 << (n - 1).bit_length() if n > 1 else 1


def ilog2(size):
    return size.bit_length() - 1


# ---- the instantiations -------------------------------------------------------------------------------------------------------------
def fft1_shapes():
    """(LOG, CNT, n): every instantiation on its full domain, and n = 2^LOG / 2 + 1 for CNT in {1, 2^LOG / 2 + 1}"""
    out = []
    for LOG in range(5):
        size = 1 << LOG
        for CNT in range(1, size + 1):
            out.append((LOG, CNT, size))
            if LOG >= 2 and CNT in (1, size // 2 + 1):
                out.append((LOG, CNT, size // 2 + 1))
    return out


def fftP_shapes():
    """(P, d + 1, n): n alternates between the full domain and max(size / 2 + 1, d + 1)"""
    out = []
    for Pn in (2, 4, 8, 16):
        dp1s = list(range(1, 17)) if Pn in (2, 16) else [1, 6, 11, 16]
        for i, dp1 in enumerate(dp1s + [17, 24, 32]):
            size = 16 * Pn
            out.append((Pn, dp1, size if i % 2 == 0 else max(size // 2 + 1, dp1)))
    return out


TRIPLE_INST = [(2, 3), (3, 3), (3, 5), (4, 5), (4, 7), (4, 9), (4, 11)]      # (LOG, d + 1) of tu_eval_triple.hip / tu_eval_triple_gold.hip
MIX_N = {"fr": list(range(3, 9)), "goldilocks": list(range(3, 17))}
SMALL_G_FFT1 = [(2, 3, 4), (3, 8, 8), (4, 6, 16), (4, 16, 16)]
SMALL_G_FFTP = [(2, 6, 17), (4, 11, 64), (16, 15, 256), (8, 32, 128)]         # (P, d + 1, n) of fftP_shapes(): n = 256 and a fold case among them
STRIDED_FFT1 = [(1, 2, 2), (3, 5, 5), (4, 11, 16)]
STRIDED_FFTP = [(2, 3, 32), (4, 16, 33), (16, 32, 256)]


def triple_shapes():
    """(LOG, d + 1, n)"""
    return [(LOG, cnt, (1 << LOG) if i % 2 == 0 else max((1 << LOG) // 2 + 1, cnt)) for i, (LOG, cnt) in enumerate(TRIPLE_INST)]


# ---- rows -------------------------------------------------------------------------------------------------------------------------------
_alpha = {}


def alpha(F, n, j, k):
    key = (F.name, domain_size(n))
    if key not in _alpha:
        _alpha[key] = F.S.domain_omega(domain_size(n))
    return pow(_alpha[key], j * k, F.mod)


def evaluate(F, row, n, j):
    return sum(c * alpha(F, n, j, k) for k, c in enumerate(row)) % F.mod


def target_points(n, P_passes, case_index):
    """the points whose outputs are targeted: every j < n up to 16 points; beyond, j = 0, j = n - 1 and one j in every pass r, its
    16-point index moving with the case so that the cases of one P cover all 16"""
    if domain_size(n) <= 16:
        return list(range(n))
    pts = [0, n - 1]
    for r in range(P_passes):
        avail = (n - r + P_passes - 1) // P_passes                 # indices idx with r + P idx < n
        pts.append(r + P_passes * ((case_index + 5 * r) % 16 % avail))
    return sorted(set(pts))


class Case:
    def __init__(self, F, family, n, d, rows, targets, P_passes, extra):
        self.F, self.family, self.n, self.d, self.rows, self.targets, self.P, self.extra = F, family, n, d, rows, targets, P_passes, extra
        self.G = len(rows)
        self.LOG = ilog2(domain_size(n)) if family != "fftP" else 4
        self.fold = d + 1 > 16
        self.inst = (self.LOG, d + 1) if family != "fftP" else (min(d + 1, 16), self.fold)

    def array(self, G=None):
        return self.F.arr(self.rows[:G or self.G])


def _gl_first_mul(n, dp1, P_passes, rows):
    """the operand and the constant of the first multiply of the transform, over a batch of rows (None: it has none)"""
    x = np.array(rows, dtype=np.uint64).reshape(-1, dp1)
    tr = M.gl_fft1(x, ilog2(domain_size(n)), dp1, n)[1] if P_passes == 1 else M.gl_fftP(x, P_passes, n)[1]
    first = [(op, c) for op, c in tr.muls if c != 1]
    return first[0] if first else None


_rare_cache = {}
RARE_SEARCH = 1 << 14


def gl_rare_operand(c):
    """an operand a whose product with the constant c takes mulm's final subtraction (r >= P): the product is then below 2^32 - 1, so the
    search is over the products 1 .. RARE_SEARCH, a = product / c, with the model's mulm deciding (None: none of them does)"""
    if c not in _rare_cache:
        inv = pow(c, P - 2, P)
        cand = np.array([res * inv % P for res in range(1, RARE_SEARCH)], dtype=np.uint64)
        tr = M.GlTrace()
        M.gl_mulm(cand, np.uint64(c), tr)
        idx = np.flatnonzero(tr.last_mul[2])
        _rare_cache[c] = int(cand[idx[0]]) if len(idx) else None
    return _rare_cache[c]


def _gl_intermediate_rows(n, dp1, P_passes, rng):
    """Goldilocks targeted intermediates.  fftP: coefficient k under twist r IS an edge value (an operand of the multiply), is an edge
    value over the twist (the product, an operand of the next add), and is an operand that takes the multiply's final subtraction.
    fft1: the first multiplied value of the transform is solved likewise (it is linear in the coefficients)."""
    rows, sites = [], []
    q = P
    if P_passes > 1:
        w = GL.S.domain_omega(16 * P_passes)
        for i, v in enumerate(EDGE_GL):
            r, k = 1 + i % (P_passes - 1), (i * 3 + 1) % dp1
            tw = pow(w, r * k, q)
            for c in (v, v * pow(tw, q - 2, q) % q):
                row = [rng.randrange(1, q) for _ in range(dp1)]
                row[k] = c
                rows.append(row)
            sites.append(("twist", r, k, v))
        for k in range(1, min(dp1, 4)):
            a = gl_rare_operand(pow(w, k, q))                      # pass r = 1
            if a is not None:
                row = [rng.randrange(1, q) for _ in range(dp1)]
                row[k] = a
                rows.append(row)
        return rows, sites
    unit = [[int(i == k) for i in range(dp1)] for k in range(dp1)]
    first = _gl_first_mul(n, dp1, 1, unit)
    if first is None:
        return rows, sites
    lin, c = [int(v) for v in first[0]], first[1]
    kstar = max(k for k in range(dp1) if lin[k])
    wanted = list(EDGE_GL) + ([gl_rare_operand(c)] if gl_rare_operand(c) is not None else [])
    for v in wanted:
        row = [rng.randrange(1, q) for _ in range(dp1)]
        rest = sum(row[k] * lin[k] for k in range(dp1) if k != kstar)
        row[kstar] = (v - rest) * pow(lin[kstar], q - 2, q) % q
        rows.append(row)
        sites.append(("first_mul", c, v))
    return rows, sites


_cases = {}


def chunk_case(field, family, n, d, P_passes=1, case_index=0):
    """the chunk-major case of one (field, n, d): rows [G][d + 1] of ints"""
    key = (field, family, n, d, P_passes, case_index)
    if key in _cases:
        return _cases[key]
    F = FIELDS[field]
    q, dp1 = F.mod, d + 1
    rng = random.Random("%s %s %d %d" % (field, family, n, d))
    rows = [[0] * dp1, [q - 1] * dp1, [ALL_ONES[field]] * dp1]
    if dp1 > 16:
        pairs = [k for k in range(16) if k + 16 < dp1]
        rows.append([ALL_ONES[field] if (k % 16) in pairs else 0 for k in range(dp1)])
        for k in (pairs[0], pairs[-1]):
            rows.append([ALL_ONES[field] if i in (k, k + 16) else 0 for i in range(dp1)])
    rows += [[v] + [0] * d for v in F.edge]
    rows += [[(q - 1) * int(i == k) for i in range(dp1)] for k in range(dp1)]
    targets = []
    for j in target_points(n, P_passes, case_index):
        for v in TARGETS[field]:
            row = [0] + [rng.randrange(1, q) for _ in range(d)]
            row[0] = (v - evaluate(F, row, n, j)) % q
            targets.append((len(rows), j, v))
            rows.append(row)
    extra = []
    if field == "goldilocks":
        more, extra = _gl_intermediate_rows(n, dp1, P_passes, rng)
        rows += more
    G = max(129, len(rows) + (1 - len(rows)) % 64)
    rows += [[rng.randrange(q) for _ in range(dp1)] for _ in range(G - len(rows))]
    assert len(rows) % 64 == 1 and len(rows) >= 129
    _cases[key] = Case(F, family, n, d, rows, targets, P_passes, extra)
    return _cases[key]


def fft1_cases(field):
    return [chunk_case(field, "fft1", n, CNT - 1) for LOG, CNT, n in fft1_shapes()]


def fftP_case(field, Pn, dp1, n):
    """the case of one entry of fftP_shapes(); its index among the cases of its P moves the targeted 16-point indices"""
    same_P = [sh for sh in fftP_shapes() if sh[0] == Pn]
    return chunk_case(field, "fftP", n, dp1 - 1, Pn, same_P.index((Pn, dp1, n)))      # ValueError: no such shape


def fftP_cases(field):
    return [fftP_case(field, Pn, dp1, n) for Pn, dp1, n in fftP_shapes()]


# ---- triple: a, b chosen, r2t solved so that the staged coefficient a b - r2t is the chunk-major row --------------------------------------
def triple_case(field, LOG, cnt, n, parties):
    """{a, b, r2t: [parties][G cnt] ints, c: [parties][G][cnt]}: party p holds the chunk-major case's rows rolled by 64 p"""
    F = FIELDS[field]
    q = F.mod
    base = chunk_case(field, "fft1", n, cnt - 1)
    rng = random.Random("triple %s %d %d %d" % (field, LOG, cnt, n))
    G = base.G
    out = {"a": [], "b": [], "r2t": [], "c": [], "G": G}
    for p in range(parties):
        rows = base.rows[64 * p:] + base.rows[:64 * p]
        a, b, r = [], [], []
        for i, c in enumerate(v for row in rows for v in row):
            av = F.edge[(i // 2 + p) % len(F.edge)] if i % 2 == 0 else rng.randrange(q)
            bv = F.edge[(i // 3 + 4 + p) % len(F.edge)] if i % 3 == 0 else rng.randrange(q)
            if field == "goldilocks" and i % 22 == 5 and bv and gl_rare_operand(bv) is not None:
                av = gl_rare_operand(bv)                       # the product a b takes mulm's final subtraction
            a.append(av), b.append(bv), r.append((av * bv - c) % q)
        out["a"].append(a), out["b"].append(b), out["r2t"].append(r), out["c"].append(rows)
    return out


# ---- the routes the GPU test relies on ---------------------------------------------------------------------------------------------------
def route_queries():
    """(query of tests/cpp/encode_routes_dump, the kernel it must name first) for every case of tests/test_gpu_fft_edges.py"""
    out = []
    for field, fl in (("fr", "fr"), ("goldilocks", "gl")):
        for c in fft1_cases(field):
            for G in (c.G,) + (SMALL_G if (c.LOG, c.d + 1, c.n) in SMALL_G_FFT1 else ()):
                out.append((("shares", K_FFT, fl, G, c.n, c.d, 1), "Fft1"))
        for c in fftP_cases(field):
            for G in (c.G,) + (SMALL_G if (c.P, c.d + 1, c.n) in SMALL_G_FFTP else ()):
                out.append((("shares", K_FFT, fl, G, c.n, c.d, 1), "FftP"))
        for (LOG, cnt, n) in STRIDED_FFT1:
            c = chunk_case(field, "fft1", n, cnt - 1)
            out.append((("strided", K_FFT, fl, c.G, n, cnt - 1, 1), "Fft1"))
            out.append((("shares", K_FFT, fl, c.G, n, cnt - 1, 3), "Fft1"))
        for (Pn, dp1, n) in STRIDED_FFTP:
            c = fftP_case(field, Pn, dp1, n)
            out.append((("strided", K_FFT, fl, c.G, n, dp1 - 1, 1), "FftP"))
            out.append((("shares", K_FFT, fl, c.G, n, dp1 - 1, 3), "FftP"))
        for LOG, cnt, n in triple_shapes():
            G = chunk_case(field, "fft1", n, cnt - 1).G
            for parties in (1, 3):
                out.append((("triple", "default", fl, G, n, cnt - 1, parties), "Fft1Triple"))
        for n in MIX_N[field]:
            out.append((("lists", "default", fl, n * mix_K(field, n), n, n - 1, 1), "Fft1Mix"))
    return out


def mix_K(field, n):
    """batch elements per party of the mixing step's case: n K >= 129 chunks (two full blocks and more), K no multiple of 64"""
    K = -(-129 // n)
    return K + 1 if K % 64 == 0 else K


def mix_rows(field, n):
    """the n K chunks of the mixing step: the (n, n - 1) chunk-major case, taken round again where it is shorter"""
    c = chunk_case(field, "fft1", n, n - 1)
    return (c.rows * 2)[:n * mix_K(field, n)]
