"""Deterministic adversarial inputs for the matrix-core kernels (k_mfma_bfly, k_mfma_rows and their team, SUB, DEG, TRIPLE and
Goldilocks variants), chosen with the integer model of tests/mfma_model.py; plain Python, numpy and oracle/ alone (no library, no GPU).

Uniform inputs keep every digit sum in the middle third of [0, 0xff0000) and reach the slow path of reduce_words about once in 10^4
elements.  Here every chunk is chosen against a table row:

  digit extremes   for every output row and every digit b the chunk that maximises and the one that minimises that digit sum: byte 0xff
                   or 0x00 by the sign of the table entry, the top byte of an element at most 0x72 (0xfe over Goldilocks) so that it
                   stays canonical; for a point pair the same for E + T and for E - T, and chunks whose T accumulator alone is negative
  value extremes   the chunks with the largest and the smallest sum as an integer (the largest quotient and top word)
  slow path        chunks whose result in a chosen row is a chosen value: 0, 1, 2 (one subtraction: the quotient estimate is one short
                   whenever the residue is tiny), r - 1, r - 2 and values from R_TOP 2^224 on (top word equal to r's: the slow path
                   with no subtraction), as constant polynomials and as random polynomials solved for one row
  layout           the slow path is taken per wave: a slow chunk alone in a tile of fast ones, a whole tile of slow chunks, and a slow
                   chunk last in the ragged final tile

tests/test_mfma_inputs.py proves with the model what these reach.  All inputs are canonical.
"""
import random

import numpy as np

from oracle import cref as O
from oracle import cref_gl as OG
from oracle import spec as SFR
from oracle.spec_gl import S as SGL
from tests import mfma_model as MM

R, P = MM.R, MM.P
TOP = MM.R_TOP << 224
FR_TARGETS = (0, 1, 2, R - 1, R - 2, TOP, TOP + 0x1234567, 1 << 200, (1 << 243) + 5, TOP - 1)
GL_TARGETS = (0, 1, (1 << 32) - 2, (1 << 32) - 1, 1 << 32, (1 << 40) + 3, P - (1 << 32), P - 2, P - 1)
TAMPER_BITS = (0, 31, 32, 127, 128, 253)          # the word and lane-half boundaries of verify_tile
_cache = {}


def _memo(fn):
    def wrapped(*key):
        k = (fn.__name__,) + key
        if k not in _cache:
            _cache[k] = fn(*key)
        return _cache[k]
    return wrapped


# ---- coefficient matrices ----------------------------------------------------------------------------------------------------------
def domain_size(n):
    return 1 << max(n - 1, 0).bit_length()


@_memo
def vandermonde(field, n, m, scale=1):
    S, q = (SFR, R) if field == "fr" else (SGL, P)
    return [[scale * pow(S.domain_element(n, j), k, q) % q for k in range(m)] for j in range(n)]


@_memo
def inverse_transform(n):
    """omega^(-i k) / n on a full domain of n points: the rows of hbmpc_dev_batch_interpolate's point-pair table"""
    el = [SFR.domain_element(n, k) for k in range(n)]
    ninv = pow(n, -1, R)
    return [[el[(n - i * k % n) % n] * ninv % R for k in range(n)] for i in range(n)]


@_memo
def decode_rows(field, n, d, t, ids):
    """the verify rows, then the coefficient rows, of the decode through the sorted senders `ids` (the first d + 1 interpolate)"""
    S = SFR if field == "fr" else SGL
    m, needed = d + 1, d + t + 1
    xs = [S.domain_element(n, i) for i in ids[:m]]
    basis = []
    for i in range(m):
        co = S.lagrange_interpolate(xs, [1 if j == i else 0 for j in range(m)])
        basis.append(co + [0] * (m - len(co)))
    rows = [[S.p_eval(basis[i], S.domain_element(n, ids[s])) for i in range(m)] for s in range(m, needed)]
    return rows + [[basis[i][k] for i in range(m)] for k in range(m)]


# ---- chunks chosen against table rows ------------------------------------------------------------------------------------------------
def _elements(byte_row, width, cap):
    """uint8 [width m] -> m canonical integers (the top byte of every element at most `cap`)"""
    b = np.array(byte_row, dtype=np.uint8).reshape(-1, width).copy()
    b[:, width - 1] = np.minimum(b[:, width - 1], cap)
    return [int.from_bytes(bytes(r), "little") for r in b]


def digit_extreme(dig, b, maximise, width=32, cap=0x72, flip_odd=False):
    """the chunk that maximises (minimises) digit sum b of a row with digits dig[width m][digits]; flip_odd: the sum E - T"""
    col = dig[:, b].copy()
    if flip_odd:
        odd = (np.arange(len(col)) // width) & 1
        col = np.where(odd == 1, -col, col)
    take = col > 0 if maximise else col < 0
    return _elements(np.where(take, 0xff, 0x00), width, cap)


def value_extreme(dig, maximise, width=32, cap=0x72, flip_odd=False):
    """the chunk with the largest (smallest) sum as an integer: every byte by the sign of its table entry's balanced value"""
    val = np.array([sum(int(v) << (8 * b) for b, v in enumerate(row)) for row in dig], dtype=object)
    if flip_odd:
        val = np.array([-v if (k // width) & 1 else v for k, v in enumerate(val)], dtype=object)
    take = np.array([(v > 0) == maximise and v != 0 for v in val])
    return _elements(np.where(take, 0xff, 0x00), width, cap)


def solve_for(coeffs, x, target, q):
    """x with x[0] replaced so that sum coeffs[i] x[i] = target (mod q)"""
    rest = sum(c * v for c, v in zip(coeffs[1:], x[1:])) % q
    return [(target - rest) * pow(coeffs[0], -1, q) % q] + list(x[1:])


class Picker:
    """random canonical elements, deterministic per case"""

    def __init__(self, seed, q):
        self.rng, self.q = random.Random(seed), q

    def chunk(self, m):
        return [self.rng.randrange(self.q) for _ in range(m)]


def fr_quick(row_sums):
    """(q', residual S - q' r) of one output element from its 32 digit sums -- the branch reduce_words takes, without the replay"""
    L = [int(v) for v in row_sums]
    S = sum(v << (8 * b) for b, v in enumerate(L))
    t3 = (((L[31] << 8) + L[30]) << 16) + (L[29] << 8) + L[28]
    q = (((t3 >> 17) * MM.Q_RECIP) >> 32) >> 13
    return q, S - q * R


def fr_is_fast(row_sums):
    return 0 <= fr_quick(row_sums)[1] < TOP


class Case:
    """the chunks of one (map, shape): .x [G][m] integers, .classes {name: [chunk indices]}, .targets {chunk: (row, value)},
    .layout {alone, full_tile, ragged: chunk indices}, .C the coefficient matrix, .rows / .pairs the model's table, .reduce_rows the
    output rows that go through reduce_words (a decode's verify rows do not)"""

    def __init__(self):
        self.x, self.classes, self.targets, self.layout = [], {}, {}, {}

    def add(self, name, chunk, target=None):
        self.classes.setdefault(name, []).append(len(self.x))
        if target is not None:
            self.targets[len(self.x)] = target
        self.x.append(chunk)

    @property
    def G(self):
        return len(self.x)


def sums_by_row(case, chunks, width=32):
    """{output row j: digit sums [G][digits]} of the chunks for every row of the case's table (a pair table: E + T for row p, E - T for
    row p + half)"""
    X = MM.chunk_bytes(chunks, width)
    if case.pairs is None:
        return {j: row.sums(X) for j, row in enumerate(case.rows)}
    out = {}
    for p, pr in enumerate(case.pairs):
        E, T, plus, minus = pr.sums(X)
        out[p] = plus
        if pr.partner:
            out[p + case.half] = minus
    return out


def _row_sums_fr(case, chunk, j):
    """the 32 digit sums of output row j for one chunk"""
    X = MM.chunk_bytes([chunk])
    if case.pairs is None:
        return case.rows[j].sums(X)[0]
    E, T, plus, minus = case.pairs[j - case.half if j >= case.half else j].sums(X)
    return (minus if j >= case.half else plus)[0]


def _all_fast(case, chunk):
    s = sums_by_row(case, [chunk])
    return all(fr_is_fast(s[j][0]) for j in case.reduce_rows)


def _fr_case(C, m, seed, pair_half=None, reduce_rows=None, min_chunks=0, search=512, extra=()):
    """the classes of the module docstring for the Fr map x -> C x (rows of C: output rows; pair_half: the point-pair table)"""
    case = Case()
    case.C, case.m, case.half = C, m, pair_half
    case.rows = MM.plain_table(C)
    case.pairs = MM.pair_table(C, pair_half) if pair_half else None
    assert pair_half is None or case.pairs is not None
    case.reduce_rows = list(range(len(C))) if reduce_rows is None else list(reduce_rows)
    pk = Picker(seed, R)
    if case.pairs is None:
        for j, row in enumerate(case.rows):
            for b in range(32):
                case.add("digit_max", digit_extreme(row.dig, b, True))
                case.add("digit_min", digit_extreme(row.dig, b, False))
            case.add("value_max", value_extreme(row.dig, True))
            case.add("value_min", value_extreme(row.dig, False))
    else:
        for p, pr in enumerate(case.pairs):
            for b in range(32):
                case.add("plus_max", digit_extreme(pr.dig, b, True))
                case.add("plus_min", digit_extreme(pr.dig, b, False))
                if pr.partner:
                    case.add("minus_max", digit_extreme(pr.dig, b, True, flip_odd=True))
                    case.add("minus_min", digit_extreme(pr.dig, b, False, flip_odd=True))
            for b in (0, 15, 16, 31):
                # T alone as low as it goes, E as high: odd elements against the sign, even elements with it
                lo, hi = digit_extreme(pr.dig, b, False), digit_extreme(pr.dig, b, True)
                case.add("T_negative", [lo[i] if i & 1 else hi[i] for i in range(m)])
                case.add("E_lowest", [hi[i] if i & 1 else lo[i] for i in range(m)])
            case.add("value_max", value_extreme(pr.dig, True))
            case.add("value_min", value_extreme(pr.dig, False))
            if pr.partner:
                case.add("value_max", value_extreme(pr.dig, True, flip_odd=True))
                case.add("value_min", value_extreme(pr.dig, False, flip_odd=True))
    for name, chunk in extra:
        case.add(name, chunk)
    # the slow path: constant results (every row whose first coefficient column is the only nonzero one sees them) and one row solved
    for i, y in enumerate(FR_TARGETS):
        j = case.reduce_rows[i % len(case.reduce_rows)]
        case.add("slow_solved", solve_for(C[j], pk.chunk(m), y, R), (j, y))
        j2 = case.reduce_rows[-1 - i % len(case.reduce_rows)]
        case.add("slow_solved", solve_for(C[j2], pk.chunk(m), y, R), (j2, y))
    # a bounded search for the deepest slow path: random chunks, then single-byte steps uphill on the residual S - q' r
    best = None
    j = case.reduce_rows[len(case.reduce_rows) // 2]
    for _ in range(search):
        ch = pk.chunk(m)
        res = fr_quick(_row_sums_fr(case, ch, j))[1]
        if best is None or res > best[0]:
            best = (res, ch)
    res, ch = best
    for _ in range(search // 4):
        i, a = pk.rng.randrange(m), pk.rng.randrange(31)
        trial = list(ch)
        trial[i] = (trial[i] & ~(0xff << (8 * a))) | (pk.rng.randrange(256) << (8 * a))
        r2 = fr_quick(_row_sums_fr(case, trial, j))[1]
        if trial[i] < R and r2 > res:
            res, ch = r2, trial
    case.add("search_best", ch, (j, None))
    case.search_row = j
    _layout(case, pk, m, min_chunks, lambda i: solve_for(C[case.reduce_rows[i % len(case.reduce_rows)]], pk.chunk(m), FR_TARGETS[i % 3], R),
            lambda ch: _all_fast(case, ch))
    return case


def _layout(case, pk, m, min_chunks, slow, is_fast):
    """the layout section: filler up to a tile boundary (and to min_chunks), a slow chunk alone in a fast tile, a whole slow tile, a ragged
    last tile of five chunks whose last one is slow"""
    def fast():
        while True:
            ch = pk.chunk(m)
            if is_fast(ch):
                return ch
    while case.G % 32 or case.G + 69 < min_chunks:
        case.add("filler", fast())
    for lane in range(32):
        if lane == 17:
            case.layout["alone"] = case.G
            case.add("slow_alone", slow(0))
        else:
            case.add("filler", fast())
    case.layout["full_tile"] = case.G
    for lane in range(32):
        case.add("slow_tile", slow(lane))
    for lane in range(4):
        case.add("filler", fast())
    case.layout["ragged"] = case.G
    case.add("slow_ragged", slow(1))
    assert case.G % 32 == 5


# ---- the cases of tests/test_gpu_mfma_edges.py ---------------------------------------------------------------------------------------
PAIR_SHAPES = [(7, 2), (16, 5), (13, 4), (16, 15), (31, 10)]       # point pairs, chunk-major
ROWS_IN_SHAPE = (16, 15)                                           # point pairs, inputs as rows
PARTIES_SHAPE = (16, 5, 3)                                         # point pairs, all parties in one launch
DEG_N = 16                                                         # the inverse transform on a full domain
TRIPLE_SHAPE = (16, 5, 16)                                         # (n, d, parties): P G = 2^14
ROW_ENCODE_SHAPES = [(31, 10), (20, 6)]                            # one table row per point
TEAM_SHAPES = [(16, 5, 5), (31, 10, 10)]                           # workgroup per tile, encode and decode
DECODE_SHAPES = [(4, 1, 1), (16, 5, 5), (16, 10, 5), (31, 10, 10), (43, 14, 13), (31, 14, 10)]
SUB_SHAPE = (16, 5)
GL_SHAPES = [(31, 10, 10), (64, 21, 21)]


def _constants(m):
    """constant polynomials: EVERY output row of the chunk is the target (all rows of the chunk on the slow path at once)"""
    return [("constant", [y] + [0] * (m - 1)) for y in FR_TARGETS]


@_memo
def pair_case(n, d, min_chunks=545):
    """x[G][d + 1] against the point-pair table of the n x (d + 1) Vandermonde map; more than 16 tiles"""
    return _fr_case(vandermonde("fr", n, d + 1), d + 1, 1000 * n + d, pair_half=domain_size(n) // 2, min_chunks=min_chunks, extra=_constants(d + 1))


@_memo
def triple_case(n, d):
    """a[G][d + 1] against the point-pair table of alpha^i 2^261: with b = 2^261 mod r and r2t = 0 the kernel's x = (a b - r2t) / 2^261 is a"""
    return _fr_case(vandermonde("fr", n, d + 1, MM.RADIX % R), d + 1, 77 * n + d, pair_half=domain_size(n) // 2, min_chunks=1024)


@_memo
def inverse_case(n):
    """shares[G][n] (party k's share is input k) against the point-pair table of the inverse transform; outputs are coefficients"""
    rng = random.Random(n)
    polys = [[0] * n, [R - 1] + [0] * (n - 1), [1] + [0] * (n - 1), [0] * (n - 1) + [1], [R - 1] * n]
    polys += [[rng.randrange(R) for _ in range(k + 1)] + [0] * (n - 1 - k) for k in (1, 5, n - 2, n - 1)]
    low = [("low_degree", [SFR.p_eval(co, SFR.domain_element(n, k)) for k in range(n)]) for co in polys]
    return _fr_case(inverse_transform(n), n, 31 * n, pair_half=n // 2, min_chunks=545, extra=low)


@_memo
def row_encode_case(n, d, min_chunks=545):
    """x[G][d + 1] against the table with one row per point"""
    return _fr_case(vandermonde("fr", n, d + 1), d + 1, 2000 * n + d, min_chunks=min_chunks, extra=_constants(d + 1))


@_memo
def decode_case(n, d, t, min_chunks=0):
    """the first d + 1 sorted senders' values (free: any values define a polynomial) against the verify rows and the coefficient rows of the
    decode through senders 0 .. n - 1; .evals(): all n senders' values by the oracle, so that every chunk verifies"""
    m = d + 1
    C = decode_rows("fr", n, d, t, tuple(range(n)))
    case = _fr_case(C, m, 3000 * n + d + t, reduce_rows=range(t, t + m), min_chunks=min_chunks)
    case.n, case.d, case.t = n, d, t
    return case


def evals_of(case, field="fr"):
    """[n][G] values of all senders for the chunks of a decode case: the polynomial through the free values by the oracle's decode (t = 0),
    its shares by the oracle's encode"""
    Or = O if field == "fr" else OG
    n, d = case.n, case.d
    free = fr_array(case.x).transpose(1, 0, 2) if field == "fr" else np.array(case.x, dtype=np.uint64).T
    rc, co, nco, st = Or.batch_recover(list(range(d + 1)), np.ascontiguousarray(free), n, d, 0)
    assert rc == 0 and not st.any()
    rc, y = Or.vandermonde_apply(np.ascontiguousarray(co), n, d)
    assert rc == 0 and np.array_equal(y[:d + 1], free)
    return y


def fr_array(vals):
    a = np.array(vals, dtype=object)
    raw = b"".join(int(v).to_bytes(32, "little") for v in a.reshape(-1))
    return np.frombuffer(raw, dtype=np.uint64).reshape(a.shape + (4,)).copy()


def fr_ints(arr):
    raw = np.ascontiguousarray(arr, dtype=np.uint64).tobytes()
    flat = [int.from_bytes(raw[i:i + 32], "little") for i in range(0, len(raw), 32)]
    return np.array(flat, dtype=object).reshape(np.asarray(arr).shape[:-1]).tolist()


def tampered(case, y, field="fr"):
    """copies of chunks in which ONE claimed value (the sender behind verify row 0, 1, ...) differs in a single bit, the flipped value still
    canonical: (evals [n][G'], [(source chunk, sender, bit)]).  G' = 32, one whole tile: two chunks per bit, the others clean copies."""
    n, d, t = case.n, case.d, case.t
    bits = TAMPER_BITS if field == "fr" else (0, 31, 32, 63)
    q = R if field == "fr" else P
    cols, info = [0], [(0, None, None)]
    src = 0
    for bi, bit in enumerate(bits):
        for rep in range(2):
            sender = d + 1 + (bi + rep) % max(t, 1)
            while True:                                   # the next chunk whose flipped value is canonical
                src = (src + 7) % case.G
                v = (fr_ints(y[sender, src:src + 1])[0] if field == "fr" else int(y[sender, src])) ^ (1 << bit)
                if v < q:
                    break
            cols.append(src)
            info.append((src, sender, bit))
    while len(cols) < 32:                                 # a whole tile, so that the chunks behind it keep their place in theirs
        cols.append(len(cols))
        info.append((cols[-1], None, None))
    out = np.ascontiguousarray(y[:, cols]).copy()
    for k, (src, sender, bit) in enumerate(info):
        if sender is not None:
            if field == "fr":
                out[sender, k, bit // 64] ^= np.uint64(1 << (bit % 64))
            else:
                out[sender, k] ^= np.uint64(1 << bit)
    return out, info


def mfma_sub_covers(m):
    """tables_mfma.hpp: the SUB instances exist for m = 2 .. 11"""
    return 2 <= m <= 11


# ---- SUB decode: the operand pairs of sub_mod_r --------------------------------------------------------------------------------------
H128 = 1 << 128
RHI = R >> 128
SUB_PAIRS = {                                                      # name: (a, x), both canonical
    "low_only": (5 * H128 + 1, 3 * H128 + 2),
    "low_only_high_words": ((RHI - 1) * H128 + 1, (RHI - 3) * H128 + (H128 - 1)),
    "high_only_no_carry": (3 * H128 + 7, 5 * H128 + 2),
    "high_only_carry": (3 * H128 + (H128 - 1), 5 * H128),
    "both_ends_equal_high_carry": (5 * H128 + 1, 5 * H128 + 2),
    "both_ends_equal_high_no_carry": (5 * H128, 5 * H128 + (H128 - 1)),
    "both_borrow": (3 * H128 + 1, 5 * H128 + 2),
    "none": (5 * H128 + 9, 3 * H128 + 2),
    "none_top": (R - 1, 0),
    "equal_zero": (0, 0),
    "equal_top": (R - 1, R - 1),
    "equal_mid": (7 * H128 + 11, 7 * H128 + 11),
    "zero_minus_top": (0, R - 1),
    "one_minus_two": (1, 2),
}


# ---- Goldilocks ----------------------------------------------------------------------------------------------------------------------
def _row_sums_gl(case, chunk, j):
    return case.rows[j].sums(MM.chunk_bytes([chunk], 8))[0]


def _gl_case(C, m, seed, reduce_rows=None, min_chunks=0):
    """Goldilocks: digit and value extremes (the largest w2), results below 2^32 - 1 (the final subtraction of p), from 2^32 - 1 on (the
    64-bit wrap) and large ones (neither), as solved rows; the layout section keeps its shape (there is no per-wave branch here)"""
    case = Case()
    case.C, case.m, case.pairs, case.half = C, m, None, None
    case.rows = MM.gl_table(C)
    case.reduce_rows = list(range(len(C))) if reduce_rows is None else list(reduce_rows)
    pk = Picker(seed, P)
    for row in case.rows:
        for b in range(8):
            case.add("digit_max", digit_extreme(row.dig, b, True, 8, 0xfe))
            case.add("digit_min", digit_extreme(row.dig, b, False, 8, 0xfe))
        case.add("value_max", value_extreme(row.dig, True, 8, 0xfe))
        case.add("value_min", value_extreme(row.dig, False, 8, 0xfe))
    for i in range(4 * len(GL_TARGETS)):
        j = case.reduce_rows[(5 * i) % len(case.reduce_rows)]
        y = GL_TARGETS[i % len(GL_TARGETS)]
        case.add("solved", solve_for(C[j], pk.chunk(m), y, P), (j, y))
    _layout(case, pk, m, min_chunks, lambda i: solve_for(C[case.reduce_rows[i % len(case.reduce_rows)]], pk.chunk(m), GL_TARGETS[i % 3], P),
            lambda ch: True)
    return case


@_memo
def gl_encode_case(n, d):
    return _gl_case(vandermonde("gl", n, d + 1), d + 1, 500 * n + d, min_chunks=300)


@_memo
def gl_decode_case(n, d, t):
    C = decode_rows("gl", n, d, t, tuple(range(n)))
    case = _gl_case(C, d + 1, 600 * n + d, reduce_rows=range(t, t + d + 1), min_chunks=300)
    case.n, case.d, case.t = n, d, t
    return case


# ---- the routes of tests/test_gpu_mfma_edges.py: (query of the planner's dump tool, what its answer starts with) ------------------------
# knobs as the dump tools spell them; the GPU test sets the same on its context (KNOB_CALLS there)
K_PAIRS = "mc1,min1,small0,wgs8"       # point pairs from 17 tiles on
K_ROWS = "mc3,min1,small0,wgs8"        # one table row per point
K_TEAM = "mc1,min1,small0"             # the workgroup-per-tile kernel: up to two tiles per workgroup
K_DECODE = "mc2,min1,small0"           # decode rows without the workgroup-per-tile kernel
K_SUB = "mc1,min32"                    # FpMul's four-launch form (tests/test_gpu_wave_edges.py::run_fpmul)
SUB_N = 64                             # elements of the SUB decode case (whole tiles)


def encode_routes():
    out = []
    for n, d in PAIR_SHAPES:
        roles = 2 if (n, d) == (31, 10) else 1
        out.append((("shares", K_PAIRS, "fr", pair_case(n, d).G, n, d, 1), "Bfly M=%d rows=%d roles=%d one" % (d + 1, 4 if n <= 8 else 8, roles)))
    n, d = ROWS_IN_SHAPE
    out.append((("rows", K_PAIRS, "fr", pair_case(n, d).G, n, d, 1), "Bfly M=16 rows=8 roles=1 one"))
    n, d, parties = PARTIES_SHAPE
    out.append((("shares", K_PAIRS, "fr", pair_case(n, d).G, n, d, parties), "BflyParties M=6 rows=8 roles=1 one"))
    n, d, parties = TRIPLE_SHAPE
    out.append((("triple", "default", "fr", triple_case(n, d).G, n, d, parties), "BflyTriple M=6 rows=8 roles=1 one"))
    for n, d in ROW_ENCODE_SHAPES:
        out.append((("shares", K_ROWS, "fr", row_encode_case(n, d).G, n, d, 1), "MfmaRows M=%d " % (d + 1)))
    for n, d, t in TEAM_SHAPES:
        out.append((("shares", K_TEAM, "fr", row_encode_case(n, d).G, n, d, 1), "MfmaRowsTeam M=%d " % (d + 1)))
    n, d, t = GL_SHAPES[0]
    out.append((("shares", K_TEAM, "gl", gl_encode_case(n, d).G, n, d, 1), "MfmaRowsGl M=11"))
    n, d, t = GL_SHAPES[1]                 # d + 1 = 22 is beyond the Goldilocks matrix-core kernel (16): the multi-pass FFT
    out.append((("shares", K_TEAM, "gl", gl_encode_case(n, d).G, n, d, 1), "FftP M=22"))
    return out


def decode_routes():
    out = []
    for n, d, t in TEAM_SHAPES:
        G = decode_case(n, d, t).G + 32
        out.append((("dev", K_TEAM, "fr", G, n, d, t, n, "-"), "MfmaRowsTeam M=%d " % (d + 1)))
        out.append((("p0", K_TEAM, "fr", G, n, d, t, n, "-"), "MfmaRowsTeam M=%d " % (d + 1)))
    for n, d, t in DECODE_SHAPES:
        G = decode_case(n, d, t).G + 32
        # (43, 14, 13): 13 verify rows of 15 488 bytes do not fit one workgroup's LDS and are never split: the lane kernel
        first = "RecoverM M=15" if (n, d, t) == (43, 14, 13) else "MfmaRows M=%d " % (d + 1)
        out.append((("dev", K_DECODE, "fr", G, n, d, t, n, "-"), first))
        out.append((("p0", K_DECODE, "fr", G, n, d, t, n, "-"), first))
    out.append((("interp_deg", K_PAIRS, "fr", inverse_case(DEG_N).G, DEG_N, DEG_N - 1, 0, DEG_N, "-"), "IdftDegrees all=IdftDegrees,Idft,Decode"))
    out.append((("interp", K_PAIRS, "fr", inverse_case(DEG_N).G, DEG_N, DEG_N - 1, 0, DEG_N, "-"), "Idft all=Idft,Decode"))
    n, t = SUB_SHAPE
    out.append((("pair%d" % SUB_N, K_SUB, "fr", 2 * SUB_N, n, t, t, 2 * t + 1, "-"), "MfmaRowsSub M=%d rows=%d roles=1 one" % (t + 1, t + 1)))
    n, d, t = GL_SHAPES[0]
    G = gl_decode_case(n, d, t).G + 32
    out.append((("dev", K_TEAM, "gl", G, n, d, t, n, "-"), "MfmaRowsGl M=11"))
    out.append((("p0", K_TEAM, "gl", G, n, d, t, n, "-"), "MfmaRowsGl M=11"))
    n, d, t = GL_SHAPES[1]                 # d + 1 = 22: beyond the Goldilocks matrix-core kernel
    G = gl_decode_case(n, d, t).G + 32
    out.append((("dev", K_TEAM, "gl", G, n, d, t, n, "-"), "Generic M=22"))
    return out


SUB_K, SUB_M = 250, 7                  # FpMul's k and m at (16, 5) (tests/edge_inputs.py FPMUL_SHAPES)


@_memo
def sub_case(n, t):
    """FpMul inputs over SUB_N elements whose first open subtracts the pairs of SUB_PAIRS: the kernel forms a_p - x_p and b_p - y_p per
    sender as it loads them, so x and the triple's a (y and b) are forced sharings through the pair's two values at t + 1 parties --
    the senders behind the interpolation rows in even elements, the verify-row senders (and sender 0) in odd ones.  z, r_int and the
    bits are those of tests/edge_inputs.py::fpmul_case, so every later step runs on valid sharings."""
    from tests import edge_inputs as E
    senders = tuple(range(2 * t + 1))
    low, ver = E.split_senders(senders, t)
    base = E.fpmul_case(n, t, senders, SUB_K, SUB_M, tile=32)["cols"]
    names = list(SUB_PAIRS)
    cols = []
    for g in range(SUB_N):
        col = dict(base[g % len(base)])
        z = E.mul_sites(E.FR, col, n, t, senders)["z"]
        forced = low if g % 2 == 0 else ver + low[:1]
        for k, (minuend, subtrahend) in enumerate((("ta", "x"), ("tb", "y"))):
            pairs = [SUB_PAIRS[names[(g // 2 + 3 * i + 5 * k) % len(names)]] for i in range(t + 1)]
            col[minuend] = E.forced_sharing(E.FR, n, t, {p: a for p, (a, x) in zip(forced, pairs)})
            col[subtrahend] = E.forced_sharing(E.FR, n, t, {p: x for p, (a, x) in zip(forced, pairs)})
        cols.append(E._mul_finish(E.FR, col, n, t, senders, z))
    ins = E._stack(cols, E.MUL_NAMES + ("rint",))
    ins["rbits"] = [[[c["bits"][j][p] for c in cols] for j in range(SUB_M)] for p in range(n)]
    return {"ins": ins, "cols": cols, "N": SUB_N, "low": low, "ver": ver}
