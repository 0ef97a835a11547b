"""An integer model of the matrix-core kernels' host tables and register epilogues.  Plain Python and numpy: no library, no GPU.

  tables     the byte-digit tables of csrc/tables_mfma.hpp (plain rows: build_mfma_table; point pairs with bE, bT and the parity
             adjustment: build_mfma_bfly_table) and csrc/tables_mfma_gl.hpp, from a coefficient matrix of Python integers, in the
             product's byte layout -- tests/test_mfma_inputs.py compares them byte for byte with tests/cpp/host_tables_dump
  digit sums what the accumulators of a lane pair hold after the MFMAs of one row: L[b] = bias[b] + sum (byte - 128) * digit, and for
             a pair row E, T, E + T and E - T
  epilogues  csrc/kernels_mfma.hpp gather / gather_pairs, add_q_nr, reduce_words, verify_tile, sub_mod_r and
             csrc/kernels_mfma_gl.hpp gl_finish replayed line by line on 32-bit and 64-bit words, each returning what it computed
             AND the branches it took (the quotient estimate, fast or slow path, the number of subtractions, what crossed from the low
             lane half to the high one)

Every replay returns the value the kernel would store; the model's own test asserts that it equals the big-int dot product, so that a
wrong model fails on the CPU, not on the GPU.
"""
import numpy as np

from oracle import spec as SFR
from oracle.spec_gl import S as SGL

R = SFR.R_MOD
P = SGL.R_MOD
M32, M64 = (1 << 32) - 1, (1 << 64) - 1
R_W = [(R >> (32 * j)) & M32 for j in range(8)]
NR_W = [(((1 << 256) - R) >> (32 * j)) & M32 for j in range(8)]
R_TOP = R >> 224                       # 0x73eda753
Q_RECIP = (1 << 62) // (R_TOP + 1)     # 0x8d54253a
LIMIT = 0xff0000                       # every Fr digit sum must lie in [0, LIMIT)
LIMIT_GL = 1 << 23
RADIX = 1 << 261                       # the Montgomery radix of fr_u29.hpp (the TRIPLE instance's table rows carry it)
SLOW_ITERATIONS = 5                    # reduce_words: conditional subtractions on the slow path
assert R_TOP == 0x73eda753 and Q_RECIP == 0x8d54253a


def row_of_digit(b):
    h, reg = b >> 4, b & 15
    return (reg & 3) + 8 * (reg >> 2) + 4 * h


def balanced(x, nd):
    """the nd balanced base-256 digits of x (each in [-128, 127]): the bytes of x + 0x80..80, each minus 128"""
    y = x + sum(0x80 << (8 * b) for b in range(nd))
    return [((y >> (8 * b)) & 0xff) - 128 for b in range(nd)]


def bias_mag(m):
    return 32 * m * 16384


# ---- Fr tables ---------------------------------------------------------------------------------------------------------------------
class Row:
    """one plain table row: dig[32 m][32] (data byte k = 32 i + a, result digit b) and bias[32]"""

    def __init__(self, coeffs):
        m = len(coeffs)
        self.m = m
        dig, tsum = [], 0
        for c in coeffs:
            c %= R
            for a in range(32):
                tsum += c
                dig.append(balanced(c, 32))
                c = c * 256 % R
        self.dig = np.array(dig, dtype=np.int64)
        e = bias_mag(m) * sum(256 ** b for b in range(32)) % R
        cr = 128 * tsum % R
        self.bias = [bias_mag(m) - ((e >> (8 * b)) & 0xff) + ((cr >> (8 * b)) & 0xff) for b in range(32)]

    def slab_bytes(self):
        out = bytearray(self.m * 1024)
        for k in range(32 * self.m):
            i, a = divmod(k, 32)
            for b in range(32):
                out[i * 1024 + (row_of_digit(b) + 32 * (a >> 4)) * 16 + (a & 15)] = int(self.dig[k][b]) & 0xff
        return bytes(out)

    def bytes(self):
        return self.slab_bytes() + b"".join(int(v).to_bytes(4, "little", signed=True) for v in self.bias)

    def sums(self, X):
        """digit sums of the chunks X[G][32 m] (raw data bytes, uint8): int64 [G][32]"""
        return (X.astype(np.int64) - 128) @ self.dig + np.array(self.bias, dtype=np.int64)

    def extremes(self):
        """per digit, over ALL byte strings: (lo[32], hi[32])"""
        neg, pos = np.minimum(self.dig, 0).sum(0), np.maximum(self.dig, 0).sum(0)
        b = np.array(self.bias, dtype=np.int64)
        return b + 127 * neg - 128 * pos, b - 128 * neg + 127 * pos


def plain_table(C):
    """build_mfma_table: one Row per coefficient row"""
    return [Row(c) for c in C]


def plain_table_bytes(C):
    return b"".join(r.bytes() for r in plain_table(C))


class PairRow:
    """pair p of build_mfma_bfly_table: the digits of row p, bE and bT; .partner: the output p + half exists"""

    def __init__(self, row, partner_row):
        self.m, self.dig, self.partner = row.m, row.dig, partner_row is not None
        b1 = list(row.bias)
        if partner_row is None:
            self.bE, self.bT, self.b2 = b1, [0] * 32, b1
        else:
            b2 = list(partner_row.bias)
            if (b1[0] ^ b2[0]) & 1:
                b2 = [v + ((R >> (8 * b)) & 0xff) for b, v in enumerate(b2)]
            for b in range(1, 32):
                if (b1[b] ^ b2[b]) & 1:
                    b2[b] += 1
                    b2[b - 1] -= 256
            assert all((x + y) % 2 == 0 for x, y in zip(b1, b2))
            self.bE = [(x + y) // 2 for x, y in zip(b1, b2)]
            self.bT = [(x - y) // 2 for x, y in zip(b1, b2)]   # C++ '/' truncates; exact here, the sum is even
            self.b2 = b2
        odd = np.array([(k // 32) & 1 for k in range(32 * self.m)], dtype=bool)
        self.dig_even, self.dig_odd = np.where(odd[:, None], 0, self.dig), np.where(odd[:, None], self.dig, 0)
        self.row = row

    def bytes(self):
        return self.row.slab_bytes() + b"".join(int(v).to_bytes(4, "little", signed=True) for v in self.bE + self.bT)

    def sums(self, X):
        """E, T (the two accumulators), E + T and E - T: int64 [G][32] each"""
        s = X.astype(np.int64) - 128
        E = s @ self.dig_even + np.array(self.bE, dtype=np.int64)
        T = s @ self.dig_odd + np.array(self.bT, dtype=np.int64)
        return E, T, E + T, E - T

    def extremes(self):
        """per digit over all byte strings: (plus_lo, plus_hi, minus_lo, minus_hi), as the builder proves them"""
        lo = [127 * np.minimum(d, 0).sum(0) - 128 * np.maximum(d, 0).sum(0) for d in (self.dig_even, self.dig_odd)]
        hi = [-128 * np.minimum(d, 0).sum(0) + 127 * np.maximum(d, 0).sum(0) for d in (self.dig_even, self.dig_odd)]
        b1, b2 = np.array(self.row.bias, dtype=np.int64), np.array(self.b2, dtype=np.int64)
        return b1 + lo[0] + lo[1], b1 + hi[0] + hi[1], b2 + lo[0] - hi[1], b2 + hi[0] - lo[1]

    def bound_holds(self):
        pl, ph, ml, mh = self.extremes()
        return bool((pl >= 0).all() and (ph < LIMIT).all() and (not self.partner or ((ml >= 0).all() and (mh < LIMIT).all())))


def pair_table(C, half):
    """build_mfma_bfly_table(C, m, half): the PairRows, or None where the builder returns an empty table"""
    rows = plain_table(C)
    n = len(C)
    out = [PairRow(rows[p], rows[p + half] if p + half < n else None) for p in range(min(half, n))]
    return out if all(p.bound_holds() for p in out) else None


def pair_table_bytes(C, half):
    t = pair_table(C, half)
    return b"" if t is None else b"".join(p.bytes() for p in t)


# ---- Goldilocks table --------------------------------------------------------------------------------------------------------------
class RowGl:
    """one row of build_mfma_table_gl: dig[8 m][8] (data byte k = 8 i + a) and bias[8]"""

    def __init__(self, coeffs):
        m = len(coeffs)
        self.m = m
        dig, tsum = [], 0
        for c in coeffs:
            c %= P
            for a in range(8):
                tsum += c
                dig.append(balanced(c if c <= 0x7f7f7f7f7f7f7f7f else c - P, 8))
                c = c * 256 % P
        self.dig = np.array(dig, dtype=np.int64)
        bmag = 8 * m * 16384
        e = sum(256 ** b for b in range(8)) % P * bmag % P
        cr = tsum % P * 128 % P
        self.bias = [bmag - ((e >> (8 * b)) & 0xff) + ((cr >> (8 * b)) & 0xff) for b in range(8)]

    def sums(self, X):
        return (X.astype(np.int64) - 128) @ self.dig + np.array(self.bias, dtype=np.int64)

    def extremes(self):
        neg, pos = np.minimum(self.dig, 0).sum(0), np.maximum(self.dig, 0).sum(0)
        b = np.array(self.bias, dtype=np.int64)
        return b + 127 * neg - 128 * pos, b - 128 * neg + 127 * pos


def gl_table(C):
    return [RowGl(c) for c in C]


def gl_table_bytes(C):
    rows = gl_table(C)
    m = rows[0].m
    KS = (8 * m + 31) // 32
    TR = KS * 1024 + 128
    out = bytearray(((len(rows) + 3) // 4) * TR)
    for r, row in enumerate(rows):
        mt, h, el = r // 4, (r % 4) // 2, r % 2
        for kk in range(8 * m):
            s, ha, j = kk // 32, (kk % 32) // 16, kk % 16
            for b in range(8):
                reg = 8 * el + b
                mrow = (reg & 3) + 8 * (reg >> 2) + 4 * h
                out[mt * TR + s * 1024 + (mrow + 32 * ha) * 16 + j] = int(row.dig[kk][b]) & 0xff
        for b in range(8):
            off = mt * TR + KS * 1024 + (h * 16 + 8 * el + b) * 4
            out[off:off + 4] = int(row.bias[b]).to_bytes(4, "little", signed=True)
    return bytes(out)


# ---- inputs as bytes ---------------------------------------------------------------------------------------------------------------
def chunk_bytes(values, width=32):
    """chunks [G][m] of integers -> uint8 [G][width m] (little-endian elements, as the kernels read them)"""
    raw = b"".join(int(v).to_bytes(width, "little") for ch in values for v in ch)
    return np.frombuffer(raw, dtype=np.uint8).reshape(len(values), -1)


def dot(coeffs, values, mod):
    return sum(c * v for c, v in zip(coeffs, values)) % mod


# ---- the Fr epilogue ---------------------------------------------------------------------------------------------------------------
def gather_pairs(acc):
    """kernels_mfma.hpp gather_pairs on one lane half's 16 accumulator registers (int32 -> uint32 arithmetic)"""
    return [(((acc[2 * j + 1] & M32) << 8) + (acc[2 * j] & M32)) & M32 for j in range(8)]


def words_from_pairs(p):
    """T[j] = p[2 j + 1] * 2^16 + p[2 j]: the un-normalised 64-bit words of a lane half"""
    return [(p[2 * j + 1] * 65536 + p[2 * j]) & M64 for j in range(4)]


def halves(L, combine=None):
    """the two lane halves' T[4] from 32 digit sums (one accumulator), or from two accumulators added / subtracted at the pair level
    as kernels_mfma_bfly.hpp does (combine = (E, T, sign))"""
    out = []
    for h in range(2):
        if combine is None:
            p = gather_pairs([int(v) for v in L[16 * h:16 * h + 16]])
        else:
            E, T, sign = combine
            pe, pt = gather_pairs([int(v) for v in E[16 * h:16 * h + 16]]), gather_pairs([int(v) for v in T[16 * h:16 * h + 16]])
            p = [(x + sign * y) & M32 for x, y in zip(pe, pt)]
        out.append(words_from_pairs(p))
    return out


def add_q_nr(q, Th):
    """U = S + q (2^256 - r) over both halves.  Returns (U_lo[4], U_hi[4], top_hi, cin): the high half's `top` (everything above
    2^256) and what the low half handed over"""
    res = []
    cin = 0
    for h in range(2):
        nr = NR_W[4 * h:4 * h + 4]
        Q = [(q * nr[j] + Th[h][j]) & M64 for j in range(4)]
        U = [Q[0] & M32]
        c = 0
        for j in range(1, 4):
            v = (Q[j] & M32) + (Q[j - 1] >> 32) + c
            U.append(v & M32)
            c = v >> 32
        top = ((Q[3] >> 32) + c) & M32
        if h == 1:
            c = cin
            for j in range(4):
                v = U[j] + c
                U[j] = v & M32
                c = v >> 32
            top = (top + c) & M32
        else:
            cin = top
        res.append((U, top))
    return res[0][0], res[1][0], res[1][1], cin


def quotient_estimate(Th):
    xq = (Th[1][3] >> 17) & M32
    return ((xq * Q_RECIP) >> 32) >> 13


def reduce_words(Th):
    """kernels_mfma.hpp reduce_words on the two halves' T.  Returns a dict: value (what the kernel stores, as an integer), q (the
    quotient estimate), fast, k (subtractions the five iterations took), k_needed (subtractions a loop WITHOUT a bound would take:
    equal to k unless the kernel is wrong for this input), top_is_rtop (the top word after S - q r equals r's), cin (the low half's
    carry words into the high half), borrows (per slow iteration: the borrow the low half handed up)"""
    q = quotient_estimate(Th)
    lo, hi, top, cin = add_q_nr(q, Th)
    fast = top == q and hi[3] < R_TOP
    out = {"q": q, "fast": fast, "k": 0, "cin": cin, "borrows": [], "top_is_rtop": hi[3] == R_TOP, "e": (top - q) & M32}
    val = sum(w << (32 * j) for j, w in enumerate(lo + hi))
    full = val + (((top - q) & M32) << 256)
    out["k_needed"] = full // R
    if not fast:
        e = (top - q) & M32
        Rw = [lo, hi]
        for _ in range(SLOW_ITERATIONS):
            D, b = [[], []], [0, 0]
            for h in range(2):
                for j in range(4):
                    d = (Rw[h][j] - R_W[4 * h + j] - b[h]) & M64
                    D[h].append(d & M32)
                    b[h] = (d >> 32) & 1
            d = (D[1][0] - b[0]) & M64                     # the high half takes the low half's borrow in
            D[1][0] = d & M32
            for j in range(1, 4):
                d = (D[1][j] - ((d >> 32) & 1)) & M64
                D[1][j] = d & M32
            bout = b[1] + ((d >> 32) & 1)
            out["borrows"].append(b[0])
            if e >= bout:
                Rw = D
                e = (e - bout) & M32
                out["k"] += 1
        lo, hi = Rw
        val = sum(w << (32 * j) for j, w in enumerate(lo + hi))
    out["value"] = val
    return out


def verify_tile(Th, y):
    """kernels_mfma.hpp verify_tile against the claimed canonical value y.  Returns a dict: bad, q, top_eq_q, words_equal"""
    yw = [(y >> (32 * j)) & M32 for j in range(8)]
    q = ((Th[0][0] & M32) - yw[0]) & M32
    lo, hi, top, cin = add_q_nr(q, Th)
    words_equal = lo + hi == yw
    return {"bad": not words_equal or top != q, "q": q, "top_eq_q": top == q, "words_equal": words_equal, "cin": cin}


def sub_mod_r(a, x):
    """kernels_mfma.hpp sub_mod_r on two canonical values.  Returns (value, info): b_lo (the low 128 bits borrow), b_hi (the high half
    borrows on its own words), b2 (the high half borrows only through the low half's borrow), neg, c (the low half's '+ r' carries)"""
    aw, xw = [(a >> (32 * j)) & M32 for j in range(8)], [(x >> (32 * j)) & M32 for j in range(8)]
    d, e, bw, cw = [[], []], [[], []], [0, 0], [0, 0]
    for h in range(2):
        b = 0
        for j in range(4):
            v = aw[4 * h + j] - xw[4 * h + j] - b
            d[h].append(v & M32)
            b = 1 if v < 0 else 0
        bw[h] = b
        c = 0
        for j in range(4):
            v = d[h][j] + R_W[4 * h + j] + c
            e[h].append(v & M32)
            c = v >> 32
        cw[h] = c
    f, bb = [], bw[0]
    for j in range(4):
        v = d[1][j] - bb
        f.append(v & M32)
        bb = 1 if v < 0 else 0
    b2 = bb
    neg = (bw[1] | b2) != 0
    g, cc = [], cw[0]
    for j in range(4):
        v = f[j] + R_W[4 + j] + cc
        g.append(v & M32)
        cc = v >> 32
    words = (e[0] + g) if neg else (d[0] + f)
    return sum(w << (32 * j) for j, w in enumerate(words)), {"b_lo": bw[0], "b_hi": bw[1], "b2": b2, "neg": neg, "c": cw[0]}


# ---- the Goldilocks epilogue -------------------------------------------------------------------------------------------------------
def gl_finish(L):
    """kernels_mfma_gl.hpp gl_finish on the 8 digit sums of one element.  Returns a dict: value, w2, wrap, ge_p"""
    acc = [int(v) & M32 for v in L]
    p = [((acc[2 * j + 1] << 8) + acc[2 * j]) & M32 for j in range(4)]
    lo, hi = (p[1] * 65536 + p[0]) & M64, (p[3] * 65536 + p[2]) & M64
    w0 = lo & M32
    v = (lo >> 32) + (hi & M32)
    w1, cy = v & M32, v >> 32
    w2 = ((hi >> 32) + cy) & M32
    x = (w1 << 32) | w0
    t1 = ((w2 << 32) - w2) & M64
    r = (x + t1) & M64
    wrap = r < x
    if wrap:
        r = (r + 0xffffffff) & M64
    ge_p = r >= P
    return {"value": r - P if ge_p else r, "w2": w2, "wrap": wrap, "ge_p": ge_p}
