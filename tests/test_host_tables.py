"""The host-side table builders of the product compiled for the CPU with AddressSanitizer + UBSan and compared value by value with
the big-int oracle, for both fields: mpc-protocols_amd/csrc/tables.hpp + host_fr.hpp (domain elements, Lagrange bases, verify
matrices, inverses: functions of (n, d, t, ids) only), the matrix-core tables, the square root's constants (tables_sqrt.hpp: every
word, and an integer model of kernels_sqrt.hpp run over those words on the chosen discrete logs of tests/sqrt_inputs.py) and the
RISS coefficients (tables_riss.hpp, up to 256 parties and 8128 sets).  Runs without a GPU."""
import itertools
import math
import os
import subprocess

import numpy as np
import pytest

from oracle import spec as SFR
from oracle.spec_gl import S as SGL
from tests import prandbit_ref as PR
from tests import randbit_ref as RB
from tests import sqrt_inputs as SX
from tests import sqrt_model as SM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "host_tables_dump")


@pytest.fixture(scope="module")
def dump():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "cpp"), "host_tables_dump"], stdout=subprocess.DEVNULL)

    def run(field, n, d, t, ids):
        p = subprocess.run([BIN, field, str(n), str(d), str(t), ",".join(map(str, ids))], capture_output=True, text=True,
                           timeout=120)
        assert p.returncode == 0, p.stderr[-2000:]          # ASan / UBSan findings abort with a non-zero code
        out = {}
        for line in p.stdout.splitlines():
            k, _, v = line.partition(" ")
            out.setdefault(k, []).append(v)
        return out
    return run


@pytest.mark.parametrize("field", ["fr", "gl"])
@pytest.mark.parametrize("n,d,t,ids", [(4, 1, 1, [3, 0, 2, 1]), (7, 2, 2, [6, 5, 4, 3, 2]), (16, 5, 5, list(range(16))),
                                       (16, 10, 5, list(range(16))), (31, 10, 10, list(range(30, -1, -1))),
                                       (100, 33, 33, list(range(0, 100)))])
def test_tables_match_oracle(dump, field, n, d, t, ids):
    S = SFR if field == "fr" else SGL
    P = S.R_MOD
    o = dump(field, n, d, t, ids)
    h = lambda xs: [int(x, 16) for x in xs]  # noqa: E731
    assert h(o["omega"]) == [S.domain_omega(n)]
    assert h(o["alpha"]) == [S.domain_element(n, j) for j in range(n)]
    m, needed = d + 1, d + t + 1
    xs = [S.domain_element(n, i) for i in ids[:m]]
    basis = []                                               # coefficients of the Lagrange basis polynomials
    for i in range(m):
        ys = [1 if j == i else 0 for j in range(m)]
        co = S.lagrange_interpolate(xs, ys)
        basis.append(co + [0] * (m - len(co)))
    assert h(o["basis"]) == [basis[i][k] for i in range(m) for k in range(m)]
    want_v = [S.p_eval(basis[i], S.domain_element(n, ids[s])) for s in range(m, needed) for i in range(m)]
    assert h(o.get("verify", [])) == want_v
    assert h(o["inv7"]) == [pow(7, -1, P)] and h(o["pow"]) == [pow(3, 1000003, P)]
    words = [int(w, 16) for w in o["const"][0].split()]
    a1 = S.domain_element(n, 1 if n > 1 else 0)
    if field == "gl":                                         # the value itself, two 32-bit words
        assert words == [a1 & 0xFFFFFFFF, a1 >> 32]
    else:                                                     # nine 29-bit limbs of a1 * 2^261 mod r (fr_u29.hpp)
        v = a1 * pow(2, 261, P) % P
        assert words == [(v >> (29 * i)) & 0x1FFFFFFF for i in range(9)]
    # second-chance tables: for every candidate window W the rows L_i^W(x_s) over the other positions of the OEC
    # prefix, then the coefficient rows of the basis
    S_cnt = len(ids)
    rmax = min(t, S_cnt - needed) if S_cnt > needed else 0
    if rmax < 1:
        assert "second" not in o
        return
    tok = o["second"][0].split()
    Pfx, nw = int(tok[0]), int(tok[1])
    starts = [int(x) for x in tok[2:2 + nw]]
    raw = [int(x, 16) for x in tok[2 + nw:]]
    assert Pfx == needed + rmax
    want_starts = []
    for off in (0, m, Pfx - m, (m + 1) // 2):
        if off + m <= Pfx and off not in want_starts:
            want_starts.append(off)
    assert starts == want_starts
    nl = 2 if field == "gl" else 9
    rinv = 1 if field == "gl" else pow(pow(2, 261, P), -1, P)
    vals = []
    for i in range(0, len(raw), nl):
        limbs = raw[i:i + nl]
        v = (limbs[0] | (limbs[1] << 32)) if field == "gl" else sum(l << (29 * j) for j, l in enumerate(limbs))
        vals.append(v * rinv % P)
    want = []
    for ws in starts:
        wx = [S.domain_element(n, ids[ws + i]) for i in range(m)]
        wb = []
        for i in range(m):
            co = S.lagrange_interpolate(wx, [1 if j == i else 0 for j in range(m)])
            wb.append(co + [0] * (m - len(co)))
        for s in range(Pfx):
            if ws <= s < ws + m:
                continue
            want += [S.p_eval(wb[i], S.domain_element(n, ids[s])) for i in range(m)]
        want += [wb[i][k] for k in range(m) for i in range(m)]
    assert vals == want


def _row_of_digit(b):
    h, reg = b >> 4, b & 15
    return (reg & 3) + 8 * (reg >> 2) + 4 * h


@pytest.mark.parametrize("field", ["fr", "gl"])
@pytest.mark.parametrize("n,d,t,ids", [(4, 1, 1, [3, 0, 2, 1]), (7, 2, 2, [6, 5, 4, 3, 2]), (10, 3, 3, list(range(10))),
                                       (16, 5, 5, list(range(16))), (31, 10, 10, list(range(31)))])
def test_matrix_core_tables(dump, field, n, d, t, ids):
    """the byte-digit tables of the matrix-core kernels: every slab entry is a balanced digit of c * 256^a mod p for the
    coefficient c the oracle computes, and the accumulator bias is 128 * (sum of the row's entries) plus a multiple of p
    (tables_mfma.hpp, tables_mfma_gl.hpp).  Small shapes are checked digit by digit, the others are built under the
    sanitizers."""
    S = SFR if field == "fr" else SGL
    P = S.R_MOD
    o = dump(field, n, d, t, ids)
    m, needed = d + 1, d + t + 1
    assert "mfma_bytes" in o
    if "mfma" not in o:
        return
    raw = b"".join(int(w, 16).to_bytes(4, "little") for w in o["mfma"][0].split())
    sid = ids   # the dump tool takes the ids in the order given (the library sorts before it builds)
    xs = [S.domain_element(n, i) for i in sid[:m]]
    basis = []
    for i in range(m):
        co = S.lagrange_interpolate(xs, [1 if j == i else 0 for j in range(m)])
        basis.append(co + [0] * (m - len(co)))
    rows = [[S.p_eval(basis[i], S.domain_element(n, sid[s])) for i in range(m)] for s in range(m, needed)]
    rows += [[basis[i][k] for i in range(m)] for k in range(m)]
    sb = lambda v: v - 256 if v >= 128 else v   # noqa: E731
    if field == "fr":
        RB = m * 1024 + 128
        assert len(raw) == len(rows) * RB
        for r, row in enumerate(rows):
            tsum = 0
            for i, c in enumerate(row):
                for a in range(32):
                    T = sum(sb(raw[r * RB + i * 1024 + (_row_of_digit(b) + 32 * (a >> 4)) * 16 + (a & 15)]) << (8 * b) for b in range(32))
                    assert T % P == c * pow(256, a, P) % P, (r, i, a)
                    tsum += T
            bias = [int.from_bytes(raw[r * RB + m * 1024 + 4 * b: r * RB + m * 1024 + 4 * b + 4], "little", signed=True) for b in range(32)]
            assert all(0 < v < (1 << 23) for v in bias)
            assert (sum(v << (8 * b) for b, v in enumerate(bias)) - 128 * tsum) % P == 0, r
    else:
        KS = (8 * m + 31) // 32
        TR = KS * 1024 + 128
        assert len(raw) == ((len(rows) + 3) // 4) * TR
        for r, row in enumerate(rows):
            mt, h, el = r // 4, (r % 4) // 2, r % 2
            tsum = 0
            for i, c in enumerate(row):
                for a in range(8):
                    kk = 8 * i + a
                    s_, ha, j = kk // 32, (kk % 32) // 16, kk % 16
                    T = 0
                    for b in range(8):
                        reg = 8 * el + b
                        mrow = (reg & 3) + 8 * (reg >> 2) + 4 * h
                        T += sb(raw[mt * TR + s_ * 1024 + (mrow + 32 * ha) * 16 + j]) << (8 * b)
                    assert T % P == c * pow(256, a, P) % P, (r, i, a)
                    tsum += T
            off = mt * TR + KS * 1024 + (h * 16 + 8 * el) * 4
            bias = [int.from_bytes(raw[off + 4 * b: off + 4 * b + 4], "little", signed=True) for b in range(8)]
            assert all(0 < v < (1 << 23) for v in bias)
            assert (sum(v << (8 * b) for b, v in enumerate(bias)) - 128 * tsum) % P == 0, r


@pytest.mark.parametrize("n,d,t,ids", [(4, 1, 1, [3, 0, 2, 1]), (7, 2, 2, [6, 5, 4, 3, 2]), (13, 4, 4, list(range(13))),
                                       (16, 5, 5, list(range(16))), (16, 14, 0, list(range(16))), (16, 15, 0, list(range(16))), (31, 10, 10, list(range(31)))])
def test_point_pair_tables_of_the_encode(dump, n, d, t, ids):
    """tables_mfma.hpp::build_mfma_bfly_table (kernels_mfma_bfly.hpp): pair p holds the digit slabs of alpha_p^i and two
    accumulator biases.  Checked here with integers: (1) the slabs are balanced digits of alpha_p^i 256^a; (2) bE + bT is a
    bias of output p and bE - bT a bias of output p + size/2 (whose odd coefficients have the opposite sign); (3) for EVERY
    input the two digit sums stay inside [0, 0xff0000) -- the interval the kernel's carry pass assumes -- by taking the
    extreme of every product digit by digit."""
    S, P = SFR, SFR.R_MOD
    o = dump("fr", n, d, t, ids)
    m = d + 1
    assert "bfly_bytes" in o and int(o["bfly_bytes"][0]) > 0, "the builder could not prove the digit-sum bound (m = 16 only)"
    if "bfly" not in o:
        return
    raw = b"".join(int(w, 16).to_bytes(4, "little") for w in o["bfly"][0].split())
    size = 1
    while size < n:
        size <<= 1
    half = size // 2
    PB = m * 1024 + 256
    assert len(raw) == half * PB
    sb = lambda v: v - 256 if v >= 128 else v   # noqa: E731
    for p in range(half):
        alpha = S.domain_element(n, p)
        dig = [[[sb(raw[p * PB + i * 1024 + (_row_of_digit(b) + 32 * (a >> 4)) * 16 + (a & 15)]) for b in range(32)] for a in range(32)]
               for i in range(m)]  # dig[i][a][b]
        tsum = [0, 0]
        for i in range(m):
            for a in range(32):
                T = sum(v << (8 * b) for b, v in enumerate(dig[i][a]))
                assert T % P == pow(alpha, i, P) * pow(256, a, P) % P, (p, i, a)
                tsum[i & 1] += T
        bE = [int.from_bytes(raw[p * PB + m * 1024 + 4 * b: p * PB + m * 1024 + 4 * b + 4], "little", signed=True) for b in range(32)]
        bT = [int.from_bytes(raw[p * PB + m * 1024 + 128 + 4 * b: p * PB + m * 1024 + 132 + 4 * b], "little", signed=True) for b in range(32)]
        val = lambda v: sum(x << (8 * b) for b, x in enumerate(v))   # noqa: E731
        plus = [e + t_ for e, t_ in zip(bE, bT)]
        minus = [e - t_ for e, t_ in zip(bE, bT)]
        assert (val(plus) - 128 * (tsum[0] + tsum[1])) % P == 0, p
        partner = p + half < n
        if partner:
            assert (val(minus) - 128 * (tsum[0] - tsum[1])) % P == 0, p
        else:
            assert all(v == 0 for v in bT)
        # the signed data bytes s are in [-128, 127]: extremes of s * digit, digit by digit
        for b in range(32):
            lo = [0, 0]
            hi = [0, 0]
            for i in range(m):
                for a in range(32):
                    v = dig[i][a][b]
                    lo[i & 1] += min(-128 * v, 127 * v)
                    hi[i & 1] += max(-128 * v, 127 * v)
            assert 0 <= plus[b] + lo[0] + lo[1] and plus[b] + hi[0] + hi[1] < 0xff0000, (p, b)
            if partner:
                assert 0 <= minus[b] + lo[0] - hi[1] and minus[b] + hi[0] - lo[1] < 0xff0000, (p, b)


# ---- the square root's constants (tables_sqrt.hpp) and the RISS coefficients (tables_riss.hpp) -----------------------------------
@pytest.fixture(scope="module")
def tool():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "cpp"), "host_tables_dump"], stdout=subprocess.DEVNULL)

    def run(*args):
        p = subprocess.run([BIN] + [str(a) for a in args], capture_output=True, timeout=120)
        assert p.returncode == 0, p.stderr[-2000:]          # ASan / UBSan findings abort with a non-zero code
        return p.stdout
    return run


_SQRT = {}


def sqrt_table(tool, impl):
    if impl not in _SQRT:
        _SQRT[impl] = SM.parse(tool("sqrt", impl))
    return _SQRT[impl]


SQRT_IMPLS = ["fr-u29", "fr-sat32", "gl"]
FIELD_OF = {"fr-u29": "fr", "fr-sat32": "fr", "gl": "goldilocks"}


@pytest.mark.parametrize("impl", SQRT_IMPLS)
def test_sqrt_table_rebuilt_from_integers(tool, impl):
    lay, words = sqrt_table(tool, impl)
    m = SM.Model(impl, lay, words)
    p, nl = m.p, m.nl
    off = 0
    for name, size in (("negw", 768 * nl), ("posw", 1024 * nl), ("r2", nl), ("one_p", nl), ("half", nl), ("half_p", nl), ("e_sqrt", 8), ("e_inv", 8)):
        assert lay[name] == off, name
        off += size
    assert lay["keyt"] == off and lay["words"] == off + ((1 << lay["kbits"]) + 4) // 4
    om = RB.omega(p)
    omi = pow(om, p - 2, p)
    assert pow(om, 1 << 31, p) == p - 1
    for r in range(4):
        assert m.posw[r] == [pow(om, j << (8 * r), p) for j in range(256)], ("posw", r)
        if r < 3:
            assert m.negw[r] == [pow(omi, j << (8 * r), p) for j in range(256)], ("negw", r)
    inv2 = (p + 1) // 2
    assert m.plain(lay["r2"]) == m.R * m.R % p and m.plain(lay["one_p"]) == 1 and m.half == inv2 and m.half_p == inv2
    assert m.e_sqrt == (p - 1) >> 33 == (RB.trace(p) - 1) // 2 and lay["bits_sqrt"] == m.e_sqrt.bit_length()
    assert m.e_inv == p - 2 and lay["bits_inv"] == (p - 2).bit_length()
    # the key slice: the smallest kbits, then the lowest kshift, at which the 256 subgroup elements have distinct keys
    zeta = pow(om, 1 << 24, p)
    sub = [pow(zeta, j, p) for j in range(256)]
    low = []
    for z in sub:
        l = m.to_limbs(z * m.R % p)
        low.append(((l[1] << 32) | l[0]) * SM.KEY_MUL & SM.M64)
    best = next((kb, sh) for kb in range(8, 21) for sh in range(0, 65 - kb) if len({(w >> sh) & ((1 << kb) - 1) for w in low}) == 256)
    assert (lay["kbits"], lay["kshift"]) == best
    assert impl == "fr-sat32" or best == {"fr-u29": (12, 9), "gl": (14, 47)}[impl]
    keys = [m.key_index(z) for z in sub]
    assert len(set(keys)) == 256 and [m.keyt[k] for k in keys] == list(range(256))
    assert len(m.keyt) == ((1 << lay["kbits"]) + 4) // 4 * 4 and sum(1 for b in m.keyt if b) == 255      # every other entry is 0


def _sweep(m, fam, powers):
    """the model over the family -> the sorted L of the values on which it differs from the restatement in L, root, has_root or s"""
    p = m.p
    bad = set()
    for (A, L, (root, ks)), pw in zip(fam, powers):
        if A == 0:
            ok = m.sqrt(0) == (None, 0, 1)
        else:
            want = (L, root or 0, int(root is not None))
            ok = m.sqrt(A, pw) == want
            s = m.finalize_s(A, pw)
            ok = ok and s == (None if root is None else pow(2 * root, p - 2, p))
        if not ok:
            bad.add(L)
    return bad


@pytest.mark.parametrize("impl", SQRT_IMPLS)
def test_sqrt_model_over_the_chosen_logs(tool, impl):
    """the integer model of sqrt_core, k_sqrt and k_randbit_finalize over the dumped words, on every family value: its L is log_of(A)
    (tests/test_sqrt_inputs.py checks the family's logs against log_of), its root ark's, its s = (2b)^-1; and three wrong copies of the
    model each fail the sweep, on the values named"""
    lay, words = sqrt_table(tool, impl)
    m = SM.Model(impl, lay, words)
    p = m.p
    fam = list(zip(SX.family_values(p), SX.family_logs(p), SX.family_roots(p)))
    powers = [m.powers(A) if A else None for A, _, _ in fam]
    assert _sweep(m, fam, powers) == set()
    for x in (1, 2, p - 1, SX.family_values(p)[5]):                  # k_inverse's exponent and bit count
        assert m.inverse(x) == pow(x, p - 2, p)
    evens = {L for _, L, _ in fam if L is not None and not L & 1}
    logs = {L for _, L, _ in fam if L is not None}
    # (a) window 1 without window 0's correction: its look-up then misses the subgroup and mostly lands on an empty entry, which reads 0 --
    # a single byte in window 0 (L = 2) goes unnoticed, the members with windows 0 AND 1 not zero are what fail
    bad = _sweep(SM.Model(impl, lay, words, bug="no_correction"), fam, powers)
    assert {0xFFFFFFFE, 0xFFFFFFFF, 0xAAAAAAAA, 0x55555554, 0x1FF, 0x5AFF, 0xFFFF} <= bad and not {0, 0x100, 2**31, 0xFF00} & bad
    assert bad <= {L for L in logs if L & 255}
    # (b) E masked with 2^32 - 1: omega^(2^31) = -1 joins the root and s of every even L but 0
    bad = _sweep(SM.Model(impl, lay, words, bug="wide_mask"), fam, powers)
    assert bad == evens - {0} and {2, 2**31, 2**32 - 2} <= bad
    # (c) negw rows 0 and 1 exchanged: windows 2 and 3 are looked up off the subgroup; again it takes a lower window that is not zero
    # UNDER an upper window that is not zero (the family's "under" members) to notice
    bad = _sweep(SM.Model(impl, lay, words, bug="swapped_rows"), fam, powers)
    assert {0xFFFFFFFE, 0xFFFFFFFF, 0xAAAAAAAA, 0x55555554, 0x1FFFF, 0x80FFFFFF, 0x5AFFFF} <= bad and not {0, 0x10000, 2**31, 0xFF000000} & bad
    assert bad <= {L for L in logs if L & 0xFFFF}


RISS_ALL = [(4, 1), (7, 2), (16, 5), (17, 5), (22, 4), (37, 3), (128, 2), (255, 1), (256, 1), (5, 0)]
RISS_OWN = [(7, 2, 0), (7, 2, 6), (7, 2, 3), (128, 2, 0), (128, 2, 127), (128, 2, 64)]


def _riss(tool, field, n, t, own):
    raw = tool("riss", field, n, t, own)
    head, _, body = raw.partition(b"\n")
    tok = head.split()
    assert tok[0] == b"riss"
    coef, red, coef2, nwords, Tn, ncols, has2 = map(int, tok[1:])
    assert len(body) == 4 * nwords
    return dict(coef=coef, red=red, coef2=coef2, words=nwords, Tn=Tn, ncols=ncols, has2=has2), np.frombuffer(body, dtype="<u4")


def _riss_check(tool, field, n, t, own):
    p = PR.P_GL if field == "gl" else PR.P_FR
    nc = 2 if field == "gl" else 8
    lay, w = _riss(tool, field, n, t, own)
    sets = PR.tsets(n, t) if own < 0 else PR.own_tsets(n, t, own)
    cols = list(range(n)) if own < 0 else [own]
    Tn, ncols = len(sets), len(cols)
    assert (lay["Tn"], lay["ncols"], lay["has2"]) == (Tn, ncols, int(n <= 255)) and Tn <= PR.MAX_TSETS
    assert Tn == (math.comb(n, t) if own < 0 else math.comb(n - 1, t))
    nred = 0 if field == "gl" else 2 * (9 if field == "fr" else 8)
    assert (lay["coef"], lay["red"], lay["coef2"]) == (0, Tn * ncols * nc, Tn * ncols * nc + nred)
    assert lay["words"] == lay["coef2"] + (Tn * ncols if n <= 255 else 0)
    coef = w[:lay["red"]].reshape(Tn, ncols, nc)
    c2 = w[lay["coef2"]:].reshape(Tn, ncols) if n <= 255 else None
    # a coefficient is zero exactly when the party is in the set: the whole table
    member = np.zeros((Tn, ncols), dtype=bool)
    for k, T in enumerate(sets):
        for mth in T:
            if own < 0:
                member[k, mth] = True
    assert np.array_equal(~coef.any(axis=2), member)
    if c2 is not None:
        assert np.array_equal(c2 == 0, member) and int(c2.max()) < 256
    val = lambda k, q: sum(int(x) << (32 * i) for i, x in enumerate(coef[k, q]))   # noqa: E731
    # all sets for a sample of columns (0, 1, n - 1 and the highest party below 255 always), all columns for a sample of sets
    rng = np.random.default_rng(n * 100 + t)
    qs = sorted({0, min(1, ncols - 1), ncols - 1, min(ncols - 1, 254)} | set(rng.choice(ncols, min(ncols, 3), replace=False).tolist()))
    ks = sorted({0, Tn - 1} | set(rng.choice(Tn, min(Tn, 24), replace=False).tolist()))
    pairs = {(k, q) for k in range(Tn) for q in qs} | {(k, q) for k in ks for q in range(ncols)}
    for k, q in sorted(pairs):
        j = cols[q]
        assert val(k, q) == PR.f_prime(p, n, sets[k], j), (k, j)
        if c2 is not None:
            assert int(c2[k, q]) == PR.f_gf(sets[k], j), (k, j)
    # the two reduction constants: 1 and 2^224 in the implementation's constant form
    if field != "gl":
        nl, lb, rb = (9, 29, 261) if field == "fr" else (8, 32, 256)
        red = [int(x) for x in w[lay["red"]:lay["coef2"]]]
        dec = lambda ws: sum(x << (lb * i) for i, x in enumerate(ws))   # noqa: E731
        assert all(x < 1 << lb for x in red)
        assert dec(red[:nl]) == pow(2, rb, p) and dec(red[nl:]) == pow(2, rb + 224, p)
    return lay, coef, c2


@pytest.mark.parametrize("field", ["fr", "gl"])
@pytest.mark.parametrize("n,t", RISS_ALL)
def test_riss_coefficients_every_set(tool, field, n, t):
    lay, coef, c2 = _riss_check(tool, field, n, t, -1)
    if (n, t) == (5, 0):                                              # the single empty set: coefficient 1 for every party
        assert lay["Tn"] == 1 and [int(x) for x in coef[0, :, 0]] == [1] * 5 and not coef[0, :, 1:].any() and [int(x) for x in c2[0]] == [1] * 5
    if n == 256:
        assert c2 is None


@pytest.mark.parametrize("n,t,own", RISS_OWN)
def test_riss_coefficients_one_party(tool, n, t, own):
    for field in ("fr", "fr-sat32", "gl"):
        lay, coef, c2 = _riss_check(tool, field, n, t, own)
        assert coef.any(axis=2).all() and (c2 != 0).all()             # the party's own sets: no coefficient is zero
