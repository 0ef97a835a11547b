"""Deterministic adversarial inputs for the wave-per-element kernels (Mul, TruncPr / FPDivConst, FpMul, triple generation).

Uniform field elements never reach the bounds the unsaturated radix-2^29 arithmetic (csrc/fr_u29.hpp) rests on: the subtracting
branch of canon_loose needs a value within 2^232 of a multiple of r (probability ~2^-21), the 64-bit columns only fill up when
every limb of every term is all ones.  Here every input is built from a short list of edge values, with plain Python integers and
oracle/ alone (no library, no GPU), in three constructions that all give VALID sharings, so that the opens succeed and every
later step runs on the values chosen:

  constant sharings      degree 0, every party holds the same value: all t + 1 terms of every table row add constructively
  forced sharings        the degree-t polynomial through chosen edge values at t + 1 chosen parties (the verify-row senders, a
                         non-sender, party n - 1), shares by the oracle's compute_shares
  targeted intermediates inputs solved so that a named intermediate (d, e, the products, z, r', the opened share, ...) IS a chosen
                         edge value

and single-bit tampering: a sender's share with one clear bit set.

SITE_TABLE names, per kernel family, the intermediates and the value classes each must take for at least one (party, element)
of the generated inputs; *_sites() compute those intermediates as integers from the inputs alone and tests/test_edge_inputs.py
enforces the table, so the GPU tests (tests/test_gpu_wave_edges.py) cannot silently miss their target.
"""
import numpy as np

from oracle import cref as O
from oracle import cref_gl as OG
from oracle import spec as S
from oracle import spec_gl

R = S.R_MOD
P = OG.P
B = 0x73EDA7 << 232                               # r's top limb with nothing below it: from here up the top limb reaches r's
MAXLIMB = (0x73EDA6 << 232) | ((1 << 232) - 1)    # canonical, every 29-bit limb below the top one is all ones
EDGE = (0, 1, 2, (1 << 232) - 1, 1 << 232, 1 << 233, B - 1, B, B + 5, R - (1 << 232), R - 2, R - 1, MAXLIMB, (R - 1) // 2, (R + 1) // 2)
EDGE_GL = (0, 1, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, 1 << 63, P - (1 << 32), P - 2, P - 1)
TAMPER_BITS = (0, 28, 29, 57, 58, 231, 232, 253)
W_VALUES = (0, 1, R - 1, MAXLIMB, (1 << 128) - 1)  # FPDivConst's public multipliers


class Fld:
    """a field: its modulus, edge values, C oracle and Python spec; arrays <-> nested lists of ints"""

    def __init__(self, name, mod, edge, cref, spec, tail):
        self.name, self.mod, self.edge, self.O, self.S, self.tail = name, mod, edge, cref, spec, tail
        self.sums = (mod - 1, mod, mod + 1, 2 * mod - 2)   # e + y_p as an integer, before any reduction

    def inv(self, a):
        return pow(a % self.mod, self.mod - 2, self.mod)

    def arr(self, vals):
        a = np.array(vals, dtype=object)
        if not self.tail:
            return a.astype(np.uint64)
        raw = b"".join(int(v).to_bytes(32, "little") for v in a.reshape(-1))
        return np.frombuffer(raw, dtype=np.uint64).reshape(a.shape + (4,)).copy()

    def ints(self, arr):
        arr = np.asarray(arr, dtype=np.uint64)
        if not self.tail:
            return arr.astype(object).tolist()
        raw = np.ascontiguousarray(arr).tobytes()
        flat = [int.from_bytes(raw[i:i + 32], "little") for i in range(0, len(raw), 32)]
        return np.array(flat, dtype=object).reshape(arr.shape[:-1]).tolist()


FR = Fld("fr", R, EDGE, O, S, (4,))
GL = Fld("goldilocks", P, EDGE_GL, OG, spec_gl.S, ())
_cache = {}


def _memo(fn):
    def wrapped(*key):
        k = (fn.__name__,) + key
        if k not in _cache:
            _cache[k] = fn(*key)
        return _cache[k]
    return wrapped


def split_senders(senders, t):
    """the sorted sender set as the decode uses it: the lowest t + 1 back the P(0) row, the upper t a verify row each"""
    srt = sorted(senders)
    return srt[:t + 1], srt[t + 1:]


def forced_parties(n, t, senders, count=None):
    """the parties whose shares a forced sharing fixes: the verify-row senders, a non-sender (party n - 1 where it is one; it is
    a verify-row sender otherwise), then the lowest senders up to `count` (t + 1 by default)"""
    low, ver = split_senders(senders, t)
    non = [p for p in range(n) if p not in senders]
    out = list(ver) + ([n - 1] if n - 1 in non else non[-1:])
    out += [p for p in low if p not in out][:(count or t + 1) - len(out)]
    assert n - 1 in out and len(out) == (count or t + 1)
    return out


@_memo
def p0_weights(F, n, parties):
    """Lagrange weights of P(0) through the domain points of `parties`"""
    xs = [F.S.domain_element(n, p) for p in parties]
    out = []
    for i, xi in enumerate(xs):
        num = den = 1
        for j, xj in enumerate(xs):
            if j != i:
                num, den = num * -xj % F.mod, den * (xi - xj) % F.mod
        out.append(num * F.inv(den) % F.mod)
    return out


def p0(F, n, parties, shares):
    return sum(w * shares[p] for w, p in zip(p0_weights(F, n, tuple(parties)), parties)) % F.mod


@_memo
def lagrange_basis(F, n, parties):
    """the Lagrange basis polynomials over the domain points of `parties` (-1: the point 0), by the spec's lagrange_interpolate"""
    xs = [0 if p < 0 else F.S.domain_element(n, p) for p in parties]
    return [F.S.lagrange_interpolate(xs, [int(i == j) for i in range(len(xs))]) for j in range(len(xs))]


def forced_sharing(F, n, deg, forced):
    """the n shares of the polynomial of degree <= deg through {party: value} (deg + 1 parties; the key -1 fixes P(0)): Lagrange
    over the domain points for the coefficients, the oracle's compute_shares for the shares; the forced parties hold exactly the
    chosen values"""
    assert len(forced) == deg + 1
    poly = [0] * (deg + 1)
    for v, basis in zip(forced.values(), lagrange_basis(F, n, tuple(forced))):
        for i, c in enumerate(basis):
            poly[i] = (poly[i] + v * c) % F.mod
    rc, sh = F.O.compute_shares(F.arr([poly]), n, deg)
    assert rc == 0
    shares = [row[0] for row in F.ints(sh)]
    assert all(shares[p] == v % F.mod for p, v in forced.items() if p >= 0)
    assert -1 not in forced or poly[0] == forced[-1] % F.mod
    return shares


def pick(F, i):
    return F.edge[i % len(F.edge)]


def tamper_value(bit):
    """(base, base | 1 << bit): a canonical value with that bit clear whose tampered form is still below r, all-ones limbs where
    that is possible"""
    for base in (MAXLIMB & ~(1 << bit), (R - 1) & ~(1 << bit), 0):
        if not base >> bit & 1 and base | 1 << bit < R:
            return base, base | 1 << bit
    raise AssertionError(bit)


def _other_forced(n, t, senders, sender):
    """t more parties to force next to `sender`"""
    seen = []
    for p in forced_parties(n, t, senders) + sorted(senders):
        if p != sender and p not in seen:
            seen.append(p)
    return seen[:t]


def _stack(cols, names):
    """columns (name -> per-party values) to name -> [party][element]"""
    return {nm: [list(v) for v in zip(*[c[nm] for c in cols])] for nm in names}


# ---- Mul: x, y and the triple (ta, tb, tc) ---------------------------------------------------------------------------------------
MUL_NAMES = ("x", "y", "ta", "tb", "tc")


def mul_sites(F, col, n, t, senders):
    """the intermediates of Multiply for one element, from its inputs alone"""
    q = F.mod
    low, ver = split_senders(senders, t)
    dsh = [(a - x) % q for a, x in zip(col["ta"], col["x"])]
    esh = [(b - y) % q for b, y in zip(col["tb"], col["y"])]
    d, e = p0(F, n, low, dsh), p0(F, n, low, esh)
    p1 = [(e + y) * d % q for y in col["y"]]
    p2 = [x * e % q for x in col["x"]]
    return {"open_share": [dsh[p] for p in low + ver] + [esh[p] for p in low + ver], "verify_row": [dsh[p] for p in ver] + [esh[p] for p in ver],
            "d": [d], "e": [e], "e_plus_y": [e + y for y in col["y"]], "prod_ey_d": p1, "prod_x_e": p2,
            "z": [(c - a - b) % q for c, a, b in zip(col["tc"], p1, p2)]}


def _mul_finish(F, col, n, t, senders, z):
    """tc so that every party's z_p is z[p] (a valid sharing whenever z is one: (e + y_p) d + x_p e has degree t)"""
    s = mul_sites(F, dict(col, tc=[0] * n), n, t, senders)
    col["tc"] = [(zp + a + b) % F.mod for zp, a, b in zip(z, s["prod_ey_d"], s["prod_x_e"])]
    return col


def mul_targeted(F, n, t, senders, d, e, p1, p2, z, spare):
    """constant sharings with the opened d, e, the products (e + y) d = p1 and x e = p2 (where d, e are not zero) and z as chosen"""
    q = F.mod
    y = (p1 * F.inv(d) - e) % q if d else spare
    x = p2 * F.inv(e) % q if e else spare
    col = {"x": [x] * n, "y": [y] * n, "ta": [(x + d) % q] * n, "tb": [(y + e) % q] * n}
    return _mul_finish(F, col, n, t, senders, [z] * n)


def mul_forced(F, n, t, senders, j):
    """forced sharings: at the forced parties x, y, a - x, b - y are edge values (so a, b differ from x, y by one) and z is one"""
    fp = forced_parties(n, t, senders)
    col = {"x": forced_sharing(F, n, t, {p: pick(F, j + 5 + i) for i, p in enumerate(fp)}),
           "y": forced_sharing(F, n, t, {p: pick(F, j + 8 + 2 * i) for i, p in enumerate(fp)})}
    col["ta"] = forced_sharing(F, n, t, {p: col["x"][p] + pick(F, j + 3 * i) for i, p in enumerate(fp)})
    col["tb"] = forced_sharing(F, n, t, {p: col["y"][p] + pick(F, j + 1 + 4 * i) for i, p in enumerate(fp)})
    return _mul_finish(F, col, n, t, senders, [pick(F, j + 2)] * n)


@_memo
def mul_columns(F, n, t, senders):
    E = len(F.edge)
    cols = [mul_targeted(F, n, t, senders, pick(F, i), pick(F, i + 4), pick(F, i + 7), pick(F, i + 9), pick(F, i + 11), pick(F, i + 3)) for i in range(E)]
    cols += [mul_targeted(F, n, t, senders, pick(F, i), pick(F, i + 8), pick(F, i + 2), pick(F, i + 12), pick(F, i + 5), pick(F, i + 6)) for i in range(E)]
    for y in (0, 1, 2, F.mod - 1):                 # e + y_p = r - 1, r, r + 1, 2r - 2 before the reduction
        cols.append(mul_targeted(F, n, t, senders, F.mod - 1, F.mod - 1, (F.mod - 1 + y) * (F.mod - 1) % F.mod, F.edge[-1], F.edge[-3], 0))
    cols += [mul_forced(F, n, t, senders, j) for j in range(E)]
    return cols


def mul_case(F, n, t, senders):
    """{name: [party][N]} over the edge columns; N <= 64"""
    cols = mul_columns(F, n, t, tuple(senders))
    return {"ins": _stack(cols, MUL_NAMES), "cols": cols, "N": len(cols)}


def mul_tamper_case(n, t, senders):
    """18 elements, x = y = 0 so that the opened shares are the triple's: element 1 + 2 i has bit TAMPER_BITS[i] set in a verify-row
    sender's share of a (chunk g fails), element 2 + 2 i in a P(0)-row sender's share of b (chunk N + g fails); elements 0 and 17
    are clean.  Returns the honest case, the tampered one and the chunks that must fail."""
    low, ver = split_senders(senders, t)
    N, cols, bad, failing = 2 * len(TAMPER_BITS) + 2, [], [], []
    for g in range(N):
        i, kind = divmod(g - 1, 2)
        col = {"x": [0] * n, "y": [0] * n}
        for nm, who in (("ta", ver), ("tb", low)):
            hit = 0 < g < N - 1 and (kind == 0) == (nm == "ta")
            sender = who[i % len(who)]
            forced = {p: pick(FR, g + 2 * k) for k, p in enumerate(_other_forced(n, t, senders, sender))}
            forced[sender] = tamper_value(TAMPER_BITS[i])[0] if hit else pick(FR, g + 7)
            col[nm] = forced_sharing(FR, n, t, forced)
            if hit:
                bad.append((nm, sender, g, tamper_value(TAMPER_BITS[i])[1]))
                failing.append(g if nm == "ta" else N + g)
        cols.append(_mul_finish(FR, col, n, t, senders, [pick(FR, g)] * n))
    honest = _stack(cols, MUL_NAMES)
    tampered = {nm: [list(row) for row in v] for nm, v in honest.items()}
    for nm, p, g, v in bad:
        assert tampered[nm][p][g] ^ v == 1 << TAMPER_BITS[(g - 1) // 2]
        tampered[nm][p][g] = v
    return {"honest": honest, "ins": tampered, "N": N, "failing": sorted(failing)}


# ---- TruncPr / FPDivConst: a, r_int, the m bit arrays and (FPDivConst) the public multiplier w ---------------------------------------
def truncpr_sites(col, n, t, senders, k, m):
    """the intermediates of TruncPr for one element, from its inputs alone (truncpr.rs:275-297, 215-220)"""
    low, ver = split_senders(senders, t)
    w = col.get("w")
    v = [a * w % R for a in col["a"]] if w is not None else list(col["a"])
    two_m = pow(2, m, R)
    s = [ri * two_m % R for ri in col["rint"]]
    rd = [sum(col["bits"][j][p] << j for j in range(m)) % R for p in range(n)]
    half = pow(2, k - 1, R)
    osh = [(v[p] + half + s[p] + rd[p]) % R for p in range(n)]
    cop = p0(FR, n, low, osh)
    cmod = S.mod_pow_2_from_field(cop, m)
    inv2m = FR.inv(pow(2, m, R))
    out = [(v[p] - (cmod - rd[p])) * inv2m % R for p in range(n)]
    sites = {"two_m_rint": s, "rdash": rd, "osh": osh, "verify_row": [osh[p] for p in ver], "cop": [cop], "cop_mod": [cmod], "out": out}
    if w is not None:
        sites["a_w"] = v
    return sites


def _bits_for(rd, m, n, i):
    """m constant bit sharings of edge values whose sum of bit_j 2^j is rd (bit 0 takes up the difference)"""
    if m == 0:
        return []
    hi = [pick(FR, i + 2 * j) for j in range(1, m)]
    b0 = (rd - sum(b << j for j, b in enumerate(hi, 1))) % R
    return [[b] * n for b in [b0] + hi]


def _truncpr_col(n, k, m, w, v, s, bits, i):
    """a column from the per-party value v that is truncated (a = v / w where there is a multiplier that is not zero), s = 2^m r_int"""
    inv2m = FR.inv(pow(2, m, R))
    col = {"rint": [sp * inv2m % R for sp in s], "bits": bits}
    if w is None:
        col["a"] = [vp % R for vp in v]
    else:
        col["w"] = w
        winv = FR.inv(w)
        col["a"] = [vp * winv % R for vp in v] if w else [pick(FR, i)] * n     # w = 0: v is zero whatever a is
    return col


def truncpr_from_operands(n, k, m, w, v, s, rd, i):
    """constant sharings with a w (or a) = v, 2^m r_int = s and r' = rd as chosen"""
    return _truncpr_col(n, k, m, w, [v] * n, [s] * n, _bits_for(rd if m else 0, m, n, i), i)


def truncpr_from_results(n, k, m, w, cop, rd, out, i):
    """constant sharings with the opened value (every party's opened share), r' and the output as chosen"""
    rd = rd if m else 0
    v = (out * pow(2, m, R) + S.mod_pow_2_from_field(cop, m) - rd) % R
    return _truncpr_col(n, k, m, w, [v] * n, [(cop - v - pow(2, k - 1, R) - rd) % R] * n, _bits_for(rd, m, n, i), i)


def truncpr_forced(n, t, senders, k, m, w, j):
    """a forced sharing of a such that the shares TruncPr opens are edge values at the forced parties; r_int and the bits constant"""
    fp = forced_parties(n, t, senders)
    s, rd = pick(FR, j + 6), (pick(FR, j + 10) if m else 0)
    rest = (pow(2, k - 1, R) + s + rd) % R
    scale = FR.inv(w) if w else 1
    a = forced_sharing(FR, n, t, {p: (pick(FR, j + 3 * i) - rest) * scale for i, p in enumerate(fp)})
    col = {"a": a, "rint": [s * FR.inv(pow(2, m, R)) % R] * n, "bits": _bits_for(rd, m, n, j)}
    if w is not None:
        col["w"] = w
    return col


@_memo
def truncpr_columns(n, t, senders, k, m, with_w, count, rot):
    """count = 0: every construction (50 columns); count > 0: that many columns of chosen results, starting at class `rot` so that
    the wide moduli m see every class between them.  The multiplier rotates through the values that are not zero (a = v / w must
    exist for v to be chosen); w = 0 has columns of its own."""
    E = len(EDGE)
    wof = (lambda i: W_VALUES[1 + i % (len(W_VALUES) - 1)]) if with_w else (lambda i: None)
    if count:
        return [truncpr_from_results(n, k, m, wof(i), pick(FR, rot + i), pick(FR, rot + i + 5), pick(FR, rot + i + 9), i) for i in range(count)]
    cols = [truncpr_from_operands(n, k, m, wof(i + 1), pick(FR, i), pick(FR, i + 4), pick(FR, i + 7), i) for i in range(E)]
    cols += [truncpr_from_results(n, k, m, wof(i + 1), pick(FR, i), pick(FR, i + 6), pick(FR, i + 11), i) for i in range(E)]
    # the maximal four-term loose sum: v = r - 1, 2^m r_int = r - 1, r' = r - 1 (then 2^(k-1))
    cols.append(truncpr_from_operands(n, k, m, wof(1), R - 1, R - 1, R - 1, 3))
    for b in (MAXLIMB, R - 1):                    # every bit share all ones: the fold interval of r' with full columns
        cols.append(_truncpr_col(n, k, m, wof(2), [b] * n, [b] * n, [[b] * n for _ in range(m)], 0))
    cols += [truncpr_forced(n, t, senders, k, m, wof(j + 1), j) for j in range(E)]
    for i in (3, 11):                              # w = 0 (the product is zero whatever a is), or two more columns without a multiplier
        cols.append(truncpr_from_operands(n, k, m, 0 if with_w else None, pick(FR, i), pick(FR, i + 1), pick(FR, i + 2), i))
    return cols


def truncpr_stack(cols, n, m):
    ins = _stack(cols, ("a", "rint"))
    ins["rbits"] = [[[c["bits"][j][p] for c in cols] for j in range(m)] for p in range(n)]     # [party][m][N]
    ins["w"] = [c["w"] for c in cols] if "w" in cols[0] else None
    return ins


def truncpr_case(n, t, senders, k, m, with_w, count=0, rot=0):
    cols = truncpr_columns(n, t, tuple(senders), k, m, with_w, count, rot)
    return {"ins": truncpr_stack(cols, n, m), "cols": cols, "N": len(cols)}


def truncpr_tamper_case(n, t, senders, k, m):
    """18 elements with 2^m r_int = -2^(k-1) and r' = 0, so that the share TruncPr opens IS a: element 1 + 2 i has bit
    TAMPER_BITS[i] set in a verify-row sender's share of a, element 2 + 2 i in a P(0)-row sender's; elements 0 and 17 are clean"""
    low, ver = split_senders(senders, t)
    N, cols, bad = 2 * len(TAMPER_BITS) + 2, [], []
    rint = -pow(2, k - 1, R) * FR.inv(pow(2, m, R)) % R
    for g in range(N):
        i, kind = divmod(g - 1, 2)
        who = ver if kind == 0 else low
        sender = who[i % len(who)]
        hit = 0 < g < N - 1
        forced = {p: pick(FR, g + 2 * j) for j, p in enumerate(_other_forced(n, t, senders, sender))}
        forced[sender] = tamper_value(TAMPER_BITS[i])[0] if hit else pick(FR, g + 7)
        cols.append({"a": forced_sharing(FR, n, t, forced), "rint": [rint] * n, "bits": [[0] * n for _ in range(m)]})
        if hit:
            bad.append((sender, g, tamper_value(TAMPER_BITS[i])[1]))
    honest = truncpr_stack(cols, n, m)
    tampered = dict(honest, a=[list(row) for row in honest["a"]])
    for p, g, v in bad:
        assert tampered["a"][p][g] ^ v == 1 << TAMPER_BITS[(g - 1) // 2]
        tampered["a"][p][g] = v
    return {"honest": honest, "ins": tampered, "N": N, "failing": [g for _, g, _ in bad]}


# ---- FpMul: the union of the two -------------------------------------------------------------------------------------------------
def fpmul_case(n, t, senders, k, m, count=0, rot=0, tile=1):
    """every Mul column with the r_int and bits of a TruncPr column (TruncPr then runs on the z chosen there), and every TruncPr
    column behind a Mul column whose tc is solved so that z_p is that column's a_p; count > 0: only `count` of the latter, of chosen
    results from class `rot` on (the wide moduli); tile: the first columns again up to a whole number of tiles of that many elements"""
    mc, tc = mul_columns(FR, n, t, tuple(senders)), truncpr_columns(n, t, tuple(senders), k, m, False, count, rot)
    cols = []
    for i, c in enumerate(mc if not count else []):
        cols.append(dict(c, rint=tc[i % len(tc)]["rint"], bits=tc[i % len(tc)]["bits"]))
    for i, c in enumerate(tc):
        cols.append(dict(_mul_finish(FR, dict(mc[i % len(mc)]), n, t, senders, c["a"]), rint=c["rint"], bits=c["bits"]))
    cols += cols[:-len(cols) % tile]
    ins = _stack(cols, MUL_NAMES + ("rint",))
    ins["rbits"] = [[[c["bits"][j][p] for c in cols] for j in range(m)] for p in range(n)]
    return {"ins": ins, "cols": cols, "N": len(cols)}


def fpmul_sites(col, n, t, senders, k, m):
    s = mul_sites(FR, col, n, t, senders)
    s2 = truncpr_sites({"a": s["z"], "rint": col["rint"], "bits": col["bits"]}, n, t, senders, k, m)
    s2.pop("verify_row")
    return dict(s, **s2)


def fpmul_tamper_case(n, t, senders, k, m):
    """the Mul tampering (the first open fails: a chunk of a - x or of b - y), then 18 more elements whose second open fails: x = y = 0,
    so z_p = tc_p - a b, and 2^m r_int = a b - 2^(k-1) with r' = 0, so the share TruncPr opens IS tc_p, which carries the bit"""
    mt = mul_tamper_case(n, t, senders)
    tt = truncpr_tamper_case(n, t, senders, k, m)
    N1, N2 = mt["N"], tt["N"]
    out = {}
    for key in ("honest", "ins"):
        cols = []
        for g in range(N1):
            cols.append({nm: [mt[key][nm][p][g] for p in range(n)] for nm in MUL_NAMES})
            cols[-1].update(rint=[pick(FR, g)] * n, bits=[[pick(FR, g + j)] * n for j in range(m)])
        for g in range(N2):
            a, b = pick(FR, g + 3), pick(FR, g + 8)
            rint = (a * b - pow(2, k - 1, R)) * FR.inv(pow(2, m, R)) % R
            col = {"x": [0] * n, "y": [0] * n, "ta": [a] * n, "tb": [b] * n, "tc": [(tt[key]["a"][p][g] + a * b) % R for p in range(n)]}
            cols.append(dict(col, rint=[rint] * n, bits=[[0] * n for _ in range(m)]))
        ins = _stack(cols, MUL_NAMES + ("rint",))
        ins["rbits"] = [[[c["bits"][j][p] for c in cols] for j in range(m)] for p in range(n)]
        out[key] = ins
    N = N1 + N2
    first = [g if g < N1 else N + g - N1 for g in mt["failing"]]          # chunks of the first open: [0, N) a - x, [N, 2 N) b - y
    return dict(out, N=N, failing_first=sorted(first), failing_second=[N1 + g for g in tt["failing"]])


# ---- triple generation: a, b (degree t), r2t (degree 2t), rt (degree t) with the same secret ----------------------------------------
TRIPLE_NAMES = ("a", "b", "r2t", "rt")


def triple_sites(F, col, n, t):
    """a_p b_p - r2t_p, and the opened value (its P(0)) plus rt_p"""
    q = F.mod
    loc = [(a * b - r) % q for a, b, r in zip(col["a"], col["b"], col["r2t"])]
    opened = p0(F, n, list(range(2 * t + 1)), loc)
    return {"local": loc, "c": [(opened + r) % q for r in col["rt"]]}


def triple_targeted(F, n, loc, c, b):
    """constant sharings with a b - r = loc and c = a b as chosen (b not zero)"""
    q = F.mod
    return {"a": [c * F.inv(b) % q] * n, "b": [b] * n, "r2t": [(c - loc) % q] * n, "rt": [(c - loc) % q] * n}


def triple_forced(F, n, t, j):
    """forced sharings (every party is a sender here: the forced parties are the upper ones, party n - 1 among them): a, b edge values
    at t + 1 parties, r2t through 2t + 1 parties such that a_p b_p - r2t_p is an edge value there, rt with r2t's secret such that
    opened + rt_p is one at t parties"""
    q = F.mod
    top = list(range(n - 1, n - 2 - 2 * t, -1))                           # 2t + 1 parties from n - 1 down
    col = {"a": forced_sharing(F, n, t, {p: pick(F, j + i) for i, p in enumerate(top[:t + 1])}),
           "b": forced_sharing(F, n, t, {p: pick(F, j + 4 + 2 * i) for i, p in enumerate(top[:t + 1])})}
    col["r2t"] = forced_sharing(F, n, 2 * t, {p: col["a"][p] * col["b"][p] - pick(F, j + 3 * i) for i, p in enumerate(top)})
    loc = [(a * b - r) % q for a, b, r in zip(col["a"], col["b"], col["r2t"])]
    opened = p0(F, n, list(range(2 * t + 1)), loc)
    secret = p0(F, n, list(range(2 * t + 1)), col["r2t"])
    forced = {p: pick(F, j + 1 + 5 * i) - opened for i, p in enumerate(top[:t])}
    forced[-1] = secret
    col["rt"] = forced_sharing(F, n, t, forced)
    return col


@_memo
def triple_columns(F, n, t):
    E = len(F.edge)
    nz = [v for v in F.edge if v]
    cols = [triple_targeted(F, n, pick(F, i), pick(F, i + 6), nz[i % len(nz)]) for i in range(E)]
    cols += [triple_forced(F, n, t, j) for j in range(E)]
    while len(cols) % (2 * t + 1):                                        # whole chunks of 2t + 1
        cols.append(triple_targeted(F, n, pick(F, len(cols) + 1), pick(F, len(cols) + 9), nz[len(cols) % len(nz)]))
    return cols


def triple_case(F, n, t):
    cols = triple_columns(F, n, t)
    return {"ins": _stack(cols, TRIPLE_NAMES), "cols": cols, "N": len(cols)}


# ---- what the GPU tests run, and what those inputs must reach ------------------------------------------------------------------------
# (n, t, senders): no lane sharing; quads; pairs; the tail load loop; 22-term rows with a lane per row; senders unsorted, no prefix
MUL_SHAPES = [(4, 1, (0, 1, 2)), (16, 5, tuple(range(11))), (31, 10, tuple(range(21))), (46, 15, tuple(range(31))), (64, 21, tuple(range(43))),
              (7, 2, (6, 1, 3, 0, 4))]
TRUNCPR_SHAPES = [(4, 1), (16, 5), (31, 10), (64, 21)]
TRUNCPR_M = (0, 1, 6, 7, 12, 13, 40)             # both sides of every fold boundary of r' (6 terms between folds)
TRUNCPR_WIDE_M = (29, 31, 32, 33, 64, 232, 254, 255, 256, 264)   # the mask of c mod 2^m on both sides of a word and of r's width
TRUNCPR_K = (1, 32, 250)
FPMUL_SHAPES = [(4, 1, 32, 13), (16, 5, 250, 7), (31, 10, 32, 6), (40, 13, 2, 1)]   # (n, t, k, m)
FPMUL_WIDE = [(4, 1, 32, 255, 5, 0), (4, 1, 250, 256, 5, 5), (4, 1, 1, 264, 5, 10)]   # (n, t, k, m, count, rot): c mod 2^m = c, every class
TRIPLE_SHAPES = [(4, 1), (7, 2), (16, 5)]


def truncpr_k(with_w, m, shape_index):
    """k in {1, 32, 250}, rotating with the case; FPDivConst runs TruncPr with an even number of bits"""
    ks = TRUNCPR_K[1:] if with_w else TRUNCPR_K
    return ks[(TRUNCPR_M.index(m) + shape_index) % len(ks)]


def truncpr_cases():
    """every (n, t, senders, k, m, with_w, count, rot) the GPU tests run"""
    out = []
    for with_w in (False, True):
        for m in TRUNCPR_M:
            for si, (n, t) in enumerate(TRUNCPR_SHAPES):
                out.append((n, t, tuple(range(2 * t + 1)), truncpr_k(with_w, m, si), m, with_w, 0, 0))
        for qi, m in enumerate(TRUNCPR_WIDE_M):
            out.append((4, 1, (0, 1, 2), (TRUNCPR_K[1:] if with_w else TRUNCPR_K)[qi % (2 if with_w else 3)], m, with_w, 4, 4 * qi + (7 if with_w else 0)))
    return out


_MUL_SITES = {"open_share": "edge", "verify_row": "edge", "d": "edge", "e": "edge", "e_plus_y": "sums", "prod_ey_d": "edge", "prod_x_e": "edge",
              "z": "edge"}
_TRUNCPR_SITES = {"two_m_rint": "edge", "rdash": "edge", "osh": "edge", "verify_row": "edge", "cop": "edge", "cop_mod": "edge", "out": "edge"}
SITE_TABLE = {                                    # "truncpr": both instances of the kernel (with and without a multiplier) together
    "mul": _MUL_SITES,
    "truncpr": dict(_TRUNCPR_SITES, a_w="edge"),
    "fpmul": dict(_MUL_SITES, **{k: v for k, v in _TRUNCPR_SITES.items() if k != "verify_row"}),
    "triplegen": {"local": "edge", "c": "edge"},
}


def missing_pairs(F, kernel, site_lists):
    """the (site, value) pairs of SITE_TABLE[kernel] that no (party, element) of the given per-column site values reaches"""
    seen = {}
    for sites in site_lists:
        for nm, vals in sites.items():
            seen.setdefault(nm, set()).update(vals)
    return [(nm, v) for nm, cls in SITE_TABLE[kernel].items() for v in (F.edge if cls == "edge" else F.sums) if v not in seen.get(nm, ())]
