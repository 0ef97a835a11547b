"""Deterministic inputs with CHOSEN discrete logs for the square-root kernels (csrc/kernels_sqrt.hpp: k_sqrt, k_inverse,
k_randbit_finalize, and sqrt_core inside k_randbit_wg), from plain Python integers and tests/randbit_ref.py alone (no library, no GPU).

Both fields have p - 1 = 2^32 T with T odd.  The kernels take u = A^((T-1)/2), find L with A^T = omega^L by four 8-bit windows
(a reverse look-up keyed by a hashed bit slice, windows 1 to 3 corrected through the negw tables), and form the root A u omega^E with
E = (-L/2) mod 2^31 and RandBit's x^-1 = u omega^(-(L+E)).  Everything that depends on the data is therefore a function of L alone,
and a uniform A has a uniform L.  Here L is chosen:

    with_log(p, L, c) = omega^(L T^-1 mod 2^32) c^(2^32)       so that  A^T = omega^L  for every cofactor c != 0

LOGS is the family of L (the same for both fields); family(p) gives it cofactors: 1 (A is a subgroup element and its Montgomery form
is a table entry), seeded random values, and the edge values of tests/edge_inputs.py taken as A directly with whatever L they have.
SITE_TABLE names what the family must reach; reached(p) computes it from the inputs alone and tests/test_sqrt_inputs.py enforces
it, so the GPU tests (tests/test_gpu_sqrt_edges.py) cannot silently miss their target.

Two rows one might ask for cannot be reached by ANY input, and the table says so instead of waiving them.  For an even L != 0,
E = 2^31 - L/2, so (1) L + E = 2^31 + L/2 < 2^32: the sum never wraps, its largest value 2^32 - 1 (L = 2^32 - 2) is a row; and
(2) -(L + E) mod 2^32 = 2^31 - L/2 = E: both omega_pow calls take the same index, which is below 2^31, so posw[3][128..255] is
never read.  The rows "never" assert exactly that over the family.

k_inverse's layout (csrc/tu_sqrt.hip launches it with B = 8 for u29 and Goldilocks and B = 2 for sat32): element i is in block
i // (256 B), lane i % 256, slot (i % (256 B)) // 256.  inverse_case() and inverse_tails() place zeros by that rule."""
import functools
import random

from tests import edge_inputs as EI
from tests import randbit_ref as RB

M32 = (1 << 32) - 1
FIELDS = {"fr": EI.FR, "goldilocks": EI.GL}


@functools.lru_cache(maxsize=None)
def _consts(p):
    T = RB.trace(p)
    assert T & 1 and (p - 1) == T << 32
    return RB.omega(p), pow(T, -1, 1 << 32), T


def with_log(p, L, c=1):
    """A with A^T = omega^L, for any cofactor c that is not zero"""
    om, tinv, _ = _consts(p)
    assert c % p
    return pow(om, (L * tinv) & M32, p) * pow(c, 1 << 32, p) % p


def log_of(A, p):
    """L in [0, 2^32) with A^T = omega^L (A not zero), by the restatement's bit-by-bit discrete log"""
    return RB.dlog_omega(pow(A, _consts(p)[2], p), p)


def ark_sqrt_trace(a, p):
    """tests/randbit_ref.py's ark_sqrt, instrumented: -> (root or None, the k_i of its loop in order)"""
    ks = []
    if a == 0:
        return 0, ks
    z = RB.omega(p)
    w = pow(a, (RB.trace(p) - 1) // 2, p)
    x = w * a % p
    b = x * w % p
    v = RB.TWO_ADICITY
    while b != 1:
        k, b2k = 0, b
        while b2k != 1:
            b2k = b2k * b2k % p
            k += 1
        ks.append(k)
        if k == RB.TWO_ADICITY:
            return None, ks
        w = z
        for _ in range(1, v - k):
            w = w * w % p
        z = w * w % p
        b = b * z % p
        x = x * w % p
        v = k
    return (x if x * x % p == a else None), ks


# ---- the family of L -----------------------------------------------------------------------------------------------------------------
NAMED = (0, 2, 2**32 - 2, 2**31, 2**31 + 2, 2**31 - 2, 0xFFFFFFFE, 0xFFFFFFFF, 0xAAAAAAAA, 0x55555554, 0x80000001, 0x7FFFFFFE)
UPPER_BYTES = (0x01, 0x5A, 0x80, 0xFF)     # the chosen byte of an upper window over lower windows that are all 0x00 / all 0xFF


def _logs():
    out = []
    for w in range(4):                       # every byte of every window, alone
        out += [("byte", j << (8 * w)) for j in range(256)]
    for i in range(32):
        out += [("bit", 1 << i), ("bit", 2**32 - (1 << i)), ("bit", M32 ^ (1 << i))]
    out += [("named", v) for v in NAMED]
    for w in (1, 2, 3):                      # the negw corrections of window w at their first and last entries
        for b in UPPER_BYTES:
            for low in (0, (1 << (8 * w)) - 1):
                for high in (0, M32 >> (8 * (w + 1)) << (8 * (w + 1)) if w < 3 else 0):
                    out.append(("under", high | b << (8 * w) | low))
    for w in range(4):                       # E = j << 8w exactly: every posw entry the kernels can read (E < 2^31)
        out += [("E", (2**32 - 2 * (j << (8 * w))) & M32) for j in range(256 if w < 3 else 128)]
    seen, uniq = set(), []
    for tag, v in out:
        assert 0 <= v <= M32
        if v not in seen:
            seen.add(v)
            uniq.append((tag, v))
    return tuple(uniq)


LOGS = _logs()                               # (tag, L), distinct L; odd L (the non-residues) stay in


def exps(L):
    """(E, the index of RandBit's omega_pow) of an even L, as the kernels compute them in 32-bit words"""
    E = (0 - (L >> 1)) & 0x7FFFFFFF
    return E, (0 - (L + E)) & M32


def sites(L):
    """what sqrt_core / omega_pow index for an A (not zero) with this L"""
    l = [(L >> (8 * w)) & 255 for w in range(4)]
    s = {"key": {(w, l[w]) for w in range(4)},
         # (negw row, entry, the window whose look-up it corrects): kernels_sqrt.hpp sqrt_core
         "negw": {(2, l[0], 1), (1, l[0], 2), (2, l[1], 2), (0, l[0], 3), (1, l[1], 3), (2, l[2], 3)}}
    if not L & 1:
        E, V = exps(L)
        s["E"] = {E}
        s["L_plus_E"] = {L + E}
        s["posw_E"] = {(w, (E >> (8 * w)) & 255) for w in range(4)}
        s["posw_inv"] = {(w, (V >> (8 * w)) & 255) for w in range(4)}
    return s


_POSW = frozenset((w, j) for w in range(4) for j in range(256) if w < 3 or j < 128)
SITE_TABLE = {
    # ark's loop (ark_sqrt_trace): ("n", iterations) of a square, ("ks", the k_i) of a short loop, ("exit", 32) of a non-residue
    "loop": frozenset({("n", 0), ("ks", (1,)), ("n", 31), ("exit", 32)}),
    "E": frozenset({0, 1, 2**31 - 1}),
    "L_plus_E": frozenset({0, 2**31 + 1, 2**32 - 1}),           # the sum's least and greatest values: it cannot reach 2^32 (docstring)
    "posw_E": _POSW,                                            # every (window, byte) omega^E can index
    "posw_inv": _POSW,                                          # every (window, byte) omega^(-(L+E)) can index
    "key": frozenset((w, j) for w in range(4) for j in range(256)),
    "negw": frozenset((m, j, w) for m, w in ((2, 1), (1, 2), (2, 2), (0, 3), (1, 3), (2, 3)) for j in range(256)),
}
NEVER = {                                                       # proved unreachable: asserted to stay unreached
    "L_plus_E": lambda v: v >= 2**32,
    "posw_E": lambda wj: wj[0] == 3 and wj[1] >= 128,
    "posw_inv": lambda wj: wj[0] == 3 and wj[1] >= 128,
}


# ---- the family of A -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def family(p):
    """[(A, L, kind)]: every L of LOGS with a seeded random cofactor ("random"), the named, single-bit and under-window ones and every
    eighth of the rest also with cofactor 1 ("subgroup"), then the field's edge values as A ("edge", L = None: tests compute it)"""
    rng = random.Random(0x5137 + p % 1009)
    out = []
    for i, (tag, L) in enumerate(LOGS):
        out.append((with_log(p, L, rng.randrange(2, p)), L, "random"))
        if tag in ("bit", "named", "under") or i % 8 == 0:
            out.append((with_log(p, L, 1), L, "subgroup"))
    edge = EI.EDGE if p == RB.P_FR else EI.EDGE_GL
    out += [(v, None, "edge") for v in dict.fromkeys(edge)]
    return tuple(out)


@functools.lru_cache(maxsize=None)
def family_values(p):
    return tuple(A for A, _, _ in family(p))


@functools.lru_cache(maxsize=None)
def family_roots(p):
    """[(ark's root or None, the loop's k_i)] of family_values(p), computed once and shared by the tests"""
    return tuple(ark_sqrt_trace(A, p) for A in family_values(p))


@functools.lru_cache(maxsize=None)
def family_logs(p):
    """L of every family value (None for A = 0); the edge values' L by log_of"""
    return tuple(L if L is not None else (log_of(A, p) if A else None) for A, L, _ in family(p))


def reached(p):
    """row of SITE_TABLE -> what the family reaches, from the inputs alone"""
    got = {k: set() for k in SITE_TABLE}
    for A, L, (root, ks) in zip(family_values(p), family_logs(p), family_roots(p)):
        if A == 0:
            continue
        for k, v in sites(L).items():
            got[k] |= v
        if root is not None:
            got["loop"].add(("n", len(ks)))
            if len(ks) <= 1:
                got["loop"].add(("ks", tuple(ks)))
        elif ks:
            got["loop"].add(("exit", ks[-1]))
    return got


def permuted(p, seed, extra=0):
    """the family's values (plus `extra` seeded random elements) in a seeded order -> (values, index of each in family_values or None)"""
    rng = random.Random(seed)
    idx = list(range(len(family_values(p)))) + [None] * extra
    rng.shuffle(idx)
    fv = family_values(p)
    return [fv[i] if i is not None else rng.randrange(p) for i in idx], idx


# ---- k_inverse: slot patterns and tails ---------------------------------------------------------------------------------------------
def slot_of(i, B):
    """(block, lane, slot) of element i under k_inverse<F, B>"""
    return i // (256 * B), i % 256, (i % (256 * B)) // 256


def lanes_of(vals, B):
    """{(block, lane): the values of its live slots in slot order}"""
    out = {}
    for i, v in enumerate(vals):
        blk, lane, slot = slot_of(i, B)
        row = out.setdefault((blk, lane), [])
        assert len(row) == slot
        row.append(v)
    return out


def lane_classes(vals, p, B, edge):
    """the pattern classes that the FULL lanes (all B slots live) of `vals` realise under slot count B"""
    got = set()
    for row in lanes_of(vals, B).values():
        if len(row) != B:
            continue
        zeros = [k for k, v in enumerate(row) if v == 0]
        if len(zeros) == 1:
            got.add(("zero_only", zeros[0]))
        if len(zeros) == B:
            got.add("all_zero")
        if len(zeros) == B - 1:
            got.add(("all_but", next(k for k, v in enumerate(row) if v)))
        if not zeros:
            got.add("no_zero")
            if set(row) == {1, p - 1}:
                got.add("ones_and_minus_ones")
            prod = 1
            for v in row:
                prod = prod * v % p
            if prod == 1 and 1 not in row and p - 1 not in row:
                got.add("product_one")
        if set(row) <= set(edge):
            got.add("edge")
    return got


def required_classes(B):
    return ({("zero_only", k) for k in range(B)} | {("all_but", k) for k in range(B)}
            | {"all_zero", "no_zero", "ones_and_minus_ones", "product_one", "edge"})


def inverse_case(F, B_slots=8):
    """one block of 256 * B_slots elements whose lanes realise every class of required_classes() for B_slots slots and, the pairs of
    adjacent slots being the lanes of a two-slot kernel, for 2 slots at once -> list of ints"""
    p, B = F.mod, B_slots
    assert B % 2 == 0
    rng = random.Random(77 + B)
    nz = lambda: rng.randrange(2, p - 1)  # noqa: E731
    lanes = []
    for k in range(B):
        lanes.append([0 if s == k else nz() for s in range(B)])            # zero in slot k only
    lanes.append([0] * B)                                                   # all slots zero
    for k in range(B):
        lanes.append([nz() if s == k else 0 for s in range(B)])            # all slots but one zero
    lanes.append([nz() for _ in range(B)])                                  # no zero
    lanes.append([1 if s % 2 == 0 else p - 1 for s in range(B)])            # only 1 and p - 1
    lanes.append([1] * B)
    lanes.append([p - 1] * B)
    pairs = []
    for _ in range(B // 2):
        x = nz()
        pairs += [x, pow(x, p - 2, p)]
    lanes.append(pairs)                                                     # x, x^-1 pairs: the product is 1
    edge = list(dict.fromkeys(F.edge))
    nze = [v for v in edge if v]
    for e in range(len(edge)):
        lanes.append([edge[(e + s) % len(edge)] for s in range(B)])         # edge values, zero among them
    for e in range(len(nze)):
        lanes.append([nze[(e + 3 * s) % len(nze)] for s in range(B)])       # edge values, none zero
    assert len(lanes) <= 256
    fam = [v for v in family_values(p) if v]
    while len(lanes) < 256:                                                 # the other lanes: family values and random ones
        lanes.append([fam[(len(lanes) * B + s) % len(fam)] if len(lanes) % 2 else nz() for s in range(B)])
    return [lanes[lane][slot] for slot in range(B) for lane in range(256)]


TAIL_R = lambda B: (1, 255, 256, 257, 256 * (B - 1) + 1)  # noqa: E731


def inverse_tails(F, B):
    """[(N, values)] with N = 256 B k + r for every r of TAIL_R(B): k = 0 with a zero in the last live slot (element N - 1) and an edge
    value in the one before, k = 1 with the two the other way round"""
    p = F.mod
    rng = random.Random(991 + B)
    out = []
    for r in dict.fromkeys(TAIL_R(B)):
        for k in (0, 1):
            N = 256 * B * k + r
            vals = [rng.randrange(1, p) for _ in range(N)]
            pair = [p - 1, 0] if k == 0 else [0, F.edge[-3]]
            for off, v in zip((2, 1), pair):
                if N - off >= 0:
                    vals[N - off] = v
            out.append((N, vals))
    return out


# ---- k_randbit_finalize: squares from the family, shares solved for the output --------------------------------------------------------
def phase2_case(F, parties, which=None):
    """squares = the family's values (`which`: indices into it; all by default), a [parties][N] with a_p = (2 out - 1) b so that the
    OUTPUT a_p (2b)^-1 + 2^-1 is a chosen edge value (store_loose's subtracting branch sees r - 1, r - 2, ...), every third share an
    edge value itself -> (sq, a, the chosen outputs [parties][N] or None where the share was not solved)"""
    p = F.mod
    fv, roots = family_values(p), family_roots(p)
    which = range(len(fv)) if which is None else which
    sq = [fv[i] for i in which]
    a, outs = [], []
    for q in range(parties):
        row, orow = [], []
        for pos, i in enumerate(which):
            b = roots[i][0]
            e = F.edge[(pos + 5 * q) % len(F.edge)]
            if (pos + q) % 3 == 0 or not b:
                row.append(e)
                orow.append(None)
            else:
                row.append((2 * e - 1) * b % p)
                orow.append(e)
        a.append(row)
        outs.append(orow)
    return sq, a, outs


def even_indices(p):
    """indices of the family values that have a root and are not zero; odd_indices: the non-residues"""
    return [i for i, (A, L) in enumerate(zip(family_values(p), family_logs(p))) if A and not L & 1]


def odd_indices(p):
    return [i for i, (A, L) in enumerate(zip(family_values(p), family_logs(p))) if A and L & 1]


def failure_layouts(F, N=300):
    """{name: (indices into the family [N], expected (first, n_failed) of the summary)}: a base of squares with roots, N no multiple
    of 256 (one full block and a partial one), and failures placed as named"""
    p = F.mod
    ev, od = even_indices(p), odd_indices(p)
    zero = family_values(p).index(0)
    assert N % 256 and N > 256
    base = [ev[(7 * i) % len(ev)] for i in range(N)]
    ST_Z, ST_N = RB.ST_ZERO, RB.ST_NO_ROOT

    def put(edits):
        idx = list(base)
        for i, kind in edits.items():
            idx[i] = zero if kind == "z" else od[(11 * i) % len(od)]
        st = {i: (ST_Z if k == "z" else ST_N) for i, k in edits.items()}
        first = min((s << 32) | i for i, s in st.items())
        return idx, (first, len(edits))

    return {
        "first_at_0": put({0: "n"}),
        "first_at_last": put({N - 1: "n"}),
        "first_in_partial_block": put({257: "n", N - 2: "n"}),
        "zero_after_non_residues": put({3: "n", 100: "n", 255: "n", 256: "n", 270: "z", 280: "n"}),
        "only_non_residues": put({5: "n", 64: "n", 256: "n", N - 1: "n"}),
        "every_element_fails": put({i: ("z" if i % 50 == 17 else "n") for i in range(N)}),
    }
