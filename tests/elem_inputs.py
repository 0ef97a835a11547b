"""Deterministic inputs for the element-wise share kernels (csrc/kernels_elem.hpp), built from the edge values of tests/edge_inputs.py
with plain Python integers: no library, no GPU.

A case is a list of C distinct COLUMNS (one element of every array of the call: a value per party for the per-party arrays, one value
for the public operands), the edge columns first; C is odd.  Element i of a shape holds column i % C, so a column sits on another
lane in every block of 256 and the expected output of a large shape is the model's output on the C columns, tiled.  The per-party
values differ from party to party and the public ones from element to element.

SITE_TABLE names, per call, the intermediates and the value classes each must take for at least one (party, element); sites()
computes those intermediates from the generated arrays alone and tests/test_elem_inputs.py enforces the table for every shape that
holds all C columns (claims()), so that the GPU tests (tests/test_gpu_elem_edges.py) cannot silently miss their target.

Column 0 of every case is chosen so that a shape of ONE element already tells the value mutations of tests/elem_model.py apart: the
add-type calls start with a + b = r with a carry out of every stored word, the sub-type calls with 0 - 1.
"""
from tests import edge_inputs as EI
from tests import elem_model as M

FLD = {"fr": EI.FR, "goldilocks": EI.GL}
GRID_SHAPES = [(1, 1), (255, 3), (256, 16), (257, 2), (513, 5)]     # (N, parties): a grid row per party
IN_THREAD_SHAPES = [(65535, 3), (65536, 3), (65537, 3)]            # both sides of the 2^16 rule; from 2^16 the thread loops over the parties
RDASH_M = (0, 1, 6, 7, 12, 13, 40, 255, 256)                       # both sides of every fold of r' (six terms between folds), and wide
FINALIZE_M = EI.TRUNCPR_WIDE_M                                     # the mask of c mod 2^m on both sides of a word and of r's width
K_VALUES = EI.TRUNCPR_K
OPEN_KM = [(1, 0), (32, 13), (250, 40), (32, 255), (250, 256)]     # truncpr_open_share's (k, m)
FPMUL_KM = [(32, 0), (32, 7), (32, 13)]
PARTY_CALLS = ("triple_finalize", "beaver_open_shares_paired", "beaver_finalize", "truncpr_rdash", "fpmul_middle", "truncpr_finalize")
CALLS = ("fr_op_add", "fr_op_sub", "fr_op_mul", "scalar_add", "scalar_sub", "scalar_mul", "scalar_rsub", "triple_local", "triple_finalize",
         "beaver_open_shares", "beaver_open_shares_paired", "beaver_finalize", "truncpr_rdash", "truncpr_open_share", "fpmul_middle",
         "truncpr_finalize")


def pk(F, i):
    return F.edge[i % len(F.edge)]


def nz(F, i):
    vals = [v for v in F.edge if v]
    return vals[i % len(vals)]


def scalars(field):
    F = FLD[field]
    return (F.mod - 1, 0, 1, pk(F, 12))


def params_of(call):
    """every parameter set the GPU tests run the call with"""
    if call.startswith("scalar_"):
        return [{"s": i} for i in range(4)]
    return {"truncpr_rdash": [{"m": m} for m in RDASH_M], "truncpr_open_share": [{"k": k, "m": m} for k, m in OPEN_KM],
            "fpmul_middle": [{"k": k, "m": m} for k, m in FPMUL_KM], "truncpr_finalize": [{"m": m} for m in FINALIZE_M]}.get(call, [{}])


def fields_of(call):
    return ("fr",) if call in M.FR_ONLY else ("fr", "goldilocks")


# ---- operand pairs of the add-type and sub-type calls ------------------------------------------------------------------------------------
def add_pairs(field):
    F, q, nw, E = FLD[field], FLD[field].mod, M.NWORDS[field], len(FLD[field].edge)
    lowones = (1 << 32 * (nw - 1)) - 1                                 # all ones below the top word
    out = [(lowones, q - lowones), (q - 1, q - 1)]                     # a + b = r, a carry out of every word below the top; 2 r - 2
    out += [(1, q - 2), (q - 1, 1), (2, q - 1), (0, 0), (1 << 32 * nw - 1, 1 << 32 * nw - 1) if field == "goldilocks" else (3, q - 3)]
    out += [((1 << 32 * (k + 1)) - 1 - k, 1 + k) for k in range(nw - 1)]       # the carry that runs up to word k, and no further
    out += [(pk(F, i), pk(F, i + 4)) for i in range(E)]
    out += [(pk(F, i), q - 1 - pk(F, i)) for i in range(E)]            # r - 1 and r, from every edge value
    out += [(pk(F, i), (q - pk(F, i)) % q) for i in range(E)]
    return out


def sub_pairs(field):
    F, q, nw, E = FLD[field], FLD[field].mod, M.NWORDS[field], len(FLD[field].edge)
    out = [(0, 1), (pk(F, 6), pk(F, 6)), (0, q - 1), (q - 1, 0)]       # -1 (a borrow out of every word), 0, -(r - 1), r - 1
    out += [(1 << 32 * (k + 1), 1) for k in range(nw - 1)]             # not negative: borrows out of words 0 .. k
    out += [(1, 1 << 32 * (k + 1)) for k in range(nw - 1)]             # negative: borrows from word k + 1 up
    out += [(1 << 32 * (k + 1), (1 << 32 * (k + 1)) + 1) for k in range(nw - 1)]
    out += [(pk(F, i), pk(F, i + 3)) for i in range(E)]
    out += [(pk(F, i + 3), pk(F, i)) for i in range(E)]
    out += [(pk(F, i), pk(F, i)) for i in range(0, E, 4)]
    return out


def _odd(cols):
    return cols if len(cols) % 2 else cols + [cols[len(cols) // 2]]


# ---- the columns of every call ------------------------------------------------------------------------------------------------------------
# a column: {array name: value (public operands, single-party calls) | [value per party]}; r_bits: [party][m]
def _bf_column(F, j, p):
    """finalize_mul's column j for party p: (d, e) depend on j alone; c, x, y are solved for the party's targets"""
    q, E = F.mod, len(F.edge)
    inv = F.inv
    if j < E:                                       # products and z in every class; d, e not zero
        d, e = nz(F, j), nz(F, j + 4)
        p1, p2, z = pk(F, j + 7 * p), pk(F, j + 2 + 2 * p), pk(F, j + 4 + 11 * p)
        y, x = (p1 * inv(d) - e) % q, p2 * inv(e) % q
    elif j < E + 4:                                 # e + y_p = r - 1, r, r + 1, 2 r - 2 before any reduction
        d, e = nz(F, j + 3), q - 1
        y, x, z = (F.sums[(j - E + p) % 4] - e), pk(F, j + p), pk(F, j + 3 + p)
        p1, p2 = (e + y) * d % q, x * e % q
    elif j < E + 6:                                 # the lazy sum's extremes: c = 0 with both products r - 1; c = r - 1 with both 0
        d, e = nz(F, j + 3), nz(F, j + 5)
        p1 = p2 = q - 1 if (j - E + p) % 2 == 0 else 0
        z = (0 if p1 else q - 1) - p1 - p2
        y, x = (p1 * inv(d) - e) % q, p2 * inv(e) % q
    else:                                           # d = 0, e = 0, both
        d, e = [(0, nz(F, 9)), (nz(F, 12), 0), (0, 0)][j - E - 6]
        y, x, z = pk(F, j + p), pk(F, j + 5 + 2 * p), pk(F, j + 8 + 4 * p)
        p1, p2 = (e + y) * d % q, x * e % q
    return d, e, (z + p1 + p2) % q, x, y, z % q


def _bf_order(F):
    """finalize_mul's columns, the nine special ones spread between the edge ones (their e repeats: r - 1 four times, 0 twice)"""
    E = len(F.edge)
    order = list(range(E))
    for t in range(9):
        order.insert(1 + 2 * t, E + t)
    return order


def _bits_column(F, j, p, m):
    """m bit shares of edge values with r' = sum 2^j bit_j as chosen (bit 0 takes up the difference); the last two columns hold the
    same full-limb value in every bit"""
    q, E = F.mod, len(F.edge)
    if m == 0:
        return []
    if j >= E:
        return [(EI.MAXLIMB, q - 1)[(j - E + p) % 2]] * m
    hi = [pk(F, j + 2 * t + 7 * p) for t in range(1, m)]
    b0 = (pk(F, j + p) - sum(b << t for t, b in enumerate(hi, 1))) % q
    return [b0] + hi


def _fin_column(F, j, p, m):
    """truncpr_finalize's column j for party p: (c_open, a, r'); the first columns put c_open around 2^m and r' around c mod 2^m"""
    q, E = F.mod, len(F.edge)
    cop = [(1 << m) + 1, (1 << m) - 1, 1 << m][j] % q if j < 3 else pk(F, j)
    cmod = M.mod_pow_2(cop, m) % q
    rd = pk(F, j + 5 + p)
    if 3 <= j < 6 and p == 0:
        rd = (cmod + j - 4) % q                     # r' - c mod 2^m = -1, 0, 1 (where c mod 2^m is neither 0 nor r - 1)
    out = pk(F, j + 9 + 2 * p)
    return cop, (out * pow(2, m, q) + cmod - rd) % q, rd


def columns(call, field, parties, prm):
    F = FLD[field]
    q, E = F.mod, len(F.edge)
    P = range(parties)
    if call in ("fr_op_add", "fr_op_sub"):
        prs = add_pairs(field) if call == "fr_op_add" else sub_pairs(field)
        return _odd([{"a": a, "b": b} for a, b in prs])
    if call == "fr_op_mul":
        return _odd([{"a": pk(F, i), "b": pk(F, i + s)} for s in (0, 1, 4, 7) for i in range(E)])
    if call.startswith("scalar_"):
        s = scalars(field)[prm["s"]]
        vals = [(q - s) % q, s, (s + 1) % q, (s - 1) % q] + list(F.edge)
        return _odd([{"a": v} for v in vals])
    if call == "triple_local":                       # a b and the result each in every class; the result 0 is r2t = a b
        cols = []
        for j in range(2 * E):
            prod, out, b = pk(F, j), pk(F, j + 4 + j // E), nz(F, j + j // E)
            cols.append({"a": prod * F.inv(b) % q, "b": b, "r2t": (prod - out) % q})
        return _odd(cols)
    if call == "triple_finalize":                    # party 0 holds the pair itself, from its second one on (2 r - 2 first)
        prs = add_pairs(field)
        C = len(prs)
        return _odd([{"opened": prs[(j + 1) % C][1], "rt": [prs[(j + 1 + 3 * p) % C][0] for p in P]} for j in range(C)])
    if call in ("beaver_open_shares", "beaver_open_shares_paired"):
        prs = sub_pairs(field)
        C = len(prs)
        cols = []
        for j in range(C):
            da, db = [prs[(j + 3 * p) % C] for p in P], [prs[(j + 11 + 5 * p) % C] for p in P]
            col = {"a": [v[0] for v in da], "x": [v[1] for v in da], "b": [v[0] for v in db], "y": [v[1] for v in db]}
            cols.append(col if call.endswith("paired") else {k: v[0] for k, v in col.items()})
        return _odd(cols)
    if call == "beaver_finalize":
        cols = []
        for j in _bf_order(F):
            per = [_bf_column(F, j, p) for p in P]
            cols.append({"d": per[0][0], "e": per[0][1], "c": [v[2] for v in per], "x": [v[3] for v in per], "y": [v[4] for v in per]})
        return _odd(cols)
    if call == "truncpr_rdash":
        return [{"r_bits": [_bits_column(F, j, p, prm["m"]) for p in P]} for j in range(E + 2)]
    if call == "truncpr_open_share":                 # the result in every class; then the three operand terms r - 1 (2^(k-1) is what k makes it)
        k, m = prm["k"], prm["m"]
        inv2m, half = F.inv(pow(2, m, q)), pow(2, k - 1, q)
        cols = []
        for j in range(E):
            a, rd, out = pk(F, j + 2), pk(F, j + 5), pk(F, j)
            cols.append({"a": a, "r_dash": rd, "r_int": (out - a - half - rd) * inv2m % q})
        cols.append({"a": q - 1, "r_dash": q - 1, "r_int": (q - 1) * inv2m % q})
        return _odd(cols)
    if call == "fpmul_middle":
        k, m = prm["k"], prm["m"]                    # r_int is solved so that the share TruncPr opens is in every class as well
        inv2m, half = F.inv(pow(2, m, q)), pow(2, k - 1, q)
        cols = []
        for j in _bf_order(F):
            per = [_bf_column(F, j, p) for p in P]
            bits = [_bits_column(F, j % (E + 2), p, m) for p in P]
            rint = [(pk(F, j + 6 + 7 * p) - per[p][5] - half - sum(b << t for t, b in enumerate(bits[p]))) * inv2m % q for p in P]
            cols.append({"d": per[0][0], "e": per[0][1], "c": [v[2] for v in per], "x": [v[3] for v in per], "y": [v[4] for v in per],
                         "r_bits": bits, "r_int": rint})
        return _odd(cols)
    if call == "truncpr_finalize":
        cols = []
        for j in range(E + 6):
            per = [_fin_column(F, j, p, prm["m"]) for p in P]
            cols.append({"c_open": per[0][0], "a": [v[1] for v in per], "r_dash": [v[2] for v in per]})
        return _odd(cols)
    raise KeyError(call)


# ---- a case: the columns in the arrays' layout --------------------------------------------------------------------------------------------
PUBLIC = ("opened", "d", "e", "c_open")


class Tiled:
    """base[i % len(base)] for i < N, without the copy"""

    def __init__(self, base, N):
        self.base, self.N = base, N

    def __len__(self):
        return self.N

    def __getitem__(self, i):
        if not 0 <= i < self.N:
            raise IndexError(i)
        return self.base[i % len(self.base)]


class Case:
    """call, field, N, parties, prm; C: the distinct columns it holds (min(N, all of them)); base: {name: array over those C columns}
    in the call's layout ([C], [parties][C], r_bits [parties][m][C])"""

    def __init__(self, call, field, N, parties, prm):
        self.call, self.field, self.N, self.parties, self.prm = call, field, N, parties, dict(prm)
        cols = columns(call, field, parties, prm)
        self.period = len(cols)
        cols = cols[:N]
        self.C = len(cols)
        self.base = {}
        for nm in cols[0]:
            if nm == "r_bits":
                self.base[nm] = [[[c[nm][p][j] for c in cols] for j in range(prm["m"])] for p in range(parties)]
            elif isinstance(cols[0][nm], list):
                self.base[nm] = [[c[nm][p] for c in cols] for p in range(parties)]
            else:
                self.base[nm] = [c[nm] for c in cols]

    def claims(self):
        """does the shape hold every column, and with it every (site, class) of SITE_TABLE?"""
        return self.N >= self.period

    def arrays(self, tiled=False):
        """the inputs over all N elements: lists, or Tiled views for the large shapes"""
        def widen(a):
            if isinstance(a[0], list):
                return [widen(x) for x in a]
            return Tiled(a, self.N) if tiled else [a[i % self.C] for i in range(self.N)]
        return {nm: (widen(a) if a and a[0] != [] else a) for nm, a in self.base.items()}


_cases = {}


def case(call, field, N, parties, prm=None):
    key = (call, field, N, parties, tuple(sorted((prm or {}).items())))
    if key not in _cases:
        _cases[key] = Case(call, field, N, parties if call in PARTY_CALLS else 1, prm or {})
    return _cases[key]


def run_model(c, ins, mut=None, N=None, elems=None):
    """the model's outputs {name: array} of a case's call on `ins` (N elements; the case's base: N = C); elems: only those elements, for
    the two calls of the large shapes"""
    f, prm, N = c.field, c.prm, c.C if N is None else N
    call = c.call
    if call.startswith("fr_op_"):
        return {"out": M.fr_op(f, call[6:], ins["a"], ins["b"], mut)}
    if call.startswith("scalar_"):
        return {"out": M.fr_op_scalar(f, call[7:], ins["a"], scalars(f)[prm["s"]], mut)}
    if call == "triple_local":
        return {"out": M.triple_local(f, ins["a"], ins["b"], ins["r2t"], mut)}
    if call == "triple_finalize":
        return {"c": M.triple_finalize_parties(f, ins["rt"], ins["opened"], mut)}
    if call == "beaver_open_shares":
        d, e = M.beaver_open_shares(f, ins["a"], ins["b"], ins["x"], ins["y"], mut)
        return {"d_sh": d, "e_sh": e}
    if call == "beaver_open_shares_paired":
        return {"de": M.beaver_open_shares_paired(f, ins["a"], ins["b"], ins["x"], ins["y"], mut)}
    if call == "beaver_finalize":
        return {"z": M.beaver_finalize_parties(f, ins["c"], ins["x"], ins["y"], ins["d"], ins["e"], mut, elems)}
    if call == "truncpr_rdash":
        return {"r_dash": M.truncpr_rdash_parties(ins["r_bits"], prm["m"], N, mut)}
    if call == "truncpr_open_share":
        return {"open": M.truncpr_open_share(ins["a"], ins["r_dash"], ins["r_int"], prm["k"], prm["m"], mut)}
    if call == "fpmul_middle":
        z, rd, op = M.fpmul_middle(ins["c"], ins["x"], ins["y"], ins["d"], ins["e"], ins["r_bits"], ins["r_int"], prm["k"], prm["m"], mut, elems)
        return {"z": z, "r_dash": rd, "open": op}
    if call == "truncpr_finalize":
        return {"out": M.truncpr_finalize_parties(ins["a"], ins["r_dash"], ins["c_open"], prm["m"], mut)}
    raise KeyError(call)


_expected = {}


def expected(c):
    """the true model on the case's distinct columns, computed once; element i of the shape holds column i % C of it"""
    if id(c) not in _expected:
        _expected[id(c)] = run_model(c, c.base)
    return _expected[id(c)]


# ---- what the inputs must reach -----------------------------------------------------------------------------------------------------------
_ADD_SITES = {"sum": "add_sums", "carry": "carries"}
_SUB_SITES = {"diff": "sub_diffs", "borrow_pos": "borrows_pos", "borrow_neg": "borrows_neg"}
_BF_SITES = {"e_plus_y": "sums", "prod_ey_d": "edge", "prod_x_e": "edge", "z": "edge", "lazy": "lazy_extremes"}
_RD_SITES = {"rdash": "edge", "bits_all": "full_bits"}
SITE_TABLE = {
    "fr_op_add": _ADD_SITES, "triple_finalize": _ADD_SITES,
    "fr_op_sub": _SUB_SITES,
    "beaver_open_shares": {h + k: v for h in ("d_", "e_") for k, v in _SUB_SITES.items()},
    "beaver_open_shares_paired": {h + k: v for h in ("d_", "e_") for k, v in _SUB_SITES.items()},
    "triple_local": {"prod": "edge", "out": "edge"},
    "beaver_finalize": _BF_SITES,
    "truncpr_rdash": _RD_SITES,                         # for m >= 1 (m = 0: r' is zero and there are no bit shares)
    "truncpr_open_share": {"terms": "three_max", "out": "edge"},
    "fpmul_middle": dict(_BF_SITES, open="edge", **_RD_SITES),       # the r' sites for m >= 1
    "truncpr_finalize": {"cop": "edge_and_2m", "sign": "signs", "out": "edge"},
}


def classes(field, name, prm):
    """the values of a class of SITE_TABLE"""
    F, q, nw = FLD[field], FLD[field].mod, M.NWORDS[field]
    if name == "edge_and_2m":
        return list(F.edge) + [((1 << prm["m"]) + s) % q for s in (-1, 0, 1)]
    return {"edge": F.edge, "sums": F.sums, "add_sums": (q - 1, q, q + 1, 2 * q - 2, 0), "sub_diffs": (0, -1, -(q - 1), q - 1),
            # the word boundaries a carry or borrow crosses.  Fr: out of words 0 .. 6 (2 r < 2^256: none out of word 7, whose borrow is the
            # sign).  Goldilocks: bit 32 and bit 64; the borrow out of bit 64 IS the negative sign, so it has no form without the + r
            "carries": tuple(range(7)) if field == "fr" else (0, 1), "borrows_pos": tuple(range(nw - 1)),
            "borrows_neg": tuple(range(7)) if field == "fr" else (0, 1),
            "lazy_extremes": ("c=0,products=r-1", "c=r-1,products=0"), "full_bits": (EI.MAXLIMB, q - 1), "three_max": ("a=2^m r_int=r'=r-1",),
            "signs": ("neg", "zero", "pos")}[name]


def _carries(field, a, b):
    nw, c, out = M.NWORDS[field], 0, set()
    for k in range(nw):
        c = ((a >> 32 * k & 0xFFFFFFFF) + (b >> 32 * k & 0xFFFFFFFF) + c) >> 32
        if c:
            out.add(k)
    return out


def _borrows(field, a, b):
    nw, bo, out = M.NWORDS[field], 0, set()
    for k in range(nw):
        bo = int((a >> 32 * k & 0xFFFFFFFF) - (b >> 32 * k & 0xFFFFFFFF) - bo < 0)
        if bo:
            out.add(k)
    return out


def _add(seen, field, pre, a, b):
    seen.setdefault(pre + "sum", set()).add(a + b)
    seen.setdefault(pre + "carry", set()).update(_carries(field, a, b))


def _sub(seen, field, pre, a, b):
    seen.setdefault(pre + "diff", set()).add(a - b)
    seen.setdefault(pre + ("borrow_pos" if a >= b else "borrow_neg"), set()).update(_borrows(field, a, b))


def _flat(a):
    return [v for row in a for v in row] if a and isinstance(a[0], list) else list(a)


def sites(c):
    """{site: the values it takes over every (party, element)} of a case, from its arrays alone"""
    F, q, B, prm, C = FLD[c.field], FLD[c.field].mod, c.base, c.prm, c.C
    seen = {}
    put = lambda nm, v: seen.setdefault(nm, set()).add(v)      # noqa: E731
    P = range(c.parties)
    if c.call in ("fr_op_add", "fr_op_sub"):
        for a, b in zip(B["a"], B["b"]):
            (_add if c.call == "fr_op_add" else _sub)(seen, c.field, "", a, b)
    elif c.call == "triple_finalize":
        for p in P:
            for i in range(C):
                _add(seen, c.field, "", B["rt"][p][i], B["opened"][i])
    elif c.call in ("beaver_open_shares", "beaver_open_shares_paired"):
        for a, x, b, y in zip(*(_flat(B[nm]) for nm in ("a", "x", "b", "y"))):
            _sub(seen, c.field, "d_", a, x), _sub(seen, c.field, "e_", b, y)
    elif c.call == "triple_local":
        for a, b, r in zip(B["a"], B["b"], B["r2t"]):
            put("prod", a * b % q), put("out", (a * b - r) % q)
    elif c.call == "truncpr_open_share":
        for a, rd, ri in zip(B["a"], B["r_dash"], B["r_int"]):
            s = ri * pow(2, prm["m"], q) % q
            put("out", (a + pow(2, prm["k"] - 1, q) + s + rd) % q)
            if a == s == rd == q - 1:
                put("terms", "a=2^m r_int=r'=r-1")
    elif c.call == "truncpr_finalize":
        m = prm["m"]
        for p in P:
            for i in range(C):
                cop, rd = B["c_open"][i], B["r_dash"][p][i]
                cmod = F.S.mod_pow_2_from_field(cop, m)
                put("cop", cop), put("sign", "neg" if rd < cmod else "pos" if rd > cmod else "zero")
                put("out", (B["a"][p][i] - (cmod - rd)) * F.inv(pow(2, m, q)) % q)
    if c.call in ("beaver_finalize", "fpmul_middle"):
        for p in P:
            for i in range(C):
                d, e, cc, x, y = B["d"][i], B["e"][i], B["c"][p][i], B["x"][p][i], B["y"][p][i]
                p1, p2 = (e + y) * d % q, x * e % q
                put("e_plus_y", e + y), put("prod_ey_d", p1), put("prod_x_e", p2), put("z", (cc - p1 - p2) % q)
                if (cc, p1, p2) in ((0, q - 1, q - 1), (q - 1, 0, 0)):
                    put("lazy", "c=0,products=r-1" if cc == 0 else "c=r-1,products=0")
                if c.call == "fpmul_middle":
                    rd = sum(B["r_bits"][p][j][i] << j for j in range(prm["m"]))
                    put("open", (cc - p1 - p2 + pow(2, prm["k"] - 1, q) + B["r_int"][p][i] * pow(2, prm["m"], q) + rd) % q)
    if c.call in ("truncpr_rdash", "fpmul_middle"):
        m = prm["m"]
        for p in P:
            for i in range(C):
                bits = [B["r_bits"][p][j][i] for j in range(m)]
                put("rdash", sum(b << j for j, b in enumerate(bits)) % q)
                if m and len(set(bits)) == 1:
                    put("bits_all", bits[0])
    return seen


def missing_pairs(c):
    """the (site, value) pairs of SITE_TABLE that no (party, element) of the case reaches"""
    table = SITE_TABLE.get(c.call, {})
    if c.prm.get("m") == 0:
        table = {k: v for k, v in table.items() if k not in _RD_SITES}
    seen = sites(c)
    return [(nm, v) for nm, cls in table.items() for v in classes(c.field, cls, c.prm) if v not in seen.get(nm, ())]
