"""The element-wise share kernels (csrc/kernels_elem.hpp, launched from csrc/tu_elem.hip) in plain Python integers.

Every call of that family is restated here per field ("fr", "goldilocks") in the array layout of the device calls: per-party
arrays [parties][N], public operands [N], r_bits [parties][m][N], the paired opens [parties][2][N]; the single-party calls take
[N].  Nothing here imports the library or the C oracle; the moduli come from oracle/spec.py and oracle/spec_gl.py, and
tests/test_elem_inputs.py shows that the functions agree with that specification.

Additions and subtractions go through add_mod / sub_mod, which work as raw_add_mod / raw_sub_mod do: a carry (borrow) chain over
the stored 32-bit words (eight for Fr, two for Goldilocks, whose sum carries out of bit 64), one comparison with the modulus, one
conditional correction.  The party-indexed calls walk the launch grid: blocks of 256 lanes, the linear block id re-read as
(element block, party) with the party fastest (HB_GID / HB_PID).

`mut` switches on ONE deliberate mistake (MUTATIONS); tests/test_elem_inputs.py shows with them that the inputs of
tests/elem_inputs.py tell a subtly wrong kernel from a right one.  No mutated kernel exists.  A cell that a mutant never writes is
None (the GPU tests prefill their outputs with a marker byte); a read past the end of an array gives 0.

The mutations, by name:
  add_gt                 add subtracts the modulus only when the sum is GREATER than it (a + b = r comes out as r)
  add_carry_drop_K       add loses the carry out of stored word K (Fr: K = 0 .. 6; Goldilocks: 0 = bit 32, 1 = bit 64)
  sub_borrow_drop_K      sub loses the borrow out of stored word K (likewise; Goldilocks' K = 1 is the borrow that asks for + r)
  sub_no_addback         sub omits the + r of a negative difference
  add_reduce_twice       add's conditional subtraction takes 2 r
  sub_addback_twice      sub's add-back gives 2 r
  ey_is_y                finalize_mul's e + y taken as y
  ex_party0              e x taken with party 0's x for every party
  public_by_ip           a public operand indexed [party * N + i] instead of [i]
  remap_swapped          the linear block id re-read with the roles swapped: element block = id % parties, party = id / parties
  rbits_m_major          r_bits read as [m][parties][N]
  paired_pair_major      the paired opens written [2][parties][N]
  mask_off_by_one        c mod 2^m keeps m + 1 bits
  wide_m_wrapped         m >= 256 keeps m & 255 bits.  (Keeping 255 bits instead cannot be told from the true kernel by any canonical
                         input, since r < 2^255; the wrapped width is the nearest mistake that can.)
  half_is_2k             2^(k-1) taken as 2^k
  rdash_first_fold_only  r' stops at the first six terms: the fold of MAX_DOT_TERMS loses the accumulator
"""
from oracle import spec as S
from oracle import spec_gl

MOD = {"fr": S.R_MOD, "goldilocks": spec_gl.P}
NWORDS = {"fr": 8, "goldilocks": 2}
BLOCK = 256                 # lanes per workgroup (tu_elem.hip)
IN_THREAD_N = 1 << 16       # from here up k_beaver_finalize and k_fpmul_middle loop over the parties inside the thread
MAX_DOT_TERMS = 6
FR_ONLY = ("truncpr_rdash", "truncpr_open_share", "fpmul_middle", "truncpr_finalize")

_WORD_MUTS = tuple(f"add_carry_drop_{k}" for k in range(7)) + tuple(f"sub_borrow_drop_{k}" for k in range(7))
MUTATIONS = ("add_gt",) + _WORD_MUTS + ("sub_no_addback", "add_reduce_twice", "sub_addback_twice", "ey_is_y", "ex_party0", "public_by_ip",
                                        "remap_swapped", "rbits_m_major", "paired_pair_major", "mask_off_by_one", "wide_m_wrapped", "half_is_2k",
                                        "rdash_first_fold_only")
_ADD = {"add_gt", "add_reduce_twice"} | {m for m in _WORD_MUTS if m.startswith("add")}
_SUB = {"sub_no_addback", "sub_addback_twice"} | {m for m in _WORD_MUTS if m.startswith("sub")}
# the calls whose restatement a mutation changes (the adds and subtractions inside the multiplying calls go through add_mod / sub_mod too)
_ADD_CALLS = ("fr_op_add", "scalar_add", "triple_finalize", "truncpr_open_share", "fpmul_middle", "truncpr_finalize")
_SUB_CALLS = ("fr_op_sub", "scalar_sub", "scalar_rsub", "triple_local", "beaver_open_shares", "beaver_open_shares_paired", "beaver_finalize",
              "fpmul_middle", "truncpr_finalize")
MUTATION_CALLS = dict({m: _ADD_CALLS for m in _ADD}, **{m: _SUB_CALLS for m in _SUB})
MUTATION_CALLS.update({
    "ey_is_y": ("beaver_finalize", "fpmul_middle"), "ex_party0": ("beaver_finalize", "fpmul_middle"),
    "public_by_ip": ("triple_finalize", "beaver_finalize", "fpmul_middle", "truncpr_finalize"),
    "remap_swapped": ("triple_finalize", "beaver_open_shares_paired", "truncpr_rdash", "truncpr_finalize"),
    "rbits_m_major": ("truncpr_rdash", "fpmul_middle"), "paired_pair_major": ("beaver_open_shares_paired",),
    "mask_off_by_one": ("truncpr_finalize",), "wide_m_wrapped": ("truncpr_finalize",), "half_is_2k": ("truncpr_open_share", "fpmul_middle"),
    "rdash_first_fold_only": ("truncpr_rdash", "fpmul_middle")})
# truncpr_finalize multiplies its sum by 2^-m: a value that is r too large, which is all that a doubled add-back or a sum of exactly r
# left standing amounts to, is reduced there
MUTATION_CALLS["sub_addback_twice"] = tuple(c for c in _SUB_CALLS if c != "truncpr_finalize")
MUTATION_CALLS["add_gt"] = tuple(c for c in _ADD_CALLS if c != "truncpr_finalize")
assert set(MUTATION_CALLS) == set(MUTATIONS)


def applies(mut, field):
    """does the mutation exist for the field?  Goldilocks has two stored words and no TruncPr"""
    if mut in _WORD_MUTS:
        return int(mut.rsplit("_", 1)[1]) < NWORDS[field] - (field == "fr")
    return field == "fr" or any(c not in FR_ONLY for c in MUTATION_CALLS[mut])


# ---- the stored-word add and subtract ------------------------------------------------------------------------------------------------------
def _split(v, nw):
    return [v >> 32 * k & 0xFFFFFFFF for k in range(nw)]


def add_mod(field, a, b, mut=None):
    """a + b mod q of canonical a, b: the carry chain over the stored words, then the conditional subtraction"""
    q, nw = MOD[field], NWORDS[field]
    drop = int(mut.rsplit("_", 1)[1]) if mut and mut.startswith("add_carry_drop_") else -1
    s, c = 0, 0
    for k, (x, y) in enumerate(zip(_split(a, nw), _split(b, nw))):
        w = x + y + c
        s |= (w & 0xFFFFFFFF) << 32 * k
        c = 0 if k == drop else w >> 32
    s |= c << 32 * nw                             # Fr: never set (2 r < 2^256); Goldilocks: bit 64 of the sum
    if s > q if mut == "add_gt" else s >= q:
        s -= 2 * q if mut == "add_reduce_twice" else q
    return s % (1 << 32 * nw)


def sub_mod(field, a, b, mut=None):
    """a - b mod q of canonical a, b: the borrow chain over the stored words, + r where the last borrow is set"""
    q, nw = MOD[field], NWORDS[field]
    drop = int(mut.rsplit("_", 1)[1]) if mut and mut.startswith("sub_borrow_drop_") else -1
    d, bo = 0, 0
    for k, (x, y) in enumerate(zip(_split(a, nw), _split(b, nw))):
        w = x - y - bo
        d |= (w & 0xFFFFFFFF) << 32 * k
        bo = 0 if k == drop else int(w < 0)
    if bo and mut != "sub_no_addback":
        d += 2 * q if mut == "sub_addback_twice" else q
    return d % (1 << 32 * nw)


# ---- the launch grid -----------------------------------------------------------------------------------------------------------------------
def _written(N, parties, mut):
    """the (party, element) cells a party-indexed launch of grid (blocks, parties) writes"""
    gx = (N + BLOCK - 1) // BLOCK
    cells = set()
    for lin in range(gx * parties):
        blk, p = (lin % parties, lin // parties) if mut == "remap_swapped" else (lin // parties, lin % parties)
        if p < parties:                           # (a party past the last one writes past the buffers: nothing the model keeps)
            cells.update((p, i) for i in range(blk * BLOCK, min((blk + 1) * BLOCK, N)))
    return cells


def _grid(N, parties, mut, fn):
    """[parties][N] of fn(p, i) over the cells the launch writes"""
    if mut != "remap_swapped":
        return [[fn(p, i) for i in range(N)] for p in range(parties)]
    cells = _written(N, parties, mut)
    return [[fn(p, i) if (p, i) in cells else None for i in range(N)] for p in range(parties)]


def _pub(arr, p, i, N, mut):
    """a public operand's element i as party p's thread reads it"""
    if mut != "public_by_ip":
        return arr[i]
    return arr[p * N + i] if p * N + i < len(arr) else 0


# ---- share (+, -, *) share, share (+, -, *) element ----------------------------------------------------------------------------------------
def fr_op(field, op, a, b, mut=None):
    q = MOD[field]
    f = {"add": lambda x, y: add_mod(field, x, y, mut), "sub": lambda x, y: sub_mod(field, x, y, mut), "mul": lambda x, y: x * y % q}[op]
    return [f(x, y) for x, y in zip(a, b)]


def fr_op_scalar(field, op, a, s, mut=None):
    q = MOD[field]
    f = {"add": lambda x: add_mod(field, x, s, mut), "sub": lambda x: sub_mod(field, x, s, mut), "mul": lambda x: x * s % q,
         "rsub": lambda x: sub_mod(field, s, x, mut)}[op]
    return [f(x) for x in a]


# ---- triple generation ---------------------------------------------------------------------------------------------------------------------
def triple_local(field, a, b, r2t, mut=None):
    q = MOD[field]
    return [sub_mod(field, x * y % q, r, mut) for x, y, r in zip(a, b, r2t)]


def triple_finalize_parties(field, rt, opened, mut=None):
    """rt [parties][N], opened [N] -> [parties][N]"""
    parties, N = len(rt), len(opened)
    return _grid(N, parties, mut, lambda p, i: add_mod(field, rt[p][i], _pub(opened, p, i, N, mut), mut))


def triple_finalize(field, rt, opened, mut=None):
    return triple_finalize_parties(field, [rt], opened, mut)[0]


# ---- Beaver multiplication -----------------------------------------------------------------------------------------------------------------
def beaver_open_shares(field, a, b, x, y, mut=None):
    return [sub_mod(field, p, q, mut) for p, q in zip(a, x)], [sub_mod(field, p, q, mut) for p, q in zip(b, y)]


def beaver_open_shares_paired(field, a, b, x, y, mut=None):
    """[parties][N] each -> [parties][2][N]: a - x, then b - y, of each party side by side"""
    parties, N = len(a), len(a[0])
    d = _grid(N, parties, mut, lambda p, i: sub_mod(field, a[p][i], x[p][i], mut))
    e = _grid(N, parties, mut, lambda p, i: sub_mod(field, b[p][i], y[p][i], mut))
    flat = [None] * (2 * parties * N)
    for p in range(parties):
        for h, src in enumerate((d, e)):
            base = (h * parties + p) * N if mut == "paired_pair_major" else (p * 2 + h) * N
            flat[base:base + N] = src[p]
    return [[flat[(p * 2 + h) * N:(p * 2 + h + 1) * N] for h in range(2)] for p in range(parties)]


def _finalize_mul(field, c, x, y, d, e, p, i, N, mut):
    q = MOD[field]
    dv, ev = _pub(d, p, i, N, mut), _pub(e, p, i, N, mut)
    dey = ((0 if mut == "ey_is_y" else ev) + y[p][i]) * dv % q      # the sum e + y stays unreduced in front of the product
    ex = x[0 if mut == "ex_party0" else p][i] * ev % q
    return sub_mod(field, sub_mod(field, c[p][i], dey, mut), ex, mut)


def beaver_finalize_parties(field, c, x, y, d, e, mut=None, elems=None):
    """z = c - d (e + y) - e x;  c, x, y [parties][N], d, e [N].  The kernel takes its party from the grid row or from its own loop
    (N >= IN_THREAD_N): the same cells either way, never through the remap of the other party-indexed kernels.
    elems: only these elements of every party (the large shapes), in that order"""
    parties, N = len(c), len(d)
    return [[_finalize_mul(field, c, x, y, d, e, p, i, N, mut) for i in (range(N) if elems is None else elems)] for p in range(parties)]


def beaver_finalize(field, c, x, y, d, e, mut=None):
    return beaver_finalize_parties(field, [c], [x], [y], d, e, mut)[0]


# ---- TruncPr -------------------------------------------------------------------------------------------------------------------------------
def _rdash(r_bits, parties, m, N, p, i, mut):
    q = MOD["fr"]
    terms = min(m, MAX_DOT_TERMS) if mut == "rdash_first_fold_only" else m
    if mut != "rbits_m_major":
        return sum(r_bits[p][j][i] << j for j in range(terms)) % q
    flat = lambda f: r_bits[f // (m * N)][f // N % m][f % N]      # noqa: E731  the array as it lies in memory
    return sum(flat((j * parties + p) * N + i) << j for j in range(terms)) % q


def truncpr_rdash_parties(r_bits, m, N, mut=None):
    """r_bits [parties][m][N] -> r' [parties][N];  m = 0: zeros"""
    parties = len(r_bits)
    return _grid(N, parties, mut, lambda p, i: _rdash(r_bits, parties, m, N, p, i, mut))


def truncpr_rdash(r_bits, m, N, mut=None):
    return truncpr_rdash_parties([r_bits], m, N, mut)[0]


def _open(a, rd, rint, k, m, mut):
    q = MOD["fr"]
    acc = add_mod("fr", a, pow(2, k if mut == "half_is_2k" else k - 1, q), mut)
    acc = add_mod("fr", acc, rint * pow(2, m, q) % q, mut)
    return add_mod("fr", acc, rd, mut)


def truncpr_open_share(a, r_dash, r_int, k, m, mut=None):
    """(a + 2^(k-1)) + (2^m r_int + r'), [N] each"""
    return [_open(x, rd, ri, k, m, mut) for x, rd, ri in zip(a, r_dash, r_int)]


def fpmul_middle(c, x, y, d, e, r_bits, r_int, k, m, mut=None, elems=None):
    """(z, r', open), [parties][N] each: beaver_finalize_parties, truncpr_rdash_parties and truncpr_open_share of every party.
    elems: only these elements of every party (the large shapes), in that order"""
    parties, N = len(c), len(d)
    el = range(N) if elems is None else elems
    z = [[_finalize_mul("fr", c, x, y, d, e, p, i, N, mut) for i in el] for p in range(parties)]
    rd = [[_rdash(r_bits, parties, m, N, p, i, mut) for i in el] for p in range(parties)]
    op = [[_open(z[p][n], rd[p][n], r_int[p][i], k, m, mut) for n, i in enumerate(el)] for p in range(parties)]
    return z, rd, op


def mod_pow_2(c, m, mut=None):
    """c mod 2^m of the canonical integer, as spec.mod_pow_2_from_field defines it for the m the library accepts (m % 8 == 0 or
    m < 256); from m = 256 on that is c itself"""
    bits = m
    if mut == "mask_off_by_one":
        bits = m + 1
    if m >= 256:
        bits = m & 255 if mut == "wide_m_wrapped" else 256
    return c & ((1 << bits) - 1)


def truncpr_finalize_parties(a, r_dash, c_open, m, mut=None):
    """(a - ((c mod 2^m) - r')) (2^m)^-1;  a, r' [parties][N], c_open [N]"""
    q = MOD["fr"]
    parties, N = len(a), len(c_open)
    inv = pow(pow(2, m, q), q - 2, q)

    def one(p, i):
        t = sub_mod("fr", r_dash[p][i], mod_pow_2(_pub(c_open, p, i, N, mut), m, mut) % q, mut)
        return add_mod("fr", t, a[p][i], mut) * inv % q
    return _grid(N, parties, mut, one)


def truncpr_finalize(a, r_dash, c_open, m, mut=None):
    return truncpr_finalize_parties([a], [r_dash], c_open, m, mut)[0]
