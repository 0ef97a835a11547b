"""The element-wise share kernels (csrc/kernels_elem.hpp) against tests/elem_model.py on the inputs of tests/elem_inputs.py, byte for byte:
every device call, over Fr (u29 and sat32) and Goldilocks, at one, two and three element blocks with party counts that do and do not
divide the block count, and -- k_beaver_finalize and k_fpmul_middle -- on both sides of N = 2^16, from where the thread loops over the
parties.  Outputs carry 64 guard elements and are prefilled with a marker; inputs are read back.  Nothing here has a tolerance.

The refusals (a null buffer, parties out of range, an N whose block count does not fit a grid dimension, the other field's context)
answer with an error code and write nothing."""
import time

import numpy as np
import pytest

from __graft_entry__ import load_package
from tests import elem_inputs as X
from tests import elem_model as M

pytestmark = pytest.mark.gpu
LIMIT = 60.0    # seconds a device call may take before the session is ended
MARK = 0x5C
GUARD = 64      # elements behind every output
ENGINES = [("fr", "u29"), ("fr", "sat32"), ("goldilocks", None)]
INVALID, TYPE_MISMATCH = 4, 5
INPUTS = {"fr_op": ("a", "b"), "scalar": ("a",), "triple_local": ("a", "b", "r2t"), "triple_finalize": ("rt", "opened"),
          "beaver_open_shares": ("a", "b", "x", "y"), "beaver_open_shares_paired": ("a", "b", "x", "y"), "beaver_finalize": ("c", "x", "y", "d", "e"),
          "truncpr_rdash": ("r_bits",), "truncpr_open_share": ("a", "r_dash", "r_int"), "fpmul_middle": ("c", "x", "y", "d", "e", "r_bits", "r_int"),
          "truncpr_finalize": ("a", "r_dash", "c_open")}
OUTPUTS = {"fr_op": ("out",), "scalar": ("out",), "triple_local": ("out",), "triple_finalize": ("c",), "beaver_open_shares": ("d_sh", "e_sh"),
           "beaver_open_shares_paired": ("de",), "beaver_finalize": ("z",), "truncpr_rdash": ("r_dash",), "truncpr_open_share": ("open",),
           "fpmul_middle": ("z", "r_dash", "open"), "truncpr_finalize": ("out",)}
SINGLE_FORMS = ("triple_finalize", "beaver_finalize", "truncpr_rdash", "truncpr_finalize")


def family(call):
    return "fr_op" if call.startswith("fr_op_") else "scalar" if call.startswith("scalar_") else call


@pytest.fixture(scope="module")
def pkg():
    return load_package()


@pytest.fixture(scope="module")
def stream():
    torch = pytest.importorskip("torch")
    return torch.cuda.Stream(device=torch.device("cuda", 0))


@pytest.fixture(scope="module")
def engines(pkg):
    made = {}

    def get(key):
        if key not in made:
            made[key] = pkg.Engine(0, impl=key[1], field=key[0])
        return made[key]
    yield get
    for e in made.values():
        e.close()


def wait(stream, what):
    """the stream's work so far, under a time limit"""
    import torch
    ev = torch.cuda.Event()
    ev.record(stream)
    t0 = time.monotonic()
    while not ev.query():
        if time.monotonic() - t0 > LIMIT:
            pytest.exit(f"{what}: the device call did not finish within {LIMIT} s", returncode=3)
        time.sleep(0.0002)


def tile(field, nested, N):
    """the model's (or the inputs') array over the distinct columns as the device array over N elements: element i is column i % C"""
    F = X.FLD[field]
    if not nested or nested[0] == []:
        return np.zeros(0, dtype=np.uint64)
    arr = F.arr(nested)
    ax = arr.ndim - 1 - len(F.tail)
    return np.ascontiguousarray(np.take(arr, np.arange(N) % arr.shape[ax], axis=ax))


class Bufs:
    """the device buffers of one call: inputs with their host copies, outputs with a guard behind them, all marked before the call"""

    def __init__(self, eng, stream):
        self.eng, self.stream, self.s = eng, stream, stream.cuda_stream
        self.ptr, self.host, self.elems, self.marks = {}, {}, {}, []

    def put(self, name, arr):
        self.host[name] = np.ascontiguousarray(arr)
        self.ptr[name] = self.eng.dev_alloc(max(arr.nbytes, 16))
        if arr.nbytes:
            self.eng.h2d(self.ptr[name], self.host[name], self.s)

    def out(self, name, elems):
        self.elems[name] = elems
        nbytes = (elems + GUARD) * self.eng.ebytes
        self.ptr[name] = self.eng.dev_alloc(nbytes)
        self.mark(name)

    def mark(self, name):
        self.marks.append(np.full((self.elems[name] + GUARD) * self.eng.ebytes, MARK, dtype=np.uint8))      # alive until the copy has run
        self.eng.h2d(self.ptr[name], self.marks[-1], self.s)

    def read(self, name):
        got = np.zeros((self.elems[name] + GUARD) * self.eng.ebytes, dtype=np.uint8)
        self.eng.d2h(got, self.ptr[name], self.s)
        wait(self.stream, "download")
        return got

    def check_out(self, name, want, what):
        got, n = self.read(name), self.elems[name] * self.eng.ebytes
        want = np.ascontiguousarray(want).view(np.uint8).reshape(-1)
        assert want.size == n, (name, what)
        bad = np.flatnonzero(got[:n] != want)
        assert bad.size == 0, (what, name, "first differing element", int(bad[0]) // self.eng.ebytes, "of", self.elems[name])
        assert (got[n:] == MARK).all(), (what, name, "guard written")

    def check_untouched(self, what):
        for name in self.elems:
            assert (self.read(name) == MARK).all(), (what, name, "written by a call that was refused")

    def check_inputs(self, what):
        for name, arr in self.host.items():
            if arr.nbytes:
                got = np.zeros_like(arr)
                self.eng.d2h(got, self.ptr[name], self.s)
                wait(self.stream, "download")
                assert np.array_equal(got, arr), (what, name, "input changed")

    def close(self):
        for p in self.ptr.values():
            self.eng.dev_free(p)


def invoke(eng, call, prm, p, N, parties, s, single=False):
    """the device call of `call` on the pointers p (a name -> device pointer; 0: null)"""
    F = X.FLD[eng.field]
    fam = family(call)
    if fam == "fr_op":
        return eng.dev_fr_op(call[6:], p["a"], p["b"], N, p["out"], s)
    if fam == "scalar":
        return eng.dev_fr_op_scalar(call[7:], p["a"], F.arr([X.scalars(eng.field)[prm["s"]]]), N, p["out"], s)
    ptrs = [p[nm] for nm in INPUTS[fam] + OUTPUTS[fam]]
    extra = {"truncpr_rdash": ("m",), "truncpr_open_share": ("k", "m"), "truncpr_finalize": ("m",)}.get(call, ())
    extra = tuple(prm[k] for k in extra)
    if call in ("triple_local", "beaver_open_shares", "truncpr_open_share") or single:
        return eng.dev_elem(call, ptrs, N, extra=extra, stream=s)
    if call == "beaver_open_shares_paired":
        return eng.dev_beaver_open_shares_paired(*ptrs[:4], N, parties, ptrs[4], stream=s)
    if call == "fpmul_middle":
        return eng.dev_fpmul_middle(*ptrs[:7], prm["k"], prm["m"], N, parties, *ptrs[7:], stream=s)
    return eng.dev_elem_parties(call, ptrs, N, parties, extra=extra, stream=s)


def prepare(eng, stream, c, party=None):
    """the case's inputs uploaded and its outputs marked; party: that party's slice alone (a one-party call).  -> (Bufs, expected arrays)"""
    b = Bufs(eng, stream)
    fam = family(c.call)
    pick = (lambda nm, a: a) if party is None else (lambda nm, a: a if nm in X.PUBLIC or c.call not in X.PARTY_CALLS else a[party:party + 1])
    for nm in INPUTS[fam]:
        b.put(nm, tile(c.field, pick(nm, c.base[nm]), c.N))
    want = {nm: tile(c.field, pick(nm, a), c.N) for nm, a in X.expected(c).items()}
    for nm in OUTPUTS[fam]:
        b.out(nm, want[nm].size // (4 if c.field == "fr" else 1))
    return b, want


def run_case(eng, stream, c, party=None, single=False, null_rbits=False):
    what = (c.call, c.field, c.N, c.parties, c.prm, party, single)
    b, want = prepare(eng, stream, c, party)
    try:
        p = dict(b.ptr, r_bits=0) if null_rbits else b.ptr
        rc = invoke(eng, c.call, c.prm, p, c.N, 1 if party is not None else c.parties, b.s, single)
        wait(stream, str(what))
        assert rc == 0, (what, eng.last_error())
        for nm in OUTPUTS[family(c.call)]:
            b.check_out(nm, want[nm], what)
        b.check_inputs(what)
    finally:
        b.close()


def calls_of(field):
    return [c for c in X.CALLS if field in X.fields_of(c)]


def name(v):
    return str(v) if isinstance(v, (int, str)) else "-".join(str(x) for x in v if x)


# the truncpr_* calls and fpmul_middle exist over Fr alone
KEY_CALLS = [(key, call) for key in ENGINES for call in calls_of(key[0])]
KEY_SINGLE = [(key, call) for key, call in KEY_CALLS if call in SINGLE_FORMS]


# ---- every call at every grid-row shape ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", X.GRID_SHAPES, ids=lambda s: f"N{s[0]}x{s[1]}")
@pytest.mark.parametrize("key,call", KEY_CALLS, ids=name)
def test_call_equals_model(engines, stream, key, call, shape):
    for prm in X.params_of(call):
        run_case(engines(key), stream, X.case(call, key[0], *shape, prm))


@pytest.mark.parametrize("key,call", KEY_SINGLE, ids=name)
def test_single_party_forms_equal_model(engines, stream, key, call):
    """hbmpc_dev_<call> and hbmpc_dev_<call>_parties with parties = 1, on party p's slice of a party-batched case: the model's slice"""
    for N, parties in ((257, 2), (513, 5)):
        for prm in X.params_of(call):
            c = X.case(call, key[0], N, parties, prm)
            for party in (0, parties - 1):
                run_case(engines(key), stream, c, party, single=True)
                run_case(engines(key), stream, c, party, single=False)


def test_rdash_without_bits(engines, stream):
    """m = 0: r_bits may be null and r' is all zeros (the model's)"""
    for key in ENGINES[:2]:
        for call, prm in (("truncpr_rdash", {"m": 0}), ("fpmul_middle", {"k": 32, "m": 0})):
            c = X.case(call, "fr", 257, 2, prm)
            assert not np.any(tile("fr", X.expected(c)["r_dash"], c.N))
            run_case(engines(key), stream, c, null_rbits=True)


# ---- the in-thread party loop ----------------------------------------------------------------------------------------------------------------
IN_THREAD = [(key, N) for key in (ENGINES[0], ENGINES[2]) for N, _ in X.IN_THREAD_SHAPES] + [(ENGINES[1], 65536)]


@pytest.mark.parametrize("key,N", IN_THREAD, ids=name)
def test_beaver_finalize_in_thread(engines, stream, key, N):
    assert (N >= M.IN_THREAD_N) == (N >= 65536)
    run_case(engines(key), stream, X.case("beaver_finalize", key[0], N, 3))


@pytest.mark.parametrize("key,N,m", [(ENGINES[0], N, m) for N, _ in X.IN_THREAD_SHAPES for _, m in X.FPMUL_KM] + [(ENGINES[1], 65536, 13)],
                         ids=name)
def test_fpmul_middle_in_thread(engines, stream, key, N, m):
    """the three outputs equal the model, and equal beaver_finalize_parties + truncpr_rdash_parties + truncpr_open_share on the same inputs"""
    eng, parties, k = engines(key), 3, 32
    c = X.case("fpmul_middle", "fr", N, parties, {"k": k, "m": m})
    what = ("fpmul_middle", key, N, m)
    b, want = prepare(eng, stream, c)
    try:
        p = b.ptr
        assert invoke(eng, "fpmul_middle", c.prm, p, N, parties, b.s) == 0, eng.last_error()
        wait(stream, str(what))
        for nm in ("z", "r_dash", "open"):
            b.check_out(nm, want[nm], what)
            b.mark(nm)
        assert eng.dev_elem_parties("beaver_finalize", [p[nm] for nm in ("c", "x", "y", "d", "e", "z")], N, parties, stream=b.s) == 0
        assert eng.dev_elem_parties("truncpr_rdash", [p["r_bits"], p["r_dash"]], N, parties, extra=(m,), stream=b.s) == 0
        assert eng.dev_elem("truncpr_open_share", [p["z"], p["r_dash"], p["r_int"], p["open"]], parties * N, extra=(k, m), stream=b.s) == 0
        wait(stream, str(what) + ": the three calls")
        for nm in ("z", "r_dash", "open"):
            b.check_out(nm, want[nm], what + ("three calls",))
        b.check_inputs(what)
    finally:
        b.close()


# ---- refusals write nothing ------------------------------------------------------------------------------------------------------------------
REFUSAL_PRM = {"truncpr_rdash": {"m": 7}, "truncpr_open_share": {"k": 32, "m": 13}, "fpmul_middle": {"k": 32, "m": 7}, "truncpr_finalize": {"m": 33}}
HUGE_N = (1 << 40) + 256     # 2^32 + 1 blocks: as a 32-bit grid dimension, one block


def refusal_case(call, field):
    prm = REFUSAL_PRM.get(call, {"s": 0} if call.startswith("scalar_") else {})
    return X.case(call, field, 513, 2, prm)              # every buffer holds more than 512 elements, whatever N the refused call names


@pytest.mark.parametrize("key,call", KEY_CALLS, ids=name)
def test_refusals_write_nothing(engines, stream, key, call):
    eng = engines(key)
    c = refusal_case(call, key[0])
    parties = c.parties
    b, _ = prepare(eng, stream, c)
    try:
        def refused(p, N, par, code, text, what):
            rc = invoke(eng, call, c.prm, p, N, par, b.s)
            wait(stream, str(what))
            assert rc == code, (call, what, rc, eng.last_error())
            assert text in eng.last_error(), (call, what, eng.last_error())
            b.check_untouched((call, what))

        for nm in INPUTS[family(call)] + OUTPUTS[family(call)]:        # every pointer argument in turn
            refused(dict(b.ptr, **{nm: 0}), 3, parties, INVALID, "null buffer", ("null", nm))
        if call in X.PARTY_CALLS:
            for par in (0, 65536):
                refused(b.ptr, 3, par, INVALID, "parties", ("parties", par))
        refused(b.ptr, HUGE_N, 1, INVALID, "N out of range", "N = 2^40 + 256")
        rc = invoke(eng, call, c.prm, {nm: 0 for nm in b.ptr}, 0, parties, b.s)      # N = 0: success, null buffers and all
        wait(stream, "N = 0")
        assert rc == 0, (call, eng.last_error())
        b.check_untouched((call, "N = 0"))
        b.check_inputs((call, "after the refusals"))
    finally:
        b.close()


@pytest.mark.parametrize("call", X.CALLS)
def test_other_fields_context_is_a_type_mismatch(engines, stream, call):
    """either field's call on the other field's context: TypeMismatch, nothing written"""
    for key, other in ((ENGINES[0], ENGINES[2]), (ENGINES[2], ENGINES[0])):
        if call not in calls_of(key[0]):
            continue
        eng, wrong = engines(key), engines(other)
        c = refusal_case(call, key[0])
        b, _ = prepare(eng, stream, c)
        saved = wrong._pfx
        wrong._pfx = eng._pfx                            # the entry points of `key`'s field, on the other field's context
        try:
            rc = invoke(wrong, call, c.prm, b.ptr, 3, c.parties, b.s)
            wait(stream, "type mismatch")
            assert rc == TYPE_MISMATCH, (call, key, rc, wrong.last_error())
            b.check_untouched((call, "type mismatch"))
        finally:
            wrong._pfx = saved
            b.close()
