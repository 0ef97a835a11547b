"""PRandBit / PRandInt on the device against the restatement (tests/prandbit_ref.py), bit for bit: the RISS-to-Shamir conversion in
all its forms for Fr (both implementations) and Goldilocks, the fold with its verdicts, the finalize, both wrappers end to end, the
error codes, and the table cache."""
import math
import random

import numpy as np
import pytest

from __graft_entry__ import load_package
from tests import prandbit_ref as PR

pytestmark = pytest.mark.gpu
CONFIGS = [("fr", "u29"), ("fr", "sat32"), ("goldilocks", None)]
SHAPES = [(4, 1), (5, 1), (7, 2), (10, 3), (13, 4), (16, 5)]
_EXPECT = {}  # (field, n, t, B, seed) -> (columns, shares, shares2): both Fr implementations must give the same bytes


@pytest.fixture(scope="module")
def pkg():
    return load_package()


def engine(pkg, field, impl):
    eng = pkg.Engine(0, field=field)
    if impl:
        eng.set_impl(impl)
    return eng


def sizes(n, t):
    return [1, 63, 64, 65, t + 1, 384, 4097] + ([1 << 14] if (n, t) == (16, 5) else [])


def max_r(n):
    """the largest folded value the capacity check allows: n 2^(l+k) with k + l + 2 + ceil(log2 n) = 63"""
    return n << (61 - math.ceil(math.log2(n)))


def riss_values(n, Tn, B, seed):
    """r [Tn][B]: uniform below the capacity bound, with columns of all 0, all 1, all the largest value, all odd, all even"""
    rng = np.random.default_rng(seed)
    top = max_r(n)
    assert top < 2**62
    r = rng.integers(0, top + 1, size=(Tn, B), dtype=np.uint64)
    for col in range(min(B, 5)):
        kind = col if B >= 5 else (col + seed) % 5  # a batch too short for all five takes them in turn
        if kind == 0:
            r[:, col] = 0
        elif kind == 1:
            r[:, col] = 1
        elif kind == 2:
            r[:, col] = top
        elif kind == 3:
            r[:, col] |= np.uint64(1)
        else:
            r[:, col] &= ~np.uint64(1)
    return r


def sample(B, seed):
    """every column of a small batch; of a large one a seeded sample of 2 000 plus the first and last 64"""
    if B <= 512:
        return np.arange(B)
    rng = np.random.default_rng(seed)
    return np.unique(np.concatenate([np.arange(64), np.arange(B - 64, B), rng.choice(B, 2000, replace=False)]))


def expected(field, n, t, r, cols, key):
    if key not in _EXPECT:
        _EXPECT[key] = PR.convert_fast(PR.PRIME[field], n, t, r[:, cols])
    return _EXPECT[key]


def dev_convert(eng, r, n, t, party_ids=None, own=False, gf2=True, form=0):
    """hbmpc_[gl_]dev_riss_convert_parties through device buffers -> (rc, out [parties][B], out2 or None)"""
    Tn, B = r.shape
    parties = n if party_ids is None else len(party_ids)
    bufs = [eng.dev_alloc(max(1, x)) for x in (Tn * B * 8, parties * B * eng.ebytes, parties * B)]
    try:
        eng.h2d(bufs[0], r)
        eng.sync()
        eng.set_riss_form(form)
        rc = eng.dev_riss_convert_parties(bufs[0], n, t, B, bufs[1], bufs[2] if gf2 else 0, party_ids=party_ids, own_sets_only=own)
        eng.set_riss_form(0)
        eng.sync()
        out, out2 = eng._new((parties, B)), np.zeros((parties, B), dtype=np.uint8)
        eng.d2h(out, bufs[1])
        eng.d2h(out2, bufs[2])
        eng.sync()
        return rc, out, (out2 if gf2 else None)
    finally:
        for b in bufs:
            eng.dev_free(b)


def check(field, out, out2, want, want2, cols):
    for q in range(len(want)):
        assert PR.to_ints(out[q][cols], field) == want[q], f"party row {q}"
        if out2 is not None:
            assert [int(v) for v in out2[q][cols]] == want2[q], f"party row {q} (GF(2^8))"


@pytest.mark.parametrize("field,impl", CONFIGS)
@pytest.mark.parametrize("n,t", SHAPES)
def test_convert_all_parties(pkg, field, impl, n, t):
    eng = engine(pkg, field, impl)
    try:
        Tn = math.comb(n, t)
        for B in sizes(n, t):
            r = riss_values(n, Tn, B, seed=B + n)
            cols = sample(B, B)
            want, want2 = expected(field, n, t, r, cols, (field, n, t, B, B + n))
            rc, out, out2 = dev_convert(eng, r, n, t)
            assert rc == 0, eng.last_error()
            check(field, out, out2, want, want2, cols)
            if B in (65, 4097, 1 << 14):  # without the GF(2^8) output, and both work layouts whatever the size picks
                for form in (1, 2):
                    rc, o, o2 = dev_convert(eng, r, n, t, gf2=False, form=form)
                    assert rc == 0 and o2 is None and np.array_equal(o, out), (B, form)
                rc, o, o2 = dev_convert(eng, r, n, t, form=1 if B < 4097 else 2)
                assert rc == 0 and np.array_equal(o, out) and np.array_equal(o2, out2), B
    finally:
        eng.close()


@pytest.mark.parametrize("field,impl", CONFIGS)
@pytest.mark.parametrize("n,t", [(5, 1), (10, 3), (16, 5)])
def test_convert_party_subsets(pkg, field, impl, n, t):
    eng = engine(pkg, field, impl)
    try:
        Tn = math.comb(n, t)
        for B, ids in ((65, [n - 1, 0, 2]), (384, [3]), (4097, list(range(n - 1, -1, -1))), (7, [1, 1, 0])):
            r = riss_values(n, Tn, B, seed=B)
            cols = sample(B, 5)
            want, want2 = PR.convert_fast(PR.PRIME[field], n, t, r[:, cols], parties=ids)
            for form in (0, 1, 2):
                rc, out, out2 = dev_convert(eng, r, n, t, party_ids=ids, form=form)
                assert rc == 0, eng.last_error()
                check(field, out, out2, want, want2, cols)
    finally:
        eng.close()


@pytest.mark.parametrize("field,impl", CONFIGS)
@pytest.mark.parametrize("gf2", [True, False])
def test_convert_one_party_form(pkg, field, impl, gf2):
    """what a deployed node calls: r over the party's own C(n-1, t) sets, for every party of (7, 2) (and one of (16, 5))"""
    eng = engine(pkg, field, impl)
    try:
        for n, t, js in ((7, 2, range(7)), (16, 5, [11])):
            sets = PR.tsets(n, t)
            for j in js:
                for B in (1, t + 1, 65, 384):
                    r = riss_values(n, len(sets), B, seed=B + j)
                    own = np.ascontiguousarray(r[[k for k, T in enumerate(sets) if j not in T]])
                    assert own.shape[0] == math.comb(n - 1, t)
                    want, want2 = PR.convert_fast(PR.PRIME[field], n, t, r, parties=[j])
                    rc, out, out2 = dev_convert(eng, own, n, t, party_ids=[j], own=True, gf2=gf2)
                    assert rc == 0, eng.last_error()
                    check(field, out, out2, want, want2, np.arange(B))
    finally:
        eng.close()


@pytest.mark.parametrize("field,impl", CONFIGS)
def test_convert_many_parties(pkg, field, impl):
    """up to the supported range (255 parties in GF(2^8), 256 without it, 8128 sets): every form, with and without the GF(2^8) output,
    against the restatement on all columns for the first, the last and a middle party, and the all-parties call on the same rows"""
    eng = engine(pkg, field, impl)
    try:
        B = 65
        for n, t in ((128, 2), (37, 3), (17, 5), (255, 1), (256, 1)):
            Tn = math.comb(n, t)
            assert Tn <= PR.MAX_TSETS
            ids = [0, 1, n // 2, n - 2, n - 1]
            r = riss_values(n, Tn, B, seed=n + t)
            assert (r[:, 2] == max_r(n)).all()
            want, want2 = PR.convert_fast(PR.PRIME[field], n, t, r, parties=ids)
            rc, full, full2 = dev_convert(eng, r, n, t, gf2=n <= 255)
            assert rc == 0, eng.last_error()
            for gf2 in ((True, False) if n <= 255 else (False,)):
                for form in (0, 1, 2):
                    rc, out, out2 = dev_convert(eng, r, n, t, party_ids=ids, gf2=gf2, form=form)
                    assert rc == 0, (eng.last_error(), n, t, gf2, form)
                    check(field, out, out2, want, want2, np.arange(B))
                    assert np.array_equal(out, full[ids]) and (not gf2 or np.array_equal(out2, full2[ids])), (n, t, gf2, form)
    finally:
        eng.close()


@pytest.mark.parametrize("field,impl", CONFIGS)
def test_convert_host_pointer_form(pkg, field, impl):
    eng = engine(pkg, field, impl)
    try:
        n, t, B = 7, 2, 100
        r = riss_values(n, 21, B, seed=9)
        want, want2 = PR.convert_fast(PR.PRIME[field], n, t, r)
        rc, out, out2 = eng.riss_convert_parties(r, n, t)
        assert rc == 0, eng.last_error()
        check(field, out, out2, want, want2, np.arange(B))
        rc, out, out2 = eng.riss_convert_parties(r, n, t, party_ids=[4, 6], with_gf2=False)
        assert rc == 0 and out2 is None
        check(field, out, None, [want[4], want[6]], None, np.arange(B))
    finally:
        eng.close()


def dev_fold(eng, contrib, lk):
    n, Tn, B = contrib.shape
    bufs = [eng.dev_alloc(max(1, x)) for x in (n * Tn * B * 8, Tn * B * 8, n * Tn)]
    try:
        eng.h2d(bufs[0], contrib)
        eng.sync()
        rc = eng.dev_riss_fold(bufs[0], n, Tn, B, lk, bufs[1], bufs[2])
        eng.sync()
        sums, bad = np.zeros((Tn, B), dtype=np.uint64), np.full((n, Tn), 7, dtype=np.uint8)
        eng.d2h(sums, bufs[1])
        eng.d2h(bad, bufs[2])
        eng.sync()
        return rc, sums, bad
    finally:
        for b in bufs:
            eng.dev_free(b)


@pytest.mark.parametrize("field", ["fr", "goldilocks"])
@pytest.mark.parametrize("n,t,B,lk", [(5, 1, 300, 55), (7, 2, 1, 50), (16, 5, 257, 57), (4, 1, 4099, 59)])
def test_fold_sums_and_verdicts(pkg, field, n, t, B, lk):
    eng = engine(pkg, field, None)
    try:
        Tn = math.comb(n, t)
        rng = np.random.default_rng(n * B)
        bound = 1 << lk
        base = rng.integers(0, bound + 1, size=(n, Tn, B), dtype=np.uint64)
        # none over; one sender; several; all senders over the bound (in one set, different elements); the bound itself is allowed
        for offenders in ([], [(n - 1, Tn - 1, B - 1)], [(0, 0, 0), (2, Tn // 2, B // 2), (2, 0, B - 1)], [(s, 1 % Tn, (7 * s) % B) for s in range(n)]):
            contrib = base.copy()
            contrib[0, 0, B // 3] = bound
            for k, (s, T, i) in enumerate(offenders):
                contrib[s, T, i] = bound + 1 if k % 2 == 0 else 2**64 - 1
            rc, sums, bad = dev_fold(eng, contrib, lk)
            assert rc == 0, eng.last_error()
            want_bad = np.zeros((n, Tn), dtype=np.uint8)
            for s, T, _ in offenders:
                want_bad[s, T] = 1
            assert np.array_equal(bad, want_bad)
            assert np.array_equal(sums, contrib.sum(axis=0, dtype=np.uint64))  # exact wherever no verdict is set (wraps only under one)
            clean = [T for T in range(Tn) if not want_bad[:, T].any()]
            ref_sums, ref_bad = PR.fold([[list(map(int, contrib[s, T, :8])) for T in clean[:3]] for s in range(n)], lk)
            assert [list(map(int, sums[T, :8])) for T in clean[:3]] == ref_sums and not any(any(row) for row in ref_bad)
    finally:
        eng.close()


@pytest.mark.parametrize("impl", ["u29", "sat32"])
@pytest.mark.parametrize("parties,B", [(1, 1), (5, 300), (16, 4097)])
def test_finalize_matches_the_restatement(pkg, impl, parties, B):
    eng = engine(pkg, "fr", impl)
    try:
        rng = random.Random(parties * B)
        v = [0, 1, PR.P_GL - 1, PR.P_GL - 2, 2**32, 2**32 - 1][:B] + [rng.randrange(PR.P_GL) for _ in range(max(0, B - 6))]
        r_p = [[rng.choice([0, 1, PR.P_FR - 1, rng.randrange(PR.P_FR)]) for _ in range(B)] for _ in range(parties)]
        r_2 = [[rng.randrange(256) for _ in range(B)] for _ in range(parties)]
        want_p, want_2 = PR.finalize(v, r_p, r_2)
        rc, bp, b2 = eng.prandbit_finalize_parties(np.array(v, dtype=np.uint64), PR.rows_from_ints(r_p, "fr"), np.array(r_2, dtype=np.uint8))
        assert rc == 0, eng.last_error()
        for q in range(parties):
            assert PR.to_ints(bp[q], "fr") == want_p[q] and [int(x) for x in b2[q]] == want_2[q]
    finally:
        eng.close()


def lk_for(n, t):
    """l + k with C(n,t) n 2^(l+k) + 1 < q, so that r + b never wraps in Goldilocks (at n = 16, t = 5: 47)"""
    lk = 55
    while math.comb(n, t) * n * 2**lk + 1 >= PR.P_GL:
        lk -= 1
    return lk


@pytest.mark.parametrize("impl", ["u29", "sat32"])
@pytest.mark.parametrize("n,t", [(5, 1), (7, 2), (16, 5)])
def test_prandbit_and_prandint_end_to_end(pkg, impl, n, t):
    gl, fr = engine(pkg, "goldilocks", None), engine(pkg, "fr", impl)
    try:
        B, lk = 3 * (t + 1), lk_for(n, t)
        assert (n, t) != (16, 5) or lk == 47
        contrib, bits, b_q = PR.make_inputs(n, t, B, lk, seed=n + t)
        d = PR.prandbit(n, t, contrib, lk, b_q, fast=True)
        c_np = np.array(contrib, dtype=np.uint64)
        pb = pkg.pipelines.PRandBit(gl, fr, n, t, B)
        pb.upload_named("contrib", c_np)
        pb.upload_named("b_q", np.array(b_q, dtype=np.uint64))
        pb.run(lk)

        def outputs():
            return (pb.download_named("sums", np.uint64, (pb.Tn, B)), pb.download_named("bad", np.uint8, (n, pb.Tn)),
                    pb.download_named("r_q", np.uint64, (n, B)), pb.download_named("r_p", np.uint64, (n, B, 4)),
                    pb.download_named("r_2", np.uint8, (n, B)), pb.download_named("opened", np.uint64, (B,)),
                    pb.download_named("b_p", np.uint64, (n, B, 4)), pb.download_named("b_2", np.uint8, (n, B)))

        sums, bad, r_q, r_p, r_2, opened, b_p, b_2 = outputs()
        assert [list(map(int, row)) for row in sums] == d["sums"] and not bad.any()
        assert [int(x) for x in opened] == d["opened"]
        for j in range(n):
            assert PR.to_ints(r_q[j], "goldilocks") == d["r_q"][j] and PR.to_ints(r_p[j], "fr") == d["r_p"][j]
            assert [int(x) for x in r_2[j]] == d["r_2"][j] and [int(x) for x in b_2[j]] == d["b_2"][j]
            assert PR.to_ints(b_p[j], "fr") == d["b_p"][j]
        got = {"opened": d["opened"], "b_p": [PR.to_ints(b_p[j], "fr") for j in range(n)], "b_2": [[int(x) for x in b_2[j]] for j in range(n)]}
        vp, v2 = PR.recovered_bits(n, t, got)
        assert vp == bits and v2 == bits
        assert all(s[1] == 0 for s in pb.open_summary())
        # one sender lies in the open: the decodes' OEC path returns the same values
        pb.prepare(lk)
        Y = pb.download_named("Y", np.uint64, (n, n, pb.G))
        Y[1] ^= np.uint64(5)
        pb.upload_named("Y", Y)
        pb.finish()
        again = outputs()
        assert np.array_equal(again[5], opened) and np.array_equal(again[6], b_p) and np.array_equal(again[7], b_2)
        assert all(s[1] == 0 for s in pb.open_summary()) and pb.open_summary()[0][0] > 0
        pb.close()
        # PRandInt: any B, the same Fr shares
        Bi = B - 1
        pi = pkg.pipelines.PRandInt(fr, n, t, Bi)
        pi.upload_named("contrib", np.ascontiguousarray(c_np[:, :, :Bi]))
        pi.run(lk)
        r_pi = pi.download_named("r_p", np.uint64, (n, Bi, 4))
        assert np.array_equal(r_pi, r_p[:, :Bi]) and not pi.download_named("bad", np.uint8, (n, pi.Tn)).any()
        pi.close()
    finally:
        gl.close()
        fr.close()


def test_error_codes(pkg):
    gl, fr = engine(pkg, "goldilocks", None), engine(pkg, "fr", None)
    try:
        with pytest.raises(RuntimeError, match="ShareErrorCode 4"):  # PRandError::Incompatible
            pkg.pipelines.PRandBit(gl, fr, 7, 2, 10)
        pkg.pipelines.PRandInt(fr, 7, 2, 10).close()
        with pytest.raises(RuntimeError, match="ShareErrorCode 4"):  # 27 132 sets
            pkg.pipelines.PRandInt(fr, 19, 6, 7)
        buf = fr.dev_alloc(1 << 20)
        try:
            for eng in (gl, fr):
                assert eng.dev_riss_convert_parties(buf, 19, 6, 4, buf, 0) == 4
                assert eng.dev_riss_convert_parties(buf, 6, 2, 4, buf, 0) == 4  # n < 3t + 1
                assert eng.dev_riss_convert_parties(buf, 256, 1, 4, buf + 65536, buf + 131072) == 4  # Gf256Domain::new: n > 255
                assert eng.dev_riss_convert_parties(buf, 7, 2, 4, buf + 65536, 0, party_ids=[7]) == 4
                assert eng.dev_riss_convert_parties(buf, 7, 2, 4, buf + 65536, 0, party_ids=[1, 2], own_sets_only=True) == 4
                # k + l + 2 + ceil(log2 n) >= 64: PRandError::SurpassedFieldCapacity
                assert eng.dev_riss_fold(buf, 16, 4, 4, 58, buf + 65536, buf + 131072) == PR.FIELD_CAPACITY == eng.FIELD_CAPACITY
                assert eng.dev_riss_fold(buf, 16, 4, 4, 57, buf + 65536, buf + 131072) == 0
                assert eng.dev_riss_fold(buf, 5, 4, 4, 59, buf + 65536, buf + 131072) == PR.FIELD_CAPACITY
            fr.sync(), gl.sync()
            # n = 256 without the byte output is a supported shape: test_convert_many_parties compares its values
            # the wrong field's entry points: TypeMismatch
            import ctypes as C
            args = (C.c_void_p(buf), C.c_size_t(7), C.c_size_t(2), C.c_size_t(4), None, C.c_size_t(7), C.c_int(0), C.c_void_p(buf), None, None)
            assert fr.L.hbmpc_gl_dev_riss_convert_parties(fr.ctx, *args) == 5 and gl.L.hbmpc_dev_riss_convert_parties(gl.ctx, *args) == 5
            assert gl.dev_prandbit_finalize_parties(buf, buf, buf, 4, 1, buf, buf) == 5
            with pytest.raises(RuntimeError, match="ShareErrorCode 5"):
                pkg.pipelines.PRandBit(fr, fr, 7, 2, 3)
        finally:
            fr.dev_free(buf)
    finally:
        gl.close()
        fr.close()


@pytest.mark.parametrize("field,impl", CONFIGS)
def test_second_call_builds_no_table(pkg, field, impl):
    eng = engine(pkg, field, impl)
    try:
        n, t, B = 10, 3, 70
        r = riss_values(n, 120, B, seed=1)
        before = eng.cache_stats()["tables"]
        rc, out, out2 = dev_convert(eng, r, n, t)
        first = eng.cache_stats()["tables"]
        assert rc == 0 and first == before + 1
        rc, again, again2 = dev_convert(eng, r, n, t, form=2)
        assert rc == 0 and eng.cache_stats()["tables"] == first and np.array_equal(out, again) and np.array_equal(out2, again2)
        # a party subset adds its column list once; one party's own sets are a table of their own, once
        for _ in range(2):
            assert dev_convert(eng, r, n, t, party_ids=[2, 5])[0] == 0
        assert eng.cache_stats()["tables"] == first + 1
        own = np.ascontiguousarray(r[:84])
        for _ in range(2):
            assert dev_convert(eng, own, n, t, party_ids=[4], own=True)[0] == 0
        assert eng.cache_stats()["tables"] == first + 2
    finally:
        eng.close()
