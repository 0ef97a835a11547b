"""ctypes binding of libhbmpc_hip.so (the C ABI in include/hbmpc_hip.h) for tests and bench.py.

This is plumbing, not a product path: the product is the shared library.  Arrays are numpy uint64
with a trailing axis of 4 limbs (least-significant first) == U256[].  Every call goes through the
C ABI; there is no fallback -- if the library or a GPU is missing, loading/creating fails loudly.

Mirrors the reference interface for the path (SecretSharingScheme / free functions):
  compute_shares        RobustShare::compute_shares        robust_interpolate.rs:52-82
  make_vandermonde / vandermonde_apply                     common/share/mod.rs:31-76
  batch_recover(_p0)    batch_recover_secret               robust_interpolate.rs:284-443
  recover_secret        RobustShare::recover_secret        robust_interpolate.rs:94-157
  gao_rs_decode                                            robust_interpolate.rs:456-538
  nonrobust_recover_secret  NonRobustShare::recover_secret common/share/shamir.rs:199-239
  triple_local/.../truncpr_finalize                        triple_gen, mul, fpmul element-wise math
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libhbmpc_hip.so")
_LIB = None


class HbmpcError(RuntimeError):
    pass


def build(jobs: int = 8) -> str:
    """Compile every HIP translation unit for gfx950 (hipcc cross-compiles without a GPU)."""
    subprocess.check_call(["make", "-C", os.path.join(_HERE, "csrc"), f"-j{jobs}"], stdout=subprocess.DEVNULL)
    return LIB_PATH


def lib():
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise HbmpcError(f"{LIB_PATH} is missing: run `make -C {_HERE}/csrc -j8` (or __graft_entry__.build())")
        _LIB = C.CDLL(LIB_PATH)
        _LIB.hbmpc_last_error.restype = C.c_char_p
        _LIB.hbmpc_version.restype = C.c_char_p
    return _LIB


def _p(a):
    if a is None:
        return None
    if isinstance(a, np.ndarray):
        return a.ctypes.data_as(C.c_void_p)
    return C.c_void_p(int(a))  # raw device pointer


def u256(shape):
    return np.zeros(tuple(shape) + (4,), dtype=np.uint64)


def _sz(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.uint64))


def riss_tsets(n, t):
    """(rc, sets): hbmpc_riss_tsets -- combinations(0..n, t) as the library enumerates them; host only, needs no device"""
    cnt = C.c_size_t()
    rc = lib().hbmpc_riss_tsets(C.c_size_t(n), C.c_size_t(t), None, C.byref(cnt))
    if rc != 0:
        return rc, []
    ids = np.zeros((cnt.value, t), dtype=np.uint64)
    rc = lib().hbmpc_riss_tsets(C.c_size_t(n), C.c_size_t(t), _p(ids), C.byref(cnt))
    return rc, [tuple(int(x) for x in row) for row in ids]


FUSED_TRUNCPR_DEFAULT = 768  # hbmpc_set_fused_truncpr's default (csrc/hbmpc_capi.hip)
FUSED_MUL_DEFAULT = 1024  # hbmpc_set_fused_mul's default (csrc/hbmpc_capi.hip)
FUSED_INPUT_DEFAULT = 768  # hbmpc_set_fused_input's default (csrc/hbmpc_capi.hip)
FUSED_RANDBIT_DEFAULT = {"fr": 256, "goldilocks": 1024}  # hbmpc_set_fused_randbit's default per field (FUSED_RANDBIT_FR / _GL, csrc/hbmpc_capi.hip)
FUSED_BATCHRECON_DEFAULT = {"fr": 512, "goldilocks": 256}  # hbmpc_set_fused_batchrecon's default per field (FUSED_BATCHRECON_FR / _GL, csrc/hbmpc_capi.hip)
FUSED_PRODUCERS_DEFAULT = {"fr": 256, "goldilocks": 256}  # hbmpc_set_fused_producers's default per field (FUSED_PRODUCERS_FR / _GL, csrc/hbmpc_capi.hip)
FUSED_PRANDBIT_DEFAULT = 256  # hbmpc_set_fused_prandbit's default (FUSED_PRANDBIT, csrc/hbmpc_capi.hip)


class TakeSlice(C.Structure):
    """hbmpc_take_slice: one slice of hbmpc_dev_take_rows (Engine.take_rows)"""
    _fields_ = [("src", C.c_void_p), ("src_row_stride", C.c_size_t), ("dst", C.c_void_p), ("dst_row_stride", C.c_size_t),
                ("elements", C.c_size_t), ("group", C.c_size_t)]


def fixed_point_reciprocal_scaled(denom, f):
    """(rc, w, first_bad): hbmpc_fixed_point_reciprocal_scaled -- fpdiv/mod.rs:8-60 for N denominators ([N] U256 -> [N] U256); host
    only, needs no device.  first_bad: the index of the first invalid divisor, or None"""
    denom = np.ascontiguousarray(denom, dtype=np.uint64)
    N = denom.shape[0]
    w, bad = u256((N,)), C.c_size_t()
    rc = lib().hbmpc_fixed_point_reciprocal_scaled(_p(denom), C.c_size_t(N), C.c_size_t(f), _p(w), C.byref(bad))
    return rc, w, (None if bad.value == C.c_size_t(-1).value else bad.value)


class Engine:
    """One hbmpc_ctx on one GPU.  Host-pointer calls take/return numpy U256 arrays; the
    dev_* calls take raw device pointers (ints, e.g. torch.Tensor.data_ptr()) and a stream."""

    def __init__(self, device: int = 0, impl: str | None = None, field: str = "fr"):
        """field: "fr" (bls12-381 Fr, U256 elements = numpy [..., 4] uint64) or "goldilocks" (8-byte elements =
        numpy uint64; the hbmpc_gl_* entry points)"""
        self.L = lib()
        self.ctx = C.c_void_p()
        self.field = field
        self.ebytes = {"fr": 32, "goldilocks": 8}[field]
        self._pfx = "hbmpc_" if field == "fr" else "hbmpc_gl_"
        rc = self.L.hbmpc_create(C.c_int(device), C.c_int(0 if field == "fr" else 1), C.byref(self.ctx))
        if rc != 0:
            msg = self.L.hbmpc_last_error(None)
            raise HbmpcError(f"hbmpc_create(device={device}) failed with code {rc}: {msg.decode() if msg else ''}")
        if impl is not None:
            self.set_impl(impl)

    def _f(self, name):  # the entry point of this context's field
        return getattr(self.L, self._pfx + name)

    def _new(self, shape):  # zeroed output array of field elements
        return u256(shape) if self.field == "fr" else np.zeros(tuple(shape), dtype=np.uint64)

    def close(self):
        if self.ctx:
            self.L.hbmpc_destroy(self.ctx)
            self.ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def last_error(self) -> str:
        m = self.L.hbmpc_last_error(self.ctx)
        return m.decode() if m else ""

    def set_impl(self, impl: str):
        rc = self.L.hbmpc_set_field_impl(self.ctx, C.c_int({"u29": 0, "sat32": 1}[impl]))
        assert rc == 0

    def set_small_call_staging(self, zero_copy: bool):
        assert self.L.hbmpc_set_small_call_staging(self.ctx, C.c_int(1 if zero_copy else 0)) == 0

    def set_small_batch_chunks(self, max_chunks: int):
        assert self.L.hbmpc_set_small_batch_chunks(self.ctx, C.c_size_t(max_chunks)) == 0

    @staticmethod
    def gather_party_major(engines, root, shards_d, counts, strides, n_rows, out_d, out_stride, sync_sources=True, stream=0):
        """hbmpc_dev_gather_party_major: one engine (context) per shard; device pointers as ints"""
        k = len(engines)
        ctxs = (C.c_void_p * k)(*[e.ctx for e in engines])
        ptrs = (C.c_void_p * k)(*shards_d)
        cnt = (C.c_size_t * k)(*counts)
        strd = (C.c_size_t * k)(*strides)
        return engines[root].L.hbmpc_dev_gather_party_major(ctxs, C.c_size_t(k), C.c_size_t(root), ptrs, cnt, strd, C.c_size_t(n_rows),
                                                            C.c_void_p(out_d), C.c_size_t(out_stride), C.c_int(1 if sync_sources else 0),
                                                            C.c_void_p(stream))

    def peer_access(self, source: "Engine") -> bool:
        """True when this engine's device reads `source`'s memory directly (same device or peer access over xGMI)"""
        out = C.c_int(0)
        rc = self.L.hbmpc_dev_peer_access(self.ctx, source.ctx, C.byref(out))
        if rc != 0:
            raise HbmpcError(rc, self.last_error())
        return bool(out.value)

    def set_matrix_cores(self, on: bool, min_chunks: int = 0):
        """large Fr decodes on the matrix cores (int8 MFMA); min_chunks = 0 keeps the current threshold"""
        # on: False / True, or 2 = matrix cores without the workgroup-per-tile kernel of small batches, 3 = large encodes with
        # one table row per point instead of per point pair, 4 = the point-pair encode without its loader wave and LDS ring, 5 = with them at every batch size (A/B and test aids)
        assert self.L.hbmpc_set_matrix_cores(self.ctx, C.c_int(int(on)), C.c_size_t(min_chunks)) == 0

    def scrub_staging(self):
        assert self.L.hbmpc_scrub_staging(self.ctx) == 0

    def set_lazy_fallback_tables(self, on):
        """a new sender set's OEC / Gao and second-chance tables are built only when the first kernel flagged a chunk:
        0 = never, 1 = host-pointer calls (default), 2 = device-pointer calls as well"""
        assert self.L.hbmpc_set_lazy_fallback_tables(self.ctx, C.c_int(int(on))) == 0

    def set_single_launch_decode(self, on: bool):
        assert self.L.hbmpc_set_single_launch_decode(self.ctx, C.c_int(1 if on else 0)) == 0

    def set_matrix_core_workgroups(self, workgroups: int):
        assert self.L.hbmpc_set_matrix_core_workgroups(self.ctx, C.c_int(workgroups)) == 0

    def set_second_chance(self, on: bool):
        assert self.L.hbmpc_set_second_chance(self.ctx, C.c_int(1 if on else 0)) == 0

    def cache_stats(self):
        out = (C.c_size_t * 4)()
        assert self.L.hbmpc_cache_stats(self.ctx, out) == 0
        return dict(zip(("tables", "pinned", "retired", "evictions"), [int(v) for v in out]))

    def set_force_generic(self, on: bool):
        assert self.L.hbmpc_set_force_generic(self.ctx, C.c_int(1 if on else 0)) == 0

    # ---- host-pointer API ----
    def compute_shares(self, coeffs, n, d, out=None):
        coeffs = np.ascontiguousarray(coeffs)
        B = coeffs.shape[0]
        if out is None:  # a fresh array: its first-touch page faults happen inside the call's device-to-host copy
            out = self._new((n, B))
        rc = self._f("compute_shares")(self.ctx, _p(coeffs), C.c_size_t(B), C.c_size_t(n), C.c_size_t(d), _p(out))
        return rc, out

    def compute_shares_seeded(self, seed, secrets, n, d, first_index=0):
        """seed: 32 bytes ("hbmpc-chacha20-v1", include/hbmpc_hip.h); secrets: [B] elements, or an int B: the
        secrets are drawn too"""
        if isinstance(secrets, int):
            B, sp = secrets, C.c_void_p(0)
        else:
            secrets = np.ascontiguousarray(secrets)
            B, sp = secrets.shape[0], _p(secrets)
        out = self._new((n, B))
        seed = (C.c_uint8 * 32).from_buffer_copy(bytes(seed))
        rc = self._f("compute_shares_seeded")(self.ctx, seed, sp, C.c_size_t(B), C.c_uint64(first_index),
                                              C.c_size_t(n), C.c_size_t(d), _p(out))
        return rc, out

    def make_vandermonde(self, n, d):
        out = self._new((n, d + 1))
        rc = self._f("make_vandermonde")(self.ctx, C.c_size_t(n), C.c_size_t(d), _p(out))
        return rc, out

    def vandermonde_apply(self, x, n, d):
        x = np.ascontiguousarray(x)
        G = x.shape[0]
        out = self._new((n, G))
        rc = self._f("vandermonde_apply")(self.ctx, _p(x), C.c_size_t(G), C.c_size_t(n), C.c_size_t(d), _p(out))
        return rc, out

    def batch_recover(self, sender_ids, evals, n, d, t):
        evals = np.ascontiguousarray(evals)
        S = len(sender_ids)
        G = evals.shape[1] if evals.ndim == (3 if self.field == "fr" else 2) else 0
        out = self._new((G, d + 1))
        nco = np.zeros(G, dtype=np.uint32)
        st = np.zeros(G, dtype=np.uint8)
        rc = self._f("batch_recover")(self.ctx, _p(_sz(sender_ids)), C.c_size_t(S), _p(evals), C.c_size_t(G),
                                        C.c_size_t(n), C.c_size_t(d), C.c_size_t(t), _p(out), _p(nco), _p(st))
        return rc, out, nco, st

    def batch_recover_p0(self, sender_ids, evals, n, d, t):
        evals = np.ascontiguousarray(evals)
        S = len(sender_ids)
        G = evals.shape[1] if evals.ndim == (3 if self.field == "fr" else 2) else 0
        out = self._new((G,))
        st = np.zeros(G, dtype=np.uint8)
        rc = self._f("batch_recover_p0")(self.ctx, _p(_sz(sender_ids)), C.c_size_t(S), _p(evals), C.c_size_t(G),
                                           C.c_size_t(n), C.c_size_t(d), C.c_size_t(t), _p(out), _p(st))
        return rc, out, st

    def recover_secret(self, ids, degrees, vals, n, t):
        vals = np.ascontiguousarray(vals)
        S = len(ids)
        cap = (int(degrees[0]) + 1) if S else 1
        out = self._new((max(cap, 1),))
        nco = C.c_size_t(0)
        sec = self._new((1,))
        rc = self._f("recover_secret")(self.ctx, _p(_sz(ids)), _p(_sz(degrees)), _p(vals), C.c_size_t(S),
                                         C.c_size_t(n), C.c_size_t(t), _p(out), C.byref(nco), _p(sec))
        return rc, out[: nco.value], sec[0]

    def gao_rs_decode(self, received, k, n, erasures):
        received = np.ascontiguousarray(received)
        out = self._new((max(k, 1),))
        nco = C.c_size_t(0)
        rc = self._f("gao_rs_decode")(self.ctx, _p(received), C.c_size_t(k), C.c_size_t(n), _p(_sz(erasures)),
                                        C.c_size_t(len(erasures)), _p(out), C.byref(nco))
        return rc, out[: nco.value]

    def nonrobust_recover_secret(self, ids, degrees, vals, n):
        vals = np.ascontiguousarray(vals)
        S = len(ids)
        out = self._new((max(S, 1),))
        nco = C.c_size_t(0)
        sec = self._new((1,))
        rc = self._f("nonrobust_recover_secret")(self.ctx, _p(_sz(ids)), _p(_sz(degrees)), _p(vals), C.c_size_t(S),
                                                   C.c_size_t(n), _p(out), C.byref(nco), _p(sec))
        return rc, out[: nco.value], sec[0]

    def batch_interpolate(self, ids, evals, n):
        evals = np.ascontiguousarray(evals)
        S, G = len(ids), evals.shape[1]
        co = self._new((G, S))
        deg = np.zeros(G, dtype=np.uint32)
        rc = self._f("batch_interpolate")(self.ctx, _p(_sz(ids)), C.c_size_t(S), _p(evals), C.c_size_t(G),
                                            C.c_size_t(n), _p(co), _p(deg))
        return rc, co, deg

    # ---- Shamirshare: the integer-point scheme (common/share/shamir.rs:13-126); points are u64 ids, NOT domain indices ----
    @staticmethod
    def _pts(points):
        return None if points is None else _sz([int(x) for x in points])

    def shamir_compute_shares(self, coeffs, points, d):
        """coeffs [B][d+1] -> (rc, shares [m][B]), shares[i][b] = sum_k coeffs[b][k] points[i]^k"""
        coeffs = np.ascontiguousarray(coeffs)
        B, m = coeffs.shape[0], (0 if points is None else len(points))
        out = self._new((m, B))
        rc = self._f("shamir_compute_shares")(self.ctx, _p(coeffs), C.c_size_t(B), _p(self._pts(points)), C.c_size_t(m), C.c_size_t(d), _p(out))
        return rc, out

    def shamir_recover_secret(self, ids, degrees, vals):
        """(rc, trimmed coefficients, secret) of one polynomial: shamir.rs:90-125"""
        vals = np.ascontiguousarray(vals)
        S = len(ids)
        out = self._new((max(S, 1),))
        nco = C.c_size_t(0)
        sec = self._new((1,))
        rc = self._f("shamir_recover_secret")(self.ctx, _p(self._pts(ids)), _p(_sz(degrees)), _p(vals), C.c_size_t(S), _p(out), C.byref(nco),
                                              _p(sec))
        return rc, out[: nco.value], sec[0]

    def shamir_batch_interpolate(self, points, evals):
        """evals [S][G] -> (rc, coeffs [G][S] untrimmed, degree [G]): plain Lagrange through all S points"""
        evals = np.ascontiguousarray(evals)
        S, G = len(points), evals.shape[1]
        co = self._new((G, S))
        deg = np.zeros(G, dtype=np.uint32)
        rc = self._f("shamir_batch_interpolate")(self.ctx, _p(self._pts(points)), C.c_size_t(S), _p(evals), C.c_size_t(G), _p(co), _p(deg))
        return rc, co, deg

    def dev_shamir_compute_shares(self, coeffs_d, B, points, d, out_d, stream=0):
        m = 0 if points is None else len(points)
        return self._f("dev_shamir_compute_shares")(self.ctx, C.c_void_p(coeffs_d), C.c_size_t(B), _p(self._pts(points)), C.c_size_t(m),
                                                    C.c_size_t(d), C.c_void_p(out_d), C.c_void_p(stream))

    def dev_shamir_batch_interpolate(self, points, evals_d, row_stride, G, coeffs_d, degree_d, stream=0):
        return self._f("dev_shamir_batch_interpolate")(self.ctx, _p(self._pts(points)), C.c_size_t(len(points)), C.c_void_p(evals_d),
                                                       C.c_size_t(row_stride), C.c_size_t(G), C.c_void_p(coeffs_d), C.c_void_p(degree_d),
                                                       C.c_void_p(stream))

    def dev_shamir_batch_interpolate_c0(self, points, evals_d, row_stride, G, tmp_coeffs_d, c0_d, degree_d, stream=0):
        return self._f("dev_shamir_batch_interpolate_c0")(self.ctx, _p(self._pts(points)), C.c_size_t(len(points)), C.c_void_p(evals_d),
                                                          C.c_size_t(row_stride), C.c_size_t(G), C.c_void_p(tmp_coeffs_d), C.c_void_p(c0_d),
                                                          C.c_void_p(degree_d), C.c_void_p(stream))

    def set_shamir_route(self, route: int):
        """0 = the planner's rule (csrc/shamir_route.hpp), 1 = the small-weight kernel wherever it covers the call, 2 = never"""
        assert self.L.hbmpc_set_shamir_route(self.ctx, C.c_int(route)) == 0

    def shamir_route(self, points, d, B):
        """(rc, kernel): the kernel the planner picks for the call (1 small-weight, 2 a wave per secret, 3 a lane per secret)"""
        k = C.c_int(0)
        rc = self.L.hbmpc_shamir_route(self.ctx, _p(self._pts(points)), C.c_size_t(len(points)), C.c_size_t(d), C.c_size_t(B), C.byref(k))
        return rc, k.value

    def _ew(self, name, ins, n_out=1, extra=()):
        ins = [np.ascontiguousarray(a) for a in ins]
        N = ins[0].shape[0]
        outs = [self._new((N,)) for _ in range(n_out)]
        args = [self.ctx] + [_p(a) for a in ins] + [C.c_size_t(e) for e in extra] + [C.c_size_t(N)] + [_p(o) for o in outs]
        rc = getattr(self.L, name.replace("hbmpc_", self._pfx, 1))(*args)
        return (rc, *outs)

    def fr_op(self, op, a, b):
        a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
        out = self._new((a.shape[0],))
        rc = self._f("fr_op")(self.ctx, C.c_int({"add": 0, "sub": 1, "mul": 2}[op]), _p(a), _p(b),
                                C.c_size_t(a.shape[0]), _p(out))
        return rc, out

    def triple_local(self, a, b, r2t):
        return self._ew("hbmpc_triple_local", [a, b, r2t])

    def triple_finalize(self, rt, opened):
        return self._ew("hbmpc_triple_finalize", [rt, opened])

    def beaver_open_shares(self, a, b, x, y):
        return self._ew("hbmpc_beaver_open_shares", [a, b, x, y], n_out=2)

    def beaver_finalize(self, c, x, y, d, e):
        return self._ew("hbmpc_beaver_finalize", [c, x, y, d, e])

    def truncpr_rdash(self, r_bits, m):
        r_bits = np.ascontiguousarray(r_bits)
        N = r_bits.shape[1]
        out = self._new((N,))
        rc = self.L.hbmpc_truncpr_rdash(self.ctx, _p(r_bits), C.c_size_t(m), C.c_size_t(N), _p(out))
        return rc, out

    def truncpr_open_share(self, a, r_dash, r_int, k, m):
        return self._ew("hbmpc_truncpr_open_share", [a, r_dash, r_int], extra=(k, m))

    def truncpr_finalize(self, a, r_dash, c_open, m):
        return self._ew("hbmpc_truncpr_finalize", [a, r_dash, c_open], extra=(m,))

    # ---- device-pointer API ----
    def dev_alloc(self, nbytes: int) -> int:
        p = C.c_void_p()
        rc = self.L.hbmpc_dev_alloc(self.ctx, C.c_size_t(nbytes), C.byref(p))
        if rc != 0:
            raise HbmpcError(f"hbmpc_dev_alloc({nbytes}) -> {rc}: {self.last_error()}")
        return p.value

    def dev_free(self, ptr: int):
        self.L.hbmpc_dev_free(self.ctx, C.c_void_p(ptr))

    def stream_pool_release_threshold(self) -> int:
        """Release threshold of the device's current stream-ordered pool (0 = the platform default, under which hipMallocAsync
        buffers are NOT safe to hand to the library: include/hbmpc_hip.h, 'Device buffers')."""
        v = C.c_uint64(0)
        rc = self.L.hbmpc_stream_pool_release_threshold(self.ctx, C.byref(v))
        if rc != 0:
            raise HbmpcError(f"hbmpc_stream_pool_release_threshold -> {rc}: {self.last_error()}")
        return v.value

    def stream_pool_retain(self):
        rc = self.L.hbmpc_stream_pool_retain(self.ctx)
        if rc != 0:
            raise HbmpcError(f"hbmpc_stream_pool_retain -> {rc}: {self.last_error()}")

    def h2d(self, dptr: int, arr: np.ndarray, stream=0):
        arr = np.ascontiguousarray(arr)
        rc = self.L.hbmpc_memcpy_h2d(self.ctx, C.c_void_p(dptr), _p(arr), C.c_size_t(arr.nbytes), C.c_void_p(stream))
        assert rc == 0, self.last_error()

    def d2h(self, arr: np.ndarray, dptr: int, stream=0):
        assert arr.flags["C_CONTIGUOUS"]
        rc = self.L.hbmpc_memcpy_d2h(self.ctx, _p(arr), C.c_void_p(dptr), C.c_size_t(arr.nbytes), C.c_void_p(stream))
        assert rc == 0, self.last_error()

    def d2d(self, dst: int, src: int, nbytes: int, stream=0):
        rc = self.L.hbmpc_memcpy_d2d(self.ctx, C.c_void_p(dst), C.c_void_p(src), C.c_size_t(nbytes), C.c_void_p(stream))
        assert rc == 0, self.last_error()

    def fr_op_scalar(self, op, a, scalar):
        """op: "add" (a + s), "sub" (a - s), "mul" (a * s), "rsub" (s - a); scalar: one element"""
        a = np.ascontiguousarray(a)
        sc = np.ascontiguousarray(scalar)
        out = self._new((a.shape[0],))
        rc = self._f("fr_op_scalar")(self.ctx, C.c_int({"add": 0, "sub": 1, "mul": 2, "rsub": 3}[op]), _p(a), _p(sc),
                                       C.c_size_t(a.shape[0]), _p(out))
        return rc, out

    def dev_fr_op_scalar(self, op, a_d, scalar, N, out_d, stream=0):
        sc = np.ascontiguousarray(scalar)
        return self._f("dev_fr_op_scalar")(self.ctx, C.c_int({"add": 0, "sub": 1, "mul": 2, "rsub": 3}[op]), C.c_void_p(a_d),
                                             _p(sc), C.c_size_t(N), C.c_void_p(out_d), C.c_void_p(stream))

    def dev_fr_op(self, op, a_d, b_d, N, out_d, stream=0):
        return self._f("dev_fr_op")(self.ctx, C.c_int({"add": 0, "sub": 1, "mul": 2}[op]), C.c_void_p(a_d),
                                      C.c_void_p(b_d), C.c_size_t(N), C.c_void_p(out_d), C.c_void_p(stream))

    def stream_create(self) -> int:
        st = C.c_void_p()
        rc = self.L.hbmpc_stream_create(self.ctx, C.byref(st))
        if rc != 0:
            raise HbmpcError(f"stream_create -> {rc}: {self.last_error()}")
        return st.value

    def stream_destroy(self, stream: int):
        self.L.hbmpc_stream_destroy(self.ctx, C.c_void_p(stream))

    # ---- HIP graphs: capture a sequence of dev_* calls once, replay it per refill of the buffers ----
    def graph_begin(self, stream):
        rc = self.L.hbmpc_graph_begin_capture(self.ctx, C.c_void_p(stream))
        if rc != 0:
            raise HbmpcError(f"graph_begin_capture -> {rc}: {self.last_error()}")

    def graph_end(self, stream) -> int:
        g = C.c_void_p()
        rc = self.L.hbmpc_graph_end_capture(self.ctx, C.c_void_p(stream), C.byref(g))
        if rc != 0:
            raise HbmpcError(f"graph_end_capture -> {rc}: {self.last_error()}")
        return g.value

    def graph_launch(self, graph: int, stream=0):
        rc = self.L.hbmpc_graph_launch(self.ctx, C.c_void_p(graph), C.c_void_p(stream))
        if rc != 0:
            raise HbmpcError(f"graph_launch -> {rc}: {self.last_error()}")

    def graph_destroy(self, graph: int):
        self.L.hbmpc_graph_destroy(C.c_void_p(graph))

    def sync(self, stream=0):
        rc = self.L.hbmpc_stream_sync(self.ctx, C.c_void_p(stream))
        if rc != 0:
            raise HbmpcError(f"stream sync -> {rc}: {self.last_error()}")

    def dev_compute_shares(self, coeffs_d, B, n, d, out_d, stream=0):
        return self._f("dev_compute_shares")(self.ctx, C.c_void_p(coeffs_d), C.c_size_t(B), C.c_size_t(n),
                                               C.c_size_t(d), C.c_void_p(out_d), C.c_void_p(stream))

    def dev_fill_coeffs(self, seed, secrets_d, B, first_index, d, coeffs_d, stream=0):
        seed = (C.c_uint8 * 32).from_buffer_copy(bytes(seed))
        return self._f("dev_fill_coeffs")(self.ctx, seed, C.c_void_p(secrets_d), C.c_size_t(B), C.c_uint64(first_index),
                                          C.c_size_t(d), C.c_void_p(coeffs_d), C.c_void_p(stream))

    def dev_compute_shares_seeded(self, seed, secrets_d, B, first_index, n, d, coeffs_ws_d, out_d, stream=0):
        seed = (C.c_uint8 * 32).from_buffer_copy(bytes(seed))
        return self._f("dev_compute_shares_seeded")(self.ctx, seed, C.c_void_p(secrets_d), C.c_size_t(B),
                                                    C.c_uint64(first_index), C.c_size_t(n), C.c_size_t(d),
                                                    C.c_void_p(coeffs_ws_d), C.c_void_p(out_d), C.c_void_p(stream))

    def dev_batch_interpolate(self, ids, evals_d, row_stride, G, n, coeffs_d, degree_d, stream=0):
        """plain Lagrange through ALL len(ids) sender rows (row s at evals_d + s * row_stride elements): coeffs[G][S], degree[G]"""
        return self._f("dev_batch_interpolate")(self.ctx, _p(_sz(ids)), C.c_size_t(len(ids)), C.c_void_p(evals_d), C.c_size_t(row_stride),
                                                C.c_size_t(G), C.c_size_t(n), C.c_void_p(coeffs_d), C.c_void_p(degree_d), C.c_void_p(stream))

    def dev_transpose(self, src_d, rows, cols, src_row_stride, dst_d, dst_row_stride, batch=1, src_batch_stride=0, dst_batch_stride=0,
                      stream=0):
        """dst[b][c][r] = src[b][r][c]; strides in elements of this engine's field"""
        return self.L.hbmpc_dev_transpose(self.ctx, C.c_void_p(src_d), C.c_size_t(rows), C.c_size_t(cols), C.c_size_t(src_row_stride),
                                          C.c_void_p(dst_d), C.c_size_t(dst_row_stride), C.c_size_t(batch), C.c_size_t(src_batch_stride),
                                          C.c_size_t(dst_batch_stride), C.c_void_p(stream))

    def take_rows(self, slices, rows, stream=0):
        """hbmpc_dev_take_rows: slices = [(src_d, src_row_stride, dst_d, dst_row_stride, elements, group), ...] (at most 8; device pointers
        as ints, strides and elements in this engine's field element): dst[r][j * (elements / group) + i] = src[r][i * group + j] for
        every row r < rows -- one launch for all of them"""
        arr = (TakeSlice * max(len(slices), 1))(*[TakeSlice(*[int(x) if x is not None else None for x in s]) for s in slices])
        return self.L.hbmpc_dev_take_rows(self.ctx, arr, C.c_size_t(len(slices)), C.c_size_t(rows), C.c_void_p(stream))

    def dev_check_degree(self, coeffs_d, status_d, G, m, want_degree, bad_d, stream=0):
        return self.L.hbmpc_dev_check_degree(self.ctx, C.c_void_p(coeffs_d), C.c_void_p(status_d), C.c_size_t(G), C.c_size_t(m),
                                             C.c_size_t(want_degree), C.c_void_p(bad_d), C.c_void_p(stream))

    def dev_check_double_share(self, ct_d, c2t_d, G, m, t, bad_d, stream=0):
        return self.L.hbmpc_dev_check_double_share(self.ctx, C.c_void_p(ct_d), C.c_void_p(c2t_d), C.c_size_t(G), C.c_size_t(m),
                                                   C.c_size_t(t), C.c_void_p(bad_d), C.c_void_p(stream))

    def dev_check_top_coeff(self, top_d, status_d, G, want_degree, bad_d, columns=None, stream=0):
        """columns=None: hbmpc_dev_check_top_coeff; a number: hbmpc_dev_check_top_coeff_columns"""
        if columns is None:
            return self.L.hbmpc_dev_check_top_coeff(self.ctx, C.c_void_p(top_d), C.c_void_p(status_d), C.c_size_t(G), C.c_size_t(want_degree),
                                                    C.c_void_p(bad_d), C.c_void_p(stream))
        return self.L.hbmpc_dev_check_top_coeff_columns(self.ctx, C.c_void_p(top_d), C.c_void_p(status_d), C.c_size_t(G), C.c_size_t(columns),
                                                        C.c_size_t(want_degree), C.c_void_p(bad_d), C.c_void_p(stream))

    def dev_check_double_share_sel(self, sel_t_d, st_t_d, sel_2t_d, st_2t_d, G, columns, t, bad_d, stream=0):
        return self.L.hbmpc_dev_check_double_share_sel(self.ctx, C.c_void_p(sel_t_d), C.c_void_p(st_t_d), C.c_void_p(sel_2t_d), C.c_void_p(st_2t_d),
                                                       C.c_size_t(G), C.c_size_t(columns), C.c_size_t(t), C.c_void_p(bad_d), C.c_void_p(stream))

    def dev_check_double_share_c0(self, c0_t_d, deg_t_d, c0_2t_d, deg_2t_d, G, t, bad_d, columns=None, stream=0):
        """columns=None: hbmpc_dev_check_double_share_c0; a number: hbmpc_dev_check_double_share_c0_columns"""
        if columns is None:
            return self.L.hbmpc_dev_check_double_share_c0(self.ctx, C.c_void_p(c0_t_d), C.c_void_p(deg_t_d), C.c_void_p(c0_2t_d), C.c_void_p(deg_2t_d),
                                                          C.c_size_t(G), C.c_size_t(t), C.c_void_p(bad_d), C.c_void_p(stream))
        return self.L.hbmpc_dev_check_double_share_c0_columns(self.ctx, C.c_void_p(c0_t_d), C.c_void_p(deg_t_d), C.c_void_p(c0_2t_d),
                                                              C.c_void_p(deg_2t_d), C.c_size_t(G), C.c_size_t(columns), C.c_size_t(t),
                                                              C.c_void_p(bad_d), C.c_void_p(stream))

    def dev_batch_interpolate_c0(self, ids, evals_d, row_stride, G, n, tmp_coeffs_d, c0_d, degree_d, stream=0):
        """what the RanDouSha verifier keeps of an interpolation through ALL len(ids) sender rows: c0[G], degree[G]; tmp_coeffs_d: G * len(ids)
        elements, or 0 where the kernel writes just these (all n shares of an 8- or 16-point domain)"""
        return self._f("dev_batch_interpolate_c0")(self.ctx, _p(_sz(ids)), C.c_size_t(len(ids)), C.c_void_p(evals_d), C.c_size_t(row_stride),
                                                   C.c_size_t(G), C.c_size_t(n), C.c_void_p(tmp_coeffs_d), C.c_void_p(c0_d), C.c_void_p(degree_d),
                                                   C.c_void_p(stream))

    def dev_recover_check_degree_strided(self, sender_ids, evals_d, row_stride, G, n, t, ws_d, status_d, bad_d, groups=1, group_stride=0,
                                         summary_d=0, stream=0):
        """RanSha's verifier in one call: `groups` verifiers of G columns each; ws_d: max(groups G, G (t + 1)) elements, status_d: groups G bytes"""
        return self._f("dev_recover_check_degree_strided")(self.ctx, _p(_sz(sender_ids)), C.c_size_t(len(sender_ids)), C.c_void_p(evals_d),
                                                           C.c_size_t(row_stride), C.c_size_t(G), C.c_size_t(n), C.c_size_t(t), C.c_size_t(groups),
                                                           C.c_size_t(group_stride), C.c_void_p(ws_d), C.c_void_p(status_d), C.c_void_p(summary_d),
                                                           C.c_void_p(bad_d), C.c_void_p(stream))

    def dev_vandermonde_apply(self, x_d, G, n, d, y_d, stream=0):
        return self._f("dev_vandermonde_apply")(self.ctx, C.c_void_p(x_d), C.c_size_t(G), C.c_size_t(n),
                                                  C.c_size_t(d), C.c_void_p(y_d), C.c_void_p(stream))

    def dev_triple_encode_parties(self, a_d, b_d, r2t_d, G, n, d, parties, tmp_d, y_d, stream=0):
        return self._f("dev_triple_encode_parties")(self.ctx, C.c_void_p(a_d), C.c_void_p(b_d), C.c_void_p(r2t_d), C.c_size_t(G),
                                                      C.c_size_t(n), C.c_size_t(d), C.c_size_t(parties), C.c_void_p(tmp_d),
                                                      C.c_void_p(y_d), C.c_void_p(stream))

    def dev_vandermonde_apply_parties(self, x_d, G, n, d, parties, y_d, stream=0):
        return self._f("dev_vandermonde_apply_parties")(self.ctx, C.c_void_p(x_d), C.c_size_t(G), C.c_size_t(n), C.c_size_t(d),
                                                        C.c_size_t(parties), C.c_void_p(y_d), C.c_void_p(stream))

    def dev_batch_recover(self, sender_ids, evals_d, G, n, d, t, out_d, nco_d=0, status_d=0, summary_d=0, stream=0,
                          p0=False):
        ids = _sz(sender_ids)
        if p0:
            return self._f("dev_batch_recover_p0")(self.ctx, _p(ids), C.c_size_t(len(sender_ids)),
                                                     C.c_void_p(evals_d), C.c_size_t(G), C.c_size_t(n), C.c_size_t(d),
                                                     C.c_size_t(t), C.c_void_p(out_d), C.c_void_p(status_d),
                                                     C.c_void_p(summary_d), C.c_void_p(stream))
        return self._f("dev_batch_recover")(self.ctx, _p(ids), C.c_size_t(len(sender_ids)), C.c_void_p(evals_d),
                                              C.c_size_t(G), C.c_size_t(n), C.c_size_t(d), C.c_size_t(t),
                                              C.c_void_p(out_d), C.c_void_p(nco_d), C.c_void_p(status_d),
                                              C.c_void_p(summary_d), C.c_void_p(stream))

    def dev_batch_recover_strided(self, sender_ids, evals_d, row_stride, G, n, d, t, out_d, p0=False, nco_d=0,
                                  status_d=0, summary_d=0, stream=0):
        ids = _sz(sender_ids)
        return self._f("dev_batch_recover_strided")(self.ctx, _p(ids), C.c_size_t(len(sender_ids)),
                                                      C.c_void_p(evals_d), C.c_size_t(row_stride), C.c_size_t(G),
                                                      C.c_size_t(n), C.c_size_t(d), C.c_size_t(t),
                                                      C.c_int(1 if p0 else 0), C.c_void_p(out_d), C.c_void_p(nco_d),
                                                      C.c_void_p(status_d), C.c_void_p(summary_d), C.c_void_p(stream))

    def dev_batch_recover_coeff_strided(self, sender_ids, evals_d, row_stride, G, n, d, t, k, out_d, status_d=0, summary_d=0, stream=0):
        """a P(0)-shaped decode that keeps coefficient k (exactly d + t + 1 senders)"""
        ids = _sz(sender_ids)
        return self._f("dev_batch_recover_coeff_strided")(self.ctx, _p(ids), C.c_size_t(len(sender_ids)), C.c_void_p(evals_d), C.c_size_t(row_stride),
                                                            C.c_size_t(G), C.c_size_t(n), C.c_size_t(d), C.c_size_t(t), C.c_size_t(k),
                                                            C.c_void_p(out_d), C.c_void_p(status_d), C.c_void_p(summary_d), C.c_void_p(stream))

    def dev_interpolate_degree_check_strided(self, ids, evals_d, row_stride, G, n, d, ws_d, sel_d, status_d, stream=0, groups=1, group_stride=0):
        """do the len(ids) points of every chunk lie on a polynomial of degree <= d?  sel[G][2] = (constant term, coefficient d), status[G]"""
        return self._f("dev_interpolate_degree_check_strided")(self.ctx, _p(_sz(ids)), C.c_size_t(len(ids)), C.c_void_p(evals_d), C.c_size_t(row_stride),
                                                                 C.c_size_t(G), C.c_size_t(n), C.c_size_t(d), C.c_size_t(groups), C.c_size_t(group_stride),
                                                                 C.c_void_p(ws_d), C.c_void_p(sel_d), C.c_void_p(status_d), C.c_void_p(stream))

    def dev_batch_recover_slots(self, sender_ids, row_slots, evals_d, row_stride, G, n, d, t, out_d, p0=False, nco_d=0,
                                status_d=0, summary_d=0, stream=0):
        return self._f("dev_batch_recover_slots")(self.ctx, _p(_sz(sender_ids)), _p(_sz(row_slots)),
                                                    C.c_size_t(len(sender_ids)), C.c_void_p(evals_d), C.c_size_t(row_stride),
                                                    C.c_size_t(G), C.c_size_t(n), C.c_size_t(d), C.c_size_t(t),
                                                    C.c_int(1 if p0 else 0), C.c_void_p(out_d), C.c_void_p(nco_d),
                                                    C.c_void_p(status_d), C.c_void_p(summary_d), C.c_void_p(stream))

    def dev_elem(self, name, ptrs, N, extra=(), stream=0):
        args = [self.ctx] + [C.c_void_p(p) for p in ptrs[: name_inputs(name)]] + [C.c_size_t(e) for e in extra] + \
               [C.c_size_t(N)] + [C.c_void_p(p) for p in ptrs[name_inputs(name):]] + [C.c_void_p(stream)]
        return getattr(self.L, self._pfx + "dev_" + name)(*args)

    def dev_elem_parties(self, name, ptrs, N, parties, extra=(), stream=0):
        """party-batched forms (hbmpc_dev_*_parties): per-party arrays [parties][N], public operands [N]"""
        args = [self.ctx] + [C.c_void_p(p) for p in ptrs[: name_inputs(name)]] + [C.c_size_t(e) for e in extra] + \
               [C.c_size_t(N), C.c_size_t(parties)] + [C.c_void_p(p) for p in ptrs[name_inputs(name):]] + [C.c_void_p(stream)]
        return getattr(self.L, self._pfx + "dev_" + name + "_parties")(*args)

    def dev_fpmul_middle(self, c_d, x_d, y_d, d_d, e_d, rbits_d, rint_d, k, m, N, parties, z_d, rdash_d, open_d, stream=0):
        """finalize_mul + r' + the share TruncPr opens, one launch (hbmpc_dev_fpmul_middle)"""
        return self.L.hbmpc_dev_fpmul_middle(self.ctx, *(C.c_void_p(p) for p in (c_d, x_d, y_d, d_d, e_d, rbits_d, rint_d)),
                                             C.c_size_t(k), C.c_size_t(m), C.c_size_t(N), C.c_size_t(parties),
                                             C.c_void_p(z_d), C.c_void_p(rdash_d), C.c_void_p(open_d), C.c_void_p(stream))

    def dev_triplegen_parties(self, a_d, b_d, r2t_d, rt_d, N, n, t, y_d, z_d, opened_d, c_d, status_d=0, summary_first_d=0, summary_d=0, stream=0):
        """TripleGenNode for all n parties of this device in one call (hbmpc_dev_triplegen_parties): one launch for a small batch, four
        otherwise; returns the ShareErrorCode"""
        return self.L.hbmpc_dev_triplegen_parties(self.ctx, *(C.c_void_p(p) for p in (a_d, b_d, r2t_d, rt_d)), C.c_size_t(N), C.c_size_t(n), C.c_size_t(t),
                                                  *(C.c_void_p(p) for p in (y_d, z_d, opened_d, c_d, status_d, summary_first_d, summary_d)), C.c_void_p(stream))

    def dev_fpmul_parties(self, sender_ids, a_d, b_d, c_d, x_d, y_d, rbits_d, rint_d, k, m, N, n, t, de_ws_d, de_d, z_d, rdash_d, osh_d,
                          cop_d, out_d, status_d=0, summary_first_d=0, summary_d=0, stream=0):
        """FPMulNode for all n parties of this device in one call (hbmpc_dev_fpmul_parties): one launch for a small batch, four or
        five otherwise; returns the ShareErrorCode"""
        ids = (C.c_size_t * len(sender_ids))(*sender_ids)
        return self.L.hbmpc_dev_fpmul_parties(self.ctx, ids, C.c_size_t(len(sender_ids)),
                                              *(C.c_void_p(p) for p in (a_d, b_d, c_d, x_d, y_d, rbits_d, rint_d)),
                                              C.c_size_t(k), C.c_size_t(m), C.c_size_t(N), C.c_size_t(n), C.c_size_t(t),
                                              *(C.c_void_p(p) for p in (de_ws_d, de_d, z_d, rdash_d, osh_d, cop_d, out_d, status_d, summary_first_d, summary_d)),
                                              C.c_void_p(stream))

    def dev_truncpr_parties(self, sender_ids, a_d, w_d, rbits_d, rint_d, k, m, N, n, t, c_d, rdash_d, osh_d, cop_d, out_d, status_d=0,
                            summary_d=0, stream=0):
        """TruncPrNode (w_d = 0) or FPDivConstNode (w_d: the public multipliers [N]; c_d then receives a * w) for all n parties of this
        device in one call (hbmpc_dev_truncpr_parties): one launch for a small batch, three otherwise; returns the ShareErrorCode"""
        ids = (C.c_size_t * len(sender_ids))(*sender_ids)
        return self.L.hbmpc_dev_truncpr_parties(self.ctx, ids, C.c_size_t(len(sender_ids)),
                                                *(C.c_void_p(p) for p in (a_d, w_d, rbits_d, rint_d)),
                                                C.c_size_t(k), C.c_size_t(m), C.c_size_t(N), C.c_size_t(n), C.c_size_t(t),
                                                *(C.c_void_p(p) for p in (c_d, rdash_d, osh_d, cop_d, out_d, status_d, summary_d)),
                                                C.c_void_p(stream))

    def set_fused_truncpr(self, max_elements: int):
        """hbmpc_dev_truncpr_parties is one launch up to this many batch elements (0: always three)"""
        assert self.L.hbmpc_set_fused_truncpr(self.ctx, C.c_size_t(max_elements)) == 0

    def dev_mul_parties(self, sender_ids, a_d, b_d, c_d, x_d, y_d, N, n, t, de_ws_d, de_d, z_d, status_d=0, summary_d=0, stream=0):
        """Multiply (Beaver) for all n parties of this device in one call (hbmpc_[gl_]dev_mul_parties; sender_ids are party ids): over
        Fr one launch for a small batch, three otherwise; returns the ShareErrorCode"""
        ids = (C.c_size_t * len(sender_ids))(*sender_ids)
        return self._f("dev_mul_parties")(self.ctx, ids, C.c_size_t(len(sender_ids)), *(C.c_void_p(p) for p in (a_d, b_d, c_d, x_d, y_d)),
                                          C.c_size_t(N), C.c_size_t(n), C.c_size_t(t),
                                          *(C.c_void_p(p) for p in (de_ws_d, de_d, z_d, status_d, summary_d)), C.c_void_p(stream))

    def set_fused_mul(self, max_elements: int):
        """hbmpc_dev_mul_parties is one launch up to this many batch elements (0: always three)"""
        assert self.L.hbmpc_set_fused_mul(self.ctx, C.c_size_t(max_elements)) == 0

    def input_parties(self, sender_ids, x_d, r_d, N, n, t, mask_d, masked_d, in_sh_d, status_d, summary_d=0, stream=0):
        """Input for all n parties of this device in one call (hbmpc_[gl_]dev_input_parties; sender_ids are party ids): the client's open
        of the masks, masked = x + mask, in_sh[p] = masked - r[p]; an element whose mask does not open (status >= 2) is refused: zeros,
        never x + 0.  Over Fr one launch for a small batch, two otherwise; returns the ShareErrorCode"""
        ids = (C.c_size_t * len(sender_ids))(*sender_ids)
        return self._f("dev_input_parties")(self.ctx, ids, C.c_size_t(len(sender_ids)), C.c_void_p(x_d), C.c_void_p(r_d), C.c_size_t(N),
                                            C.c_size_t(n), C.c_size_t(t),
                                            *(C.c_void_p(p) for p in (mask_d, masked_d, in_sh_d, status_d, summary_d)), C.c_void_p(stream))

    def output_parties(self, sender_ids, sh_d, N, n, t, out_d, status_d=0, summary_d=0, stream=0):
        """Output's client side (hbmpc_[gl_]dev_output_parties; sender_ids are party ids): the P(0) decode of degree t of the senders'
        rows of sh [party][N], read in place; returns the ShareErrorCode"""
        ids = (C.c_size_t * len(sender_ids))(*sender_ids)
        return self._f("dev_output_parties")(self.ctx, ids, C.c_size_t(len(sender_ids)), C.c_void_p(sh_d), C.c_size_t(N), C.c_size_t(n),
                                             C.c_size_t(t), *(C.c_void_p(p) for p in (out_d, status_d, summary_d)), C.c_void_p(stream))

    def set_fused_input(self, max_elements: int):
        """hbmpc_dev_input_parties is one launch up to this many batch elements (0: always two)"""
        assert self.L.hbmpc_set_fused_input(self.ctx, C.c_size_t(max_elements)) == 0

    def batchrecon_parties(self, eval_senders, reveal_senders, x_d, N, n, d, t, y_d, z_d, opened_d, rstatus_d=0, status_d=0, summary_first_d=0,
                           summary_d=0, stream=0):
        """BatchRecon for all n parties of this device in one call (hbmpc_[gl_]dev_batchrecon_parties; the sender lists are party ids in
        any order): every party's encode of its chunks of d + 1, the recipients' P(0) decodes from eval_senders, the coefficient decode
        of the revealed values from reveal_senders.  One launch for a small batch with exactly d + t + 1 senders in both sets and
        n <= 16, three otherwise; returns the ShareErrorCode"""
        ids1 = (C.c_size_t * max(len(eval_senders), 1))(*eval_senders)
        ids2 = (C.c_size_t * max(len(reveal_senders), 1))(*reveal_senders)
        return self._f("dev_batchrecon_parties")(self.ctx, ids1, C.c_size_t(len(eval_senders)), ids2, C.c_size_t(len(reveal_senders)),
                                                 C.c_void_p(x_d), C.c_size_t(N), C.c_size_t(n), C.c_size_t(d), C.c_size_t(t),
                                                 *(C.c_void_p(p) for p in (y_d, z_d, opened_d, rstatus_d, status_d, summary_first_d, summary_d)),
                                                 C.c_void_p(stream))

    def set_fused_batchrecon(self, max_chunks: int):
        """hbmpc_[gl_]dev_batchrecon_parties is one launch up to this many chunks of d + 1 elements (0: always three)"""
        assert self.L.hbmpc_set_fused_batchrecon(self.ctx, C.c_size_t(max_chunks)) == 0

    def ransha_parties(self, coeffs_d, dealt_d, K, n, t, verify_senders, out_d, yv_d, ws_d, status_d=0, summary_d=0, bad_d=0, stream=0):
        """RanSha for all n parties of this device in one call (hbmpc_[gl_]dev_ransha_parties): coeffs_d [dealer][K][t + 1] -> dealt_d
        [dealer][recipient][K], or with coeffs_d = 0 dealt_d is the input; out_d [party][K][n - 2t], yv_d [party][verifier][K],
        ws_d 2 n n K + max(2t, t + 1) K elements, bad_d [2] uint32 (written).  One launch for a small batch with exactly 2t + 1
        verify senders and 3t + 1 <= n <= 16, the handle's together form otherwise; returns the ShareErrorCode"""
        return self._f("dev_ransha_parties")(self.ctx, C.c_void_p(coeffs_d), C.c_void_p(dealt_d), C.c_size_t(K), C.c_size_t(n), C.c_size_t(t),
                                             C.c_size_t(verify_senders),
                                             *(C.c_void_p(p) for p in (out_d, yv_d, ws_d, status_d, summary_d, bad_d)), C.c_void_p(stream))

    def randousha_parties(self, coeffs_t_d, coeffs_2t_d, dealt_t_d, dealt_2t_d, K, n, t, out_t_d, out_2t_d, yv_t_d, yv_2t_d, ws_d, sel_t_d,
                          sel_2t_d, st_t_d, st_2t_d, bad_d, stream=0):
        """DouSha + RanDouSha for all n parties of this device in one call (hbmpc_[gl_]dev_randousha_parties): two of every buffer of
        ransha_parties, out_* [party][K][t + 1], yv_* [party][n - t - 1][K], ws_d 2 n n K + (n - t - 1) n K elements; sel_* / st_*:
        what the field's verifier calls leave (Fr: (constant term, top coefficient) pairs and status bytes; Goldilocks: constant terms
        and uint32 degrees).  One launch for a small batch with n <= 16; returns the ShareErrorCode"""
        return self._f("dev_randousha_parties")(self.ctx, *(C.c_void_p(p) for p in (coeffs_t_d, coeffs_2t_d, dealt_t_d, dealt_2t_d)), C.c_size_t(K),
                                                C.c_size_t(n), C.c_size_t(t),
                                                *(C.c_void_p(p) for p in (out_t_d, out_2t_d, yv_t_d, yv_2t_d, ws_d, sel_t_d, sel_2t_d, st_t_d,
                                                                          st_2t_d, bad_d)), C.c_void_p(stream))

    def set_fused_producers(self, max_columns: int):
        """hbmpc_[gl_]dev_ransha_parties / _randousha_parties are one launch up to this many columns per dealer (0: never)"""
        assert self.L.hbmpc_set_fused_producers(self.ctx, C.c_size_t(max_columns)) == 0

    def dev_beaver_open_shares_paired(self, a_d, b_d, x_d, y_d, N, parties, de_d, stream=0):
        """de[party][0][N] = a - x, de[party][1][N] = b - y: one P(0) decode over 2 N values per sender opens both"""
        return self._f("dev_beaver_open_shares_paired")(self.ctx, C.c_void_p(a_d), C.c_void_p(b_d), C.c_void_p(x_d), C.c_void_p(y_d),
                                                          C.c_size_t(N), C.c_size_t(parties), C.c_void_p(de_d), C.c_void_p(stream))

    # ---- square roots, inverses, RandBit's phase 2 (csrc/kernels_sqrt.hpp) ----
    def fr_sqrt(self, a):
        """ark's Field::sqrt of every element: (rc, roots, has_root bytes); a root is 0 where ark returns None"""
        a = np.ascontiguousarray(a)
        N = a.shape[0]
        root, ok = self._new((N,)), np.zeros(N, dtype=np.uint8)
        rc = self._f("fr_sqrt")(self.ctx, _p(a), C.c_size_t(N), _p(root), _p(ok))
        return rc, root, ok

    def fr_inverse(self, a):
        """Field::inverse of every element: (rc, inverses, ok bytes); zero has none (inverse 0, ok 0)"""
        a = np.ascontiguousarray(a)
        N = a.shape[0]
        inv, ok = self._new((N,)), np.zeros(N, dtype=np.uint8)
        rc = self._f("fr_inverse")(self.ctx, _p(a), C.c_size_t(N), _p(inv), _p(ok))
        return rc, inv, ok

    def dev_fr_sqrt(self, a_d, N, root_d, has_root_d, stream=0):
        return self._f("dev_fr_sqrt")(self.ctx, C.c_void_p(a_d), C.c_size_t(N), C.c_void_p(root_d), C.c_void_p(has_root_d), C.c_void_p(stream))

    def dev_fr_inverse(self, a_d, N, inv_d, ok_d, stream=0):
        return self._f("dev_fr_inverse")(self.ctx, C.c_void_p(a_d), C.c_size_t(N), C.c_void_p(inv_d), C.c_void_p(ok_d), C.c_void_p(stream))

    def randbit_finalize_parties(self, a_d, sq_d, N, parties, out_d, status_d, summary_d, stream=0):
        """RandBit phase 2 for `parties` parties (hbmpc_[gl_]dev_randbit_finalize_parties; device pointers): a [parties][N], sq [N] the
        opened squares -> out [parties][N], status [N] bytes (0 ok, 1 zero square, 2 no root), summary (16 bytes: u64 first =
        (status << 32) | index, u32 n_failed); returns the ShareErrorCode"""
        return self._f("dev_randbit_finalize_parties")(self.ctx, C.c_void_p(a_d), C.c_void_p(sq_d), C.c_size_t(N), C.c_size_t(parties),
                                                         C.c_void_p(out_d), C.c_void_p(status_d), C.c_void_p(summary_d), C.c_void_p(stream))

    def randbit_parties(self, a_d, ta_d, tb_d, tc_d, N, n, t, desh_d, y_d, z_d, deop_d, sq_d, sqop_d, out_d, status_d, rstatus_de_d, rstatus_sq_d,
                        summary_de_first_d=0, summary_de_d=0, summary_sq_first_d=0, summary_sq_d=0, summary_d=0, stream=0):
        """RandBit for all n parties of this device in one call (hbmpc_[gl_]dev_randbit_parties; device pointers): one launch up to
        hbmpc_set_fused_randbit chunks of t + 1 elements when n <= 16, nine otherwise; returns the ShareErrorCode"""
        return self._f("dev_randbit_parties")(self.ctx, *(C.c_void_p(p) for p in (a_d, ta_d, tb_d, tc_d)), C.c_size_t(N), C.c_size_t(n), C.c_size_t(t),
                                              *(C.c_void_p(p) for p in (desh_d, y_d, z_d, deop_d, sq_d, sqop_d, out_d, status_d, rstatus_de_d,
                                                                        rstatus_sq_d, summary_de_first_d, summary_de_d, summary_sq_first_d,
                                                                        summary_sq_d, summary_d)), C.c_void_p(stream))

    def set_fused_randbit(self, max_chunks: int):
        """hbmpc_[gl_]dev_randbit_parties is one launch up to this many chunks of t + 1 elements (0: always nine)"""
        assert self.L.hbmpc_set_fused_randbit(self.ctx, C.c_size_t(max_chunks)) == 0

    # ---- PRandBit / PRandInt: RISS fold, RISS-to-Shamir conversion, finalize (csrc/kernels_riss.hpp) ----
    FIELD_CAPACITY = 104  # HBMPC_FIELD_CAPACITY

    def riss_tsets(self, n, t):
        """(rc, sets) the maximal unqualified sets in the order the conversion indexes r: combinations(0..n, t) (host only)"""
        return riss_tsets(n, t)

    def dev_riss_fold(self, contrib_d, n, Tn, B, lk_bits, sums_d, bad_d, stream=0):
        """contrib [n][Tn][B] u64 -> sums [Tn][B] u64, bad [n][Tn] bytes (1: a value of (sender, set) exceeds 2^lk_bits)"""
        return self.L.hbmpc_dev_riss_fold(self.ctx, C.c_void_p(contrib_d), C.c_size_t(n), C.c_size_t(Tn), C.c_size_t(B), C.c_size_t(lk_bits),
                                          C.c_void_p(sums_d), C.c_void_p(bad_d), C.c_void_p(stream))

    def dev_riss_convert_parties(self, r_d, n, t, B, out_d, out2_d=0, party_ids=None, own_sets_only=False, stream=0):
        """r [sets][B] u64 -> out [parties][B] elements of this engine's field, out2 [parties][B] GF(2^8) bytes (0: skipped).
        party_ids None: all n parties over all C(n,t) sets; own_sets_only: one party over its own C(n-1,t) sets"""
        ids = None if party_ids is None else _sz(party_ids)
        parties = n if party_ids is None else len(party_ids)
        return self._f("dev_riss_convert_parties")(self.ctx, C.c_void_p(r_d), C.c_size_t(n), C.c_size_t(t), C.c_size_t(B), _p(ids),
                                                     C.c_size_t(parties), C.c_int(1 if own_sets_only else 0), C.c_void_p(out_d),
                                                     C.c_void_p(out2_d), C.c_void_p(stream))

    def riss_convert_parties(self, r, n, t, party_ids=None, own_sets_only=False, with_gf2=True):
        """host-pointer form: r [sets][B] u64 -> (rc, out [parties][B], out2 [parties][B] bytes or None)"""
        r = np.ascontiguousarray(r, dtype=np.uint64)
        B = r.shape[1]
        ids = None if party_ids is None else _sz(party_ids)
        parties = n if party_ids is None else len(party_ids)
        out = self._new((parties, B))
        out2 = np.zeros((parties, B), dtype=np.uint8) if with_gf2 else None
        rc = self._f("riss_convert_parties")(self.ctx, _p(r), C.c_size_t(n), C.c_size_t(t), C.c_size_t(B), _p(ids), C.c_size_t(parties),
                                               C.c_int(1 if own_sets_only else 0), _p(out), _p(out2))
        return rc, out, out2

    def dev_prandbit_finalize_parties(self, opened_d, rp_d, r2_d, B, parties, bp_d, b2_d, stream=0):
        """opened [B] u64 (Goldilocks values), r_p [parties][B] Fr, r_2 [parties][B] bytes -> bp = G(opened) - r_p, b2 = r_2 ^ lsb(opened)"""
        return self.L.hbmpc_dev_prandbit_finalize_parties(self.ctx, C.c_void_p(opened_d), C.c_void_p(rp_d), C.c_void_p(r2_d), C.c_size_t(B),
                                                          C.c_size_t(parties), C.c_void_p(bp_d), C.c_void_p(b2_d), C.c_void_p(stream))

    def prandbit_finalize_parties(self, opened, r_p, r_2):
        """host-pointer form -> (rc, bp [parties][B], b2 [parties][B] bytes)"""
        opened, r_p, r_2 = np.ascontiguousarray(opened, dtype=np.uint64), np.ascontiguousarray(r_p), np.ascontiguousarray(r_2, dtype=np.uint8)
        parties, B = r_2.shape
        bp, b2 = u256((parties, B)), np.zeros((parties, B), dtype=np.uint8)
        rc = self.L.hbmpc_prandbit_finalize_parties(self.ctx, _p(opened), _p(r_p), _p(r_2), C.c_size_t(B), C.c_size_t(parties), _p(bp), _p(b2))
        return rc, bp, b2

    def prandbit_parties(self, eng_gl, contrib_d, bq_d, n, t, B, lk_bits, sums_d, bad_d, rp_d, r2_d, rq_d, rb_d, y_d, z_d, opened_d, bp_d, b2_d,
                         rstatus_d, summary_first_d=0, summary_d=0, open_senders=0, stream=0):
        """PRandBit for all n parties in one call (hbmpc_dev_prandbit_parties; device pointers), on this Fr engine and the Goldilocks
        engine eng_gl of the same device: one launch up to hbmpc_set_fused_prandbit chunks of t + 1 elements for the shapes whose
        tables fit a workgroup's LDS, the eight separate launches otherwise; returns the ShareErrorCode"""
        return self.L.hbmpc_dev_prandbit_parties(self.ctx, eng_gl.ctx if eng_gl is not None else None, C.c_void_p(contrib_d), C.c_void_p(bq_d),
                                                 *(C.c_size_t(v) for v in (n, t, B, lk_bits, open_senders)),
                                                 *(C.c_void_p(p) for p in (sums_d, bad_d, rp_d, r2_d, rq_d, rb_d, y_d, z_d, opened_d, bp_d, b2_d,
                                                                           rstatus_d, summary_first_d, summary_d)), C.c_void_p(stream))

    def prandint_parties(self, contrib_d, n, t, B, lk_bits, sums_d, bad_d, rp_d, stream=0):
        """PRandInt for all n parties in one call (hbmpc_dev_prandint_parties; device pointers); returns the ShareErrorCode"""
        return self.L.hbmpc_dev_prandint_parties(self.ctx, C.c_void_p(contrib_d), *(C.c_size_t(v) for v in (n, t, B, lk_bits)),
                                                 *(C.c_void_p(p) for p in (sums_d, bad_d, rp_d)), C.c_void_p(stream))

    # ---- seeded RISS dealing: contract "hbmpc-riss-chacha20-v1" (include/hbmpc_hip.h, csrc/kernels_riss_sample.hpp) ----
    @staticmethod
    def _seed(seed):
        return (C.c_uint8 * 32).from_buffer_copy(bytes(seed))

    def dev_riss_sample(self, seed, n, t, domain, B, first_index, lk_bits, out_d, stream=0):
        """one sender's contributions from its 32-byte seed -> out [C(n,t)][B] u64 (device pointer); returns the ShareErrorCode"""
        return self.L.hbmpc_dev_riss_sample(self.ctx, None if seed is None else self._seed(seed), C.c_size_t(n), C.c_size_t(t), C.c_size_t(domain),
                                            C.c_size_t(B), C.c_uint64(first_index), C.c_size_t(lk_bits), C.c_void_p(out_d), C.c_void_p(stream))

    def riss_sample(self, seed, n, t, domain, B, first_index, lk_bits):
        """host-pointer form -> (rc, out [C(n,t)][B] uint64)"""
        rc, sets = riss_tsets(n, t)
        out = np.zeros((len(sets) if rc == 0 else 0, B), dtype=np.uint64)
        rc = self.L.hbmpc_riss_sample(self.ctx, self._seed(seed), C.c_size_t(n), C.c_size_t(t), C.c_size_t(domain), C.c_size_t(B),
                                      C.c_uint64(first_index), C.c_size_t(lk_bits), _p(out))
        return rc, out

    def riss_sample_fold(self, seeds_d, n, t, domain, B, first_index, lk_bits, sums_d, stream=0):
        """seeds [n][32] bytes (device pointer) -> sums [C(n,t)][B] u64 over all n senders, contrib never materialised; returns the
        ShareErrorCode"""
        return self.L.hbmpc_dev_riss_sample_fold(self.ctx, C.c_void_p(seeds_d), C.c_size_t(n), C.c_size_t(t), C.c_size_t(domain), C.c_size_t(B),
                                                 C.c_uint64(first_index), C.c_size_t(lk_bits), C.c_void_p(sums_d), C.c_void_p(stream))

    def prandbit_parties_seeded(self, eng_gl, seeds_d, first_index, bq_d, n, t, B, lk_bits, sums_d, bad_d, rp_d, r2_d, rq_d, rb_d, y_d, z_d, opened_d,
                                bp_d, b2_d, rstatus_d, summary_first_d=0, summary_d=0, open_senders=0, stream=0):
        """prandbit_parties with contrib replaced by (seeds [n][32] bytes on the device, first_index): the contributions are drawn in
        domain 0 and folded in registers; always the separate launches; returns the ShareErrorCode"""
        return self.L.hbmpc_dev_prandbit_parties_seeded(self.ctx, eng_gl.ctx if eng_gl is not None else None, C.c_void_p(seeds_d),
                                                        C.c_uint64(first_index), C.c_void_p(bq_d),
                                                        *(C.c_size_t(v) for v in (n, t, B, lk_bits, open_senders)),
                                                        *(C.c_void_p(p) for p in (sums_d, bad_d, rp_d, r2_d, rq_d, rb_d, y_d, z_d, opened_d, bp_d, b2_d,
                                                                                  rstatus_d, summary_first_d, summary_d)), C.c_void_p(stream))

    def prandint_parties_seeded(self, seeds_d, first_index, n, t, B, lk_bits, sums_d, bad_d, rp_d, stream=0):
        """prandint_parties with contrib replaced by (seeds, first_index), drawn in domain 1; returns the ShareErrorCode"""
        return self.L.hbmpc_dev_prandint_parties_seeded(self.ctx, C.c_void_p(seeds_d), C.c_uint64(first_index),
                                                        *(C.c_size_t(v) for v in (n, t, B, lk_bits)),
                                                        *(C.c_void_p(p) for p in (sums_d, bad_d, rp_d)), C.c_void_p(stream))

    def set_fused_prandbit(self, max_chunks: int):
        """hbmpc_dev_prandbit_parties / _prandint_parties are one launch up to this many chunks of t + 1 elements (0: always the
        separate launches); read from the Fr engine"""
        assert self.L.hbmpc_set_fused_prandbit(self.ctx, C.c_size_t(max_chunks)) == 0

    def set_riss_form(self, form: int):
        """A/B aid: 0 by size, 1 a workgroup per 16 parties, 2 a workgroup per party with the sets in slices"""
        assert self.L.hbmpc_set_riss_form(self.ctx, C.c_int(form)) == 0

    # ---- wire codec ----
    def dev_pack_fvec(self, rows_d, row_stride, G, n_rows, payloads_d, payload_stride_bytes, stream=0):
        return self.L.hbmpc_dev_pack_fvec(self.ctx, C.c_void_p(rows_d), C.c_size_t(row_stride), C.c_size_t(G),
                                          C.c_size_t(n_rows), C.c_void_p(payloads_d), C.c_size_t(payload_stride_bytes),
                                          C.c_void_p(stream))

    def dev_unpack_fvec(self, payloads_d, payload_stride_bytes, payload_bytes, G, n_rows, rows_d, row_stride, status_d,
                        stream=0):
        return self.L.hbmpc_dev_unpack_fvec(self.ctx, C.c_void_p(payloads_d), C.c_size_t(payload_stride_bytes),
                                            C.c_size_t(payload_bytes), C.c_size_t(G), C.c_size_t(n_rows),
                                            C.c_void_p(rows_d), C.c_size_t(row_stride), C.c_void_p(status_d),
                                            C.c_void_p(stream))

    def dev_vandermonde_apply_rows(self, x_rows_d, x_row_stride, G, n, d, tmp_d, y_d, stream=0):
        """x as d + 1 rows of G elements (x_row_stride apart) -> y[n][G]; tmp_d: G * (d + 1) elements or 0"""
        return self._f("dev_vandermonde_apply_rows")(self.ctx, C.c_void_p(x_rows_d), C.c_size_t(x_row_stride), C.c_size_t(G), C.c_size_t(n),
                                                       C.c_size_t(d), C.c_void_p(tmp_d), C.c_void_p(y_d), C.c_void_p(stream))

    def dev_vandermonde_apply_rows_split(self, x_rows_d, x_row_stride, G, n, d, tmp_d, y_d, list_row0, list_rows, K, slices, others_d, stream=0):
        """The producers' mixing step: output rows [list_row0, list_row0 + list_rows) as the parties' lists (slices: (dst_dev, party_stride,
        k0, count), at most two), the other rows party-major to others_d [(party (n - list_rows) + r') K + k]
        (hbmpc_dev_vandermonde_apply_rows_split); others_d = None: the other rows to y_d[row][G] (hbmpc_dev_vandermonde_apply_rows_lists)"""
        class _Slice(C.Structure):
            _fields_ = [("dst_dev", C.c_void_p), ("party_stride", C.c_size_t), ("k0", C.c_size_t), ("count", C.c_size_t)]
        arr = (_Slice * len(slices))(*[_Slice(*sl) for sl in slices])
        common = (self.ctx, C.c_void_p(x_rows_d), C.c_size_t(x_row_stride), C.c_size_t(G), C.c_size_t(n), C.c_size_t(d), C.c_void_p(tmp_d),
                  C.c_void_p(y_d), C.c_size_t(list_row0), C.c_size_t(list_rows), C.c_size_t(K), arr, C.c_size_t(len(slices)))
        if others_d is None:
            return self._f("dev_vandermonde_apply_rows_lists")(*common, C.c_void_p(stream))
        return self._f("dev_vandermonde_apply_rows_split")(*common, C.c_void_p(others_d), C.c_void_p(stream))

    def apply_rows_lists_in_kernel(self, G, n, d) -> bool:
        yes = C.c_int(0)
        rc = self.L.hbmpc_dev_apply_rows_lists_in_kernel(self.ctx, C.c_size_t(G), C.c_size_t(n), C.c_size_t(d), C.byref(yes))
        assert rc == 0, self.last_error()
        return bool(yes.value)

    def dev_vandermonde_apply_strided(self, x_d, G, n, d, y_d, y_row_stride, stream=0):
        return self._f("dev_vandermonde_apply_strided")(self.ctx, C.c_void_p(x_d), C.c_size_t(G), C.c_size_t(n), C.c_size_t(d),
                                                        C.c_void_p(y_d), C.c_size_t(y_row_stride), C.c_void_p(stream))

    def dev_encode_fvec(self, x_d, G, n, d, payloads_d, payload_stride_bytes, stream=0):
        return self._f("dev_encode_fvec")(self.ctx, C.c_void_p(x_d), C.c_size_t(G), C.c_size_t(n), C.c_size_t(d),
                                            C.c_void_p(payloads_d), C.c_size_t(payload_stride_bytes), C.c_void_p(stream))

    def dev_validate_fvec(self, payloads_d, payload_stride_bytes, payload_bytes, G, n_rows, status_d, stream=0):
        return self._f("dev_validate_fvec")(self.ctx, C.c_void_p(payloads_d), C.c_size_t(payload_stride_bytes),
                                              C.c_size_t(payload_bytes), C.c_size_t(G), C.c_size_t(n_rows),
                                              C.c_void_p(status_d), C.c_void_p(stream))

    def dev_pack_shares(self, values_d, N, id, degree, payload_d, stream=0):
        return self.L.hbmpc_dev_pack_shares(self.ctx, C.c_void_p(values_d), C.c_size_t(N), C.c_size_t(id),
                                            C.c_size_t(degree), C.c_void_p(payload_d), C.c_void_p(stream))

    def dev_unpack_shares(self, payload_d, payload_bytes, N, id, degree, values_d, status_d, stream=0):
        return self.L.hbmpc_dev_unpack_shares(self.ctx, C.c_void_p(payload_d), C.c_size_t(payload_bytes), C.c_size_t(N),
                                              C.c_size_t(id), C.c_size_t(degree), C.c_void_p(values_d),
                                              C.c_void_p(status_d), C.c_void_p(stream))

    def dev_validate_canonical(self, a_d, N, status_d, stream=0):
        return self.L.hbmpc_dev_validate_canonical(self.ctx, C.c_void_p(a_d), C.c_size_t(N), C.c_void_p(status_d),
                                                   C.c_void_p(stream))

    def dev_traffic_ubench(self, x_d, G, m, y_d, n, stream=0):
        """x[G][m] -> y[n][G] with no arithmetic: what the memory system delivers for an encode's loads and stores"""
        return self.L.hbmpc_dev_traffic_ubench(self.ctx, C.c_void_p(x_d), C.c_size_t(G), C.c_size_t(m), C.c_void_p(y_d), C.c_size_t(n),
                                               C.c_void_p(stream))

    def dev_modmul_ubench(self, out_d, threads, iters, stream=0):
        return self.L.hbmpc_dev_modmul_ubench(self.ctx, C.c_void_p(out_d), C.c_size_t(threads), C.c_uint32(iters),
                                              C.c_void_p(stream))


_N_IN = {"triple_local": 3, "triple_finalize": 2, "beaver_open_shares": 4, "beaver_finalize": 5, "truncpr_rdash": 1,
         "truncpr_open_share": 3, "truncpr_finalize": 3}


def name_inputs(name):
    return _N_IN[name]
