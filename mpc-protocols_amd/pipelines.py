"""Device-resident replays of the reference's arithmetic pipelines for ALL n simulated parties on one GPU (how every
reference test / bench runs: n parties in one process on FakeNetwork) -- thin wrappers over the hbmpc_pipe_* handles of
the C ABI (include/hbmpc_hip.h, csrc/capi_pipelines.hip): the call sequencing, the arena layout and the capture rules live
in the library; this file only names things for the tests and bench.py.

  TripleGen      TripleGenNode::init_batch + BatchReconNode (degree 2t) + try_finalize_triple_gen
                 triple_gen/triple_generation.rs:304-364,164-232; batch_recon/batch_recon.rs:144-185,332-481
  FpMul          FPMulNode::init = Multiply (Beaver, RBC path) + TruncPrNode
                 fpmul/fpmul.rs:61-110, mul/multiplication.rs:417-426,57-139, fpmul/truncpr.rs:185-318
  RanSha         RanShaNode::init_batch + init_ransha_batch + reconstruction_handler + try_finalize
                 share_gen/share_gen.rs:232-289,401-454,516-530,199-203
  RanDouSha      DouShaNode::init_batch + RanDouShaNode::init_batch + reconstruction_handler + try_finalize
                 double_share/double_share_generation.rs:151-215, ran_dou_sha/mod.rs:371-449,569-602,314-331
  Preprocessing  run_preprocessing's triple part (honeybadger/mod.rs:1239-1393): RanSha -> a, b; RanDouSha -> r; TripleGen
  Mul            Multiply (Beaver, RBC path): the opened shares, the open, finalize_mul
                 honeybadger/mod.rs:543-628, mul/multiplication.rs:417-426,102-139,57-100
  Input          the client's open of the masks, masked = x + mask, the servers' masked - r
                 honeybadger/input/input.rs:489-506, 85-100, 300-301
  Output         the client's open of the result shares                      honeybadger/output/output.rs:157-177
  TruncPr        TruncPrNode on its own                                      fpmul/truncpr.rs:185-318
  FpDivConst     FPDivConstNode: a * w for a public reciprocal w, then TruncPr   fpdiv/fpdiv_const.rs:61-99, fpdiv/mod.rs:8-60
  RandBit        RandBit: Beaver square of a, BatchRecon of a^2, phase 2   fpmul/rand_bit.rs:242-293,197-220
  PRandInt       fold of the RISS contributions, conversion to Fr shares   fpmul/prandbitd.rs:667-684,311-356
  PRandBit       ... and to Goldilocks and GF(2^8), open r + b, finalize   fpmul/prandbitd.rs:311-356,437-446,189-211
  PRandIntPipe / PRandBitPipe  the same two over the hbmpc_pipe_prandint / _prandbit handles: run() is ONE device call
                 (hbmpc_dev_prandint_parties / hbmpc_dev_prandbit_parties), one launch for a small batch
  FixedPrep      run_preprocessing's steps 5 and 6: RanSha -> RanDouSha -> TripleGen -> RandBit over Goldilocks, PRandBit / PRandInt over
                 Fr, and take() from the pools they fill          honeybadger/mod.rs:1396-1410, 1951-2150, 1031-1045 (csrc/capi_pipelines_fixedprep.hip)
PRandInt and PRandBit are the compositions of eight device calls over two contexts (their prepare() / finish() seam lets a test stand
between the parties' messages and the open); PRandIntPipe and PRandBitPipe are the handles (csrc/capi_pipelines_riss.hip).
"""
from __future__ import annotations

import ctypes as C

import numpy as np


class _Pipe:
    """One hbmpc_pipe handle.  Device buffers are reached by name: `pipe.a`, `pipe.out`, ... are raw device pointers
    (hbmpc_pipe_buffer).  run(check=False) only enqueues on the stream; run(check=True) reads the summary back after every
    decode and raises where the reference's `?` would return the error."""
    _own = True

    def __init__(self, eng, handle, stream):
        self.eng, self.h, self.stream = eng, handle, stream
        self.U = eng.ebytes  # bytes per element of the engine's field
        self._ptrs = {}

    def _rc(self, rc, what):
        if rc != 0:
            raise RuntimeError(f"{what} -> ShareErrorCode {rc}: {self.eng.last_error()}")

    @classmethod
    def _create(cls, eng, fn, *args, stream=0):
        h = C.c_void_p()
        rc = getattr(eng.L, fn)(eng.ctx, *[C.c_size_t(a) for a in args], C.c_void_p(stream), C.byref(h))
        if rc != 0:
            raise RuntimeError(f"{fn}{args} -> ShareErrorCode {rc}: {eng.last_error()}")
        return h

    def buffer(self, name):
        """(device pointer, elements) of a named buffer of this pipeline"""
        if name not in self._ptrs:
            p, n = C.c_void_p(), C.c_size_t()
            self._rc(self.eng.L.hbmpc_pipe_buffer(self.h, name.encode(), C.byref(p), C.byref(n)), f"buffer {name!r}")
            self._ptrs[name] = (p.value or 0, n.value)
        return self._ptrs[name]

    def __getattr__(self, name):  # pipe.a, pipe.coeffs, ...: the device pointer of that buffer
        if name.startswith("_") or name in ("eng", "h", "stream", "U"):
            raise AttributeError(name)
        try:
            return self.buffer(name)[0]
        except RuntimeError:
            raise AttributeError(name) from None

    def upload_named(self, name, arr):
        arr = np.ascontiguousarray(arr)
        self._rc(self.eng.L.hbmpc_pipe_upload(self.h, name.encode(), arr.ctypes.data_as(C.c_void_p), C.c_size_t(arr.nbytes // self.eng.ebytes)),
                 f"upload {name!r}")

    def download_named(self, name, shape):
        out = self.eng._new(shape)
        self._rc(self.eng.L.hbmpc_pipe_download(self.h, name.encode(), out.ctypes.data_as(C.c_void_p), C.c_size_t(out.nbytes // self.eng.ebytes)),
                 f"download {name!r}")
        return out

    def _call(self, fn, check):
        self.eng.L.hbmpc_pipe_set_checked(self.h, C.c_int(1 if check else 0))
        self._rc(getattr(self.eng.L, fn)(self.h), fn)

    def run(self, check=True):
        self._call("hbmpc_pipe_run", check)

    def capture(self):
        assert self.stream, "capture needs an explicit stream"
        self._rc(self.eng.L.hbmpc_pipe_capture(self.h), "capture")

    def replay(self):
        self._rc(self.eng.L.hbmpc_pipe_replay(self.h), "replay")

    def sync(self):
        self._rc(self.eng.L.hbmpc_pipe_sync(self.h), "sync")

    def summary(self):
        s = np.zeros(4, dtype=np.uint32)
        self._rc(self.eng.L.hbmpc_pipe_summary(self.h, s.ctypes.data_as(C.c_void_p)), "summary")
        return s

    def _bad(self):
        """{verifier checks that failed, first failing batch element} of a producer (synchronises)"""
        b = np.zeros(2, dtype=np.uint32)
        self._rc(self.eng.L.hbmpc_pipe_verdict(self.h, b.ctypes.data_as(C.c_void_p)), "verdict")
        return int(b[0]), int(b[1])

    def close(self):
        if self.h and self._own:
            self.eng.L.hbmpc_pipe_destroy(self.h)
        self.h = None


class TripleGen(_Pipe):
    """n parties, threshold t, N triples (N a multiple of 2t+1).  Buffers a, b, r2t, rt, c are [party][N] canonical.
    Works in either field: the reference runs TripleGenNode over Fr and, in PreprocNodesSmallField
    (honeybadger/mod.rs:316-324), over GoldilocksField -- the element size follows the engine's field.  run() is one library call
    (hbmpc_[gl_]dev_triplegen_parties): one launch up to 1 024 chunks of 2t + 1 triples when n = 3t + 1 <= 16, four launches beyond."""

    def __init__(self, eng, n, t, N, stream=0, _handle=None):
        self.n, self.t, self.N, self.m, self.G = n, t, N, 2 * t + 1, N // (2 * t + 1)
        super().__init__(eng, _handle or self._create(eng, "hbmpc_pipe_triplegen_create", n, t, N, stream=stream), stream)

    def upload(self, a, b, r2t, rt):
        for name, src in (("a", a), ("b", b), ("r2t", r2t), ("rt", rt)):
            self.upload_named(name, src)

    def download_c(self):
        return self.download_named("c", (self.n, self.N))


class FpMul(_Pipe):
    """Fixed-point multiplication of N element pairs for n parties: Beaver mul (a-x, b-y opened by direct robust
    interpolation, i.e. the RBC path of Multiply::init for < t+1 leftovers that FPMulNode always takes) followed by TruncPr
    with k-bit values and m fractional bits.  open_senders: how many parties' shares an open interpolates from.  Default
    2t+1: the reference opens as soon as that many have arrived (multiplication.rs:388,617, truncpr.rs:202) -- with d = t
    that is exactly d + t + 1, a decode with no OEC round, which the library runs as one launch.  n = every party's share.
    run() is one library call (hbmpc_dev_fpmul_parties): ONE launch up to 2 048 elements, five launches up to 8 192, four beyond
    (the first open then forms its senders' shares itself); summary_first / summary hold the two opens' summaries."""

    def __init__(self, eng, n, t, N, k, m, stream=0, open_senders=None):
        self.n, self.t, self.N, self.k, self.m = n, t, N, k, m
        self.open_senders = 2 * t + 1 if open_senders is None else open_senders
        super().__init__(eng, self._create(eng, "hbmpc_pipe_fpmul_create", n, t, N, k, m, self.open_senders, stream=stream), stream)

    def upload(self, x, y, ta, tb, tc, rbits, rint):
        for name, src in (("x", x), ("y", y), ("ta", ta), ("tb", tb), ("tc", tc), ("rbits", rbits), ("rint", rint)):
            self.upload_named(name, src)

    def download(self, which="out"):
        return self.download_named(which, (self.n, self.N))


class Mul(_Pipe):
    """Multiply (Beaver; honeybadger/mod.rs:543-628) of N element pairs for n parties, in either field: a - x and b - y opened by direct
    robust interpolation, then finalize_mul.  Buffers x, y, ta, tb, tc, out are [party][N], desh [party][2][N], deop [2 N] (dop, eop:
    its halves, [N] each), status 2 N bytes (chunk g: the a - x of element g, chunk N + g its b - y), summary the open's.
    open_senders as in FpMul.  run() is one library call (hbmpc_[gl_]dev_mul_parties): over Fr ONE launch up to hbmpc_set_fused_mul
    elements when the open has exactly 2t + 1 senders, three launches otherwise."""

    def __init__(self, eng, n, t, N, stream=0, open_senders=None):
        self.n, self.t, self.N = n, t, N
        self.open_senders = 2 * t + 1 if open_senders is None else open_senders
        super().__init__(eng, self._create(eng, "hbmpc_pipe_mul_create", n, t, N, self.open_senders, stream=stream), stream)

    def upload(self, x, y, ta, tb, tc):
        for name, src in (("x", x), ("y", y), ("ta", ta), ("tb", tb), ("tc", tc)):
            self.upload_named(name, src)

    def download(self, which="out"):
        shape = {"deop": (2 * self.N,), "dop": (self.N,), "eop": (self.N,), "desh": (self.n, 2, self.N)}.get(which, (self.n, self.N))
        return self.download_named(which, shape)


class Input(_Pipe):
    """Input (honeybadger/input/input.rs:489-506, 85-100, 300-301) of N client values for n parties, in either field: the masks are
    opened from parties 0 .. open_senders - 1 (default 2t + 1), masked = x + mask, out[p] = masked - r[p].  Buffers x, mask, masked
    are [N], r and out [party][N], status N bytes, summary the open's.  An element whose mask does not open is refused: zeros in mask,
    masked and out, never x + 0; run(check=True) then raises where the reference's `?` returns the error.  run() is one library call
    (hbmpc_[gl_]dev_input_parties): over Fr ONE launch up to hbmpc_set_fused_input elements when the open has exactly 2t + 1 senders,
    two launches otherwise."""

    def __init__(self, eng, n, t, N, stream=0, open_senders=None):
        self.n, self.t, self.N = n, t, N
        self.open_senders = 2 * t + 1 if open_senders is None else open_senders
        super().__init__(eng, self._create(eng, "hbmpc_pipe_input_create", n, t, N, self.open_senders, stream=stream), stream)

    def upload(self, x, r):
        self.upload_named("x", x)
        self.upload_named("r", r)

    def download(self, which="out"):
        return self.download_named(which, (self.n, self.N) if which in ("out", "r") else (self.N,))


class Output(_Pipe):
    """Output (honeybadger/output/output.rs:157-177) of N result values from n parties' shares sh [party][N], in either field: out [N]
    is the P(0) decode of degree t from parties 0 .. open_senders - 1 (default 2t + 1); status N bytes, summary the open's.  run() is
    one library call (hbmpc_[gl_]dev_output_parties); run(check=True) raises where the reference's first error aborts."""

    def __init__(self, eng, n, t, N, stream=0, open_senders=None):
        self.n, self.t, self.N = n, t, N
        self.open_senders = 2 * t + 1 if open_senders is None else open_senders
        super().__init__(eng, self._create(eng, "hbmpc_pipe_output_create", n, t, N, self.open_senders, stream=stream), stream)

    def upload(self, sh):
        self.upload_named("sh", sh)

    def download(self, which="out"):
        return self.download_named(which, (self.n, self.N) if which == "sh" else (self.N,))


class BatchRecon(_Pipe):
    """BatchRecon (honeybadger/batch_recon/batch_recon.rs) of N = G (d + 1) shared values of degree d for n parties, in either field.
    Buffers: x [party][N] (input); Y [party][recipient][G] the EvalBatch messages; Z [recipient][G] the RevealBatch messages; opened [N];
    rstatus n G bytes (byte j G + g: recipient j's decode of chunk g), status G bytes; summary_first / summary the two decodes'.
    eval_senders / reveal_senders: parties 0 .. S - 1 whose messages everyone decodes from (0: d + t + 1, a decode with no OEC round).
    run() is one library call (hbmpc_[gl_]dev_batchrecon_parties): ONE launch up to hbmpc_set_fused_batchrecon chunks (512 over Fr, 256 over Goldilocks) when both
    sets have exactly d + t + 1 senders and n <= 16, three launches otherwise.  deal() / finish() are its two arms as separate launches (the
    encode and the recipients' decodes up to Z; the decode of Z): rows of Z may be rewritten in between."""

    def __init__(self, eng, n, t, d, N, eval_senders=0, reveal_senders=0, stream=None):
        self.n, self.t, self.d, self.N, self.G = n, t, d, N, N // (d + 1) if d + 1 else 0
        super().__init__(eng, self._create(eng, "hbmpc_pipe_batchrecon_create", n, t, d, N, eval_senders, reveal_senders, stream=stream or 0), stream or 0)

    def upload(self, x):
        self.upload_named("x", x)

    def deal(self, check=False):
        self._call("hbmpc_pipe_deal", check)

    def finish(self, check=False):
        self._call("hbmpc_pipe_finish", check)

    def download(self, which="opened"):
        shape = {"x": (self.n, self.N), "Y": (self.n, self.n, self.G), "Z": (self.n, self.G), "opened": (self.N,)}[which]
        return self.download_named(which, shape)

    def bytes_of(self, name, nbytes):
        """raw bytes of a named buffer (status bytes, summaries): hbmpc_pipe_download counts field elements"""
        out = np.zeros(nbytes, dtype=np.uint8)
        self.sync()
        self._rc(self.eng.L.hbmpc_memcpy_d2h(self.eng.ctx, out.ctypes.data_as(C.c_void_p), C.c_void_p(self.buffer(name)[0]),
                                             C.c_size_t(nbytes), C.c_void_p(self.stream)), f"bytes of {name!r}")
        self.sync()
        return out

    def status(self, which="status"):
        """the status bytes: "status" [G] of the revealed values' decode, "rstatus" [n][G] of the recipients' decodes"""
        return self.bytes_of("rstatus", self.n * self.G).reshape(self.n, self.G) if which == "rstatus" else self.bytes_of("status", self.G)

    def summary_first(self):
        return self.bytes_of("summary_first", 16).view(np.uint32)


class TruncPr(_Pipe):
    """TruncPr (fpmul/truncpr.rs:185-318) of N values for n parties: k-bit values, m fractional bits dropped.  Buffers a, rint, rdash,
    osh, out are [party][N], rbits [party][m][N], cop [N] the opened value, status [N] bytes, summary the open's.  open_senders as in
    FpMul.  run() is one library call (hbmpc_dev_truncpr_parties): ONE launch up to hbmpc_set_fused_truncpr elements when the open
    has exactly 2t + 1 senders, three launches otherwise."""
    _with_multiplier = 0

    def __init__(self, eng, n, t, N, k, m, stream=0, open_senders=None):
        self.n, self.t, self.N, self.k, self.m = n, t, N, k, m
        self.open_senders = 2 * t + 1 if open_senders is None else open_senders
        h = C.c_void_p()
        rc = eng.L.hbmpc_pipe_truncpr_create(eng.ctx, *[C.c_size_t(v) for v in (n, t, N, k, m, self.open_senders)], C.c_int(self._with_multiplier),
                                             C.c_void_p(stream), C.byref(h))
        if rc != 0:
            raise RuntimeError(f"hbmpc_pipe_truncpr_create{(n, t, N, k, m, self.open_senders, self._with_multiplier)} -> ShareErrorCode {rc}: {eng.last_error()}")
        super().__init__(eng, h, stream)

    def upload(self, a, rbits, rint):
        for name, src in (("a", a), ("rbits", rbits), ("rint", rint)):
            self.upload_named(name, src)

    def download(self, which="out"):
        return self.download_named(which, (self.N,) if which in ("cop", "w") else (self.n, self.N))


class FpDivConst(TruncPr):
    """FPDivConstNode (fpdiv/fpdiv_const.rs:61-99) for n parties: N fixed-point values of k bits with f fractional bits, each divided
    by a PUBLIC denominator -- c = a * w with w = fixed_point_reciprocal_scaled(denominator) (fpdiv/mod.rs:8-60), then TruncPr of c
    with 2 k bits and m = f.  Adds the buffers w [N] and c [party][N]."""
    _with_multiplier = 1

    def __init__(self, eng, n, t, N, k, f, stream=0, open_senders=None):
        self.k_fixed, self.f = k, f
        super().__init__(eng, n, t, N, 2 * k, f, stream=stream, open_senders=open_senders)

    def set_denominators(self, denom):
        """denom [N] canonical field elements (the integers of ClearFixedPoint): runs the host helper, uploads w; raises on an invalid divisor"""
        from .hbmpc import fixed_point_reciprocal_scaled
        rc, w, bad = fixed_point_reciprocal_scaled(denom, self.f)
        if rc != 0:
            raise RuntimeError(f"hbmpc_fixed_point_reciprocal_scaled -> ShareErrorCode {rc} (first invalid divisor: {bad})")
        self.upload_named("w", w)
        return w


class _Producer(_Pipe):
    """What RanSha and RanDouSha share: every dealer p deals K secrets to the n recipients (the dealers' polynomials are the
    INPUT: coefficient rows [dealer][K][deg + 1], column 0 the secret -- filled by the host, or on the device by
    hbmpc_dev_fill_coeffs: the reference draws them from each party's rng), recipient j multiplies the vector of the n
    shares it received for batch element k by the n x n Vandermonde matrix make_vandermonde(n, n - 1), row i of the result
    goes to verifier i, and the other rows are the party's output.  deal() / finish() are the two halves of run()."""

    def deal(self):
        self._call("hbmpc_pipe_deal", False)

    def finish(self, check=True):
        self._call("hbmpc_pipe_finish", False)
        if check:
            bad, first = self._bad()
            if bad:
                raise RuntimeError(f"{type(self).__name__}: {bad} verifier checks failed (first: column {first})")

    def run(self, check=True):
        self.deal()
        self.finish(check)


class RanSha(_Producer):
    """K batch elements per dealer -> (n - 2t) K random degree-t sharings per party, verified by parties 0 .. 2t - 1.
    verify_senders: how many parties' shares a verifier reconstructs from.  Default 2t + 1: the reference's handler fires
    as soon as that many have arrived (share_gen.rs:497), i.e. the first 2t + 1 senders -- a decode with no OEC round."""

    def __init__(self, eng, n, t, K, stream=0, verify_senders=None, _handle=None):
        self.n, self.t, self.K, self.nout = n, t, K, (n - 2 * t) * K
        self.verify_senders = 2 * t + 1 if verify_senders is None else verify_senders
        super().__init__(eng, _handle or self._create(eng, "hbmpc_pipe_ransha_create", n, t, K, self.verify_senders, stream=stream), stream)

    def upload(self, coeffs):
        self.upload_named("coeffs", coeffs)

    def download(self):
        return self.download_named("out", (self.n, self.nout))


class RanDouSha(_Producer):
    """K batch elements per dealer -> (t + 1) K double sharings ([r]_t, [r]_2t) per party, verified by parties t + 1 .. n - 1
    (each reconstructs both polynomials through ALL n shares: ran_dou_sha/mod.rs:557-559 waits for 2t + 1 degree-t and n
    degree-2t shares, and in one process all n of both have arrived)."""

    def __init__(self, eng, n, t, K, stream=0, _handle=None):
        self.n, self.t, self.K, self.nout = n, t, K, (t + 1) * K
        super().__init__(eng, _handle or self._create(eng, "hbmpc_pipe_randousha_create", n, t, K, stream=stream), stream)

    def upload(self, coeffs_t, coeffs_2t):
        self.upload_named("coeffs_t", coeffs_t)
        self.upload_named("coeffs_2t", coeffs_2t)

    def download(self):
        return self.download_named("out_t", (self.n, self.nout)), self.download_named("out_2t", (self.n, self.nout))


class Preprocessing(_Pipe):
    """run_preprocessing's triple part (honeybadger/mod.rs:1239-1393) for all n parties, device-resident from the dealers'
    polynomials to [c]_t: RanSha produces 2 N random sharings per party (a = the first N, b = the next N:
    take_random_shares twice, :1307-1316), RanDouSha the N double sharings, TripleGen consumes them where they lie."""

    def __init__(self, eng, n, t, N, stream=0):
        assert N % (2 * t + 1) == 0
        self.n, self.t, self.N = n, t, N
        self.K_rs = -(-2 * N // (n - 2 * t))             # RanSha batch elements per dealer: (n - 2t) K >= 2 N
        self.K_rd = -(-N // (t + 1))                     # RanDouSha: (t + 1) K >= N
        super().__init__(eng, self._create(eng, "hbmpc_pipe_preprocessing_create", n, t, N, stream=stream), stream)
        self.rs = RanSha(eng, n, t, self.K_rs, stream, _handle=self._part("ransha"))
        self.rd = RanDouSha(eng, n, t, self.K_rd, stream, _handle=self._part("randousha"))
        self.tg = TripleGen(eng, n, t, N, stream, _handle=self._part("triplegen"))
        for part in (self.rs, self.rd, self.tg):
            part._own = False  # borrowed: destroyed with this handle

    def _part(self, name):
        h = C.c_void_p()
        self._rc(self.eng.L.hbmpc_pipe_part(self.h, name.encode(), C.byref(h)), f"part {name!r}")
        return h

    def run(self, check=True):
        super().run(check)
        if check:
            bad, first = self._bad()
            if bad:
                raise RuntimeError(f"Preprocessing: {bad} verifier checks failed (first: column {first})")


class RandBit(_Pipe):
    """N random bits for n parties from N shared values a and one Beaver triple (ta, tb, tc) each, over either field (N a
    multiple of t + 1).  Buffers a, ta, tb, tc, out, sq are [party][N]; sqop [N] the opened squares; status [N] bytes and summary
    (u64 first, u32 n_failed) the finalize's; rstatus_de / rstatus_sq and summary_de_first, summary_de, summary_sq_first,
    summary_sq the four decodes'.  run(check=True) raises with HBMPC_ZERO_SQUARE (102) / HBMPC_NO_SQUARE_ROOT (103) where
    phase 2's `?` returns, or with a failed open's error.  run() is one library call (hbmpc_[gl_]dev_randbit_parties): ONE launch up to
    hbmpc_set_fused_randbit chunks of t + 1 elements when n <= 16 (256 over Fr, 1 024 over Goldilocks), nine launches beyond."""

    ZERO_SQUARE, NO_SQUARE_ROOT = 102, 103

    def __init__(self, eng, n, t, N, stream=0, _handle=None):
        self.n, self.t, self.N = n, t, N
        super().__init__(eng, _handle or self._create(eng, "hbmpc_pipe_randbit_create", n, t, N, stream=stream), stream)

    def upload(self, a, ta, tb, tc):
        for name, src in (("a", a), ("ta", ta), ("tb", tb), ("tc", tc)):
            self.upload_named(name, src)

    def download(self, which="out"):
        shape = (self.N,) if which == "sqop" else (self.n, self.N)
        return self.download_named(which, shape)

    def bytes_of(self, name, nbytes):
        """raw bytes of a named buffer (status bytes, summaries): hbmpc_pipe_download counts field elements"""
        out = np.zeros(nbytes, dtype=np.uint8)
        self.sync()
        self._rc(self.eng.L.hbmpc_memcpy_d2h(self.eng.ctx, out.ctypes.data_as(C.c_void_p), C.c_void_p(self.buffer(name)[0]),
                                             C.c_size_t(nbytes), C.c_void_p(self.stream)), f"bytes of {name!r}")
        self.sync()
        return out

    def status(self):
        return self.bytes_of("status", self.N)

    def rb_summary(self):
        """(first, n_failed) of the finalize"""
        b = self.bytes_of("summary", 16)
        return int(b[:8].view(np.uint64)[0]), int(b[8:12].view(np.uint32)[0])


class _RissPipe(_Pipe):
    """What the PRandBit / PRandInt handles share: every buffer has an element type of its own (u64, U256 or bytes), and
    hbmpc_pipe_upload / _download count elements of that type."""
    _EB = {"contrib": 8, "b_q": 8, "sums": 8, "bad": 1, "r_p": 32, "r_2": 1, "r_q": 8, "rb": 8, "Y": 8, "Z": 8, "opened": 8, "b_p": 32, "b_2": 1,
           "rstatus": 1, "summary_first": 1, "summary": 1}

    def _seeded_names(self):
        """a seeded handle's own table of buffers: seeds ([n][32] bytes) where contrib was"""
        self._EB = {k: v for k, v in self._EB.items() if k != "contrib"} | {"seeds": 1}

    def upload_named(self, name, arr):
        arr = np.ascontiguousarray(arr)
        self._rc(self.eng.L.hbmpc_pipe_upload(self.h, name.encode(), arr.ctypes.data_as(C.c_void_p), C.c_size_t(arr.nbytes // self._EB[name])),
                 f"upload {name!r}")

    def download_named(self, name, shape=None):
        """the whole buffer (shape: of the result; default flat): uint64 ([..., 4] for the U256 buffers) or uint8"""
        eb, count = self._EB[name], self.buffer(name)[1]
        out = np.zeros((count, 4) if eb == 32 else (count,), dtype=np.uint8 if eb == 1 else np.uint64)
        self._rc(self.eng.L.hbmpc_pipe_download(self.h, name.encode(), out.ctypes.data_as(C.c_void_p), C.c_size_t(count)), f"download {name!r}")
        return out if shape is None else out.reshape(shape)

    def set_stream_index(self, index):
        """seeded handles (hbmpc_pipe_set_stream_index): the next run() draws at [index, index + B) and then advances by B"""
        self._rc(self.eng.L.hbmpc_pipe_set_stream_index(self.h, C.c_uint64(index)), "set_stream_index")

    def upload_seeds(self, seeds):
        """seeded handles: one 32-byte seed per sender"""
        seeds = np.frombuffer(b"".join(bytes(s) for s in seeds), dtype=np.uint8)
        assert seeds.size == 32 * self.n
        self.upload_named("seeds", seeds)


class PRandIntPipe(_RissPipe):
    """PRandInt for all n parties as one handle (hbmpc_pipe_prandint_create; prandbitd.rs:667-684, 311-356): contrib [n][C(n,t)][B] u64
    -> sums [C(n,t)][B], bad [n][C(n,t)] verdict bytes, r_p [n][B] the Fr shares.  Any B.  run() is one library call
    (hbmpc_dev_prandint_parties): ONE launch up to hbmpc_set_fused_prandbit chunks of t + 1 elements for the shapes whose tables fit a
    workgroup's LDS, two launches otherwise.  seeded=True (hbmpc_pipe_prandint_create_seeded): a buffer seeds [n][32] bytes and no
    contrib; run() draws the contributions on the device at the handle's stream index (contract "hbmpc-riss-chacha20-v1", domain 1) and
    advances it by B; capture() is refused."""

    def __init__(self, eng_fr, n, t, B, lk_bits, stream=0, _handle=None, seeded=False):
        self.n, self.t, self.B, self.lk_bits, self.seeded = n, t, B, lk_bits, seeded
        if seeded:
            self._seeded_names()
        h = _handle or C.c_void_p()
        fn = "hbmpc_pipe_prandint_create_seeded" if seeded else "hbmpc_pipe_prandint_create"
        rc = 0 if _handle else getattr(eng_fr.L, fn)(eng_fr.ctx, *[C.c_size_t(v) for v in (n, t, B, lk_bits)], C.c_void_p(stream), C.byref(h))
        if rc != 0:
            raise RuntimeError(f"{fn}{(n, t, B, lk_bits)} -> ShareErrorCode {rc}: {eng_fr.last_error()}")
        super().__init__(eng_fr, h, stream)


class PRandBitPipe(_RissPipe):
    """PRandBit for all n parties as one handle (hbmpc_pipe_prandbit_create; prandbitd.rs:667-684, 311-356, 437-446, 189-211), from an Fr
    engine and a Goldilocks engine on the same device.  Inputs contrib [n][C(n,t)][B] u64, b_q [n][B]; outputs sums, bad, r_p, r_2, r_q, rb,
    opened [B], b_p [n][B] Fr, b_2 [n][B] bytes, rstatus, summary_first, summary.  B a multiple of t + 1.  open_senders: how many parties'
    messages the open decodes from; default 2t + 1 (no OEC round: BatchRecon acts as soon as d + t + 1 values have arrived).  run() is one
    library call (hbmpc_dev_prandbit_parties): ONE launch up to hbmpc_set_fused_prandbit chunks when the open has exactly 2t + 1 senders
    and the tables fit a workgroup's LDS ((4,1) .. (12,3)), eight launches otherwise.  seeded=True (hbmpc_pipe_prandbit_create_seeded):
    seeds [n][32] bytes instead of contrib, drawn in domain 0 at the handle's stream index, always the separate launches; capture() is
    refused."""

    def __init__(self, eng_gl, eng_fr, n, t, B, lk_bits, stream=0, open_senders=None, _handle=None, seeded=False):
        self.n, self.t, self.B, self.lk_bits, self.G, self.seeded = n, t, B, lk_bits, B // (t + 1), seeded
        self.open_senders = 2 * t + 1 if open_senders is None else open_senders
        self.fr = eng_fr
        if seeded:
            self._seeded_names()
        h = _handle or C.c_void_p()
        fn = "hbmpc_pipe_prandbit_create_seeded" if seeded else "hbmpc_pipe_prandbit_create"
        rc = 0 if _handle else getattr(eng_fr.L, fn)(eng_fr.ctx, eng_gl.ctx, *[C.c_size_t(v) for v in (n, t, B, lk_bits, self.open_senders)],
                                                     C.c_void_p(stream), C.byref(h))
        if rc != 0:
            raise RuntimeError(f"{fn}{(n, t, B, lk_bits, self.open_senders)} -> ShareErrorCode {rc}: {eng_fr.last_error()}")
        super().__init__(eng_gl, h, stream)  # the handle's own context is the Goldilocks one (the open's decode counters are its)

    def open_summary(self):
        """(n_fallback, n_failed, first_failed, first_error) of the two decodes of the open"""
        return [tuple(int(v) for v in self.download_named(k).view(np.uint32)) for k in ("summary_first", "summary")]


class FixedPrep(_RissPipe):
    """The second half of run_preprocessing (honeybadger/mod.rs:1396-1410, 1951-2150) for all n parties as one handle
    (hbmpc_pipe_fixedprep_create): one refill of the r_bits / r_int pools that mul_fixed drains, from the dealers' Goldilocks polynomials
    and the RISS contributions.  Sizes (the reference's arithmetic): R = n_prandbit up to a multiple of t + 1, T = R up to a multiple of
    2t + 1, K1 = ceil((R + 2T) / (n - 2t)) RanSha columns per dealer, K2 = ceil(T / (t + 1)) RanDouSha columns.  Parts (borrowed): rs, rd,
    tg, rb over Goldilocks, pb (PRandBitPipe), pi (PRandIntPipe); None where that half is absent.  Buffers r_bits [n][R] U256, r_bits2
    [n][R] bytes, r_int [n][n_prandint] U256.  deal() / finish() are the halves of run(); take(consumer, N) moves N elements' worth from
    the front of the pools into an FpMul / TruncPr handle's rbits / rint.  seeded=True (hbmpc_pipe_fixedprep_create_seeded): pb and pi are
    seeded handles, fed from this handle's own seeds [n][32] bytes and stream index before each run; capture() is refused."""
    _EB = {"r_bits": 32, "r_bits2": 1, "r_int": 32}

    @staticmethod
    def sizes(n, t, n_prandbit):
        """(R, T, K1, K2)"""
        R = -(-n_prandbit // (t + 1)) * (t + 1)
        T = -(-R // (2 * t + 1)) * (2 * t + 1)
        return R, T, -(-(R + 2 * T) // (n - 2 * t)), -(-T // (t + 1))

    def __init__(self, eng_gl, eng_fr, n, t, n_prandbit, n_prandint, lk_bits, stream=0, seeded=False):
        self.n, self.t, self.n_prandbit, self.n_prandint, self.lk_bits, self.fr = n, t, n_prandbit, n_prandint, lk_bits, eng_fr
        self.seeded = seeded
        if seeded:
            self._seeded_names()
        h = C.c_void_p()
        fn = "hbmpc_pipe_fixedprep_create_seeded" if seeded else "hbmpc_pipe_fixedprep_create"
        rc = getattr(eng_fr.L, fn)(eng_fr.ctx, eng_gl.ctx, *[C.c_size_t(v) for v in (n, t, n_prandbit, n_prandint, lk_bits)], C.c_void_p(stream),
                                   C.byref(h))
        if rc != 0:
            raise RuntimeError(f"{fn}{(n, t, n_prandbit, n_prandint, lk_bits)} -> ShareErrorCode {rc}: {eng_fr.last_error()}")
        super().__init__(eng_gl, h, stream)
        self.rs = self.rd = self.tg = self.rb = self.pb = self.pi = None
        if n_prandbit:
            self.R, self.T, self.K1, self.K2 = self.sizes(n, t, n_prandbit)
            self.rs = RanSha(eng_gl, n, t, self.K1, stream, _handle=self._part("ransha"))
            self.rd = RanDouSha(eng_gl, n, t, self.K2, stream, _handle=self._part("randousha"))
            self.tg = TripleGen(eng_gl, n, t, self.T, stream, _handle=self._part("triplegen"))
            self.rb = RandBit(eng_gl, n, t, self.R, stream, _handle=self._part("randbit"))
            self.pb = PRandBitPipe(eng_gl, eng_fr, n, t, self.R, lk_bits, stream, _handle=self._part("prandbit"), seeded=seeded)
        if n_prandint:
            self.pi = PRandIntPipe(eng_fr, n, t, n_prandint, lk_bits, stream, _handle=self._part("prandint"), seeded=seeded)
        for part in (self.rs, self.rd, self.tg, self.rb, self.pb, self.pi):
            if part is not None:
                part._own = False  # borrowed: destroyed with this handle

    _part = Preprocessing._part

    def deal(self):
        self._call("hbmpc_pipe_deal", False)

    def finish(self, check=False):
        self._call("hbmpc_pipe_finish", check)

    def verdict(self):
        return self._bad()

    def available(self):
        """(bits, integers) left in the pools"""
        out = (C.c_size_t * 2)()
        self._rc(self.eng.L.hbmpc_pipe_fixedprep_available(self.h, out), "available")
        return int(out[0]), int(out[1])

    def take_raw(self, m, N, rbits_d, rint_d):
        """hbmpc_pipe_fixedprep_take -> ShareErrorCode (1 = InsufficientShares: nothing written, cursors unchanged)"""
        return self.eng.L.hbmpc_pipe_fixedprep_take(self.h, C.c_size_t(m), C.c_size_t(N), C.c_void_p(rbits_d or None), C.c_void_p(rint_d or None))

    def take(self, consumer, N=None):
        """N (default: all of the consumer's) elements' worth into consumer.rbits [n][m][N] and consumer.rint [n][N]; the consumer (FpMul,
        TruncPr, FpDivConst) holds exactly N elements"""
        N = consumer.N if N is None else N
        assert N == consumer.N, "the consumer's rbits are [n][m][N] for its own N"
        self._rc(self.take_raw(consumer.m, N, consumer.rbits, consumer.rint), "take")


class _Riss:
    """device buffers of the two RISS compositions: named, allocated once, freed by close()"""

    def __init__(self, eng_fr, n, t, B, stream):
        if eng_fr.field != "fr":
            raise RuntimeError("PRandInt / PRandBit -> ShareErrorCode 5: the large field is bls12-381 Fr")
        self.fr, self.n, self.t, self.B = eng_fr, n, t, B
        self._own_stream = not stream  # two contexts share the stream, so stream 0 (each context's own) will not do
        self.stream = stream or eng_fr.stream_create()
        rc, sets = eng_fr.riss_tsets(n, t)
        if rc == 0 and (n < 3 * t + 1 or B == 0):
            rc = 4
        self._rc(rc, f"shape n = {n}, t = {t}, B = {B}")
        self.Tn = len(sets)
        self._bufs = {}

    def _rc(self, rc, what):
        if rc != 0:
            raise RuntimeError(f"{what} -> ShareErrorCode {rc}: {self.fr.last_error()}")

    def _alloc(self, name, nbytes):
        self._bufs[name] = (self.fr.dev_alloc(max(1, nbytes)), nbytes)
        return self._bufs[name][0]

    def __getattr__(self, name):  # pipe.contrib, pipe.r_p, ...: the device pointer of that buffer
        bufs = self.__dict__.get("_bufs", {})
        if name in bufs:
            return bufs[name][0]
        raise AttributeError(name)

    def upload_named(self, name, arr):
        arr = np.ascontiguousarray(arr)
        assert arr.nbytes == self._bufs[name][1], (name, arr.nbytes, self._bufs[name][1])
        self.fr.h2d(self._bufs[name][0], arr, self.stream)
        self.fr.sync(self.stream)

    def download_named(self, name, dtype, shape):
        out = np.zeros(shape, dtype=dtype)
        assert out.nbytes == self._bufs[name][1], (name, out.nbytes, self._bufs[name][1])
        self.fr.sync(self.stream)
        self.fr.d2h(out, self._bufs[name][0], self.stream)
        self.fr.sync(self.stream)
        return out

    def sync(self):
        self.fr.sync(self.stream)

    def close(self):
        for p, _ in self._bufs.values():
            self.fr.dev_free(p)
        self._bufs = {}
        if self._own_stream and self.stream:
            self.fr.stream_destroy(self.stream)
            self.stream = 0

    def _fold_and_fr(self, lk_bits, with_gf2):
        n, t, B = self.n, self.t, self.B
        self._rc(self.fr.dev_riss_fold(self.contrib, n, self.Tn, B, lk_bits, self.sums, self.bad, self.stream), "hbmpc_dev_riss_fold")
        self._rc(self.fr.dev_riss_convert_parties(self.sums, n, t, B, self.r_p, self.r_2 if with_gf2 else 0, stream=self.stream),
                 "hbmpc_dev_riss_convert_parties")


class PRandInt(_Riss):
    """PRandInt for all n parties (prandbitd.rs:667-684, 311-356): contrib [n][C(n,t)][B] u64 the senders' values ->
    sums [C(n,t)][B], bad [n][C(n,t)] verdict bytes, r_p [n][B] the Fr shares of the random integers.  Any B."""

    def __init__(self, eng_fr, n, t, B, stream=0):
        super().__init__(eng_fr, n, t, B, stream)
        self._alloc("contrib", n * self.Tn * B * 8), self._alloc("sums", self.Tn * B * 8), self._alloc("bad", n * self.Tn)
        self._alloc("r_p", n * B * 32)

    def run(self, lk_bits):
        self._fold_and_fr(lk_bits, False)


class PRandBit(_Riss):
    """PRandBit for all n parties on one stream (prandbitd.rs:667-684, 311-356, 437-446, 189-211), from a Goldilocks engine and an Fr
    engine on the same device.  Inputs: contrib [n][C(n,t)][B] u64, b_q [n][B] the Goldilocks shares of the bits.  run():
      fold -> sums, bad;  convert over Fr -> r_p, r_2 (GF(2^8));  convert over Goldilocks -> r_q;  rb = r_q + b_q (fr_op);
      BatchRecon of rb in chunks of t + 1 from all n senders (encode, the recipients' P(0) decodes, the coefficient decode;
      up to t wrong senders are corrected by the decodes' OEC path) -> opened [B];
      finalize -> b_p [n][B] Fr, b_2 [n][B] bytes.
    B must be a multiple of t + 1 (PRandError::Incompatible; here ShareErrorCode 4)."""

    def __init__(self, eng_gl, eng_fr, n, t, B, stream=0):
        super().__init__(eng_fr, n, t, B, stream)
        if eng_gl.field != "goldilocks":
            raise RuntimeError("PRandBit -> ShareErrorCode 5: the small field is Goldilocks")
        if B % (t + 1) != 0:
            raise RuntimeError(f"PRandBit -> ShareErrorCode 4: B = {B} is not a multiple of t + 1")  # prandbitd.rs:472-476
        self.gl = eng_gl
        self.G = G = B // (t + 1)
        self._alloc("contrib", n * self.Tn * B * 8), self._alloc("sums", self.Tn * B * 8), self._alloc("bad", n * self.Tn)
        for name in ("r_p", "b_p"):
            self._alloc(name, n * B * 32)
        for name in ("r_2", "b_2"):
            self._alloc(name, n * B)
        for name in ("b_q", "r_q", "rb"):
            self._alloc(name, n * B * 8)
        self._alloc("Y", n * n * G * 8), self._alloc("Z", n * G * 8), self._alloc("opened", B * 8)
        self._alloc("rstatus", n * G), self._alloc("summary_first", 16), self._alloc("summary", 16)
        self.ids = list(range(n))

    def open(self):
        """BatchRecon of rb [party][G (t + 1)] (batch_recon.rs:157-165, 384-391, 457-467): Y [party][recipient][chunk], Z [recipient][chunk]"""
        n, t, G, gl, st = self.n, self.t, self.G, self.gl, self.stream
        self._rc(gl.dev_batch_recover_strided(self.ids, self.Y, n * G, n * G, n, t, t, self.Z, p0=True, status_d=self.rstatus,
                                              summary_d=self.summary_first, stream=st), "open: P(0) decodes")
        self._rc(gl.dev_batch_recover(self.ids, self.Z, G, n, t, t, self.opened, 0, self.rstatus, self.summary, st), "open: coefficient decode")

    def prepare(self, lk_bits):
        """everything before the parties' messages of the open are exchanged: ... -> Y, every sender's encoded r + b"""
        n, t, B, gl, st = self.n, self.t, self.B, self.gl, self.stream
        self._fold_and_fr(lk_bits, True)
        self._rc(gl.dev_riss_convert_parties(self.sums, n, t, B, self.r_q, 0, stream=st), "hbmpc_gl_dev_riss_convert_parties")
        self._rc(gl.dev_fr_op("add", self.r_q, self.b_q, n * B, self.rb, st), "r + b")
        self._rc(gl.dev_vandermonde_apply_parties(self.rb, self.G, n, t, n, self.Y, st), "open: encode")

    def finish(self):
        self.open()
        self._rc(self.fr.dev_prandbit_finalize_parties(self.opened, self.r_p, self.r_2, self.B, self.n, self.b_p, self.b_2, self.stream),
                 "hbmpc_dev_prandbit_finalize_parties")

    def run(self, lk_bits):
        self.prepare(lk_bits)
        self.finish()

    def open_summary(self):
        """(n_fallback, n_failed, first_failed, first_error) of the two decodes of the open"""
        return [tuple(int(v) for v in self.download_named(k, np.uint32, (4,))) for k in ("summary_first", "summary")]
