#!/usr/bin/env python3
"""FixedPrep timing.  Two measurements, each from a host clock around work that ends in a stream synchronise:

  refill   one refill of the r_bits / r_int pools for all n parties: hbmpc_pipe_fixedprep_create's run(), eager and replayed as a HIP
           graph, against the composition a caller had to assemble before the handle existed -- the six handles (ransha, randousha,
           triplegen, randbit, prandbit, prandint) on one stream with hbmpc_memcpy_d2d_rows for the nine moves between them -- eager and
           replayed.  Honest inputs (random polynomials with equal secrets in the double sharing; contributions below 2^lk).
  take     hbmpc_dev_take_rows at bench.py cfg5's shape (n = 16, m = 16, N = 2^18, 32-byte elements: [16][2^22] -> [16][16][2^18],
           2.1 GB read and 2.1 GB written) against hbmpc_dev_transpose making the same move (one launch, batch = 16) and against a plain
           device copy of the same bytes: GB/s of read + written bytes.  The buffers (4.3 GB together) are larger than the Infinity
           Cache.

    python tools/bench_fixedprep.py [--what refill,take] [--shapes 4:1,7:2,16:5] [--bits 20,65536] [--samples 15] [--calls 5]
Prints ms per call as median (p10 .. p90); run it twice and compare for the run-to-run spread.  A shape whose RISS contributions
(n C(n,t) B u64) exceed --max-contrib-gb is skipped and named."""
import argparse
import ctypes as C
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
P_GL = 2**64 - 2**32 + 1


def lk_for(n, t):
    lk = 55
    while math.comb(n, t) * n * 2**lk + 1 >= P_GL:
        lk -= 1
    return lk


def stats(samples):
    s = np.sort(np.array(samples))
    return "%9.4f (%.4f .. %.4f)" % (float(np.median(s)), float(s[len(s) // 10]), float(s[(len(s) * 9) // 10]))


def timed(fn, sync, samples, calls):
    for _ in range(3):
        fn()
    sync()
    out = []
    for _ in range(samples):
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        sync()
        out.append((time.perf_counter() - t0) * 1e3 / calls)
    return out


def gl_rand(rng, shape):
    return rng.integers(0, P_GL, size=shape, dtype=np.uint64)


def fill(parts, rng, n, t, K1, K2, lk):
    rs, rd, pb, pi = parts
    rs.upload(gl_rand(rng, (n, K1, t + 1)))
    ct, c2 = gl_rand(rng, (n, K2, t + 1)), gl_rand(rng, (n, K2, 2 * t + 1))
    c2[:, :, 0] = ct[:, :, 0]
    rd.upload(ct, c2)
    for h in (pb, pi):
        B = h.B
        Tn = math.comb(n, t)
        h.upload_named("contrib", rng.integers(0, 1 << lk, size=(n, Tn, B), dtype=np.uint64))


def refill(pkg, fr, gl, n, t, nbit, nint, samples, calls):
    pl = pkg.pipelines
    lk = lk_for(n, t)
    st = gl.stream_create()
    R, T, K1, K2 = pl.FixedPrep.sizes(n, t, nbit)
    rng = np.random.default_rng(n * 1000 + nbit)
    prep = pl.FixedPrep(gl, fr, n, t, nbit, nint, lk, stream=st)
    fill((prep.rs, prep.rd, prep.pb, prep.pi), rng, n, t, K1, K2, lk)
    rs, rd = pl.RanSha(gl, n, t, K1, stream=st), pl.RanDouSha(gl, n, t, K2, stream=st)
    tg, rb = pl.TripleGen(gl, n, t, T, stream=st), pl.RandBit(gl, n, t, R, stream=st)
    pb, pi = pl.PRandBitPipe(gl, fr, n, t, R, lk, stream=st), pl.PRandIntPipe(fr, n, t, nint, lk, stream=st)
    fill((rs, rd, pb, pi), np.random.default_rng(n * 1000 + nbit), n, t, K1, K2, lk)
    l1, l2 = (n - 2 * t) * K1, (t + 1) * K2

    def rows(dst, dpitch, src, spitch, width):
        rc = gl.L.hbmpc_memcpy_d2d_rows(gl.ctx, C.c_void_p(dst), C.c_size_t(dpitch * 8), C.c_void_p(src), C.c_size_t(spitch * 8), C.c_size_t(width * 8),
                                        C.c_size_t(n), C.c_void_p(st))
        assert rc == 0, gl.last_error()

    def composed():
        rs.run(check=False)
        rd.run(check=False)
        rows(rb.a, R, rs.out, l1, R)
        rows(tg.a, T, rs.out + R * 8, l1, T)
        rows(tg.b, T, rs.out + (R + T) * 8, l1, T)
        rows(tg.rt, T, rd.out_t, l2, T)
        rows(tg.r2t, T, rd.out_2t, l2, T)
        tg.run(check=False)
        for dst, src in ((rb.ta, tg.a), (rb.tb, tg.b), (rb.tc, tg.c)):
            rows(dst, R, src, T, R)
        rb.run(check=False)
        rows(pb.b_q, R, rb.out, R, R)
        pb.run(check=False)
        pi.run(check=False)

    sync = lambda: gl.sync(st)  # noqa: E731
    prep.run(check=True)                                              # honest inputs: every check passes
    composed()
    sync()
    same = all(np.array_equal(a.download_named(nm), b.download_named(nm)) for a, b, nm in ((prep.pb, pb, "b_p"), (prep.pi, pi, "r_p")))
    res = {"handle eager": timed(lambda: prep.run(check=False), sync, samples, calls), "composition eager": timed(composed, sync, samples, calls)}
    prep.capture()
    res["handle graph"] = timed(prep.replay, sync, samples, calls)
    composed()
    composed()
    sync()
    gl.graph_begin(st)
    composed()
    g = gl.graph_end(st)
    res["composition graph"] = timed(lambda: gl.graph_launch(g, st), sync, samples, calls)
    gl.graph_destroy(g)
    print("refill n=%d t=%d n_prandbit=%d n_prandint=%d (R=%d T=%d K1=%d K2=%d); same pools as the composition: %s" % (n, t, nbit, nint, R, T, K1, K2, same))
    for k in ("handle eager", "composition eager", "handle graph", "composition graph"):
        print("    %-20s %s ms" % (k, stats(res[k])))
    for h in (prep, rs, rd, tg, rb, pb, pi):
        h.close()
    gl.stream_destroy(st)


def take(pkg, fr, samples, calls):
    n, m, N = 16, 16, 1 << 18
    el = m * N
    nbytes = n * el * 32
    src, dst = fr.dev_alloc(nbytes), fr.dev_alloc(nbytes)
    st = fr.stream_create()
    ones = np.ones(1 << 20, dtype=np.uint64)
    for off in range(0, nbytes, ones.nbytes):
        fr.h2d(src + off, ones, st)
    sync = lambda: fr.sync(st)  # noqa: E731

    def do_take():
        assert fr.take_rows([(src, el, dst, el, el, m)], n, st) == 0

    def do_transpose():   # per party an [N][m] matrix -> [m][N]
        assert fr.dev_transpose(src, N, m, m, dst, N, n, el, el, st) == 0

    def do_copy():
        fr.d2d(dst, src, nbytes, st)

    moved = 2 * nbytes
    print("take at cfg5's shape: n=%d m=%d N=%d, 32-byte elements, %.2f GB read + %.2f GB written" % (n, m, N, nbytes / 1e9, nbytes / 1e9))
    # alternating, so that all three see the same machine
    res = {"take_rows": [], "transpose": [], "device copy": []}
    fns = {"take_rows": do_take, "transpose": do_transpose, "device copy": do_copy}
    for fn in fns.values():
        for _ in range(3):
            fn()
    sync()
    for _ in range(samples):
        for k, fn in fns.items():
            t0 = time.perf_counter()
            for _ in range(calls):
                fn()
            sync()
            res[k].append((time.perf_counter() - t0) * 1e3 / calls)
    for k, v in res.items():
        med = float(np.median(v))
        print("    %-12s %s ms   %.0f GB/s" % (k, stats(v), moved / med / 1e6))
    fr.stream_destroy(st)
    fr.dev_free(src)
    fr.dev_free(dst)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="refill,take")
    ap.add_argument("--shapes", default="4:1,7:2,16:5")
    ap.add_argument("--bits", default="20,65536")
    ap.add_argument("--samples", type=int, default=15)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--max-contrib-gb", type=float, default=2.0)
    args = ap.parse_args()
    from __graft_entry__ import load_package
    pkg = load_package()
    fr, gl = pkg.Engine(0, field="fr"), pkg.Engine(0, field="goldilocks")
    if "refill" in args.what:
        for shape in args.shapes.split(","):
            n, t = map(int, shape.split(":"))
            for nbit in map(int, args.bits.split(",")):
                R = pkg.pipelines.FixedPrep.sizes(n, t, nbit)[0]
                gb = n * math.comb(n, t) * R * 8 / 1e9
                if gb > args.max_contrib_gb:
                    print("refill n=%d t=%d n_prandbit=%d: not measured, the RISS contributions alone are %.1f GB" % (n, t, nbit, gb))
                    continue
                refill(pkg, fr, gl, n, t, nbit, max(nbit // 4, 1), args.samples, args.calls)
    if "take" in args.what:
        take(pkg, fr, args.samples, args.calls)
    fr.close()
    gl.close()


if __name__ == "__main__":
    main()
