#!/usr/bin/env python3
"""Seeded RISS dealing timing (contract "hbmpc-riss-chacha20-v1").  Two measurements, each from a host clock around work that ends in a
stream synchronise, the alternatives of one measurement alternating sample by sample:

  fold     the sums [C(n,t)][B] of all n senders' contributions: hbmpc_dev_riss_sample_fold (drawn and added in registers) against the
           route a caller had before it -- the contributions on the host, uploaded (pageable numpy memory, as a caller's would be) and
           folded by hbmpc_dev_riss_fold -- and against hbmpc_dev_riss_fold alone.  The contributions are the same values (each
           sender's hbmpc_dev_riss_sample output), and both routes' sums are compared.  ChaCha20 blocks per second of the seeded
           fold (n C(n,t) B values, 1 + 2^-8 blocks each) against tools/ubench_chacha's register-only block loop, the ceiling.
           A shape whose contributions exceed --max-contrib-gb is timed seeded only.
  refill   hbmpc_pipe_fixedprep_create_seeded's run() against hbmpc_pipe_fixedprep_create's, eager (a seeded handle has no capture),
           honest polynomials, n_prandint = n_prandbit / 4.  The seeded RISS parts always run their separate launches.

    python tools/bench_riss_seeded.py [--what fold,refill] [--fold 4:1:65536,7:2:65536,16:5:4096,16:5:65536]
        [--shapes 4:1,7:2,16:5] [--bits 20,65536] [--samples 15] [--calls 5] [--max-contrib-gb 4]
Prints ms per call as median (p10 .. p90); run it twice and compare for the run-to-run spread."""
import argparse
import json
import math
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_fixedprep import gl_rand, lk_for, stats  # noqa: E402

UBENCH = os.path.join(ROOT, "tools", "ubench_chacha")


def seeds_of(n):
    return np.frombuffer(b"".join(bytes((b + 37 * s) & 0xFF for b in range(32)) for s in range(n)), dtype=np.uint8)


def alternate(fns, sync, samples, calls):
    """{name: [ms per call]}: the functions take turns, so that all of them see the same machine"""
    for fn in fns.values():
        for _ in range(2):
            fn()
    sync()
    res = {k: [] for k in fns}
    for _ in range(samples):
        for k, fn in fns.items():
            t0 = time.perf_counter()
            for _ in range(calls):
                fn()
            sync()
            res[k].append((time.perf_counter() - t0) * 1e3 / calls)
    return res


def ceiling():
    """blocks per second of the register-only ChaCha20 loop (built on first use: hipcc cross-compiles it anywhere)"""
    if not os.path.exists(UBENCH):
        subprocess.check_call(["hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-I", os.path.join(ROOT, "mpc-protocols_amd", "csrc"),
                               UBENCH + ".hip", "-o", UBENCH])
    row = json.loads(subprocess.run([UBENCH], check=True, capture_output=True, text=True, timeout=120).stdout)
    print("ceiling: register-only ChaCha20 loop, %.3g blocks in %.3f (%.3f .. %.3f) ms: %.3e blocks/s on %d CUs" %
          (row["chacha_blocks"], row["ms_median"], row["ms_p10"], row["ms_p90"], row["blocks_per_s"], row["cus"]))
    return row["blocks_per_s"]


def fold(fr, n, t, B, samples, calls, max_gb, peak):
    Tn, lk = math.comb(n, t), lk_for(n, t)
    st = fr.stream_create()
    sync = lambda: fr.sync(st)  # noqa: E731
    gb = n * Tn * B * 8 / 1e9
    seeds, sums = fr.dev_alloc(n * 32), fr.dev_alloc(Tn * B * 8)
    fr.h2d(seeds, seeds_of(n), st)

    def seeded():
        assert fr.riss_sample_fold(seeds, n, t, 0, B, 0, lk, sums, st) == 0, fr.last_error()

    fns = {"sample_fold": seeded}
    with_contrib = gb <= max_gb
    if with_contrib:
        contrib_d, sums2, bad = fr.dev_alloc(n * Tn * B * 8), fr.dev_alloc(Tn * B * 8), fr.dev_alloc(n * Tn)
        raw = seeds_of(n).tobytes()
        for s in range(n):
            assert fr.dev_riss_sample(raw[32 * s:32 * s + 32], n, t, 0, B, 0, lk, contrib_d + s * Tn * B * 8, st) == 0, fr.last_error()
        contrib = np.zeros((n, Tn, B), dtype=np.uint64)
        fr.d2h(contrib, contrib_d, st)
        sync()

        def fold_only():
            assert fr.dev_riss_fold(contrib_d, n, Tn, B, lk, sums2, bad, st) == 0, fr.last_error()

        def upload_fold():
            fr.h2d(contrib_d, contrib, st)
            fold_only()

        fns["upload + riss_fold"], fns["riss_fold alone"] = upload_fold, fold_only
        seeded(), fold_only()
        a, b = np.zeros(Tn * B, dtype=np.uint64), np.zeros(Tn * B, dtype=np.uint64)
        fr.d2h(a, sums, st), fr.d2h(b, sums2, st)
        sync()
        assert np.array_equal(a, b), "the seeded fold and the fold of the materialised contributions disagree"
    heavy = gb >= 0.5 or n * Tn * B >= 1 << 30                       # a long upload or a long draw per call: fewer, single calls
    res = alternate(fns, sync, max(5, samples // 3) if heavy else samples, 1 if heavy else calls)
    print("fold n=%d t=%d B=%d lk=%d: C(n,t)=%d, contrib %.3f GB, sums %.3f GB%s" %
          (n, t, B, lk, Tn, gb, Tn * B * 8 / 1e9, "" if with_contrib else " (contrib not materialised: seeded only)"))
    for k, v in res.items():
        print("    %-20s %s ms" % (k, stats(v)))
    med = float(np.median(res["sample_fold"]))
    rate = n * Tn * B * (1 + 2.0**-8) / (med * 1e-3)
    print("    sample_fold: %.3e ChaCha20 blocks/s%s" % (rate, "" if not peak else ", %.0f %% of the register-only loop" % (100 * rate / peak)))
    if with_contrib:
        print("    sample_fold against upload + riss_fold: %.1f x; against riss_fold alone: %.2f x" %
              (float(np.median(res["upload + riss_fold"])) / med, float(np.median(res["riss_fold alone"])) / med))
        for p in (contrib_d, sums2, bad):
            fr.dev_free(p)
    for p in (seeds, sums):
        fr.dev_free(p)
    fr.stream_destroy(st)


def refill(pkg, fr, gl, n, t, nbit, nint, samples, calls, max_gb):
    pl = pkg.pipelines
    lk, Tn = lk_for(n, t), math.comb(n, t)
    st = gl.stream_create()
    sync = lambda: gl.sync(st)  # noqa: E731
    R, T, K1, K2 = pl.FixedPrep.sizes(n, t, nbit)
    gb = n * Tn * R * 8 / 1e9
    kinds = ("seeded", "unseeded") if gb <= max_gb else ("seeded",)
    preps = {}
    for kind in kinds:
        rng = np.random.default_rng(n * 1000 + nbit)
        prep = preps[kind] = pl.FixedPrep(gl, fr, n, t, nbit, nint, lk, stream=st, seeded=(kind == "seeded"))
        prep.rs.upload(gl_rand(rng, (n, K1, t + 1)))
        ct, c2 = gl_rand(rng, (n, K2, t + 1)), gl_rand(rng, (n, K2, 2 * t + 1))
        c2[:, :, 0] = ct[:, :, 0]
        prep.rd.upload(ct, c2)
        if kind == "seeded":
            prep.upload_named("seeds", seeds_of(n))
        else:
            for h in (prep.pb, prep.pi):
                h.upload_named("contrib", rng.integers(0, 1 << lk, size=(n, Tn, h.B), dtype=np.uint64))
        prep.run(check=True)                                          # honest inputs: every check passes
    big = gb > max_gb
    res = alternate({k: (lambda p=p: p.run(check=False)) for k, p in preps.items()}, sync, max(3, samples // 3) if big else samples, 1 if big else calls)
    print("refill n=%d t=%d n_prandbit=%d n_prandint=%d (R=%d T=%d K1=%d K2=%d)%s" %
          (n, t, nbit, nint, R, T, K1, K2, "" if not big else ": unseeded not measured, its RISS contributions alone are %.1f GB" % gb))
    for k, v in res.items():
        print("    %-20s %s ms" % (k + " eager", stats(v)))
    if len(res) == 2:
        print("    seeded / unseeded: %.2f x" % (float(np.median(res["seeded"])) / float(np.median(res["unseeded"]))))
    for p in preps.values():
        p.close()
    gl.stream_destroy(st)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="fold,refill")
    ap.add_argument("--fold", default="4:1:65536,7:2:65536,16:5:4096,16:5:65536")
    ap.add_argument("--shapes", default="4:1,7:2,16:5")
    ap.add_argument("--bits", default="20,65536")
    ap.add_argument("--samples", type=int, default=15)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--max-contrib-gb", type=float, default=4.0)
    args = ap.parse_args()
    from __graft_entry__ import load_package
    pkg = load_package()
    fr, gl = pkg.Engine(0, field="fr"), pkg.Engine(0, field="goldilocks")
    if "fold" in args.what:
        peak = ceiling()
        for shape in args.fold.split(","):
            n, t, B = map(int, shape.split(":"))
            fold(fr, n, t, B, args.samples, args.calls, args.max_contrib_gb, peak)
    if "refill" in args.what:
        for shape in args.shapes.split(","):
            n, t = map(int, shape.split(":"))
            for nbit in map(int, args.bits.split(",")):
                refill(pkg, fr, gl, n, t, nbit, max(nbit // 4, 1), args.samples, args.calls, args.max_contrib_gb)
    fr.close()
    gl.close()


if __name__ == "__main__":
    main()
