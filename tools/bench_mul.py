#!/usr/bin/env python3
"""Multiply (Beaver) timing for all parties on one device: hbmpc_dev_mul_parties as ONE launch (a wave per element,
csrc/kernels_mul_wave.hpp) and as its separate launches (the opened shares, the P(0) decode of 2 N values, finalize_mul; the first
two as one from hbmpc_set_fpmul_pair_decode elements on), with FpMul (k = 32, m = 16: Multiply followed by TruncPr, at the library's
defaults) for scale.  Each is timed eager and replayed as a HIP graph, in the same process, alternating, from device events
(alternating_medians of tools/bench_fpdiv.py).  One JSON line per batch size; the one-launch form is forced where the size is
beyond the threshold and null beyond --one-max.
    python tools/bench_mul.py [--n 16] [--t 5] [--sizes 5,256,1024,16384,262144]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def setup_mul(pkg, eng, torch, dev, stream, n, t, N):
    """a Mul pipeline whose device buffers hold VALID degree-t sharings (uniform x, y and a triple with c = a b), produced by the
    compute_shares kernel itself"""
    import bench
    mp = pkg.pipelines.Mul(eng, n, t, N, stream=stream)
    x, y, ta, tb = (bench._rand_fr(torch, dev, N) for _ in range(4))
    tc = torch.empty_like(ta)
    torch.cuda.synchronize()
    assert eng.dev_fr_op("mul", ta.data_ptr(), tb.data_ptr(), N, tc.data_ptr(), stream) == 0
    for sec, ptr in ((x, mp.x), (y, mp.y), (ta, mp.ta), (tb, mp.tb), (tc, mp.tc)):
        bench._share_on_device(eng, torch, dev, stream, sec, n, t, ptr)
    torch.cuda.synchronize()
    return mp


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=16)
    ap.add_argument("--t", type=int, default=5)
    ap.add_argument("--sizes", default="5,256,1024,16384,262144")
    ap.add_argument("--one-max", type=int, default=16384, help="the one-launch form is not timed beyond this many elements")
    ap.add_argument("--samples", type=int, default=25)
    args = ap.parse_args()
    import torch

    import bench
    from __graft_entry__ import load_package
    from bench_fpdiv import alternating_medians
    pkg = load_package()
    H = pkg.hbmpc
    eng = pkg.Engine(0)
    dev = torch.device("cuda", 0)
    ts = torch.cuda.Stream(device=dev)
    st = ts.cuda_stream
    n, t, k, m = args.n, args.t, 32, 16
    try:
        for N in [int(s) for s in args.sizes.split(",")]:
            pipes, outs = {}, {}
            for form, fused in (("one", 1 << 30), ("multi", 0)):
                if form == "one" and N > args.one_max:
                    continue
                eng.set_fused_mul(fused)
                mp = setup_mul(pkg, eng, torch, dev, st, n, t, N)
                mp.run(check=True)
                mp.capture()  # records the form that the threshold selects now
                outs[form] = (mp.download("out"), mp.summary().tolist())
                pipes[form] = (mp, fused)
            eng.set_fused_mul(H.FUSED_MUL_DEFAULT)
            assert all(s == [0, 0, 0xffffffff, 0] for _, s in outs.values()), "an open failed"
            fp = bench.setup_fpmul(eng, torch, dev, st, n, t, N, k, m)
            fp.run(check=True)
            fp.capture()

            def eager(form):
                if form not in pipes:
                    return None
                mp, fused = pipes[form]

                def run():
                    eng.set_fused_mul(fused)
                    mp.run(check=False)
                return run

            inner = 20 if N <= 16384 else 5
            res = alternating_medians(torch, ts, {"one eager": eager("one"), "multi eager": eager("multi"), "fpmul eager": lambda: fp.run(check=False),
                                                  "one graph": pipes["one"][0].replay if "one" in pipes else None,
                                                  "multi graph": pipes["multi"][0].replay, "fpmul graph": fp.replay}, args.samples, inner, 3)
            eng.set_fused_mul(H.FUSED_MUL_DEFAULT)
            print(json.dumps({"what": "mul", "n": n, "t": t, "N": N, "fpmul_k_m": [k, m], "one_launch_forced": bool("one" in pipes and N > H.FUSED_MUL_DEFAULT),
                              "ms_median_p10_p90": res, "samples": args.samples, "calls_per_sample": inner}), flush=True)
            for mp, _ in pipes.values():
                mp.close()
            fp.close()
    finally:
        eng.set_fused_mul(H.FUSED_MUL_DEFAULT)
        eng.close()


if __name__ == "__main__":
    main()
