#!/usr/bin/env python3
"""PRandBit at small batches (all parties on one device): hbmpc_dev_prandbit_parties as ONE launch (a workgroup per chunk of t + 1
elements, csrc/kernels_prandbit_wg.hpp) against its separate launches and against the composition of eight device calls over two
contexts that callers had before (pipelines.PRandBit.run: the baseline), over chunk counts -- where hbmpc_set_fused_prandbit's default
comes from.  The variants of a size are timed alternating in one process (medians of device-event samples, tools/bench_fpdiv.py):
  one eager / eight eager   the handle's run() with the threshold at 2^30 / at 0
  composition               pipelines.PRandBit.run (all n senders in the open, as it always ran)
  one graph / eight graph   the handle's replay() of either form
    python tools/sweep_fused_prandbit.py [--shapes 5:1,7:2,10:3] [--chunks 1,16,64,256,1024,4096]
The table goes to stdout."""
import argparse
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from __graft_entry__ import load_package  # noqa: E402
from bench_fpdiv import alternating_medians  # noqa: E402

P_GL = 2**64 - 2**32 + 1


def lk_for(n, t):
    """l + k with C(n,t) n 2^(l+k) + 1 < q: r + b never wraps in Goldilocks"""
    lk = 55
    while math.comb(n, t) * n * 2**lk + 1 >= P_GL:
        lk -= 1
    return lk


def inputs(n, t, B, lk):
    """contrib uniform in [0, 2^lk]; the bits shared as constant polynomials (a valid sharing of degree <= t)"""
    rng = np.random.default_rng(B + n)
    contrib = rng.integers(0, (1 << lk) + 1, size=(n, math.comb(n, t), B), dtype=np.uint64)
    bits = rng.integers(0, 2, size=B, dtype=np.uint64)
    return contrib, np.ascontiguousarray(np.broadcast_to(bits, (n, B)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="5:1,7:2,10:3")
    ap.add_argument("--chunks", default="1,16,64,256,1024,4096")
    ap.add_argument("--samples", type=int, default=25)
    ap.add_argument("--inner", type=int, default=10)
    args = ap.parse_args()
    pkg = load_package()
    dev = torch.device("cuda", 0)
    ts = torch.cuda.Stream(device=dev)
    st = ts.cuda_stream
    fr, gl = pkg.Engine(0, field="fr"), pkg.Engine(0, field="goldilocks")
    forms = (("one", 1 << 30), ("eight", 0))
    names = ["one eager", "eight eager", "composition", "one graph", "eight graph"]
    try:
        for shape in args.shapes.split(","):
            n, t = (int(v) for v in shape.split(":"))
            lk = lk_for(n, t)
            print(f"prandbit n={n} t={t} sets={math.comb(n, t)} l+k={lk}; ms per call, median (p10 .. p90) of {args.samples} samples of {args.inner} calls")
            print(f"{'chunks':>7} {'elements':>9} " + " ".join(f"{k:>26}" for k in names))
            for G in (int(v) for v in args.chunks.split(",")):
                B = G * (t + 1)
                contrib, b_q = inputs(n, t, B, lk)
                pipes = {}
                for form, fused in forms:
                    fr.set_fused_prandbit(fused)
                    pb = pkg.pipelines.PRandBitPipe(gl, fr, n, t, B, lk, stream=st)
                    pb.upload_named("contrib", contrib)
                    pb.upload_named("b_q", b_q)
                    pb.run(check=True)
                    pb.capture()  # records the form that the threshold selects now
                    pipes[form] = (pb, fused)
                comp = pkg.pipelines.PRandBit(gl, fr, n, t, B, stream=st)
                comp.upload_named("contrib", contrib)
                comp.upload_named("b_q", b_q)
                comp.run(lk)
                comp.sync()

                def eager(form):
                    pb, fused = pipes[form]

                    def run():
                        fr.set_fused_prandbit(fused)
                        pb.run(check=False)
                    return run

                fns = {f"{f} eager": eager(f) for f, _ in forms}
                fns["composition"] = lambda: comp.run(lk)
                fns.update({f"{f} graph": pipes[f][0].replay for f, _ in forms})
                res = alternating_medians(torch, ts, fns, args.samples, args.inner, 3)
                print(f"{G:7d} {B:9d} " + " ".join(f"{res[k][0]:10.4f} ({res[k][1]:.4f} .. {res[k][2]:.4f})".rjust(26) for k in names), flush=True)
                opened = comp.download_named("opened", np.uint64, (B,))
                for pb, _ in pipes.values():
                    assert pb.open_summary()[1][1] == 0 and np.array_equal(pb.download_named("opened"), opened)
                    pb.close()
                comp.close()
    finally:
        fr.set_fused_prandbit(pkg.hbmpc.FUSED_PRANDBIT_DEFAULT)
        fr.close()
        gl.close()


if __name__ == "__main__":
    main()
