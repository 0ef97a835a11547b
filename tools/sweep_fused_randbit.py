#!/usr/bin/env python3
"""RandBit at small batches (all parties on one device): hbmpc_[gl_]dev_randbit_parties as ONE launch (a workgroup per chunk of
t + 1 elements, csrc/kernels_randbit_wg.hpp) against its nine launches, eager and as a HIP graph, over chunk counts -- where
hbmpc_set_fused_randbit's defaults come from.  The four variants of a size are timed alternating in one process (medians of
device-event samples, tools/bench_fpdiv.py).
    python tools/sweep_fused_randbit.py [--fields goldilocks,fr] [--shapes 16:5,4:1] [--chunks 1,8,64,256,1024,4096]
    python tools/sweep_fused_randbit.py --baseline-lib PATH     the pipeline of another build of the library (one without the device
                                                                call: only `eager` and `graph` of its pipeline are timed)
The table goes to stdout."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from __graft_entry__ import load_package  # noqa: E402
from bench_fpdiv import alternating_medians  # noqa: E402
from bench_randbit import rand_elems, shares  # noqa: E402


def setup_randbit(pkg, eng, st, n, t, N):
    """a RandBit pipeline over N random elements with valid triples, run once"""
    rng = np.random.default_rng(N + n)
    a, ta, tb = (rand_elems(eng.field, rng, N) for _ in range(3))
    rc, tc = eng.fr_op("mul", ta, tb)
    assert rc == 0
    rb = pkg.pipelines.RandBit(eng, n, t, N, stream=st)
    rb.upload(shares(eng, a, n, t, rng), shares(eng, ta, n, t, rng), shares(eng, tb, n, t, rng), shares(eng, tc, n, t, rng))
    rb.run(check=True)
    return rb


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fields", default="goldilocks,fr")
    ap.add_argument("--shapes", default="16:5,4:1")
    ap.add_argument("--chunks", default="1,8,64,256,1024,4096")
    ap.add_argument("--samples", type=int, default=25)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--baseline-lib", default=None)
    args = ap.parse_args()
    pkg = load_package()
    if args.baseline_lib:
        pkg.hbmpc.LIB_PATH = os.path.abspath(args.baseline_lib)  # before the first call loads the library
    dev = torch.device("cuda", 0)
    ts = torch.cuda.Stream(device=dev)
    st = ts.cuda_stream
    forms = (("pipe", None),) if args.baseline_lib else (("one", 1 << 30), ("nine", 0))
    names = [f"{f} {mode}" for mode in ("eager", "graph") for f, _ in forms]
    for field in args.fields.split(","):
        eng = pkg.Engine(0, field=field)
        try:
            for shape in args.shapes.split(","):
                n, t = (int(v) for v in shape.split(":"))
                print(f"randbit {field} n={n} t={t}{' (baseline library)' if args.baseline_lib else ''}; ms per call, median (p10 .. p90) of "
                      f"{args.samples} samples of {args.inner} calls")
                print(f"{'chunks':>7} {'elements':>9} " + " ".join(f"{k:>26}" for k in names))
                for G in (int(v) for v in args.chunks.split(",")):
                    N = G * (t + 1)
                    pipes = {}
                    for form, fused in forms:
                        if fused is not None:
                            eng.set_fused_randbit(fused)
                        rb = setup_randbit(pkg, eng, st, n, t, N)
                        rb.capture()  # records the form that the threshold selects now
                        pipes[form] = (rb, fused)

                    def eager(form):
                        rb, fused = pipes[form]

                        def run():
                            if fused is not None:
                                eng.set_fused_randbit(fused)
                            rb.run(check=False)
                        return run

                    fns = {f"{f} eager": eager(f) for f, _ in forms}
                    fns.update({f"{f} graph": pipes[f][0].replay for f, _ in forms})
                    res = alternating_medians(torch, ts, fns, args.samples, args.inner, 3)
                    print(f"{G:7d} {N:9d} " + " ".join(f"{res[k][0]:10.4f} ({res[k][1]:.4f} .. {res[k][2]:.4f})".rjust(26) for k in names), flush=True)
                    for rb, _ in pipes.values():
                        assert not rb.status().any()
                        rb.close()
        finally:
            if not args.baseline_lib:
                eng.set_fused_randbit(pkg.hbmpc.FUSED_RANDBIT_DEFAULT[field])
            eng.close()


if __name__ == "__main__":
    main()
