#!/usr/bin/env python3
"""TruncPr / FPDivConst at small batches (all parties on one device): hbmpc_dev_truncpr_parties as ONE launch (a wave per element,
csrc/kernels_truncpr_wave.hpp) against its three launches, eager and as a HIP graph, over batch sizes -- where
hbmpc_set_fused_truncpr's default comes from.  The four variants of a size are timed alternating in one process (medians of
device-event samples, tools/bench_fpdiv.py).
    python tools/sweep_fused_truncpr.py [--no-multiplier] [sizes ...]        (the table goes to stdout)"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from __graft_entry__ import load_package  # noqa: E402
from bench_fpdiv import alternating_medians, setup_truncpr  # noqa: E402


def main():
    argv = sys.argv[1:]
    with_w = "--no-multiplier" not in argv
    sizes = [int(v) for v in argv if not v.startswith("--")] or [64, 256, 512, 1024, 2048, 3072, 4096, 6144, 8192, 16384]
    pkg = load_package()
    eng = pkg.Engine(0)
    dev = torch.device("cuda", 0)
    ts = torch.cuda.Stream(device=dev)
    st = ts.cuda_stream
    n, t, k, m = 16, 5, 32, 16
    print(f"{'fpdivconst' if with_w else 'truncpr'} n={n} t={t} (k, m)=({k}, {m}); ms per call, median (p10 .. p90) of 25 samples of 20 calls")
    print(f"{'elements':>9} {'one eager':>26} {'three eager':>26} {'one graph':>26} {'three graph':>26}")
    try:
        for N in sizes:
            pipes = {}
            for form, fused in (("one", 1 << 30), ("three", 0)):
                eng.set_fused_truncpr(fused)
                tp = setup_truncpr(pkg, eng, torch, dev, st, n, t, N, k, m, with_w)
                tp.run(check=True)
                tp.capture()  # records the form that the threshold selects now
                pipes[form] = (tp, fused)

            def eager(form):
                tp, fused = pipes[form]

                def run():
                    eng.set_fused_truncpr(fused)
                    tp.run(check=False)
                return run

            res = alternating_medians(torch, ts, {"one eager": eager("one"), "three eager": eager("three"), "one graph": pipes["one"][0].replay,
                                                  "three graph": pipes["three"][0].replay}, 25, 20, 3)
            print(f"{N:9d} " + " ".join(f"{v[0]:10.4f} ({v[1]:.4f} .. {v[2]:.4f})".rjust(26) for v in res.values()), flush=True)
            for tp, _ in pipes.values():
                tp.close()
    finally:
        eng.set_fused_truncpr(pkg.hbmpc.FUSED_TRUNCPR_DEFAULT)
        eng.close()


if __name__ == "__main__":
    main()
