#!/usr/bin/env python3
"""Multiply (Beaver) at small batches (all parties on one device): hbmpc_dev_mul_parties as ONE launch (a wave per element,
csrc/kernels_mul_wave.hpp) against its separate launches, eager and as a HIP graph, over batch sizes -- where hbmpc_set_fused_mul's
default comes from.  The four variants of a size are timed alternating in one process (medians of device-event samples,
tools/bench_fpdiv.py).
    python tools/sweep_fused_mul.py [sizes ...]        (the table goes to stdout)"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from __graft_entry__ import load_package  # noqa: E402
from bench_fpdiv import alternating_medians  # noqa: E402
from bench_mul import setup_mul  # noqa: E402


def main():
    sizes = [int(v) for v in sys.argv[1:]] or [64, 256, 512, 768, 1024, 1280, 1536, 2048, 3072, 4096, 8192, 16384]
    pkg = load_package()
    eng = pkg.Engine(0)
    dev = torch.device("cuda", 0)
    ts = torch.cuda.Stream(device=dev)
    st = ts.cuda_stream
    n, t = 16, 5
    print(f"mul n={n} t={t}; ms per call, median (p10 .. p90) of 25 samples of 20 calls")
    print(f"{'elements':>9} {'one eager':>26} {'multi eager':>26} {'one graph':>26} {'multi graph':>26}")
    try:
        for N in sizes:
            pipes = {}
            for form, fused in (("one", 1 << 30), ("multi", 0)):
                eng.set_fused_mul(fused)
                mp = setup_mul(pkg, eng, torch, dev, st, n, t, N)
                mp.run(check=True)
                mp.capture()  # records the form that the threshold selects now
                pipes[form] = (mp, fused)

            def eager(form):
                mp, fused = pipes[form]

                def run():
                    eng.set_fused_mul(fused)
                    mp.run(check=False)
                return run

            res = alternating_medians(torch, ts, {"one eager": eager("one"), "multi eager": eager("multi"), "one graph": pipes["one"][0].replay,
                                                  "multi graph": pipes["multi"][0].replay}, 25, 20, 3)
            print(f"{N:9d} " + " ".join(f"{v[0]:10.4f} ({v[1]:.4f} .. {v[2]:.4f})".rjust(26) for v in res.values()), flush=True)
            for mp, _ in pipes.values():
                mp.close()
    finally:
        eng.set_fused_mul(pkg.hbmpc.FUSED_MUL_DEFAULT)
        eng.close()


if __name__ == "__main__":
    main()
