#!/usr/bin/env python3
"""Input at small batches (all parties on one device): hbmpc_dev_input_parties as ONE launch (a wave per element,
csrc/kernels_input_wave.hpp) against its two separate launches, eager and as a HIP graph, over batch sizes and shapes -- where
hbmpc_set_fused_input's default comes from: the largest swept size at which one launch is not slower than the separate launches at
both (4, 1) and (16, 5).  The four variants of a size are timed alternating in one process (medians of device-event samples,
tools/bench_fpdiv.py).
    python tools/sweep_fused_input.py [sizes ...]        (the table goes to stdout)"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from __graft_entry__ import load_package  # noqa: E402
from bench_fpdiv import alternating_medians  # noqa: E402
from bench_input import setup_input  # noqa: E402

SHAPES = ((4, 1), (16, 5), (31, 10))


def main():
    sizes = [int(v) for v in sys.argv[1:]] or [1, 64, 256, 768, 1024, 4096, 16384]
    pkg = load_package()
    eng = pkg.Engine(0)
    dev = torch.device("cuda", 0)
    ts = torch.cuda.Stream(device=dev)
    st = ts.cuda_stream
    try:
        for n, t in SHAPES:
            print(f"input n={n} t={t}; ms per call, median (p10 .. p90) of 25 samples of 20 calls")
            print(f"{'elements':>9} {'one eager':>26} {'multi eager':>26} {'one graph':>26} {'multi graph':>26}")
            for N in sizes:
                pipes = {}
                for form, fused in (("one", 1 << 30), ("multi", 0)):
                    eng.set_fused_input(fused)
                    ip = setup_input(pkg, eng, torch, dev, st, n, t, N)
                    ip.run(check=True)
                    ip.capture()  # records the form that the threshold selects now
                    pipes[form] = (ip, fused)

                def eager(form):
                    ip, fused = pipes[form]

                    def run():
                        eng.set_fused_input(fused)
                        ip.run(check=False)
                    return run

                res = alternating_medians(torch, ts, {"one eager": eager("one"), "multi eager": eager("multi"), "one graph": pipes["one"][0].replay,
                                                      "multi graph": pipes["multi"][0].replay}, 25, 20, 3)
                print(f"{N:9d} " + " ".join(f"{v[0]:10.4f} ({v[1]:.4f} .. {v[2]:.4f})".rjust(26) for v in res.values()), flush=True)
                for ip, _ in pipes.values():
                    ip.close()
    finally:
        eng.set_fused_input(pkg.hbmpc.FUSED_INPUT_DEFAULT)
        eng.close()


if __name__ == "__main__":
    main()
