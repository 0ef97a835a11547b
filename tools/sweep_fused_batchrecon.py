#!/usr/bin/env python3
"""BatchRecon at small batches (all parties on one device): hbmpc_[gl_]dev_batchrecon_parties as ONE launch (a workgroup per chunk of
d + 1 elements, csrc/kernels_batchrecon_wg.hpp) against its three separate launches and against the composition of the three public
calls, eager and as a HIP graph, over chunk counts, shapes and both fields -- where hbmpc_set_fused_batchrecon's defaults come from:
per field, the largest swept count at which one launch is not slower than the three launches at all three shapes.  The variants of a
size are timed alternating in one process (tools/bench_batchrecon.py).
    python tools/sweep_fused_batchrecon.py [chunks ...] > profiles/fused_batchrecon_sweep.txt"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from __graft_entry__ import load_package  # noqa: E402
from bench_batchrecon import table  # noqa: E402

SHAPES = ((4, 1, 1), (16, 5, 5), (16, 5, 10))


def main():
    chunks = [int(v) for v in sys.argv[1:]] or [1, 16, 64, 256, 512, 1024, 2048, 4096]
    pkg = load_package()
    dev = torch.device("cuda", 0)
    ts = torch.cuda.Stream(device=dev)
    for field in ("fr", "goldilocks"):
        eng = pkg.Engine(0, field=field)
        try:
            best = None
            for n, t, d in SHAPES:
                rows = table(pkg, eng, torch, dev, ts, n, t, d, chunks)
                ok = [G for G in chunks if rows[G]["one eager"][0] <= rows[G]["three eager"][0] and rows[G]["one graph"][0] <= rows[G]["three graph"][0]]
                top = 0
                for G in chunks:  # the largest count up to which one launch is never slower
                    if G not in ok:
                        break
                    top = G
                print(f"  one launch not slower than the three launches, eager and replayed, through {top} chunks")
                best = top if best is None else min(best, top)
            print(f"{field}: the largest swept count at which one launch is not slower at all three shapes: {best}\n", flush=True)
        finally:
            eng.set_fused_batchrecon(pkg.hbmpc.FUSED_BATCHRECON_DEFAULT[field])
            eng.close()


if __name__ == "__main__":
    main()
