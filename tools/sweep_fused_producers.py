#!/usr/bin/env python3
"""RanSha and RanDouSha at small batches (all parties on one device): hbmpc_[gl_]dev_ransha_parties / _randousha_parties as ONE launch (a
workgroup per column, csrc/kernels_producers_wg.hpp) against the separate launches and against the existing handle at the same shape
(run() from the dealers' polynomials, finish() from the dealt shares), eager and as a HIP graph, over column counts, shapes, both
producers, both input modes and both fields -- where hbmpc_set_fused_producers' defaults come from: per field, the largest swept count at
which one launch is not slower than the separate launches at all three shapes, for both producers and both input modes, eager and
replayed.  The variants of a size are timed alternating in one process (tools/bench_producers_parties.py); the whole sweep runs
`--repeat` times (default 2) and the answer is the smaller one: the run-to-run spread is in the table.
    python tools/sweep_fused_producers.py [--repeat 2] [columns ...] > profiles/fused_producers_sweep.txt"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from __graft_entry__ import load_package  # noqa: E402
from bench_producers_parties import table  # noqa: E402

SHAPES = ((4, 1), (7, 2), (16, 5))


def main():
    argv = sys.argv[1:]
    repeat = 2
    if argv[:1] == ["--repeat"]:
        repeat, argv = int(argv[1]), argv[2:]
    columns = [int(v) for v in argv] or [1, 16, 64, 256, 1024, 1536, 2048]
    pkg = load_package()
    dev = torch.device("cuda", 0)
    ts = torch.cuda.Stream(device=dev)
    answer = {}
    for run in range(repeat):
        print(f"==== run {run + 1} of {repeat} ====")
        for field in ("fr", "goldilocks"):
            eng = pkg.Engine(0, field=field)
            try:
                best = None
                for kind in ("ransha", "randousha"):
                    for from_coeffs in (True, False):
                        for n, t in SHAPES:
                            rows = table(pkg, eng, torch, dev, ts, kind, n, t, columns, from_coeffs)
                            top = 0
                            for K in columns:  # the largest count up to which one launch is never slower
                                r = rows[K]
                                if not (r["one eager"][0] <= r["separate eager"][0] and r["one graph"][0] <= r["separate graph"][0]):
                                    break
                                top = K
                            print(f"  one launch not slower than the separate launches, eager and replayed, through {top} columns")
                            best = top if best is None else min(best, top)
                print(f"{field}: the largest swept count at which one launch is not slower at all three shapes, both producers, both modes: {best}\n", flush=True)
                answer[field] = best if field not in answer else min(answer[field], best)
            finally:
                eng.set_fused_producers(pkg.hbmpc.FUSED_PRODUCERS_DEFAULT[field])
                eng.close()
    print("the defaults these runs support: " + ", ".join(f"{f} {v}" for f, v in answer.items()))


if __name__ == "__main__":
    main()
