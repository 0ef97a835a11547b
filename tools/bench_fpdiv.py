#!/usr/bin/env python3
"""FPDivConst (and TruncPr alone) timing for all parties on one device: hbmpc_dev_truncpr_parties as ONE launch (a wave per element,
csrc/kernels_truncpr_wave.hpp) and as THREE (k_truncpr_front, the P(0) decode, the last step), against the composition a caller
had to assemble from existing calls before it:
    hbmpc_dev_fr_op (mul, by the multipliers replicated per party: one launch, the cheaper of the two ways),
    hbmpc_dev_truncpr_rdash_parties, hbmpc_dev_truncpr_open_share, hbmpc_dev_batch_recover_p0, hbmpc_dev_truncpr_finalize_parties.
The three are timed in the same process, alternating, from device events: each sample is `inner` back-to-back calls on one
stream between two events; the figure is the median over `samples`, with the 10th and 90th percentiles as the spread.  One JSON
line per batch size; a form that does not apply at a size (the one-launch form beyond --one-max) is null.
    python tools/bench_fpdiv.py [--n 16] [--t 5] [--k 32] [--m 16] [--sizes 5,256,1024,16384,262144] [--no-multiplier]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def setup_truncpr(pkg, eng, torch, dev, stream, n, t, N, k, m, with_w):
    """a TruncPr / FpDivConst pipeline (k = TruncPr's bit count, even with a multiplier) whose device buffers hold VALID degree-t
    sharings, produced by the compute_shares kernel itself: a uniform, r_int < 2^40, bits in {0, 1}; w = reciprocals of i << m"""
    import bench
    tp = pkg.pipelines.FpDivConst(eng, n, t, N, k // 2, m, stream=stream) if with_w else pkg.pipelines.TruncPr(eng, n, t, N, k, m, stream=stream)
    rint = torch.zeros((N, 4), dtype=torch.int64, device=dev)
    rint[:, 0] = torch.randint(0, 1 << 40, (N,), device=dev)
    bench._share_on_device(eng, torch, dev, stream, bench._rand_fr(torch, dev, N), n, t, tp.a)
    bench._share_on_device(eng, torch, dev, stream, rint, n, t, tp.rint)
    tmp = torch.empty((n, N, 4), dtype=torch.int64, device=dev)
    for j in range(m):  # r_bits[party][bit][N]
        bit = torch.zeros((N, 4), dtype=torch.int64, device=dev)
        bit[:, 0] = torch.randint(0, 2, (N,), device=dev)
        bench._share_on_device(eng, torch, dev, stream, bit, n, t, tmp.data_ptr())
        for p in range(n):
            eng.d2d(tp.rbits + (p * m + j) * N * 32, tmp.data_ptr() + p * N * 32, N * 32, stream)
    if with_w:
        den = np.zeros((N, 4), dtype=np.uint64)
        den[:, 0] = (np.arange(N, dtype=np.uint64) % np.uint64(1000) + np.uint64(1)) << np.uint64(m)
        tp.set_denominators(den)
    torch.cuda.synchronize()
    return tp


def composition(eng, tp, ws, stream):
    """the same result from the calls that existed before hbmpc_dev_truncpr_parties; ws: {"wrep": [n][N] multipliers or 0, "c", "rdash", "osh",
    "cop", "out", "status", "summary"} device pointers of its own outputs"""
    n, t, N, k, m = tp.n, tp.t, tp.N, tp.k, tp.m
    ids = list(range(2 * t + 1))

    def run():
        v = tp.a
        if ws["wrep"]:
            assert eng.dev_fr_op("mul", tp.a, ws["wrep"], n * N, ws["c"], stream) == 0
            v = ws["c"]
        assert eng.dev_elem_parties("truncpr_rdash", [tp.rbits, ws["rdash"]], N, n, extra=(m,), stream=stream) == 0
        assert eng.dev_elem("truncpr_open_share", [v, ws["rdash"], tp.rint, ws["osh"]], n * N, extra=(k, m), stream=stream) == 0
        assert eng.dev_batch_recover(ids, ws["osh"], N, n, t, t, ws["cop"], status_d=ws["status"], summary_d=ws["summary"], stream=stream, p0=True) == 0
        assert eng.dev_elem_parties("truncpr_finalize", [v, ws["rdash"], ws["cop"], ws["out"]], N, n, extra=(m,), stream=stream) == 0
    return run


def alternating_medians(torch, ts, fns, samples, inner, warm):
    """{name: (median, p10, p90)} ms per call; fns: {name: callable or None}.  Sample i times every form once, in turn."""
    live = {k: f for k, f in fns.items() if f is not None}
    with torch.cuda.stream(ts):
        for _ in range(warm):
            for f in live.values():
                f()
        torch.cuda.synchronize()
        got = {k: [] for k in live}
        for _ in range(samples):
            for k, f in live.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(inner):
                    f()
                e1.record()
                e1.synchronize()
                got[k].append(e0.elapsed_time(e1) / inner)
    return {k: (tuple(round(float(np.percentile(got[k], q)), 5) for q in (50, 10, 90)) if k in got else None) for k in fns}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=16)
    ap.add_argument("--t", type=int, default=5)
    ap.add_argument("--k", type=int, default=32)
    ap.add_argument("--m", type=int, default=16)
    ap.add_argument("--sizes", default="5,256,1024,16384,262144")
    ap.add_argument("--one-max", type=int, default=16384, help="the one-launch form is not timed beyond this many elements")
    ap.add_argument("--samples", type=int, default=25)
    ap.add_argument("--no-multiplier", action="store_true", help="TruncPr alone")
    args = ap.parse_args()
    import torch
    from __graft_entry__ import load_package
    pkg = load_package()
    H = pkg.hbmpc
    eng = pkg.Engine(0)
    dev = torch.device("cuda", 0)
    ts = torch.cuda.Stream(device=dev)
    st = ts.cuda_stream
    n, t, k, m, with_w = args.n, args.t, args.k, args.m, not args.no_multiplier
    for N in [int(s) for s in args.sizes.split(",")]:
        tp = setup_truncpr(pkg, eng, torch, dev, st, n, t, N, k, m, with_w)
        own = {nm: torch.empty((cnt, 4), dtype=torch.int64, device=dev) for nm, cnt in (("c", n * N), ("rdash", n * N), ("osh", n * N), ("out", n * N), ("cop", N))}
        own["status"], own["summary"] = torch.empty(N, dtype=torch.uint8, device=dev), torch.empty(4, dtype=torch.int32, device=dev)
        ws = {nm: v.data_ptr() for nm, v in own.items()}
        wrep = None
        if with_w:
            wrep = torch.empty((n, N, 4), dtype=torch.int64, device=dev)
            for p in range(n):
                eng.d2d(wrep.data_ptr() + p * N * 32, tp.w, N * 32, st)
        ws["wrep"] = wrep.data_ptr() if with_w else 0
        comp = composition(eng, tp, ws, st)

        def form(fused):
            def run():
                eng.set_fused_truncpr(fused)
                tp.run(check=False)
            return run

        # all three leave the same bytes: checked once per size before anything is timed
        outs = {}
        for name, fn in (("one", form(1 << 30) if N <= args.one_max else None), ("three", form(0)), ("composition", comp)):
            if fn is None:
                continue
            fn()
            eng.sync(st)
            src = ws["out"] if name == "composition" else tp.out
            host = np.zeros((n, N, 4), dtype=np.uint64)
            eng.d2h(host, src, st)
            eng.sync(st)
            outs[name] = host
        same = all(np.array_equal(v, outs["three"]) for v in outs.values())
        assert same and tp.summary().tolist() == [0, 0, 0xffffffff, 0], "the forms disagree, or an open failed"
        inner = 20 if N <= 16384 else 5
        res = alternating_medians(torch, ts, {"one": form(1 << 30) if N <= args.one_max else None, "three": form(0), "composition": comp},
                                  args.samples, inner, 3)
        eng.set_fused_truncpr(H.FUSED_TRUNCPR_DEFAULT)
        print(json.dumps({"what": "fpdivconst" if with_w else "truncpr", "n": n, "t": t, "k": k, "m": m, "N": N, "same_bytes": bool(same),
                          "ms_median_p10_p90": res, "samples": args.samples, "calls_per_sample": inner}), flush=True)
        tp.close()
        del own, wrep
    eng.close()


if __name__ == "__main__":
    main()
