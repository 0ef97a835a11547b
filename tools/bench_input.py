#!/usr/bin/env python3
"""Input timing for all parties on one device: hbmpc_dev_input_parties as ONE launch (a wave per element,
csrc/kernels_input_wave.hpp) and as its two launches (the P(0) decode of the masks, k_input_finish), against the composition a
caller had to write before the call existed, from calls that were there already: hbmpc_dev_batch_recover_p0 of the masks, one
hbmpc_dev_fr_op to add the inputs, and one hbmpc_dev_fr_op per party for masked - r (2 + n launches; no failure rule).  The three
are timed eager in the same process, alternating, from device events (alternating_medians of tools/bench_fpdiv.py); the two forms of
the call also replayed as HIP graphs.  One JSON line per shape and batch size; the one-launch form is forced where the size is
beyond the threshold.
    python tools/bench_input.py [--shapes 4:1,16:5] [--sizes 1,64,256,768,1024]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def setup_input(pkg, eng, torch, dev, stream, n, t, N):
    """an Input pipeline whose device buffers hold uniform client values and VALID degree-t sharings of uniform masks, produced by the
    compute_shares kernel itself"""
    import bench
    ip = pkg.pipelines.Input(eng, n, t, N, stream=stream)
    x, mask = bench._rand_fr(torch, dev, N), bench._rand_fr(torch, dev, N)
    torch.cuda.synchronize()
    eng.d2d(ip.x, x.data_ptr(), N * 32, stream)
    bench._share_on_device(eng, torch, dev, stream, mask, n, t, ip.r)
    torch.cuda.synchronize()
    return ip


def composition(eng, ip, n, t, N, stream):
    """what a caller wrote before hbmpc_dev_input_parties: senders 0 .. 2t are rows 0 .. 2t of r, so the plain p0 decode reads them"""
    ids = list(range(2 * t + 1))
    status, summary = ip.buffer("status")[0], ip.buffer("summary")[0]

    def run():
        assert eng.dev_batch_recover(ids, ip.r, N, n, t, t, ip.mask, status_d=status, summary_d=summary, stream=stream, p0=True) == 0
        assert eng.dev_fr_op("add", ip.x, ip.mask, N, ip.masked, stream) == 0
        for p in range(n):
            assert eng.dev_fr_op("sub", ip.masked, ip.r + p * N * 32, N, ip.out + p * N * 32, stream) == 0
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="4:1,16:5")
    ap.add_argument("--sizes", default="1,64,256,768,1024")
    ap.add_argument("--samples", type=int, default=25)
    args = ap.parse_args()
    import torch

    from __graft_entry__ import load_package
    from bench_fpdiv import alternating_medians
    pkg = load_package()
    H = pkg.hbmpc
    eng = pkg.Engine(0)
    dev = torch.device("cuda", 0)
    ts = torch.cuda.Stream(device=dev)
    st = ts.cuda_stream
    try:
        for n, t in [tuple(int(v) for v in s.split(":")) for s in args.shapes.split(",")]:
            for N in [int(s) for s in args.sizes.split(",")]:
                pipes, outs = {}, {}
                for form, fused in (("one", 1 << 30), ("multi", 0)):
                    eng.set_fused_input(fused)
                    ip = setup_input(pkg, eng, torch, dev, st, n, t, N)
                    ip.run(check=True)
                    ip.capture()  # records the form that the threshold selects now
                    outs[form] = ip.summary().tolist()
                    pipes[form] = (ip, fused)
                eng.set_fused_input(H.FUSED_INPUT_DEFAULT)
                assert all(s == [0, 0, 0xffffffff, 0] for s in outs.values()), "an open failed"
                # the composition on the one-launch handle's inputs must leave the call's own bytes
                ip = pipes["one"][0]
                want = ip.download("out").copy()
                comp = composition(eng, ip, n, t, N, st)
                comp()
                assert (ip.download("out") == want).all(), "the composition and the call differ"

                def eager(form):
                    p, fused = pipes[form]

                    def run():
                        eng.set_fused_input(fused)
                        p.run(check=False)
                    return run

                res = alternating_medians(torch, ts, {"one eager": eager("one"), "multi eager": eager("multi"), "composition eager": comp,
                                                      "one graph": pipes["one"][0].replay, "multi graph": pipes["multi"][0].replay}, args.samples, 20, 3)
                eng.set_fused_input(H.FUSED_INPUT_DEFAULT)
                print(json.dumps({"what": "input", "n": n, "t": t, "N": N, "composition_launches": 2 + n,
                                  "one_launch_forced": bool(N > H.FUSED_INPUT_DEFAULT), "ms_median_p10_p90": res, "samples": args.samples,
                                  "calls_per_sample": 20}), flush=True)
                for p, _ in pipes.values():
                    p.close()
    finally:
        eng.set_fused_input(H.FUSED_INPUT_DEFAULT)
        eng.close()


if __name__ == "__main__":
    main()
