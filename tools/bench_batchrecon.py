#!/usr/bin/env python3
"""BatchRecon for all parties on one device: hbmpc_[gl_]dev_batchrecon_parties as ONE launch (a workgroup per chunk of d + 1 elements,
csrc/kernels_batchrecon_wg.hpp) and as its three launches, against the composition a caller wrote before the call existed
(hbmpc_dev_vandermonde_apply_parties and hbmpc_dev_batch_recover_slots twice: the handle's deal() + finish()), eager and replayed as a
HIP graph.  The six variants of a size are timed alternating in one process (medians of device-event samples, tools/bench_fpdiv.py).
    python tools/bench_batchrecon.py [--field fr|goldilocks] [--n 16 --t 5 --d 5] [--chunks 1,64,1024] [--repeat 2]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_fpdiv import alternating_medians  # noqa: E402

VARIANTS = ("one eager", "three eager", "composed eager", "one graph", "three graph", "composed graph")


def rand_elements(torch, dev, field, *shape):
    """uniform-ish canonical field elements generated on the device"""
    if field == "goldilocks":
        return torch.randint(0, 1 << 62, shape, dtype=torch.int64, device=dev)
    import bench
    return bench._rand_fr(torch, dev, *shape)


def setup_batchrecon(pkg, eng, torch, dev, stream, n, t, d, G):
    """a BatchRecon handle whose x holds VALID degree-d sharings of uniform secrets, produced by the compute_shares kernel itself"""
    N = G * (d + 1)
    bp = pkg.pipelines.BatchRecon(eng, n, t, d, N, stream=stream)
    co = rand_elements(torch, dev, eng.field, N, d + 1)
    torch.cuda.synchronize()
    assert eng.dev_compute_shares(co.data_ptr(), N, n, d, bp.x, stream) == 0, eng.last_error()
    torch.cuda.synchronize()
    return bp


def variants(pkg, eng, torch, dev, stream, n, t, d, G):
    """({variant: callable}, close): the six ways of one shape; every graph is recorded after two eager runs of its form"""
    pipes, graphs, fns = [], [], {}
    for form, fused in (("one", 1 << 30), ("three", 0)):
        eng.set_fused_batchrecon(fused)
        bp = setup_batchrecon(pkg, eng, torch, dev, stream, n, t, d, G)
        bp.run(check=True)
        bp.capture()  # records the form that the threshold selects now
        pipes.append(bp)

        def eager(bp=bp, fused=fused):
            eng.set_fused_batchrecon(fused)
            bp.run(check=False)
        fns[form + " eager"], fns[form + " graph"] = eager, bp.replay
    bp = setup_batchrecon(pkg, eng, torch, dev, stream, n, t, d, G)
    pipes.append(bp)

    def composed(bp=bp):
        bp.deal()
        bp.finish()
    composed()
    composed()
    eng.sync(stream)
    eng.graph_begin(stream)
    composed()
    graph = eng.graph_end(stream)
    graphs.append(graph)
    fns["composed eager"], fns["composed graph"] = composed, lambda: eng.graph_launch(graph, stream)

    def close():
        eng.sync(stream)
        for g in graphs:
            eng.graph_destroy(g)
        for p in pipes:
            p.close()
    return {k: fns[k] for k in VARIANTS}, close


def table(pkg, eng, torch, dev, ts, n, t, d, chunks, samples=25, inner=20):
    print(f"batchrecon {eng.field} n={n} t={t} d={d}; ms per call, median (p10 .. p90) of {samples} samples of {inner} calls")
    print(f"{'chunks':>7} " + " ".join(f"{v:>26}" for v in VARIANTS))
    rows = {}
    for G in chunks:
        fns, close = variants(pkg, eng, torch, dev, ts.cuda_stream, n, t, d, G)
        try:
            res = alternating_medians(torch, ts, fns, samples, inner, 3)
        finally:
            close()
        rows[G] = res
        print(f"{G:7d} " + " ".join(f"{v[0]:10.4f} ({v[1]:.4f} .. {v[2]:.4f})".rjust(26) for v in res.values()), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--field", default="fr")
    ap.add_argument("--n", type=int, default=16)
    ap.add_argument("--t", type=int, default=5)
    ap.add_argument("--d", type=int, default=5)
    ap.add_argument("--chunks", default="1,64,256,1024")
    ap.add_argument("--repeat", type=int, default=2, help="the whole table this many times: the run-to-run spread")
    args = ap.parse_args()
    import torch
    from __graft_entry__ import load_package
    pkg = load_package()
    eng = pkg.Engine(0, field=args.field)
    dev = torch.device("cuda", 0)
    ts = torch.cuda.Stream(device=dev)
    try:
        for _ in range(args.repeat):
            table(pkg, eng, torch, dev, ts, args.n, args.t, args.d, [int(v) for v in args.chunks.split(",")])
    finally:
        eng.set_fused_batchrecon(pkg.hbmpc.FUSED_BATCHRECON_DEFAULT[args.field])
        eng.close()


if __name__ == "__main__":
    main()
