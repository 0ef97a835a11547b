#!/usr/bin/env python3
"""RandBit timing: the phase-2 kernel (hbmpc_[gl_]dev_randbit_finalize_parties) from device events, and the whole pipeline
(hbmpc_pipe_randbit_create) eager and replayed as a HIP graph, in both forms of hbmpc_[gl_]dev_randbit_parties: ONE launch (forced by
hbmpc_set_fused_randbit; not timed beyond --one-max chunks) and the nine launches (threshold 0).  One JSON line per (field, n, N), with the bytes the finalize moves,
its modular multiplications per element and the two floors they give:
  bytes / 4.2-5.0 TB/s  (the measured mixed read/write stream band, profiles/r04_hbm_mix_ubench.txt)
  multiplications / 1.85e11 per second  (register-resident Fr modmul rate; Goldilocks' mulm is far cheaper,
  so its compute floor is quoted for comparison only)
    python tools/bench_randbit.py [--fields fr,goldilocks] [--n 16] [--t 5] [--sizes 1048576,1024] [--iters 20]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

R_FR = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
P_GL = 2**64 - 2**32 + 1
HBM_BAND = (4.2e12, 5.0e12)
FR_MODMUL_RATE = 1.85e11


def muls_per_element(p, parties):
    """modular products per element of k_randbit_finalize, counted from csrc/kernels_sqrt.hpp: to_mont 1; pow_fixed of (T-1)/2
    (bits - 1 squarings + popcount - 1 products); g = u^2 A 2; 24 squarings; the dlog's table products 1 + 2 + 3; omega_pow 3, times u
    1, times 2^-1 1; then one per party"""
    e = (p - 1) >> 33
    pow_muls = (e.bit_length() - 1) + (bin(e).count("1") - 1)
    return 1 + pow_muls + 2 + 24 + 6 + 5 + parties


def rand_elems(field, rng, count):
    if field == "goldilocks":
        return (rng.integers(0, 2**63, size=count, dtype=np.uint64) * np.uint64(2)) % np.uint64(P_GL)
    x = rng.integers(0, 2**63, size=(count, 4), dtype=np.uint64) * np.uint64(2)
    x[:, 3] %= np.uint64(0x73EDA753299D7D48)  # top limb below r's: canonical
    return x


def shares(eng, secrets, n, t, rng):
    co = np.stack([secrets] + [rand_elems(eng.field, rng, secrets.shape[0]) for _ in range(t)], axis=1)
    rc, sh = eng.compute_shares(np.ascontiguousarray(co), n, t)
    assert rc == 0, eng.last_error()
    return sh


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fields", default="goldilocks,fr")
    ap.add_argument("--n", type=int, default=16)
    ap.add_argument("--t", type=int, default=5)
    ap.add_argument("--sizes", default=str(1 << 20) + ",1024")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--one-max", type=int, default=16384, help="the one-launch form is not timed beyond this many chunks of t + 1 elements")
    args = ap.parse_args()
    import torch
    from __graft_entry__ import load_package
    pkg = load_package()
    n, t = args.n, args.t
    for field in args.fields.split(","):
        eng = pkg.Engine(0, field=field)
        p = R_FR if field == "fr" else P_GL
        for N0 in [int(s) for s in args.sizes.split(",")]:
            N = (N0 // (t + 1)) * (t + 1)
            rng = np.random.default_rng(N)
            a, ta, tb = (rand_elems(field, rng, N) for _ in range(3))
            rc, tc = eng.fr_op("mul", ta, tb)
            assert rc == 0
            ts = torch.cuda.Stream(device=torch.device("cuda", 0))
            st = ts.cuda_stream
            rb = pkg.pipelines.RandBit(eng, n, t, N, stream=st)
            rb.upload(shares(eng, a, n, t, rng), shares(eng, ta, n, t, rng), shares(eng, tb, n, t, rng), shares(eng, tc, n, t, rng))
            rb.run(check=True)

            def timed(fn):
                fn()
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                with torch.cuda.stream(ts):
                    e0.record()
                    for _ in range(args.iters):
                        fn()
                    e1.record()
                e1.synchronize()
                return e0.elapsed_time(e1) / args.iters

            ptr = {k: rb.buffer(k)[0] for k in ("a", "sqop", "out", "status", "summary")}
            fin = lambda: eng.randbit_finalize_parties(ptr["a"], ptr["sqop"], N, n, ptr["out"], ptr["status"], ptr["summary"], st)  # noqa: E731
            ms_fin = timed(fin)
            forms = {}
            for form, fused in (("one", 1 << 30), ("nine", 0)):
                if form == "one" and N // (t + 1) > args.one_max:
                    forms[form] = (None, None)
                    continue
                eng.set_fused_randbit(fused)
                ms_eager = timed(lambda: rb.run(check=False))
                rb.capture()  # records the form that the threshold selects now
                forms[form] = (round(ms_eager, 4), round(timed(rb.replay), 4))
                assert not rb.status().any()
            eng.set_fused_randbit(pkg.hbmpc.FUSED_RANDBIT_DEFAULT[field])
            eb = eng.ebytes
            nbytes = (1 + 2 * n) * N * eb + N
            muls = muls_per_element(p, n)
            floor_hbm = [nbytes / bw * 1e3 for bw in HBM_BAND[::-1]]
            floor_alu = muls * N / FR_MODMUL_RATE * 1e3
            print(json.dumps({"field": field, "n": n, "t": t, "N": N, "finalize_ms": round(ms_fin, 4),
                              "pipeline_one_launch_ms": {"eager": forms["one"][0], "graph": forms["one"][1]},
                              "pipeline_nine_launches_ms": {"eager": forms["nine"][0], "graph": forms["nine"][1]},
                              "finalize_bytes": nbytes, "modmul_per_element": muls,
                              "floor_hbm_ms": [round(x, 4) for x in floor_hbm], "floor_modmul_ms": round(floor_alu, 4),
                              "finalize_over_floor": round(ms_fin / max(floor_hbm[1], floor_alu if field == "fr" else 0.0), 2)}), flush=True)
            rb.close()
        eng.close()


if __name__ == "__main__":
    main()
