#!/usr/bin/env python3
"""PRandBit / PRandInt timing from device events: the fold, the RISS-to-Shamir conversion (Fr and Goldilocks, with and without the
GF(2^8) output, all parties and the one-party form, both work layouts) and the finalize.  One JSON line per (n, t, B) with each
kernel's bytes and its floors:
  bytes / 5.05 TB/s                     (the copy rate of profiles/r04_hbm_mix_ubench.txt)
  Fr conversion: terms x 32/203 / 1.85e11 per second  -- a 64 x 256-bit multiply-add into lazy columns is 32 vector instructions,
                                        the register-resident modmul hbmpc_dev_modmul_ubench measures is 203 (fr_u29.hpp)
At n = 16, t = 5 and B = 384, 4 096 the one-party conversion is also spelled with what the library had before -- one
hbmpc_dev_fr_op_scalar (multiply by f_T(alpha_j)) and one hbmpc_dev_fr_op (add) per set, r_T widened to U256 -- and timed in the same
process: `baseline_one_party_ms` and `speedup_one_party`.  Where B is a multiple of t + 1 the whole protocol as one device call
(hbmpc_dev_prandbit_parties) is timed too, with the one-launch threshold at 2^30 and at 0: `parties_call_one_ms`,
`parties_call_launches_ms`, and `parties_call_form` (which form the first ran as; tools/sweep_fused_prandbit.py sweeps the small batches).
    python tools/bench_prandbit.py [--shapes 16:5:384,16:5:4096,16:5:16384,4:1:1048576] [--iters 10] [--no-baseline]"""
import argparse
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

R_FR = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
HBM_RATE = 5.05e12
FR_MODMUL_RATE = 1.85e11
MAC_PER_MODMUL = 32 / 203


def f_T(p, n, T, j):
    """f_T(alpha_j) = prod (1 - alpha_j / alpha_m) over the domain of the next power of two (generator 7, two-adicity 32)"""
    size = 1 << max(0, (n - 1).bit_length())
    w = pow(pow(7, (p - 1) >> 32, p), 2**32 // size, p)
    r = 1
    for m in T:
        r = r * (1 - pow(w, j, p) * pow(pow(w, m, p), p - 2, p)) % p
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="16:5:384,16:5:4096,16:5:16384,4:1:1048576")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--no-baseline", action="store_true")
    args = ap.parse_args()
    import itertools

    import torch
    from __graft_entry__ import load_package
    pkg = load_package()
    dev = torch.device("cuda", 0)
    fr, gl = pkg.Engine(0, field="fr"), pkg.Engine(0, field="goldilocks")
    ts = torch.cuda.Stream(device=dev)
    st = ts.cuda_stream

    def timed(fn, iters=args.iters):
        for _ in range(2):
            assert fn() == 0
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(ts):
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / iters

    for shape in args.shapes.split(","):
        n, t, B = (int(x) for x in shape.split(":"))
        Tn, Town = math.comb(n, t), math.comb(n - 1, t)
        lk = 61 - math.ceil(math.log2(n))
        gen = torch.Generator(device=dev).manual_seed(B)
        contrib = torch.randint(0, (1 << lk) + 1, (n, Tn, B), dtype=torch.int64, device=dev, generator=gen)
        sums = torch.zeros((Tn, B), dtype=torch.int64, device=dev)
        bad = torch.zeros((n, Tn), dtype=torch.uint8, device=dev)
        out_p = torch.zeros((n, B, 4), dtype=torch.int64, device=dev)
        out_q = torch.zeros((n, B), dtype=torch.int64, device=dev)
        out_2 = torch.zeros((n, B), dtype=torch.uint8, device=dev)
        bp = torch.zeros((n, B, 4), dtype=torch.int64, device=dev)
        b2 = torch.zeros((n, B), dtype=torch.uint8, device=dev)
        opened = torch.randint(0, 2**62, (B,), dtype=torch.int64, device=dev, generator=gen)
        j = n - 1  # the one-party form: the last party's sets are the first C(n-1, t) of the enumeration's non-members
        sets = list(itertools.combinations(range(n), t))
        own_rows = torch.tensor([k for k, T in enumerate(sets) if j not in T], device=dev)
        row = {"n": n, "t": t, "B": B, "tsets": Tn, "own_tsets": Town}
        row["fold_ms"] = timed(lambda: fr.dev_riss_fold(contrib.data_ptr(), n, Tn, B, lk, sums.data_ptr(), bad.data_ptr(), st))
        torch.cuda.synchronize()
        assert not bool(bad.any())
        own = sums[own_rows].contiguous()
        P, Q, R2, S, O = out_p.data_ptr(), out_q.data_ptr(), out_2.data_ptr(), sums.data_ptr(), own.data_ptr()
        row["convert_fr_gf2_ms"] = timed(lambda: fr.dev_riss_convert_parties(S, n, t, B, P, R2, stream=st))
        row["convert_fr_ms"] = timed(lambda: fr.dev_riss_convert_parties(S, n, t, B, P, 0, stream=st))
        row["convert_gl_gf2_ms"] = timed(lambda: gl.dev_riss_convert_parties(S, n, t, B, Q, R2, stream=st))
        row["convert_gl_ms"] = timed(lambda: gl.dev_riss_convert_parties(S, n, t, B, Q, 0, stream=st))
        for form, name in ((1, "wide"), (2, "sliced")):  # the two work layouts, whatever the size would pick
            fr.set_riss_form(form), gl.set_riss_form(form)
            row[f"convert_fr_{name}_ms"] = timed(lambda: fr.dev_riss_convert_parties(S, n, t, B, P, 0, stream=st))
            row[f"convert_gl_{name}_ms"] = timed(lambda: gl.dev_riss_convert_parties(S, n, t, B, Q, 0, stream=st))
        fr.set_riss_form(0), gl.set_riss_form(0)
        row["convert_fr_one_party_gf2_ms"] = timed(lambda: fr.dev_riss_convert_parties(O, n, t, B, P, R2, party_ids=[j], own_sets_only=True, stream=st))
        row["convert_fr_one_party_ms"] = timed(lambda: fr.dev_riss_convert_parties(O, n, t, B, P, 0, party_ids=[j], own_sets_only=True, stream=st))
        row["convert_gl_one_party_ms"] = timed(lambda: gl.dev_riss_convert_parties(O, n, t, B, Q, 0, party_ids=[j], own_sets_only=True, stream=st))
        row["finalize_ms"] = timed(lambda: fr.dev_prandbit_finalize_parties(opened.data_ptr(), P, R2, B, n, bp.data_ptr(), b2.data_ptr(), st))
        if B % (t + 1) == 0 and n * n * (B // (t + 1)) * 8 <= 1 << 30:
            # the whole protocol as one device call (hbmpc_dev_prandbit_parties): with the threshold at 2^30 (ONE launch where the shape's
            # tables fit a workgroup's LDS and the batch is small; `parties_call_form` says which ran) and at 0 (the eight launches)
            G = B // (t + 1)
            b_q = torch.zeros((n, B), dtype=torch.int64, device=dev)  # the constant sharing of the bit 0
            rb = torch.zeros((n, B), dtype=torch.int64, device=dev)
            Y = torch.full((n, n, G), -1, dtype=torch.int64, device=dev)
            Z = torch.zeros((n, G), dtype=torch.int64, device=dev)
            rst = torch.zeros((n, G), dtype=torch.uint8, device=dev)

            def whole():
                return fr.prandbit_parties(gl, contrib.data_ptr(), b_q.data_ptr(), n, t, B, lk, S, bad.data_ptr(), P, R2, Q, rb.data_ptr(), Y.data_ptr(),
                                           Z.data_ptr(), opened.data_ptr(), bp.data_ptr(), b2.data_ptr(), rst.data_ptr(), stream=st)

            for name, fused in (("one", 1 << 30), ("launches", 0)):
                fr.set_fused_prandbit(fused)
                Y.fill_(-1)
                row[f"parties_call_{name}_ms"] = timed(whole)
                torch.cuda.synchronize()
                if fused:
                    row["parties_call_form"] = "one launch" if bool((Y == -1).all()) else "separate launches"  # the one launch leaves the workspace alone
            fr.set_fused_prandbit(pkg.hbmpc.FUSED_PRANDBIT_DEFAULT)
        if not args.no_baseline and (n, t) == (16, 5) and B <= 4096:
            # the same one-party conversion with the element-wise calls: 2 launches per set
            r256 = torch.zeros((Town, B, 4), dtype=torch.int64, device=dev)
            r256[:, :, 0] = own
            acc = torch.zeros((B, 4), dtype=torch.int64, device=dev)
            tmp = torch.zeros((B, 4), dtype=torch.int64, device=dev)
            coef = []
            for T in (T for T in sets if j not in T):
                v = f_T(R_FR, n, T, j)
                coef.append(np.array([(v >> (64 * k)) & (2**64 - 1) for k in range(4)], dtype=np.uint64))
            base = r256.data_ptr()

            def baseline():
                with torch.cuda.stream(ts):
                    acc.zero_()
                for k in range(Town):
                    rc = fr.dev_fr_op_scalar("mul", base + k * B * 32, coef[k], B, tmp.data_ptr(), st)
                    rc |= fr.dev_fr_op("add", acc.data_ptr(), tmp.data_ptr(), B, acc.data_ptr(), st)
                    if rc:
                        return rc
                return 0

            row["baseline_one_party_ms"] = timed(baseline, iters=3)
            torch.cuda.synchronize()
            assert fr.dev_riss_convert_parties(O, n, t, B, P, 0, party_ids=[j], own_sets_only=True, stream=st) == 0
            torch.cuda.synchronize()
            assert torch.equal(acc, out_p[0]), "the element-wise composition and the conversion kernel disagree"
            row["baseline_launches"] = 2 * Town
            row["speedup_one_party"] = round(row["baseline_one_party_ms"] / row["convert_fr_one_party_ms"], 1)
        terms = (n - t) * Tn * B  # a set's term exists for the n - t parties outside it
        floors = {
            "fold": (n + 1) * Tn * B * 8 / HBM_RATE,
            "convert_fr": max((Tn * B * 8 + n * B * 32) / HBM_RATE, terms * MAC_PER_MODMUL / FR_MODMUL_RATE),
            "convert_gl": (Tn * B * 8 + n * B * 8) / HBM_RATE,
            "convert_fr_one_party": max((Town * B * 8 + B * 32) / HBM_RATE, Town * B * MAC_PER_MODMUL / FR_MODMUL_RATE),
            "finalize": (B * 8 + n * B * 66) / HBM_RATE,
        }
        row["floor_ms"] = {k: round(v * 1e3, 5) for k, v in floors.items()}
        row["over_floor"] = {k: round(row[k + "_ms"] / (v * 1e3), 2) for k, v in floors.items()}
        print(json.dumps({k: (round(v, 5) if isinstance(v, float) else v) for k, v in row.items()}), flush=True)
        del contrib, sums, own
        torch.cuda.empty_cache()
    fr.close(), gl.close()


if __name__ == "__main__":
    main()
