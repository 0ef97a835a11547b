#!/usr/bin/env python3
"""RanSha and RanDouSha for all parties on one device: hbmpc_[gl_]dev_ransha_parties / _randousha_parties as ONE launch (a workgroup per
column, csrc/kernels_producers_wg.hpp) and as the separate launches, against the existing handle at the same shape (run() from the
dealers' polynomials, finish() from the dealt shares), eager and replayed as a HIP graph.  The six variants of a size are timed
alternating in one process (medians of device-event samples, tools/bench_fpdiv.py).

With --triples: the triple factory from the dealers' polynomials, ransha_parties + randousha_parties + triplegen_parties (three launches)
against the Preprocessing handle's run(), at N triples per party.
    python tools/bench_producers_parties.py [--field fr|goldilocks] [--kind ransha|randousha] [--n 16 --t 5] [--columns 1,256,2048]
    python tools/bench_producers_parties.py --triples 1100 [--n 16 --t 5]"""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_fpdiv import alternating_medians  # noqa: E402

VARIANTS = ("one eager", "separate eager", "handle eager", "one graph", "separate graph", "handle graph")


def rand_elements(torch, dev, field, *shape):
    """uniform-ish canonical field elements generated on the device"""
    if field == "goldilocks":
        return torch.randint(0, 1 << 62, shape, dtype=torch.int64, device=dev)
    import bench
    return bench._rand_fr(torch, dev, *shape)


def polynomials(torch, dev, field, kind, n, t, K):
    """the dealers' coefficient arrays [dealer][K][deg + 1]; RanDouSha's two share their secrets"""
    cs = [rand_elements(torch, dev, field, n, K, t + 1)]
    if kind == "randousha":
        cs.append(rand_elements(torch, dev, field, n, K, 2 * t + 1))
        cs[1][:, :, 0] = cs[0][:, :, 0]
    torch.cuda.synchronize()
    return cs


class Direct:
    """the buffers of one device call, as torch tensors"""

    def __init__(self, eng, torch, dev, kind, n, t, K, coeffs):
        self.eng, self.kind, self.n, self.t, self.K, self.coeffs = eng, kind, n, t, K, coeffs
        eb, dou = eng.ebytes, kind == "randousha"
        nver = n - t - 1 if dou else 2 * t
        buf = lambda nbytes: torch.zeros(max(nbytes, 16), dtype=torch.uint8, device=dev)  # noqa: E731
        self.b = {"ws": buf((2 * n * n * K + max(nver * n, 2 * t, t + 1) * K) * eb), "bad": buf(8), "status": buf(nver * K), "summary": buf(16)}
        for sfx in ("t", "2t") if dou else ("t",):
            self.b.update({"dealt_" + sfx: buf(n * n * K * eb), "out_" + sfx: buf(n * K * (t + 1 if dou else n - 2 * t) * eb), "yv_" + sfx: buf(n * nver * K * eb),
                           "sel_" + sfx: buf(2 * nver * K * eb), "st_" + sfx: buf(4 * nver * K)})

    def call(self, from_coeffs, stream):
        p = {k: v.data_ptr() for k, v in self.b.items()}
        co = [c.data_ptr() for c in self.coeffs] if from_coeffs else [0, 0]
        if self.kind == "ransha":
            rc = self.eng.ransha_parties(co[0], p["dealt_t"], self.K, self.n, self.t, 2 * self.t + 1, p["out_t"], p["yv_t"], p["ws"], p["status"], p["summary"],
                                         p["bad"], stream=stream)
        else:
            rc = self.eng.randousha_parties(co[0], co[1], p["dealt_t"], p["dealt_2t"], self.K, self.n, self.t, p["out_t"], p["out_2t"], p["yv_t"], p["yv_2t"],
                                            p["ws"], p["sel_t"], p["sel_2t"], p["st_t"], p["st_2t"], p["bad"], stream=stream)
        assert rc == 0, self.eng.last_error()


def variants(pkg, eng, torch, dev, stream, kind, n, t, K, from_coeffs):
    """({variant: callable}, close): the six ways of one shape; every graph is recorded after two eager runs of its form"""
    graphs, fns = [], {}
    coeffs = polynomials(torch, dev, eng.field, kind, n, t, K)
    d = Direct(eng, torch, dev, kind, n, t, K, coeffs)
    eng.set_fused_producers(0)
    d.call(True, stream)  # the dealt shares exist from here on
    for form, fused in (("one", 1 << 30), ("separate", 0)):
        def eager(fused=fused):
            eng.set_fused_producers(fused)
            d.call(from_coeffs, stream)
        eager()
        eager()
        eng.sync(stream)
        eng.graph_begin(stream)
        try:
            eager()
        finally:
            g = eng.graph_end(stream)
        graphs.append(g)
        fns[form + " eager"], fns[form + " graph"] = eager, (lambda g=g: eng.graph_launch(g, stream))
    P = pkg.pipelines
    h = P.RanSha(eng, n, t, K, stream=stream) if kind == "ransha" else P.RanDouSha(eng, n, t, K, stream=stream)
    for name, c in zip(("coeffs",) if kind == "ransha" else ("coeffs_t", "coeffs_2t"), coeffs):
        eng.d2d(h.buffer(name)[0], c.data_ptr(), c.numel() * 8, stream)
    h.deal()
    hrun = (lambda: h.run(check=False)) if from_coeffs else (lambda: h.finish(check=False))
    hrun()
    hrun()
    eng.sync(stream)
    eng.graph_begin(stream)
    try:
        hrun()
    finally:
        hg = eng.graph_end(stream)
    graphs.append(hg)
    fns["handle eager"], fns["handle graph"] = hrun, (lambda: eng.graph_launch(hg, stream))

    def close():
        eng.sync(stream)
        for g in graphs:
            eng.graph_destroy(g)
        h.close()
    return {k: fns[k] for k in VARIANTS}, close


def table(pkg, eng, torch, dev, ts, kind, n, t, columns, from_coeffs, samples=15, inner=10):
    mode = "from coefficients" if from_coeffs else "from dealt shares"
    print(f"{kind} {eng.field} n={n} t={t} {mode}; ms per call, median (p10 .. p90) of {samples} samples of {inner} calls")
    print(f"{'columns':>7} " + " ".join(f"{v:>26}" for v in VARIANTS))
    rows = {}
    for K in columns:
        fns, close = variants(pkg, eng, torch, dev, ts.cuda_stream, kind, n, t, K, from_coeffs)
        try:
            res = alternating_medians(torch, ts, fns, samples, inner, 3)
        finally:
            close()
        rows[K] = res
        print(f"{K:7d} " + " ".join(f"{v[0]:10.4f} ({v[1]:.4f} .. {v[2]:.4f})".rjust(26) for v in res.values()), flush=True)
    return rows


def triples(pkg, eng, torch, dev, ts, n, t, N, samples=15, inner=10):
    """dealers' polynomials -> [c]_t: the three device calls and the four strided copies of the parties' lists into TripleGen's [party][N]
    arrays (what the handle does when N is no multiple of n - 2t and t + 1) against the Preprocessing handle's run()"""
    assert N % (2 * t + 1) == 0
    s, eb = ts.cuda_stream, eng.ebytes
    K_rs, K_rd = -(-2 * N // (n - 2 * t)), -(-N // (t + 1))
    rs = Direct(eng, torch, dev, "ransha", n, t, K_rs, polynomials(torch, dev, eng.field, "ransha", n, t, K_rs))
    rd = Direct(eng, torch, dev, "randousha", n, t, K_rd, polynomials(torch, dev, eng.field, "randousha", n, t, K_rd))
    G = N // (2 * t + 1)
    buf = lambda nbytes: torch.zeros(nbytes, dtype=torch.uint8, device=dev)  # noqa: E731
    sizes = {"a": n * N * eb, "b": n * N * eb, "rt": n * N * eb, "r2t": n * N * eb, "Y": n * n * G * eb, "Z": n * G * eb, "opened": N * eb, "c": n * N * eb}
    tg = {k: buf(v) for k, v in sizes.items()}
    L = pkg.lib()
    fn = getattr(L, ("hbmpc_" if eng.field == "fr" else "hbmpc_gl_") + "dev_triplegen_parties")
    row = N * eb
    pitch_rs, pitch_rd = (n - 2 * t) * K_rs * eb, (t + 1) * K_rd * eb

    def three():
        rs.call(True, s)
        rd.call(True, s)
        # a = the first N of every party's RanSha list, b = the next N (take_random_shares twice), r_t and r_2t the first N of RanDouSha's
        for name, src, pitch in (("a", rs.b["out_t"].data_ptr(), pitch_rs), ("b", rs.b["out_t"].data_ptr() + row, pitch_rs),
                                 ("rt", rd.b["out_t"].data_ptr(), pitch_rd), ("r2t", rd.b["out_2t"].data_ptr(), pitch_rd)):
            rc = L.hbmpc_memcpy_d2d_rows(eng.ctx, C.c_void_p(tg[name].data_ptr()), C.c_size_t(row), C.c_void_p(src), C.c_size_t(pitch), C.c_size_t(row),
                                         C.c_size_t(n), C.c_void_p(s))
            assert rc == 0, eng.last_error()
        rc = fn(eng.ctx, *(C.c_void_p(tg[k].data_ptr()) for k in ("a", "b", "r2t", "rt")), C.c_size_t(N), C.c_size_t(n), C.c_size_t(t),
                *(C.c_void_p(tg[k].data_ptr()) for k in ("Y", "Z", "opened", "c")), None, None, None, C.c_void_p(s))
        assert rc == 0, eng.last_error()
    pp = pkg.pipelines.Preprocessing(eng, n, t, N, stream=s)
    for h, names, d in ((pp.rs, ("coeffs",), rs), (pp.rd, ("coeffs_t", "coeffs_2t"), rd)):
        for name, c in zip(names, d.coeffs):
            eng.d2d(h.buffer(name)[0], c.data_ptr(), c.numel() * 8, s)
    fns = {"three calls eager": three, "handle eager": lambda: pp.run(check=False)}
    graphs = []
    for k in list(fns):
        f = fns[k]
        f()
        f()
        eng.sync(s)
        eng.graph_begin(s)
        try:
            f()
        finally:
            g = eng.graph_end(s)
        graphs.append(g)
        fns[k.replace("eager", "graph")] = lambda g=g: eng.graph_launch(g, s)
    try:
        res = alternating_medians(torch, ts, fns, samples, inner, 3)
    finally:
        eng.sync(s)
        for g in graphs:
            eng.graph_destroy(g)
        pp.close()
    print(f"triples {eng.field} n={n} t={t} N={N} (RanSha {K_rs} columns, RanDouSha {K_rd}); ms per run, median (p10 .. p90)")
    for k, v in res.items():
        print(f"  {k:>20}: {v[0]:.4f} ({v[1]:.4f} .. {v[2]:.4f})", flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--field", default="fr")
    ap.add_argument("--kind", default="ransha")
    ap.add_argument("--n", type=int, default=16)
    ap.add_argument("--t", type=int, default=5)
    ap.add_argument("--columns", default="1,64,256,2048")
    ap.add_argument("--dealt", action="store_true", help="from the dealt shares (the handle's finish()) instead of the coefficients")
    ap.add_argument("--triples", type=int, default=0, help="time dealers -> triples at this many triples per party instead")
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
            if args.triples:
                triples(pkg, eng, torch, dev, ts, args.n, args.t, args.triples)
            else:
                table(pkg, eng, torch, dev, ts, args.kind, args.n, args.t, [int(v) for v in args.columns.split(",")], not args.dealt)
    finally:
        eng.set_fused_producers(pkg.hbmpc.FUSED_PRODUCERS_DEFAULT[args.field])
        eng.close()


if __name__ == "__main__":
    main()
