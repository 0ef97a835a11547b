#!/usr/bin/env python3
"""Integer-point Shamir timing (hbmpc_[gl_]dev_shamir_compute_shares, hbmpc_[gl_]dev_shamir_batch_interpolate_c0), eager, each number
from a host clock around calls that end in a stream synchronise, the alternatives of one shape taking turns sample by sample.

  encode   at (m, d, B) over points 1..m: the small-weight route forced, the Horner route forced on the same points, the planner's
           own choice, and hbmpc_dev_compute_shares at the same (n = m, d, B), which moves the same bytes on the roots-of-unity domain.
           ms per call, TB/s over ebytes B (d + 1 + m) bytes.  The routes' outputs are compared before anything is timed.
  open     dev_shamir_batch_interpolate_c0 through the points 1..S against dev_batch_interpolate_c0 through the domain ids 0..S-1
           (n = S), G columns.

    python tools/bench_shamir.py [--encode fr:4:1:1048576,fr:16:5:1048576,fr:31:10:262144,gl:16:5:1048576,fr:16:5:2048,fr:16:5:8192]
        [--open fr:6:1048576,fr:16:1048576] [--samples 15] [--calls 5] [--out profiles/shamir_bench.txt]
Run it twice: the second run appends, and the two medians of a line are its run-to-run spread."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stats(v):
    s = np.sort(np.array(v))
    return "%8.4f (%.4f .. %.4f)" % (float(np.median(s)), float(s[len(s) // 10]), float(s[(len(s) * 9) // 10]))


def alternate(fns, sync, samples, calls):
    """{name: [ms per call]}: the functions take turns, so that all of them see the same machine"""
    for fn in fns.values():
        for _ in range(3):
            fn()
    sync()
    res = {k: [] for k in fns}
    for _ in range(samples):
        for k, fn in fns.items():
            t0 = time.perf_counter()
            for _ in range(calls):
                fn()
            sync()
            res[k].append((time.perf_counter() - t0) * 1e3 / calls)
    return res


def rand_elems(eng, rng, shape):
    """canonical field elements: 64 random bits per limb, the top limb cut below the modulus's"""
    if eng.field == "fr":
        a = rng.integers(0, 1 << 64, size=tuple(shape) + (4,), dtype=np.uint64)
        a[..., 3] &= np.uint64((1 << 62) - 1)
        return a
    return rng.integers(0, (1 << 64) - (1 << 32), size=tuple(shape), dtype=np.uint64)


def encode(eng, m, d, B, samples, calls, emit):
    rng = np.random.default_rng(m * 1000 + d)
    st = eng.stream_create()
    sync = lambda: eng.sync(st)  # noqa: E731
    eb = eng.ebytes
    pts = list(range(1, m + 1))
    c = eng.dev_alloc(B * (d + 1) * eb)
    outs = [eng.dev_alloc(B * m * eb) for _ in range(2)]
    eng.h2d(c, rand_elems(eng, rng, (B, d + 1)), st)

    def shamir(route, o):
        def fn():
            eng.set_shamir_route(route)
            assert eng.dev_shamir_compute_shares(c, B, pts, d, o, st) == 0, eng.last_error()
        return fn

    def domain():
        assert eng.dev_compute_shares(c, B, m, d, outs[0], st) == 0, eng.last_error()

    shamir(1, outs[0])(), shamir(2, outs[1])()
    a, b = np.zeros(B * m * eb // 8, dtype=np.uint64), np.zeros(B * m * eb // 8, dtype=np.uint64)
    eng.d2h(a, outs[0], st), eng.d2h(b, outs[1], st)
    sync()
    assert np.array_equal(a, b), "the small-weight and the Horner route disagree"
    kernels = {}
    for route in (1, 2, 0):
        eng.set_shamir_route(route)
        kernels[route] = eng.shamir_route(pts, d, B)[1]
    names = {1: "small-weight", 2: "wave per secret", 3: "lane per secret"}
    fns = {"shamir small-weight forced": shamir(1, outs[0]), "shamir Horner forced": shamir(2, outs[0]), "shamir planner": shamir(0, outs[0]),
           "domain compute_shares": domain}
    res = alternate(fns, sync, samples, calls)
    eng.set_shamir_route(0)
    nbytes = eb * B * (d + 1 + m)
    emit("encode %s m=%d d=%d B=%d (%.1f MB moved): forced 1 -> %s, forced 2 -> %s, planner -> %s" %
         (eng.field, m, d, B, nbytes / 1e6, names[kernels[1]], names[kernels[2]], names[kernels[0]]))
    for k, v in res.items():
        emit("    %-28s %s ms   %6.3f TB/s" % (k, stats(v), nbytes / (float(np.median(v)) * 1e-3) / 1e12))
    for p in [c] + outs:
        eng.dev_free(p)
    eng.stream_destroy(st)


def open_c0(eng, S, G, samples, calls, emit):
    rng = np.random.default_rng(S)
    st = eng.stream_create()
    sync = lambda: eng.sync(st)  # noqa: E731
    eb = eng.ebytes
    ev, tmp, c0, deg = eng.dev_alloc(S * G * eb), eng.dev_alloc(S * G * eb), eng.dev_alloc(G * eb), eng.dev_alloc(G * 4)
    eng.h2d(ev, rand_elems(eng, rng, (S, G)), st)
    pts, ids = list(range(1, S + 1)), list(range(S))

    def points():
        assert eng.dev_shamir_batch_interpolate_c0(pts, ev, G, G, tmp, c0, deg, st) == 0, eng.last_error()

    def domain():
        assert eng.dev_batch_interpolate_c0(ids, ev, G, G, S, tmp, c0, deg, st) == 0, eng.last_error()

    res = alternate({"shamir points 1..S": points, "domain ids 0..S-1": domain}, sync, samples, calls)
    emit("open (c0 form) %s S=%d G=%d" % (eng.field, S, G))
    for k, v in res.items():
        emit("    %-28s %s ms" % (k, stats(v)))
    for p in (ev, tmp, c0, deg):
        eng.dev_free(p)
    eng.stream_destroy(st)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--encode", default="fr:4:1:1048576,fr:16:5:1048576,fr:31:10:262144,gl:16:5:1048576,fr:16:5:2048,fr:16:5:8192")
    ap.add_argument("--open", default="fr:6:1048576,fr:16:1048576")
    ap.add_argument("--samples", type=int, default=15)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    from __graft_entry__ import load_package
    pkg = load_package()
    engs = {"fr": pkg.Engine(0, field="fr"), "gl": pkg.Engine(0, field="goldilocks")}
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit("# tools/bench_shamir.py --samples %d --calls %d: ms per call, median (p10 .. p90), eager" % (args.samples, args.calls))
    for shape in filter(None, args.encode.split(",")):
        f, m, d, B = shape.split(":")
        encode(engs[f], int(m), int(d), int(B), args.samples, args.calls, emit)
    for shape in filter(None, args.open.split(",")):
        f, S, G = shape.split(":")
        open_c0(engs[f], int(S), int(G), args.samples, args.calls, emit)
    if args.out:
        with open(args.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")
    for e in engs.values():
        e.close()


if __name__ == "__main__":
    main()
