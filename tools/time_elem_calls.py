"""Host cost of the element-wise device entry points at a small batch, where the launch is nearly all there is: microseconds per
call of hbmpc_dev_fr_op, _fr_op_scalar, _triple_finalize_parties, _beaver_finalize_parties and _fpmul_middle, eager on the default
stream.  Each row: REPS blocks of CALLS calls, a synchronise after every block; the median, minimum and maximum over the blocks.

    python3 tools/time_elem_calls.py [--root OTHER_TREE] [--n 1024] [--parties 16]

--root: time the library of another checkout (built there) with the same script: run the two alternately for an A/B of host-side
changes.  Prints one JSON line."""
import argparse
import importlib.util
import json
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--n", type=int, default=1024)
ap.add_argument("--parties", type=int, default=16)
ap.add_argument("--calls", type=int, default=2000)
ap.add_argument("--reps", type=int, default=15)
a = ap.parse_args()
root = os.path.abspath(a.root)
sys.path.insert(0, root)
spec = importlib.util.spec_from_file_location("graft_entry_of_root", os.path.join(root, "__graft_entry__.py"))
entry = importlib.util.module_from_spec(spec)
spec.loader.exec_module(entry)
import numpy as np  # noqa: E402

from oracle import cref  # noqa: E402  (seeded canonical field elements)

eng = entry.load_package().Engine(0)
N, P, M, K = a.n, a.parties, 8, 16
eb = 32


def buf(elements):
    p = eng.dev_alloc(elements * eb)
    eng.h2d(p, cref.fill_random(0xE1E0 + elements, elements).reshape(elements, 4))
    return p


pub = [buf(N) for _ in range(3)]          # public operands [N]
per = [buf(P * N) for _ in range(8)]      # per-party operands and outputs [P][N]
rbits = buf(P * M * N)
scalar = cref.fill_random(7, 1).reshape(4)
eng.sync()

rows = {
    "fr_op_add": lambda: eng.dev_fr_op("add", pub[0], pub[1], N, pub[2]),
    "fr_op_mul": lambda: eng.dev_fr_op("mul", pub[0], pub[1], N, pub[2]),
    "fr_op_scalar_mul": lambda: eng.dev_fr_op_scalar("mul", pub[0], scalar, N, pub[2]),
    "triple_finalize_parties": lambda: eng.dev_elem_parties("triple_finalize", [per[0], pub[0], per[1]], N, P),
    "beaver_finalize_parties": lambda: eng.dev_elem_parties("beaver_finalize", [per[0], per[1], per[2], pub[0], pub[1], per[3]], N, P),
    "fpmul_middle": lambda: eng.dev_fpmul_middle(per[0], per[1], per[2], pub[0], pub[1], rbits, per[3], K, M, N, P, per[4], per[5], per[6]),
}
out = {"root": root, "n": N, "parties": P, "calls": a.calls, "reps": a.reps, "us_per_call": {}}
for name, fn in rows.items():
    assert fn() == 0, name
    eng.sync()
    t_w = time.perf_counter()
    while time.perf_counter() - t_w < 0.2:  # clocks up, code objects loaded
        fn()
    eng.sync()
    us = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        for _ in range(a.calls):
            fn()
        eng.sync()
        us.append((time.perf_counter() - t0) / a.calls * 1e6)
    out["us_per_call"][name] = {"median": round(statistics.median(us), 3), "min": round(min(us), 3), "max": round(max(us), 3)}
print(json.dumps(out))
