"""Which kernels a batch decode takes: the route planner (mpc-protocols_amd/csrc/recover_route.hpp) compiled for the CPU under ASan +
UBSan (tests/cpp/recover_routes_dump.cpp) over a grid of shapes, forms and knob settings.  The GPU tests compare bytes, and every route
gives the same bytes; this pins the routes themselves -- the BASELINE decode's two roles and its tail, BatchRecon's one launch on the
workgroup-per-tile kernel from 2 048 chunks on, the lazy fallback tables of host calls.  Runs without a GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "recover_routes_dump")
KNOBS = ["default", "mc0", "mc1,min1", "mc2", "generic", "small0", "wgs8", "single0", "second0", "lazy0", "lazy1", "lazy2"]
NS = [4, 5, 7, 10, 16, 17, 31, 32, 64, 100, 255]
FACTS = ["-", "capturing", "cached"]


def ds(n):
    t = (n - 1) // 3
    return sorted({(t, t), (2 * t, t), (1, t)} if t >= 1 else set())


def gs(knobs):
    """a small batch, and batch sizes at every threshold: 2 048 / 4 096 (matrix cores without / with OEC rounds), 8 192 (wave per chunk), 8 193
    (Goldilocks with OEC rounds), two tiles per workgroup (16 384 with 256 CUs, 512 with 8 workgroups), 2^20"""
    base = {1000, 1024, 2047, 2048, 2049, 4095, 4096, 4097, 8191, 8192, 8193, 8194, 16384, 16385, 1 << 20}
    if "wgs8" in knobs:
        base |= {512, 513}
    return sorted(base)


@pytest.fixture(scope="module")
def plan():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "cpp"), "recover_routes_dump"], stdout=subprocess.DEVNULL)

    def run(queries):
        text = "".join(" ".join(map(str, q)) + "\n" for q in queries)
        p = subprocess.run([BIN], input=text, capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stderr[-2000:]          # ASan / UBSan findings abort with a non-zero code
        lines = p.stdout.splitlines()
        assert len(lines) == len(queries)
        return dict(zip(queries, lines))
    return run


# (call, knobs, field, G, n, d, t, S, facts) -> the plan's first route and its tail
ANCHORS = [
    # BASELINE configs[2]: two roles of 10 and 11 rows, then k_second_chance_m, k_gao and k_unscale
    (("dev", "default", "fr", 1 << 20, 31, 10, 10, 31, "-"),
     "MfmaRows M=11 rows=10,11 roles=2 tail rmax=10 second=m tables=eager gao=unscale"),
    # BatchRecon's decode (S = d + t + 1, P(0)): the workgroup-per-tile kernel, one launch, from 2 048 chunks on
    (("p0", "default", "fr", 16384, 16, 5, 5, 11, "-"), "MfmaRowsTeam M=6 rows=6 roles=1 one rmax=0"),
    (("p0", "default", "fr", 2048, 16, 5, 5, 11, "-"), "MfmaRowsTeam M=6 rows=6 roles=1 one rmax=0"),
    (("p0", "default", "fr", 2047, 16, 5, 5, 11, "-"), "Wide M=6 rows=0 roles=0 one rmax=0"),
    # a small decode with OEC rounds: the second chance inside the wave-per-chunk kernel, then k_gao un-scaling inline
    (("dev", "default", "fr", 1000, 16, 5, 5, 16, "-"), "Wide M=6 rows=0 roles=0 tail rmax=5 second=kernel tables=eager gao=inline"),
    # the same from the host, first sight of the sender set: lazy tables, the second chance as its own launch if a chunk is flagged
    (("host", "default", "fr", 1000, 16, 5, 5, 16, "-"), "Wide M=6 rows=0 roles=0 tail rmax=5 second=m tables=lazy gao=inline"),
    (("host", "default", "fr", 1000, 16, 5, 5, 16, "cached"), "Wide M=6 rows=0 roles=0 tail rmax=5 second=kernel tables=eager gao=inline"),
    (("p0", "default", "gl", 1 << 20, 16, 5, 5, 11, "-"), "MfmaRowsGl M=6 rows=0 roles=0 one"),
    (("dev", "default", "sat32", 1 << 20, 31, 10, 10, 31, "-"), "Generic M=11 rows=0 roles=0 tail rmax=10 second=generic tables=eager gao=unscale"),
    # the fpmul pair form: 2 x 2^18 values per sender row
    (("pair262144", "default", "fr", 1 << 19, 16, 5, 5, 11, "-"), "MfmaRowsSub M=6 rows=6 roles=1 one"),
    (("p0", "mc0", "fr", 20000, 10, 3, 3, 7, "-"), "RecoverM M=4 rows=0 roles=0 one rmax=0 second=none tables=eager gao=none all=RecoverM,Generic"),
    # the RanDouSha verifier's interpolation of 16 shares: the inverse DFT with c0 and the degrees from the kernel
    (("interp_c0", "default", "fr", 699050, 16, 15, 0, 16, "-"), "IdftDegrees all=IdftDegrees,Idft,Decode c0_only=1"),
    (("interp", "default", "fr", 699050, 16, 15, 0, 16, "-"), "Idft all=Idft,Decode c0_only=0"),
    (("interp_deg", "default", "fr", 1000, 16, 15, 0, 16, "-"), "Decode all=Decode"),
]


def test_anchor_routes(plan):
    got = plan([q for q, _ in ANCHORS])
    for q, want in ANCHORS:
        assert got[q].startswith(want), (q, got[q])


def forms(d):
    """every form of the call: plain (device / host pointers, P(0), row slots), one coefficient, the grouped exact-degree test,
    select-two, select-two in groups, the fpmul pair form"""
    out = ["dev", "host", "p0", "p0_host", "slots", "coeff%d" % d, "top%d_group%d" % (d, 1024), "pair%d" % 4096]
    out += ["sel0_%d" % d, "sel0_%d_group%d" % (d, 1024)]
    return out


def test_grid_invariants(plan):
    queries = []
    for knobs in KNOBS:
        for field in ("fr", "gl", "sat32"):
            for n in NS:
                for d, t in ds(n):
                    needed = d + t + 1
                    for S in sorted({needed, needed + 1, n} & set(range(needed, n + 1))):
                        for form in forms(d):
                            for i, G in enumerate(gs(knobs)):
                                # select-two calls pass t = S - d - 1 (every point beyond the first d + 1 verifies)
                                tt = S - d - 1 if form.startswith("sel") else t
                                queries.append((form, knobs, field, G, n, d, tt, S, FACTS[i % len(FACTS)]))
    got = plan(queries)
    for q, line in got.items():
        form, knobs, field, G, n, d, t, S, facts = q
        kn = knobs.split(",")
        needed = d + t + 1
        fg = "generic" in kn
        direct_fail = "single0" not in kn
        wide_max = 0 if "small0" in kn else 8192
        grouped = "_group" in form
        if grouped:                                         # the grouped form: covered exactly under this condition
            g = int(form.split("_group")[1])
            covered = G % g == 0 and S == needed and direct_fail and G <= wide_max and not fg
            assert (line != "notfused-early") == covered, (q, line)
        if line in ("notfused-early", "notfused", "single-invalid"):
            continue
        head, all_ = line.split(" all=")
        routes = all_.split(",") if all_ else []
        fields = dict(kv.split("=") for kv in head.split()[1:] if "=" in kv)
        first = head.split()[0]
        general = not form.startswith(("sel", "pair"))
        if general:                                         # a covered general-form plan ends in a route that cannot decline
            assert routes and routes[-1] in ("Generic", "Wide"), (q, line)
        if fg:
            assert first == "Generic", (q, line)
        if "mc0" in kn:
            assert not any(r.startswith("Mfma") for r in routes), (q, line)
        if field == "sat32":
            assert not any(r.startswith("Mfma") or r == "RecoverM" for r in routes), (q, line)
        if field != "gl":
            assert "MfmaRowsGl" not in routes and "GoldRecoverM" not in routes, (q, line)
        if not routes:                                      # runs out: HBMPC_NOT_FUSED after the tables (pair, select-two)
            assert not general, (q, line)
            continue
        rmax = int(fields["rmax"])
        assert rmax == (min(t, S - needed) if S > needed else 0), (q, line)
        one = head.split()[4] == "one"
        two_role = first in ("MfmaRows", "MfmaRowsTeam") and int(fields["roles"]) > 1
        assert one == (rmax == 0 and direct_fail and not two_role), (q, line)
        second = fields["second"]
        assert (second != "none") == (rmax > 0 and "second0" not in kn), (q, line)
        lazy_policy = "lazy2" in kn or ("lazy0" not in kn and form in ("host", "p0_host"))
        lazy = fields["tables"] == "lazy"
        assert lazy == (lazy_policy and facts not in ("capturing", "cached") and rmax > 0), (q, line)
        if lazy:
            assert second in ("none", "m", "generic"), (q, line)   # never inside the first kernel: its tables do not exist yet
        if form.startswith("pair"):
            assert routes == ["MfmaRowsSub"] and one, (q, line)
        if form.startswith("sel"):
            assert set(routes) <= {"MfmaRows", "MfmaRowsTeam", "Wide"}, (q, line)


def test_cover_answers(plan):
    """where each form answers: the grouped form before the senders are validated, select-two and the pair form after them with
    HBMPC_NOT_FUSED, a single coefficient of a call with OEC rounds with its InvalidInput message"""
    got = plan([
        ("top5_group1000", "default", "fr", 1024, 16, 5, 5, 11, "-"),   # G not a multiple of the group
        ("top5_group1024", "small0", "fr", 2048, 16, 5, 5, 11, "-"),    # beyond the wave-per-chunk range
        ("sel0_5", "default", "gl", 1000, 16, 5, 5, 11, "-"),           # select-two over Goldilocks
        ("sel0_5", "mc0", "fr", 8193, 16, 5, 5, 11, "-"),               # beyond the wave-per-chunk range without matrix cores
        ("coeff5", "default", "fr", 1000, 16, 5, 5, 12, "-"),           # one coefficient with an OEC round
        ("pair4096", "default", "fr", 8192, 16, 11, 1, 13, "-"),        # m = 12: no SUB instance
        ("pair4100", "default", "fr", 8200, 16, 5, 5, 11, "-"),         # N not a multiple of 32
        ("pair4096", "default", "fr", 8192, 16, 5, 5, 11, "-"),
        ("pair512", "default", "fr", 1024, 16, 5, 5, 11, "-"),          # below the one-launch threshold: runs out
    ])
    assert list(got.values())[:7] == ["notfused-early", "notfused-early", "notfused", "notfused", "single-invalid", "notfused", "notfused"]
    assert list(got.values())[7].startswith("MfmaRowsSub M=6 rows=6 roles=1 one")
    assert list(got.values())[8].startswith("none rmax=0 all=")
