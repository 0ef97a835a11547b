"""The integer-point Shamir encode without a GPU (tests/cpp/shamir_dump.cpp, built by tests/cpp/shamir.mk under ASan + UBSan):
  - the planner's route (mpc-protocols_amd/csrc/shamir_route.hpp) for a table of shapes, with the boundary id^d < 2^64 <= (id + 1)^d
    computed here for d = 1, 2, 5, 10;
  - the host-built interpolation table over arbitrary points (tables.hpp: point_coeff_rows) against the model's Lagrange basis;
  - the arithmetic of one output exactly as the kernel runs it (shamir_arith.hpp) against Python integers: the accumulator's maximum
    (every coefficient p - 1, every weight at the boundary value), zeros, a single top coefficient, d = 0 and 1 000 seeded random rows."""
import os
import random
import subprocess

import pytest

from tests import shamir_ref as M
from tests.shamir_ref import FR, GL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "shamir_dump")
U64 = 1 << 64
SMALL, WIDE, GENERIC = 1, 2, 3
MODS = {8: FR.R_MOD, 2: GL.R_MOD}


@pytest.fixture(scope="module")
def dump():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "cpp"), "-f", "shamir.mk"], stdout=subprocess.DEVNULL)

    def run(mode, lines=()):
        p = subprocess.run([BIN, mode], input="".join(l + "\n" for l in lines), capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stderr[-2000:]          # ASan / UBSan findings abort with a non-zero code
        return p.stdout.splitlines()
    return run


def boundary(d):
    """the largest id with id^d < 2^64"""
    x = int(round(U64 ** (1.0 / d)))
    while x ** d >= U64:
        x -= 1
    while (x + 1) ** d < U64:
        x += 1
    return x


def test_boundary_values():
    assert boundary(1) == U64 - 1 and boundary(2) == (1 << 32) - 1 and boundary(5) == 7131 and boundary(10) == 84
    for d in (1, 2, 5, 10):
        b = boundary(d)
        assert b ** d < U64 <= (b + 1) ** d


def rule(nl, forced, wide, m, d, B, pts):
    """the rule restated: small-weight when every pts[i]^d < 2^64 as integers, the weights fit the table and the rows the LDS; small
    batches (up to wide / 4 secrets) a wave per secret unless forced"""
    ru = (d + 1) * (nl // 2)
    su = ru + 2 if nl == 8 else ru | 1
    fits = all(x ** d < U64 for x in pts) and m * (d + 1) <= 1 << 16 and 64 * su * 8 <= 64 * 1024
    wide_size = B <= wide // 4
    if fits and forced != 2 and (forced == 1 or not wide_size):
        waves = min(4, 64 * 1024 // (64 * su * 8))
        return (SMALL, 1 if max(x ** d for x in pts) < 1 << 32 else 0, waves, waves * 64 * su * 8, su)
    return (WIDE if wide_size else GENERIC, 0, 0, 0, 0)


def test_routes(dump):
    big = 1 << 20
    shapes = []
    for nl in (8, 2):
        for d in (1, 2, 5, 10):
            b = boundary(d)
            for pts in ([b], [b + 1] if b + 1 < U64 else [b], [1, 2, b], [1, b + 1, 3] if b + 1 < U64 else [1, 2]):
                pts = pts + [x for x in range(4, 4 + d + 1) if x not in pts][: max(0, d + 1 - len(pts))]  # d + 1 points, the others small
                for forced in (0, 1, 2):
                    for B in (1, 2048, 2049, big):
                        shapes.append((nl, forced, 8192, len(pts), d, B, pts))
        # the 32-bit weight flag, the LDS bound per field, d = 0, the weights' table bound, small-batch knob off
        shapes += [(nl, 0, 8192, 16, 5, big, list(range(1, 17))), (nl, 0, 8192, 6, 5, big, [7, 1, 3, 20, 9, 84]), (nl, 0, 8192, 6, 5, big, [7, 1, 3, 20, 9, 85]),
                   (nl, 0, 8192, 1, 0, big, [U64 - 1]), (nl, 0, 0, 4, 1, 1, [1, 2, 3, 4]), (nl, 0, 8192, 31, 30, big, list(range(1, 32))),
                   (nl, 0, 8192, 32, 31, big, list(range(1, 33))), (nl, 0, 8192, 126, 125, big, list(range(1, 127))),
                   (nl, 0, 8192, 127, 126, big, list(range(1, 128))), (nl, 0, 8192, 2048, 31, big, list(range(1, 2049))),
                   (nl, 0, 8192, 2049, 31, big, list(range(1, 2050)))]
    p = GL.R_MOD  # Goldilocks ids at and beyond p: integers, not reduced
    shapes += [(2, 0, 8192, 2, 1, big, [1, p + 1]), (2, 0, 8192, 3, 2, big, [1, p + 1, 2]), (2, 0, 8192, 2, 1, big, [U64 - 1, 2])]
    lines = ["%d %d %d %d %d %d %s" % (nl, f, w, m, d, B, " ".join(map(str, pts))) for nl, f, w, m, d, B, pts in shapes]
    got = dump("route", lines)
    assert len(got) == len(shapes)
    for sh, line in zip(shapes, got):
        assert tuple(int(x) for x in line.split()) == rule(*sh), (sh[:6], sh[6][:4], line)


def test_route_anchors(dump):
    """derived by hand from the rule: either side of the boundary at d = 5 (7131^5 < 2^64 <= 7132^5), the size split at 2048 secrets"""
    q = ["8 0 8192 6 5 1048576 1 2 3 4 5 7131", "8 0 8192 6 5 1048576 1 2 3 4 5 7132", "8 0 8192 6 5 2048 1 2 3 4 5 6", "8 0 8192 6 5 2049 1 2 3 4 5 6",
         "8 1 8192 6 5 1 1 2 3 4 5 6", "8 2 8192 6 5 1048576 1 2 3 4 5 6", "2 0 8192 16 5 1048576 " + " ".join(map(str, range(1, 17)))]
    got = [l.split()[0] for l in dump("route", q)]
    assert got == ["1", "3", "2", "1", "1", "3", "1"]
    # 16^5 = 2^20: one 32-bit chain per term; Fr rows of 26 units -> 13 KiB a wave, four waves; Goldilocks rows of 7 units
    assert dump("route", q[-1:])[0] == "1 1 4 14336 7"
    assert dump("route", ["8 0 8192 16 5 1048576 " + " ".join(map(str, range(1, 17)))])[0] == "1 1 4 53248 26"


def test_constants(dump):
    want = {8: FR.R_MOD, 2: GL.R_MOD}
    for line in dump("consts"):
        nl, p, mu = line.split()
        nl = int(nl)
        assert int(p, 16) == want[nl] and int(mu, 16) == (1 << (32 * (nl + 3))) // want[nl]


@pytest.mark.parametrize("spec,name", [(FR, "fr"), (GL, "gl")])
def test_interpolation_table(dump, spec, name):
    sets = [[1, 2, 3, 4, 5, 6], [7, 1, 3, 20], [(1 << 32) + 5, 1, 2]] + ([[GL.R_MOD + 1, 2]] if spec is GL else [])
    out = dump("table", ["%s %s" % (name, " ".join(map(str, s))) for s in sets])
    pos = 0
    for s in sets:
        want = M.lagrange_basis(spec, s)
        for i in range(len(s)):
            assert [int(x, 16) for x in out[pos].split()] == want[i], (s, i)
            pos += 1
    assert pos == len(out)


def arith_line(nl, w32, coeffs, weights):
    return "%d %d %d %s %s" % (nl, w32, len(coeffs), " ".join("%x" % c for c in coeffs), " ".join("%x" % w for w in weights))


def arith_cases(nl):
    p = MODS[nl]
    rng = random.Random(0x5A17 + nl)
    cases = []
    for d in (0, 1, 2, 5, 10, 30):
        top = [boundary(k) ** k if k else 1 for k in range(d + 1)]           # each weight the largest power below 2^64
        cases.append(([p - 1] * (d + 1), [U64 - 1] * (d + 1), 0))              # the accumulator's maximum
        cases.append(([p - 1] * (d + 1), top, 0))                              # ... at the route's boundary weights
        cases.append(([p - 1] * (d + 1), [(1 << 32) - 1] * (d + 1), 1))        # the 32-bit form's maximum
        cases.append(([0] * (d + 1), top, 0))
        cases.append(([0] * d + [p - 1], top, 0))                              # a single non-zero top coefficient
        cases.append(([0] * d + [1], [1] * (d + 1), 1))
        cases.append(([p - 1] * (d + 1), [1] * (d + 1), 1))
    cases.append(([p - 1] * 4096, [U64 - 1] * 4096, 0))                        # many terms: the top limbs of the accumulator
    for _ in range(1000):
        d = rng.randrange(0, 12)
        w32 = rng.randrange(2)
        cases.append(([rng.randrange(p) for _ in range(d + 1)], [rng.randrange(1 << 32 if w32 else U64) for _ in range(d + 1)], w32))
    for x in (1, 2, 7131, 84):                                                 # weights as the encode forms them: powers of a point
        cases.append(([rng.randrange(p) for _ in range(6)], [x ** k for k in range(6)], 0))
    return cases


@pytest.mark.parametrize("nl", [8, 2])
def test_arithmetic_header(dump, nl):
    p = MODS[nl]
    cases = arith_cases(nl)
    got = dump("arith", [arith_line(nl, w32, c, w) for c, w, w32 in cases])
    assert len(got) == len(cases)
    for (c, w, w32), line in zip(cases, got):
        assert int(line, 16) == sum(a * b for a, b in zip(c, w)) % p, (nl, w32, len(c), c[:2], w[:2])
