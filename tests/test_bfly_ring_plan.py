"""The ring encode's static schedule (csrc/bfly_ring_plan.hpp), simulated on the CPU by tests/cpp/bfly_ring_sim.cpp: one loader and
CW consumers per workgroup under four interleavings (round-robin, loader always first, loader always last, seeded random) over
G in {1, 31, 32, 33, the tile counts around CW, S and 2 S per workgroup, 2^20} with 8 and 256 workgroups.  The program asserts that
every wait is satisfied, every tile is consumed exactly once by its wave, no slot is refilled before it was read out or read before
it was published, and every source range lies inside the input.  It is built here, in one compiler call, with AddressSanitizer and
UBSan where the toolchain has their runtimes, and run directly."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "bfly_ring_sim.cpp")


def _compile(cxx, out, flags):
    return subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", *flags, SRC, "-o", out],
                          capture_output=True, text=True)


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no C++ compiler")
    out = str(tmp_path_factory.mktemp("bfly_ring") / "bfly_ring_sim")
    r = _compile(cxx, out, ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    sanitized = r.returncode == 0
    if not sanitized:  # no sanitizer runtimes in this toolchain: the plain build still checks every property
        r = _compile(cxx, out, [])
    assert r.returncode == 0, r.stderr
    return out, sanitized


def test_ring_schedule_simulation(sim):
    exe, sanitized = sim
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout, "(sanitized build)" if sanitized else "(plain build)")
    assert r.returncode == 0, r.stdout + r.stderr
    assert "every wait satisfied" in r.stdout
