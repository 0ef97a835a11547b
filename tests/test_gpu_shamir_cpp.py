"""Runs tests/cpp/test_shamir_units: the reference's Shamirshare unit tests (common/share/shamir.rs:250-326) restated over `Shamirshare`
of include/hbmpc_shares.hpp at the reference's own points, both fields, and the plain C99 caller of the integer-point host calls
(tests/cpp/test_shamir_abi.c)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "test_shamir_units")


def test_shamir_units_build():
    # host-only compile (the caller as strict C99) + link against the in-tree library: no GPU needed
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "cpp"), "-f", "shamir_units.mk"], stdout=subprocess.DEVNULL)
    assert os.path.exists(BIN)


@pytest.mark.gpu
def test_shamir_units_run():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "cpp"), "-f", "shamir_units.mk"], stdout=subprocess.DEVNULL)
    p = subprocess.run([BIN], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-2000:]
    assert "C99 Shamir calls passed" in p.stdout and "all Shamirshare unit tests passed" in p.stdout
