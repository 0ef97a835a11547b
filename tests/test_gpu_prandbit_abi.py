"""The PRandBit / PRandInt entry points from a plain C99 caller (tests/cpp/test_prandbit_abi.c, built by tests/cpp/prandbit.mk)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "test_prandbit_abi")
PBIN = os.path.join(ROOT, "tests", "cpp", "test_prandbit_pipeline")


def test_prandbit_caller_builds():
    # host-only compile + link against the in-tree library (no GPU needed)
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "cpp"), "-f", "prandbit.mk"], stdout=subprocess.DEVNULL)
    assert os.path.exists(BIN) and os.path.exists(PBIN)


@pytest.mark.gpu
def test_prandbit_c99_caller():
    if not os.path.exists(BIN):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "cpp"), "-f", "prandbit.mk"], stdout=subprocess.DEVNULL)
    p = subprocess.run([BIN], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "PRandBit C ABI calls passed" in p.stdout, p.stdout[-2000:] + p.stderr[-2000:]


@pytest.mark.gpu
def test_prandbit_cpp_compositions():
    if not os.path.exists(PBIN):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "cpp"), "-f", "prandbit.mk"], stdout=subprocess.DEVNULL)
    p = subprocess.run([PBIN], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "PRandBit pipelines passed" in p.stdout, p.stdout[-2000:] + p.stderr[-2000:]
