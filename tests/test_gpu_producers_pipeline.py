"""tests/cpp/test_producers_pipeline (include/hbmpc_pipelines.hpp's ransha_parties / randousha_parties and DevBlock at n = 4, t = 1, three
columns, against the RanSha / RanDouSha handles from the same polynomials, in both forms of the device calls) in a child process."""
import os
import subprocess

import pytest

from __graft_entry__ import ROOT

pytestmark = pytest.mark.gpu


def test_cpp_wrappers():
    exe = os.path.join(ROOT, "tests", "cpp", "test_producers_pipeline")
    assert os.path.exists(exe), "built by make -C tests/cpp -f producers.mk (build())"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
