"""tests/cpp/test_batchrecon_pipeline (include/hbmpc_pipelines.hpp's BatchRecon at n = 4, t = 1, d = 1, three chunks: run(), deal() +
finish() and a replayed graph, in both forms of the device call) in a child process."""
import os
import subprocess

import pytest

from __graft_entry__ import ROOT

pytestmark = pytest.mark.gpu


def test_cpp_wrapper():
    exe = os.path.join(ROOT, "tests", "cpp", "test_batchrecon_pipeline")
    assert os.path.exists(exe), "built by make -C tests/cpp -f batchrecon.mk (build())"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
