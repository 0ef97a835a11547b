"""bench.py --dump-outputs and the lean plain run.  On CPU: the dump format itself (a seeded column sample of a [n][B] array of
256-bit elements, written as the exact u32 words in float64) and the command line.  On the GPU: a plain run writes the
shares its last timed step computed, they equal the oracle's compute_shares of the same seeded inputs, and the line holds
only the headline figures (--full adds the rest)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _env():
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    return env


def _limbs(words):
    """float64 [..][8] u32 words -> uint64 [..][4] limbs"""
    assert words.dtype == np.float64 and np.all(words == np.floor(words)) and words.min() >= 0 and words.max() < 2 ** 32
    return np.ascontiguousarray(words.astype(np.uint32)).view(np.uint64)


@pytest.mark.parametrize("B", [1000, bench.DUMP_COLUMNS, 3 * bench.DUMP_COLUMNS + 5])
def test_dump_columns_is_an_exact_seeded_sample(tmp_path, B):
    import torch
    n = 3
    g = torch.Generator().manual_seed(7)
    rows = torch.randint(-(1 << 62), 1 << 62, (n, B, 4), dtype=torch.int64, generator=g)
    bench.dump_columns(str(tmp_path / "a"), "shares", n, B, lambda p: rows[p])
    bench.dump_columns(str(tmp_path / "b"), "shares", n, B, lambda p: rows[p])
    words = np.load(tmp_path / "a" / "shares.npy")
    cols = np.load(tmp_path / "a" / "shares_columns.npy")
    S = min(B, bench.DUMP_COLUMNS)
    assert words.shape == (n, S, 8) and cols.shape == (S,) and cols.dtype == np.float64
    idx = cols.astype(np.int64)
    assert np.all(np.diff(idx) > 0) and idx[0] >= 0 and idx[-1] < B
    assert np.array_equal(_limbs(words), rows.numpy().view(np.uint64)[:, idx])
    # the same arguments give the same files
    for f in ("shares.npy", "shares_columns.npy"):
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f))


def test_dump_of_the_headline_shape_stays_under_64_mb():
    n = 16  # BASELINE configs[1]; one float64 [n][S][8] array and its [S] column indices
    assert n * bench.DUMP_COLUMNS * 8 * 8 + bench.DUMP_COLUMNS * 8 <= 64 * 2 ** 20


def test_command_line_has_full_and_dump_outputs():
    out = subprocess.run([sys.executable, BENCH, "--help"], capture_output=True, text=True, env=_env(), timeout=120)
    assert out.returncode == 0, out.stderr
    assert "--full" in out.stdout and "--dump-outputs" in out.stdout


@pytest.mark.gpu
def test_plain_run_dumps_the_shares_of_its_last_step(tmp_path):
    import torch
    from oracle import cref
    log2_batch, steps = 15, 3
    out = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", str(steps), "--warmup", "1", "--log2-batch", str(log2_batch),
                          "--prewarm-seconds", "0.05", "--dump-outputs", str(tmp_path)],
                         capture_output=True, text=True, env=_env(), timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    rec = json.loads(out.stdout.strip().splitlines()[-1])
    assert rec["steps"] == steps and rec["ms_per_step"] > 0 and rec["value"] > 0 and rec["unit"] == "shares/s"
    assert rec["higher_is_better"] is True and rec["dtype"] == "u32" and rec["metric"].startswith("shares/sec (compute_shares)")
    for k in ("recon", "cpu_baseline", "extra"):  # --full only
        assert k not in rec
    n, d, B = 16, 5, 1 << log2_batch
    words = np.load(tmp_path / "shares.npy")
    idx = np.load(tmp_path / "shares_columns.npy").astype(np.int64)
    assert words.shape == (n, min(B, bench.DUMP_COLUMNS), 8)
    # the benchmark's inputs, drawn again from the same seed on the same device
    dev = torch.device("cuda", 0)
    torch.manual_seed(0xC0FFEE01)
    coeffs = bench._rand_fr(torch, dev, B, d + 1).cpu().numpy().view(np.uint64)
    rc, want = cref.compute_shares(np.ascontiguousarray(coeffs[idx]), n, d)
    assert rc == 0 and np.array_equal(_limbs(words), want)
