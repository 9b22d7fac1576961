"""bench.py --dump-outputs: the array written for a result is the result itself when it fits the size limit and
otherwise a fixed sample of its trajectories (first, last, a seeded draw, ascending), the same rows in every run,
so that two builds can be compared array for array.  The helper is checked on host tensors; one GPU test runs
the plain benchmark command itself at a small batch."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def test_small_result_is_written_whole(tmp_path):
    x = torch.arange(7 * 5, dtype=torch.float64).reshape(7, 5)
    info = bench.dump_outputs(str(tmp_path / "d"), "du", x, max_bytes=7 * 5 * 8)
    a = np.load(tmp_path / "d" / "du.npy")
    assert a.dtype == np.float64 and np.array_equal(a, x.numpy())
    assert info["shape"] == [7, 5] and info["sample"] == "whole"


def test_large_result_is_a_fixed_ascending_sample_within_the_limit(tmp_path):
    B, n, rows = 1001, 3, 64
    x = torch.arange(B, dtype=torch.float64)[:, None] + torch.tensor([0.0, 0.25, 0.5], dtype=torch.float64)
    bench.dump_outputs(str(tmp_path / "a"), "du", x, max_bytes=rows * n * 8 + 5)    # (not a whole number of rows)
    bench.dump_outputs(str(tmp_path / "b"), "du", x.clone(), max_bytes=rows * n * 8 + 5)
    a, b = np.load(tmp_path / "a" / "du.npy"), np.load(tmp_path / "b" / "du.npy")
    assert a.shape == (rows, n) and a.nbytes <= rows * n * 8 + 5
    assert np.array_equal(a, b)
    idx = a[:, 0].astype(int)                      # row i of x starts with the value i
    assert idx[0] == 0 and idx[-1] == B - 1 and np.all(np.diff(idx) > 0)
    assert np.array_equal(a, x.numpy()[idx])


def test_limit_is_below_64_mb_over_all_ranks():
    assert bench.DUMP_MAX_BYTES <= 64 * 10 ** 6


@pytest.mark.gpu
def test_plain_run_is_the_headline_alone_and_dumps_the_last_step(tmp_path):
    """`bench.py --gpus 1 --steps N --warmup W --dump-outputs DIR` as a command (what every later measurement runs):
    one JSON line with the headline fields and none of the --full legs, and DIR/du.npy = the RHS of the run's seeded
    inputs at the parameters of its last timed step, within the fp64 parity tolerance of the
    oracle."""
    import json
    import subprocess

    from gpu_util import RTOL, assert_close, device, fk_scale
    from oracle import oracle as O

    import kanode

    B, N, W, nx, D = 4096, 3, 2, 256, 0.01
    dx = 1.0 / (nx - 1)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(N), "--warmup",
                        str(W), "--batch-total", str(B), "--dump-outputs", str(tmp_path / "out")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["metric"] == bench.METRIC and d["unit"] == "RHS-evals/s" and d["higher_is_better"] is True
    assert d["dtype"] == "f64" and d["steps"] == N and d["warmup"] == W and d["full"] is False
    assert d["ms_per_step"] > 0 and abs(d["value"] - B / (d["ms_per_step"] * 1e-3)) <= 1e-9 * d["value"]
    for leg in ("vjp", "cpu_baseline", "epoch", "epoch_adaptive", "lv4096", "lv1_train", "lv4096_train", "fk26_train",
                "surrogates"):
        assert leg not in d, leg
    assert d["shard_ceiling"] is None and d["roofline"]["torch_copy_GBps"] is None
    assert os.listdir(tmp_path / "out") == ["du.npy"]
    du = np.load(tmp_path / "out" / "du.npy")
    assert du.dtype == np.float64 and du.shape == (B, nx)
    # the run's inputs: fk_ics(seed 1000 + rank) evaluated on the device as the run does, Chain.setup(seed 0), and
    # the last timed step's parameter vector of the alternating pair
    u = bench.fk_ics(B, nx, dx, seed=1000, device=device()).cpu().numpy()
    kan1 = kanode.Chain(kanode.KDense(1, 1, 10, normalizer="softsign", basis_func="rbf"))
    p = kan1.setup(np.random.default_rng(0))[0].astype(np.float64)
    if (W + N - 1) & 1:
        p = p * (1.0 + 2.0 ** -40)
    ref = O.fk_rhs(O.LayerSpec(1, 1, 10, "softsign"), p, D, dx, u)
    assert_close(du, ref, fk_scale(p, D, dx, u), RTOL[torch.float64], "dumped du")
