"""bench.py command-line contract, exercised on the CPU path.

A plain run prints one JSON result line and nothing from the secondary
measurements; ``--dump-outputs DIR`` writes the last timed step's outputs
as float32 ``.npy`` files that repeat exactly from run to run (same
arguments -> same seeded weights and data, and the dumped step restarts
from the seeded state; CPU kernels are deterministic at a fixed thread
count).
"""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")


def _run_bench(tmp_path, name, *extra):
    env = dict(os.environ)
    # keep this a CPU test on GPU boxes too, with a fixed thread partition
    env["HIP_VISIBLE_DEVICES"] = ""
    env["CUDA_VISIBLE_DEVICES"] = ""
    env["OMP_NUM_THREADS"] = "4"
    out_dir = tmp_path / name
    r = subprocess.run(
        [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1",
         "--steps", "2", "--warmup", "1", "--dump-outputs", str(out_dir),
         *extra],
        capture_output=True, text=True, timeout=300, env=env,
        cwd=str(tmp_path),
    )
    assert r.returncode == 0, r.stderr
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0]), out_dir


@pytest.fixture(scope="module")
def two_runs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("bench")
    return _run_bench(tmp, "a"), _run_bench(tmp, "b")


class TestBenchCli:
    def test_plain_result_line(self, two_runs):
        (result, _), _ = two_runs
        assert result["metric"] == "samples_per_s"
        assert result["unit"] == "samples/s"
        assert result["higher_is_better"] is True
        assert result["dtype"] == "fp32"
        assert result["steps"] == 2 and result["warmup"] == 1
        assert result["ms_per_step"] > 0
        # value and ms_per_step describe the same timed steps
        assert result["value"] == pytest.approx(
            16 * 1000.0 / result["ms_per_step"], rel=1e-9
        )
        # the scheduler simulation belongs to --full
        assert "sim_makespan_h" not in result["config"]

    def test_dump_outputs_float32_and_bounded(self, two_runs):
        (_, out_dir), _ = two_runs
        names = sorted(os.listdir(out_dir))
        assert names == ["buffers.npy", "loss.npy", "params.npy"]
        total = 0
        for n in names:
            a = np.load(os.path.join(out_dir, n))
            assert a.dtype == np.float32
            assert np.isfinite(a).all()
            total += a.nbytes
        assert total <= 64 * 1000 * 1000
        assert np.load(os.path.join(out_dir, "loss.npy")).shape == (1,)
        from shockwave_amd.models import resnet18_cifar

        n_params = sum(p.numel() for p in resnet18_cifar().parameters())
        assert np.load(os.path.join(out_dir, "params.npy")).shape == (
            n_params,
        )

    def test_dump_is_one_step_from_seeded_state(self, two_runs):
        """The last timed step restarts from the seeded initial state, so
        its outputs equal one stock-SGD step on the batch at its position
        (warmup 1 + steps 2 -> third batch of the stream)."""
        import torch

        from shockwave_amd.data.synthetic import SyntheticImages
        from shockwave_amd.models import resnet18_cifar

        (_, out_dir), _ = two_runs
        torch.manual_seed(0)
        model = resnet18_cifar()
        opt = torch.optim.SGD(model.parameters(), lr=0.1, momentum=0.9,
                              weight_decay=5e-4)
        data = SyntheticImages(50000, image_size=32, num_classes=10, seed=0)
        x = torch.stack([data[i][0] for i in range(32, 48)])
        y = torch.stack([data[i][1] for i in range(32, 48)])
        model.train()
        loss = torch.nn.CrossEntropyLoss()(model(x), y)
        loss.backward()
        opt.step()
        want = torch.cat([p.detach().reshape(-1) for p in model.parameters()])
        got = np.load(os.path.join(out_dir, "params.npy"))
        # same CPU gradients; the fused update may order its fp32
        # arithmetic differently: a few ulp of weights of O(1)
        np.testing.assert_allclose(got, want.numpy(), rtol=0, atol=1e-6)
        np.testing.assert_allclose(
            np.load(os.path.join(out_dir, "loss.npy"))[0], loss.item(),
            rtol=1e-5,
        )

    def test_same_arguments_same_outputs(self, two_runs):
        (_, a_dir), (_, b_dir) = two_runs
        for n in ("loss.npy", "params.npy", "buffers.npy"):
            a = np.load(os.path.join(a_dir, n))
            b = np.load(os.path.join(b_dir, n))
            assert np.array_equal(a, b), n
