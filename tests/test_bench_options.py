"""bench.py's plain / --full split and --dump-outputs: the options parse, the
dump holds the timed steps' losses in float32 (CPU), and one plain run of the
smallest config on the GPU prints the contract line without the --full figures
and writes the dump."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT


def _bench():
    import bench
    return bench


def test_full_and_dump_outputs_default_off(monkeypatch):
    bench = _bench()
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, None, 7, 2)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full and a.dump_outputs == "d"


def test_dump_outputs_writes_the_losses_in_step_order(tmp_path):
    bench = _bench()
    # a step's loss is valid for GraphStep.LOSS_RING later steps: no more are kept
    from gsplat_hip.graph_step import GraphStep
    assert bench.LOSS_KEEP <= GraphStep.LOSS_RING
    losses = [torch.tensor(0.5, dtype=torch.float64), torch.tensor(0.25), torch.tensor(0.125)]
    bench.dump_outputs(str(tmp_path / "d"), losses)
    x = np.load(tmp_path / "d" / "loss.npy")
    assert x.dtype == np.float32 and x.tolist() == [0.5, 0.25, 0.125]
    assert os.listdir(tmp_path / "d") == ["loss.npy"]


@pytest.mark.gpu
def test_plain_run_prints_the_contract_line_and_dumps(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config",
                        "m1", "--steps", "3", "--warmup", "1", "--dump-outputs", str(out)],
                       stdout=subprocess.PIPE, timeout=120)
    assert r.returncode == 0
    lines = r.stdout.decode().splitlines()
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["unit"] == "images/s"
    assert d["higher_is_better"] is True and d["dtype"] == "f32" and d["metric"]
    assert d["value"] > 0 and d["ms_per_step"] == pytest.approx(1e3 / d["value"])
    # a plain run measures nothing but its timed steps
    assert d["full"] is False and d["roofline"] is None and "cpu_baseline" not in d
    x = np.load(out / "loss.npy")
    # one loss per timed step, each 0.8 L1 + 0.2 (1 - SSIM) of images in [0, 1]
    assert x.dtype == np.float32 and x.shape == (3,) and np.all((x > 0) & (x < 1))
