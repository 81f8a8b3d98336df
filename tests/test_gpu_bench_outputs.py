"""GPU: a plain ``bench.py`` run is lean, and ``--dump-outputs`` shows what it computed.

One small run (256^2, bs 2, 1 warmup + 2 timed steps):

* the result line holds the headline fields and none of the ``--full`` legs;
* ``--steps`` is the number of timed steps the line reports;
* ``DIR/<name>.npy`` exist, are float32, finite and below 64 MB in all; the loss file equals
  the line's ``final_loss``, and the state files show that the steps ran (non-zero first
  moments and weights);
* the bench's input pool is a function of its arguments alone (same seed, same tensors), so two
  builds run with equal arguments see equal inputs.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("roofline", "roofline_attention", "roofline_decoder", "input_pipeline", "cpu_baseline", "dice_vs_ref")


def _run(out):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--img", "256", "--batch", "2",
           "--steps", "2", "--warmup", "1", "--dump-outputs", out]
    r = subprocess.run(cmd, env=env, cwd=REPO, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0]), {f[:-4]: np.load(os.path.join(out, f)) for f in sorted(os.listdir(out))}


def test_plain_run_is_lean_and_dumps_its_outputs(tmp_path):
    res, a = _run(str(tmp_path / "a"))
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in res, k
    assert res["steps"] == 2 and res["warmup"] == 1 and res["ms_per_step"] > 0
    assert abs(res["value"] - 2 * 1e3 / res["ms_per_step"]) <= 1e-2 * res["value"]
    assert not [k for k in FULL_ONLY if k in res]
    assert set(a) == {"loss", "params_decay", "params_no_decay", "exp_avg_decay", "exp_avg_no_decay"}
    assert sum(v.nbytes for v in a.values()) <= 64 * 1000 * 1000
    for name, v in a.items():
        assert v.dtype == np.float32 and v.ndim == 1 and v.size > 0, name
        assert np.isfinite(v).all(), name
    assert abs(float(a["loss"][0]) - res["config"]["final_loss"]) <= 1e-6
    assert a["exp_avg_decay"].any() and a["params_decay"].any()


def test_bench_inputs_depend_on_arguments_only():
    from semantic_segmentation_of_stylegan2_artifacts_amd.data import batch_pool
    a = batch_pool(2, 2, 256, torch.device("cuda", 0), 1234)
    b = batch_pool(2, 2, 256, torch.device("cuda", 0), 1234)
    assert len(a) == len(b) == 2
    for (xa, ya), (xb, yb) in zip(a, b):
        assert torch.equal(xa, xb) and torch.equal(ya, yb)
    assert not torch.equal(a[0][0], a[1][0])
