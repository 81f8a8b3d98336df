"""Cost of gradient accumulation (``Trainer(accum_steps=k)``): A/B on one GPU, arms alternating.

Two parts, each printing JSON lines (``--out FILE`` appends them to a file too):

* ``step``   -- the Swin-T 1024^2 bf16 eager Trainer.  Arm A: ``k`` plain steps of ``batch`` samples on
  ``Trainer(accum_steps=1)``, which is the step as it was before accumulation, launch for launch
  (tests/test_gpu_accum.py pins its loss entries).  Arm B: one window of ``k * batch`` samples on
  ``Trainer(accum_steps=k)``.  Two trainers in one process, warm-up first, then alternating rounds,
  device events around each round; ms per ``k * batch`` samples by round (median / min / max over
  rounds), so the two arms read in the same unit.  B drops ``k - 1`` of A's AdamW passes,
  non-finite checks and shadow refreshes.
* ``memory`` -- peak ``torch.cuda.max_memory_allocated`` over one plain step of ``batch`` (A) and over
  one window of ``k * batch`` (B), each after ``reset_peak_memory_stats`` with both trainers
  resident; ``resident_MB`` is what was allocated before the measured call.  The window's input
  buffers are k times the plain step's; its activations are one micro-batch's.

    python tools/accum_ab.py [--k 4] [--parts step,memory] [--rounds 8] [--steps 5] [--warmup 3] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from semantic_segmentation_of_stylegan2_artifacts_amd import load_config  # noqa: E402
from semantic_segmentation_of_stylegan2_artifacts_amd.data import batch_pool  # noqa: E402
from semantic_segmentation_of_stylegan2_artifacts_amd.network import MSUNet  # noqa: E402
from semantic_segmentation_of_stylegan2_artifacts_amd.trainer import Trainer  # noqa: E402

DEV = "cuda"
OUT = None


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if OUT:
        with open(OUT, "a") as f:
            f.write(line + "\n")


def make_trainers(img, batch, k):
    cfg = load_config(None, "swin_t", **{"DATA.IMG_SIZE": img, "DATA.BATCH_SIZE": batch})
    torch.manual_seed(cfg.SEED)
    state = MSUNet(cfg, img_size=img, num_classes=1).state_dict()
    out = {}
    for name, steps in ((f"A {k} plain steps of {batch}", 1), (f"B one window of {k * batch}, accum_steps={k}", k)):
        model = MSUNet(cfg, img_size=img, num_classes=1)
        model.load_state_dict(state, strict=True)
        out[name] = Trainer(model.to(DEV).train(), cfg, DEV, seed=cfg.SEED, use_graph=False, accum_steps=steps)
    return cfg, out


def make_inputs(cfg, img, batch, k):
    """Two windows of k * batch samples; arm A walks the same samples batch by batch."""
    pool = batch_pool(2 * k, batch, img, DEV, cfg.SEED + 1000)
    return [(torch.cat([pool[w * k + i][0] for i in range(k)]), torch.cat([pool[w * k + i][1] for i in range(k)]))
            for w in range(2)]


def run(tr, window, batch):
    """One window's worth of samples through a trainer: k plain steps, or one accumulated step."""
    x, y = window
    if tr.accum_steps == 1:
        for a in range(0, x.shape[0], batch):
            tr.step(x[a:a + batch], y[a:a + batch])
    else:
        tr.step(x, y)


def step_part(trainers, windows, img, batch, k, rounds, steps, warmup):
    names = list(trainers)
    for name in names:
        for i in range(warmup):
            run(trainers[name], windows[i % 2], batch)
    ms = {name: [] for name in names}
    for r in range(rounds):
        for name in (names if r % 2 == 0 else names[::-1]):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for i in range(steps):
                run(trainers[name], windows[i % 2], batch)
            e1.record()
            torch.cuda.synchronize()
            ms[name].append(e0.elapsed_time(e1) / steps)
    for name in names:
        v, tr = ms[name], trainers[name]
        emit({"what": "step", "workload": f"Swin-T {img}^2 bf16, {k * batch} samples", "arm": name, "execution": "eager",
              "rounds": rounds, "windows_per_round": steps, "median_ms": round(statistics.median(v), 4),
              "min_ms": round(min(v), 4), "max_ms": round(max(v), 4), "by_round_ms": [round(x, 3) for x in v],
              "applied": tr.optimizer_steps(), "skipped": tr.skipped_steps()})
    a, b = (ms[name] for name in names)
    emit({"what": "step_ratio", "k": k, "B_over_A_at_median": round(statistics.median(b) / statistics.median(a), 4),
          "B_minus_A_ms_at_median": round(statistics.median(b) - statistics.median(a), 3),
          "A_max_minus_min_ms": round(max(a) - min(a), 3)})


def memory_part(trainers, windows, batch, k):
    names = list(trainers)
    x, y = windows[0]
    calls = {names[0]: lambda: trainers[names[0]].step(x[:batch], y[:batch]),
             names[1]: lambda: trainers[names[1]].step(x, y)}
    peaks = {}
    for name in names:
        calls[name]()  # the allocator's pools are warm for this shape
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        resident = torch.cuda.memory_allocated()
        calls[name]()
        torch.cuda.synchronize()
        peaks[name] = torch.cuda.max_memory_allocated()
        emit({"what": "memory", "arm": name if name == names[1] else f"A one plain step of {batch}",
              "resident_MB": round(resident / 2 ** 20, 1), "peak_MB": round(peaks[name] / 2 ** 20, 1),
              "peak_minus_resident_MB": round((peaks[name] - resident) / 2 ** 20, 1)})
    emit({"what": "memory_diff", "k": k, "B_minus_A_peak_MB": round((peaks[names[1]] - peaks[names[0]]) / 2 ** 20, 1),
          "window_inputs_MB": round((x.numel() * x.element_size() + y.numel() * y.element_size()) / 2 ** 20, 1)})


def main():
    global OUT
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--parts", default="step,memory")
    ap.add_argument("--k", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--steps", type=int, default=5, help="windows per round")
    ap.add_argument("--warmup", type=int, default=3, help="warm-up windows per arm")
    ap.add_argument("--img", type=int, default=1024)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    OUT = a.out
    if OUT:
        os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    if not torch.cuda.is_available():
        raise SystemExit("accum_ab: needs a HIP device (timings are not taken on a CPU)")
    parts = [s for s in a.parts.split(",") if s]
    cfg, trainers = make_trainers(a.img, a.batch, a.k)
    windows = make_inputs(cfg, a.img, a.batch, a.k)
    if "step" in parts:
        step_part(trainers, windows, a.img, a.batch, a.k, a.rounds, a.steps, a.warmup)
    if "memory" in parts:
        memory_part(trainers, windows, a.batch, a.k)
    return 0


if __name__ == "__main__":
    sys.exit(main())
