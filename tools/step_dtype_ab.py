"""Training-step time by 16-bit dtype: the bf16 Trainer, the f16 Trainer with a dynamic loss
scale, and the reference's fp16 autocast + torch GradScaler + torch.optim.AdamW loop.

Swin-T MS-UNet at 1024^2, batch 8, eager.  Every arm keeps its own model (same initial weights)
and is timed in alternating rounds inside one process: per round and arm ``--warmup`` untimed
steps, then ``--steps`` steps between two device events.  Arms:

* ``bf16``  -- ``Trainer(...)`` as bench.py runs it;
* ``f16``   -- ``Trainer(amp_dtype=torch.float16, loss_scale="dynamic")``;
* ``ref16`` -- trainer.py:299-316 of the reference on these modules (``scaler.scale(loss)
  .backward()``, ``scaler.step``, ``scaler.update``), without its ``loss.item()``: the only host
  sync left in the loop is GradScaler's own.

Gate (exit status 1 when missed): f16's mean step is shorter than ref16's by more than ref16's
spread (max - min of its round means).  f16 against bf16 is reported, not gated.

    python tools/step_dtype_ab.py [--arms bf16,f16,ref16] [--rounds 3] [--steps 15] [--warmup 5] [--out FILE]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from semantic_segmentation_of_stylegan2_artifacts_amd import load_config  # noqa: E402
from semantic_segmentation_of_stylegan2_artifacts_amd.data import batch_pool  # noqa: E402
from semantic_segmentation_of_stylegan2_artifacts_amd.loss import DynamicLoss  # noqa: E402
from semantic_segmentation_of_stylegan2_artifacts_amd.network import MSUNet  # noqa: E402
from semantic_segmentation_of_stylegan2_artifacts_amd.trainer import Trainer, is_no_decay  # noqa: E402

DEV = "cuda"


def make_arm(name, cfg, state, img):
    """step(images, labels) of one arm, on a model of its own."""
    model = MSUNet(cfg, img_size=img, num_classes=1)
    model.load_state_dict(state, strict=True)
    model = model.to(DEV).train()
    if name == "bf16":
        return Trainer(model, cfg, DEV, seed=cfg.SEED, use_graph=False).step
    if name == "f16":
        return Trainer(model, cfg, DEV, seed=cfg.SEED, use_graph=False, amp_dtype=torch.float16,
                       loss_scale="dynamic").step
    if name != "ref16":
        raise SystemExit(f"unknown arm {name!r}")
    t = cfg.TRAIN
    decay = [p for n, p in model.named_parameters() if p.requires_grad and not is_no_decay(n, p)]
    no_decay = [p for n, p in model.named_parameters() if p.requires_grad and is_no_decay(n, p)]
    opt = torch.optim.AdamW([{"params": decay, "weight_decay": t.WEIGHT_DECAY},
                             {"params": no_decay, "weight_decay": 0.0}], lr=t.BASE_LR,
                            betas=tuple(t.OPTIMIZER.BETAS), eps=float(t.OPTIMIZER.EPS), amsgrad=False)
    scaler = torch.amp.GradScaler("cuda")
    loss_fn = DynamicLoss(alpha=t.TVERSKY_LOSS_ALPHA, beta=t.TVERSKY_LOSS_BETA, tversky_bce_mix=t.LOSS_TVERSKY_BCE_MIX)

    def step(images, labels):
        with torch.amp.autocast("cuda", dtype=torch.float16):
            loss = loss_fn(model(images), labels)
            opt.zero_grad(set_to_none=True)
            scaler.scale(loss).backward()
            scaler.step(opt)
            scaler.update()
        return loss.detach()

    return step


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--arms", default="bf16,f16,ref16")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--img", type=int, default=1024)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--out", default=None, help="also append the report to this file")
    a = ap.parse_args()
    arms = [s for s in a.arms.split(",") if s]
    cfg = load_config(None, "swin_t", **{"DATA.IMG_SIZE": a.img, "DATA.BATCH_SIZE": a.batch})
    torch.manual_seed(cfg.SEED)
    state = MSUNet(cfg, img_size=a.img, num_classes=1).state_dict()
    pool = batch_pool(2, a.batch, a.img, DEV, cfg.SEED + 1000)
    steps = {name: make_arm(name, cfg, state, a.img) for name in arms}
    ms = {name: [] for name in arms}
    last = {}
    for r in range(a.rounds):
        for name in (arms if r % 2 == 0 else arms[::-1]):
            for i in range(a.warmup):
                steps[name](*pool[i % 2])
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for i in range(a.steps):
                last[name] = steps[name](*pool[i % 2])
            e1.record()
            torch.cuda.synchronize()
            ms[name].append(e0.elapsed_time(e1) / a.steps)
    rep = {"img": a.img, "batch": a.batch, "rounds": a.rounds, "steps": a.steps, "warmup": a.warmup, "arms": {}}
    lines = [f"step_dtype_ab: Swin-T {a.img}^2 batch {a.batch}, eager, {a.rounds} rounds x ({a.warmup} warmup + "
             f"{a.steps} timed steps), ms per step",
             f"{'arm':6s} {'rounds':>30s} {'mean':>8s} {'spread':>8s} {'img/s':>8s}  last loss"]
    for name in arms:
        v = ms[name]
        mean, spread = sum(v) / len(v), max(v) - min(v)
        rep["arms"][name] = {"ms": [round(x, 3) for x in v], "mean_ms": round(mean, 3), "spread_ms": round(spread, 3),
                             "last_loss": float(last[name])}
        lines.append(f"{name:6s} {' '.join(f'{x:9.3f}' for x in v):>30s} {mean:8.3f} {spread:8.3f} "
                     f"{a.batch * 1e3 / mean:8.1f}  {float(last[name]):.5f}")
    ok = True
    A = rep["arms"]
    if "f16" in A and "ref16" in A:
        gain = A["ref16"]["mean_ms"] - A["f16"]["mean_ms"]
        ok = gain > A["ref16"]["spread_ms"]
        rep["gate"] = {"ref16_minus_f16_ms": round(gain, 3), "ref16_spread_ms": A["ref16"]["spread_ms"], "pass": ok}
        lines.append(f"gate: ref16 - f16 = {gain:.3f} ms against ref16's spread {A['ref16']['spread_ms']:.3f} ms: "
                     f"{'pass' if ok else 'FAIL'}")
    if "f16" in A and "bf16" in A:
        d = A["f16"]["mean_ms"] - A["bf16"]["mean_ms"]
        rep["f16_minus_bf16_ms"] = round(d, 3)
        lines.append(f"reported: f16 - bf16 = {d:+.3f} ms against bf16's spread {A['bf16']['spread_ms']:.3f} ms")
    lines.append(json.dumps(rep))
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(text + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
