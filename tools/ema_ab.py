"""Cost of the weight EMA (``Trainer(ema_decay=...)``): A/B on one GPU, arms alternating.

Three parts, each printing JSON lines (``--out FILE`` appends them to a file too):

* ``kernel`` -- ``msu_adamw_dev2`` (A) against ``msu_adamw_dev3`` (B) on flat buffers of the Swin-T
  Trainer's two group sizes (bf16 shadow, ``zero_grad=1``, randn contents), one launch per event
  pair, the arms alternating launch by launch.  The bytes each moves per element (A: p, g, m, v
  read, p, m, v, g written, a 2-byte shadow = 34; B: + ema read and written = 42) over the median
  time give the achieved GB/s; the byte ratio is what B should cost over A.
* ``step``   -- the Swin-T 1024^2 bs 8 bf16 Trainer with ``ema_decay=None`` (A) and ``0.999`` (B),
  two trainers in one process, warm-up first, then alternating rounds of timed steps; ms per step
  by round (median / min / max over rounds).
* ``scope``  -- one ``ema_scope()`` entry plus exit on trainer B, timed with device events.

    python tools/ema_ab.py [--parts kernel,step,scope] [--rounds 8] [--steps 20] [--warmup 10] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from semantic_segmentation_of_stylegan2_artifacts_amd import _lib, load_config, ops  # noqa: E402
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


def pct(v, q):
    v = sorted(v)
    return v[min(len(v) - 1, int(q * len(v)))]


def kernel_part(sizes, warm=20, timed=300):
    for label, n in sizes:
        p, g, m, ema = (torch.randn(n, device=DEV) for _ in range(4))
        v = torch.rand(n, device=DEV)
        shadow = torch.empty(n, device=DEV, dtype=torch.bfloat16)
        hyper = torch.tensor([1e-5, 1.0], device=DEV, dtype=torch.float64)
        found = torch.zeros(1, device=DEV)
        st = ops._s(p)
        common = (hyper.data_ptr(), 0.9, 0.999, 1e-8, 0.05)

        def a():
            _lib.call("msu_adamw_dev2", p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, *common, None,
                      found.data_ptr(), shadow.data_ptr(), 1, 1, st)

        def b():
            _lib.call("msu_adamw_dev3", p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), ema.data_ptr(), n,
                      *common, 0.999, None, found.data_ptr(), shadow.data_ptr(), 1, 1, st)

        arms = (("A msu_adamw_dev2", a, 34), ("B msu_adamw_dev3", b, 42))
        us = {name: [] for name, _, _ in arms}
        for i in range(warm + timed):
            for name, fn, _ in (arms if i % 2 == 0 else arms[::-1]):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                if i >= warm:
                    us[name].append(e0.elapsed_time(e1) * 1e3)
        for name, _, bytes_per in arms:
            t = us[name]
            med = statistics.median(t)
            emit({"what": "kernel", "group": label, "elements": n, "arm": name, "bytes_per_element": bytes_per,
                  "MB": round(n * bytes_per / 1e6, 2), "n": len(t), "median_us": round(med, 2),
                  "p10_us": round(pct(t, 0.1), 2), "p90_us": round(pct(t, 0.9), 2), "min_us": round(min(t), 2),
                  "GB_per_s_at_median": round(n * bytes_per / med / 1e3, 1)})
        ma, mb = (statistics.median(us[name]) for name, _, _ in arms)
        emit({"what": "kernel_ratio", "group": label, "B_over_A_at_median": round(mb / ma, 4), "byte_ratio": round(42 / 34, 4),
              "A_p90_minus_p10_us": round(pct(us[arms[0][0]], 0.9) - pct(us[arms[0][0]], 0.1), 2),
              "B_minus_A_times_byte_ratio_us": round(mb - ma * 42 / 34, 2)})
        torch.cuda.synchronize()
        assert found.item() == 0.0 and torch.isfinite(ema).all() and torch.isfinite(p).all()


def make_trainers(img, batch):
    cfg = load_config(None, "swin_t", **{"DATA.IMG_SIZE": img, "DATA.BATCH_SIZE": batch})
    torch.manual_seed(cfg.SEED)
    state = MSUNet(cfg, img_size=img, num_classes=1).state_dict()
    out = {}
    for name, decay in (("A ema_decay=None", None), ("B ema_decay=0.999", 0.999)):
        model = MSUNet(cfg, img_size=img, num_classes=1)
        model.load_state_dict(state, strict=True)
        out[name] = Trainer(model.to(DEV).train(), cfg, DEV, seed=cfg.SEED, use_graph=False, ema_decay=decay)
    return cfg, out


def step_part(cfg, trainers, img, batch, rounds, steps, warmup):
    pool = batch_pool(2, batch, img, DEV, cfg.SEED + 1000)
    names = list(trainers)
    for name in names:
        for i in range(warmup):
            trainers[name].step(*pool[i % 2])
    ms = {name: [] for name in names}
    for r in range(rounds):
        for name in (names if r % 2 == 0 else names[::-1]):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for i in range(steps):
                trainers[name].step(*pool[i % 2])
            e1.record()
            torch.cuda.synchronize()
            ms[name].append(e0.elapsed_time(e1) / steps)
    for name in names:
        v, tr = ms[name], trainers[name]
        emit({"what": "step", "workload": f"Swin-T {img}^2 bs {batch} bf16", "arm": name, "execution": "eager",
              "rounds": rounds, "steps_per_round": steps, "median_ms": round(statistics.median(v), 4),
              "min_ms": round(min(v), 4), "max_ms": round(max(v), 4), "by_round_ms": [round(x, 3) for x in v],
              "applied": tr.optimizer_steps(),
              "ema_minus_weights_max": None if tr.ema_decay is None else
              max(float((g.ema - g.data).abs().max()) for g in tr.groups)})


def scope_part(tr, reps=20):
    ms = []
    for i in range(3 + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        with tr.ema_scope():
            pass
        e1.record()
        e1.synchronize()
        if i >= 3:
            ms.append(e0.elapsed_time(e1))
    n = sum(g.numel for g in tr.groups)
    emit({"what": "scope", "workload": "Swin-T bf16, ema_scope() entry + exit, empty body", "elements": n, "n": reps,
          "median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
          "launches": 2 * sum(1 + (g.tshadow is not None) for g in tr.groups)})


def main():
    global OUT
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--parts", default="kernel,step,scope")
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--img", type=int, default=1024)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    OUT = a.out
    if OUT:
        os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    if not torch.cuda.is_available():
        raise SystemExit("ema_ab: needs a HIP device (timings are not taken on a CPU)")
    parts = [s for s in a.parts.split(",") if s]
    cfg, trainers = make_trainers(a.img, a.batch)
    tb = trainers["B ema_decay=0.999"]
    if "kernel" in parts:
        kernel_part([("decay", tb.groups[0].numel), ("no_decay", tb.groups[1].numel)])
    if "step" in parts:
        step_part(cfg, trainers, a.img, a.batch, a.rounds, a.steps, a.warmup)
    if "scope" in parts:
        scope_part(tb)
    return 0


if __name__ == "__main__":
    sys.exit(main())
