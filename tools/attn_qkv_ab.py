"""Standalone A/B of the fused stage-0 attention unit against the unfused three-launch sequence
(ops.linear -> window_attention -> ops.linear) of the same tree, at 8 x 256^2 tokens, shift 3, bf16:
the training forward (qkv, o and keep words written) and the no-grad forward.  HIP events around
`launches` back-to-back forwards, arms alternating round by round; median (min-max) ms per forward.
    python tools/attn_qkv_ab.py [C] [heads] [rounds] [launches] [p_drop]
MSU_LIB_OVERRIDE=<path> times another build of the library (tools/build_exp.sh)."""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from semantic_segmentation_of_stylegan2_artifacts_amd import ops  # noqa: E402

C = int(sys.argv[1]) if len(sys.argv) > 1 else 128
nh = int(sys.argv[2]) if len(sys.argv) > 2 else C // 32
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 7
launches = int(sys.argv[4]) if len(sys.argv) > 4 else 5
p_drop = float(sys.argv[5]) if len(sys.argv) > 5 else 0.05
B, R, shift = 8, 256, 3
torch.manual_seed(0)
x = (torch.randn(B, R, R, C, device="cuda") * 0.5).bfloat16()
w = torch.randn(3 * C, C, device="cuda") * 0.05
b = torch.randn(3 * C, device="cuda") * 0.05
tb = torch.randn(169, nh, device="cuda") * 0.02
wp = torch.randn(C, C, device="cuda") * 0.05
bp = torch.randn(C, device="cuda") * 0.05


def fused(store, p):
    return torch.ops.msunet.window_attention_qkv(x, w, b, tb, wp, bp, nh, shift, p, 7, None, store)[0]


def unfused(store, p):
    qkv = ops.linear(x, w, b)
    o = torch.ops.msunet.window_attention(qkv, b, tb, nh, shift, p, 7, None)[0]
    return ops.linear(o, wp, bp)


def timed(fn, *a):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        fn(*a)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / launches


with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
    assert ops.window_attention_qkv_fusable(x, nh, b), (C, nh)
    arms = {"train fused": (fused, True, p_drop), "train unfused": (unfused, True, p_drop),
            "nograd fused": (fused, False, 0.0), "nograd unfused": (unfused, False, 0.0)}
    for fn, *a in arms.values():  # warm up: shadows, workspaces, code objects
        for _ in range(3):
            fn(*a)
    torch.cuda.synchronize()
    times = {k: [] for k in arms}
    for _ in range(rounds):
        for k, (fn, *a) in arms.items():
            times[k].append(timed(fn, *a))
print(f"C={C} heads={nh} {B}x{R}^2 shift={shift} p={p_drop} bf16, {rounds} rounds x {launches} launches, ms per forward")
for k, v in times.items():
    print(f"{k:15s} median {statistics.median(v):.4f}  min {min(v):.4f}  max {max(v):.4f}")
