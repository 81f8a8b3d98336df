"""A/B of the refine-conv launches at one width: the persistent kernel against the generic one
(msu_conv_mode bit 1) in the same process, at the bench shape 8 x 1024^2, bf16.
    python tools/conv_ab.py [C = 128] [rounds = 7] [reps = 5] [B = 8] [H = 1024]
Each round times `reps` back-to-back launches of every launch form with HIP events, first on one
route, then on the other, the order alternating from round to round; reported per form: median
and min-max of the per-launch time over the rounds for both routes, and the fraction of the bf16
MFMA peak at the median (2 * 9 * C^2 FLOP per output pixel).  The weight gradients are timed too.
At C = 96 bit 1 changes nothing: both columns are the persistent kernel."""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from semantic_segmentation_of_stylegan2_artifacts_amd import _lib, ops  # noqa: E402

PEAK = 2500.0  # TFLOP/s, MI355X dense bf16 (as bench.py)
arg = lambda i, d: int(sys.argv[i]) if len(sys.argv) > i else d  # noqa: E731
C, ROUNDS, REPS, B, H = arg(1, 128), arg(2, 7), arg(3, 5), arg(4, 8), arg(5, 1024)
dt = torch.bfloat16
g = torch.Generator(device="cuda").manual_seed(5)
rnd = lambda *s: torch.randn(*s, device="cuda", generator=g).to(dt)  # noqa: E731
x1 = rnd(B, H // 4, H // 4, 16 * C)   # refine1's pre-activation (pre-d2s layout)
a1 = torch.nn.functional.gelu(x1)
z1, a2 = torch.empty(B, H, H, C, device="cuda", dtype=dt), torch.empty(B, H, H, C, device="cuda", dtype=dt)
z2 = torch.empty_like(z1)
dz = rnd(B, H, H, C)
dx1, dx2 = torch.empty_like(x1), torch.empty_like(z1)
w = torch.randn(C, C, 3, 3, device="cuda", generator=g) / (9 * C) ** 0.5
b = torch.zeros(C, device="cuda")
wt, wf = ops._conv_weight(w, dt, 0), ops._conv_weight(w, dt, 1)
L = _lib.lib()
s = torch.cuda.current_stream().cuda_stream
p = lambda t: t.data_ptr()  # noqa: E731
D = 1  # MSU_BF16


def wgrad(a, mode):
    ops._conv_wgrad(a, dz, mode, B, H, H, C, C)


FORMS = [
    ("refine1 fwd (d2s, bias, dual)", lambda: _lib.call("msu_conv3x3_fwd2", D, 2, p(a1), p(wt), p(b), p(z1), p(a2), B, H, H, C, C, s)),
    ("refine2 fwd (bias)", lambda: _lib.call("msu_conv3x3_fwd2", D, 0, p(a2), p(wt), p(b), p(z2), None, B, H, H, C, C, s)),
    ("refine2 dgrad (GELU')", lambda: _lib.call("msu_conv3x3_dgrad", D, 1, p(dz), p(wf), p(z1), p(dx2), B, H, H, C, C, s)),
    ("refine1 dgrad (d2s, GELU')", lambda: _lib.call("msu_conv3x3_dgrad", D, 3, p(dz), p(wf), p(x1), p(dx1), B, H, H, C, C, s)),
    ("refine1 wgrad (d2s)", lambda: wgrad(a1, 2)),
    ("refine2 wgrad", lambda: wgrad(a2, 0)),
]


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPS):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / REPS


base = L.msu_conv_mode(1) & 1
res = {name: {0: [], 2: []} for name, _ in FORMS}
try:
    for bit in (0, 2):  # warm-up of both routes (first launches set kernel attributes)
        L.msu_conv_mode(base | bit)
        for _, fn in FORMS:
            fn()
    torch.cuda.synchronize()
    for r in range(ROUNDS):
        for bit in ((0, 2) if r % 2 == 0 else (2, 0)):
            L.msu_conv_mode(base | bit)
            for name, fn in FORMS:
                res[name][bit].append(timed(fn))
finally:
    L.msu_conv_mode(base)

flop = 2.0 * 9 * C * C * B * H * H
print(f"C = {C}, {B} x {H}^2, bf16, route {L.msu_conv3x3_route(D, C, C)}; {ROUNDS} rounds x {REPS} launches, ms per launch")
print(f"{'launch':32s} {'persistent med (min-max)':>28s} {'peak':>6s}   {'generic med (min-max)':>28s} {'peak':>6s}  ratio")
for name, _ in FORMS:
    out = []
    for bit in (0, 2):
        t = res[name][bit]
        med = statistics.median(t)
        out.append((med, f"{med:8.3f} ({min(t):.3f}-{max(t):.3f})", f"{flop / (med * 1e-3) / 1e12 / PEAK:6.3f}"))
    print(f"{name:32s} {out[0][1]:>28s} {out[0][2]}   {out[1][1]:>28s} {out[1][2]}  {out[1][0] / out[0][0]:5.2f}x")
