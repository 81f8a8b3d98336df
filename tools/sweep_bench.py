"""msu_seg_sweep at the workload's shape (8 x 1024^2 bf16 logits) against the only way to get
the same counts without it, K successive msu_seg_metrics calls on the same tensors, and against
one such call, in one process: device events around `iters` back-to-back launches on
preallocated buffers, `reps` alternating rounds, medians.
    python tools/sweep_bench.py [iters] [reps]
The inputs are a realistic mix: half the images all background (logits around -7: every pixel
below the lowest threshold), half with about 5 % confident foreground (+7 inside, -7 outside),
unit normal noise on every logit.  Prints one JSON line per K (99 and 1024): us per sweep, us per
K metrics calls, us per single metrics call, and the share of pixels in interior bins."""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from semantic_segmentation_of_stylegan2_artifacts_amd import _lib, ops, validation  # noqa: E402

iters = int(sys.argv[1]) if len(sys.argv) > 1 else 200
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
B, H, W = 8, 1024, 1024
N = H * W
dev = "cuda"


def timed(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / n  # us per call


g = torch.Generator(device=dev).manual_seed(0)
label = torch.zeros(B, H, W, device=dev)
for b in range(B // 2, B):  # a 230 x 230 square: 5.0 % of the image
    y0, x0 = 100 * b, 700 - 80 * b
    label[b, y0:y0 + 230, x0:x0 + 230] = 1.0
logits = ((label * 14.0 - 7.0) + torch.randn(B, H, W, device=dev, generator=g)).to(torch.bfloat16).view(B, 1, H, W)
L = _lib.lib()
nblk = L.msu_metrics_nblk(N)
part = torch.empty(B * nblk * 12, device=dev)
out = torch.empty(B, 12, device=dev, dtype=torch.float64)
st = ops._s(logits)
dt = ops._dt(logits)

for K in (99, 1024):
    ts = validation.default_thresholds(K)
    t32 = [float(v) for v in validation.check_thresholds(ts)]
    thr = torch.tensor(t32, dtype=torch.float32, device=dev)
    hist = torch.empty(B, 2, K + 1, device=dev, dtype=torch.int64)

    def sweep():
        _lib.call("msu_seg_sweep", dt, logits.data_ptr(), label.data_ptr(), B, N, thr.data_ptr(), K, hist.data_ptr(), st)

    def one():
        _lib.call("msu_seg_metrics", dt, logits.data_ptr(), label.data_ptr(), B, N, 0.5, part.data_ptr(), nblk,
                  out.data_ptr(), st)

    def many():
        for t in t32:
            _lib.call("msu_seg_metrics", dt, logits.data_ptr(), label.data_ptr(), B, N, t, part.data_ptr(), nblk,
                      out.data_ptr(), st)

    n_many = max(2, iters * 10 // K)
    for fn, n in ((sweep, iters), (one, iters), (many, 1)):  # warm
        timed(fn, n)
    tsw, tone, tmany = [], [], []
    for _ in range(reps):
        tsw.append(timed(sweep, iters))
        tone.append(timed(one, iters))
        tmany.append(timed(many, n_many))
    h = hist.cpu()
    assert int(h.sum()) == B * N
    interior = int(h[:, :, 1:-1].sum()) / (B * N)
    s, o, m = statistics.median(tsw), statistics.median(tone), statistics.median(tmany)
    print(json.dumps({"kernel": "msu_seg_sweep", "shape": [B, H, W], "logits": "bfloat16", "K": K,
                      "interior_share": round(interior, 5), "sweep_us": round(s, 2),
                      "sweep_us_min_max": [round(min(tsw), 2), round(max(tsw), 2)],
                      "metrics_x1_us": round(o, 2), "metrics_x1_us_min_max": [round(min(tone), 2), round(max(tone), 2)],
                      "metrics_xK_us": round(m, 2), "metrics_xK_us_min_max": [round(min(tmany), 2), round(max(tmany), 2)],
                      "sweep_over_x1": round(s / o, 3), "xK_over_sweep": round(m / s, 1),
                      "iters": iters, "iters_xK": n_many, "reps": reps}))
