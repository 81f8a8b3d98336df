"""msu_pred_maps at the workload's shape (8 x 1024^2, every output requested) against a
device-to-device copy moving the same number of bytes, in one process: device events around
`iters` back-to-back launches on preallocated buffers, `reps` alternating rounds, medians.
    python tools/predmaps_bench.py [iters] [reps]
Prints one JSON line per logits dtype: us per call, GB/s over the algorithmic bytes (inputs
read once + outputs written once; the halo re-reads and the partial rows are not counted) and
the ratio to the copy."""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from semantic_segmentation_of_stylegan2_artifacts_amd import _lib, ops  # noqa: E402

iters = int(sys.argv[1]) if len(sys.argv) > 1 else 200
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 7
B, H, W = 8, 1024, 1024
dev = "cuda"


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters  # us per call


g = torch.Generator(device=dev).manual_seed(0)
image = torch.randint(0, 256, (B, 3, H, W), device=dev, generator=g).float() / 255.0
label = (torch.rand(B, H, W, device=dev, generator=g) < 0.05).float()
prob = torch.empty(B, H, W, device=dev)
heat, mask = (torch.empty(B, H, W, device=dev, dtype=torch.uint8) for _ in range(2))
heat_rgb, mask_rgb = (torch.empty(B, H, W, 3, device=dev, dtype=torch.uint8) for _ in range(2))
nblk = _lib.lib().msu_pred_maps_nblk(H, W)
part = torch.empty(B * nblk * 12, device=dev)
sums = torch.empty(B, 12, device=dev, dtype=torch.float64)

for dtype in (torch.float32, torch.bfloat16):
    logits = (torch.randn(B, 1, H, W, device=dev, generator=g) * 3).to(dtype)
    nbytes = B * H * W * (logits.element_size() + 12 + 4 + 4 + 1 + 1 + 3 + 3)
    src = torch.empty(nbytes // 2, device=dev, dtype=torch.uint8).fill_(1)  # the copy reads and writes: same traffic
    dst = torch.empty_like(src)
    st = ops._s(logits)

    def maps():
        _lib.call("msu_pred_maps", ops._dt(logits), logits.data_ptr(), image.data_ptr(), label.data_ptr(), B, H, W,
                  0.5, 0.4, 0.45, 0.25, 0xFF00FF, 1, prob.data_ptr(), heat.data_ptr(), mask.data_ptr(),
                  heat_rgb.data_ptr(), mask_rgb.data_ptr(), part.data_ptr(), sums.data_ptr(), st)

    def copy():
        dst.copy_(src)

    for fn in (maps, copy):  # warm
        timed(fn)
    tm, tc = [], []
    for _ in range(reps):
        tm.append(timed(maps))
        tc.append(timed(copy))
    m, c = statistics.median(tm), statistics.median(tc)
    print(json.dumps({"kernel": "msu_pred_maps", "shape": [B, H, W], "logits": str(dtype).split(".")[-1],
                      "outputs": "all", "bytes": nbytes, "us": round(m, 2), "us_min_max": [round(min(tm), 2), round(max(tm), 2)],
                      "GB_per_s": round(nbytes / m / 1e3, 1), "copy_us": round(c, 2),
                      "copy_GB_per_s": round(nbytes / c / 1e3, 1), "ratio_to_copy": round(m / c, 3),
                      "iters": iters, "reps": reps}))
