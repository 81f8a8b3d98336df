"""One MLP forward (C -> 4 C -> C over M tokens; training form: H kept, and the no-grad form) on
the fused kernel (csrc/mlp_s1.hip; csrc/mlp_fused.hip at C = 96) vs the GEMM pair, same process,
HIP events, the arms interleaved round by round.
    python tools/mlp_s1_one.py [C [M [reps]]]      default: 192, 8 x 128^2, 20
(C 128, M 524288: Swin-B stage 0 at 1024^2, bs 8; C 192, M 131072: Swin-T/S stage 1)"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from semantic_segmentation_of_stylegan2_artifacts_amd import _lib, ops  # noqa: E402

C = int(sys.argv[1]) if len(sys.argv) > 1 else 192
M = int(sys.argv[2]) if len(sys.argv) > 2 else 8 * 128 * 128
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 20
Hd = 4 * C
g = torch.Generator().manual_seed(0)
x = torch.randn(M, C, generator=g).to("cuda", torch.bfloat16)
w1 = (torch.randn(Hd, C, generator=g) / C ** 0.5).to("cuda")
b1 = (0.1 * torch.randn(Hd, generator=g)).to("cuda")
w2 = (torch.randn(C, Hd, generator=g) / Hd ** 0.5).to("cuda")
b2 = (0.1 * torch.randn(C, generator=g)).to("cuda")
shapes = {"fused": ops.MLP_KERNEL_SHAPES, "pair": ()}
if (C, Hd) not in ops.MLP_KERNEL_SHAPES:
    print(f"mlp_s1 C={C}: no fused kernel for this width, both arms run the pair")
elif not _lib.lib().msu_mlp_fused_supported(C, Hd):
    # an older library loaded with MSU_LIB_OVERRIDE (A/B runs): it would answer -2
    print(f"mlp_s1 C={C}: the loaded library ({_lib.LIB_PATH}) has no fused kernel for this width, "
          "both arms run the pair")
    shapes["fused"] = ()
res = {}
for rnd in range(3):
    for name, sh in shapes.items():
        ops.MLP_FUSED_SHAPES = sh
        for keep in (True, False):
            fn = lambda: torch.ops.msunet.mlp(x, w1, b1, w2, b2, keep)  # noqa: E731
            with torch.autocast("cuda", dtype=torch.bfloat16):
                fn()
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(reps):
                    fn()
                e1.record()
            torch.cuda.synchronize()
            res.setdefault((name, keep), []).append(e0.elapsed_time(e1) / reps * 1e3)
for (name, keep), v in res.items():
    print(f"mlp_s1 C={C} M={M} {name} keep={keep}: {min(v):.1f} us (min of {len(v)}; "
          f"all {', '.join(f'{t:.1f}' for t in v)})")
