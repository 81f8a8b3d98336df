"""SHA-256 digests of y and H of the streamed-weight fused MLP (csrc/mlp_s1.hip) on seeded inputs:
C = 128 / 192 / 256, both 16-bit formats, with and without H, at M = 1, TT + 1, 8209 and
TT (CUs + 1) + 5 (TT = the workgroup tile: 256 tokens, 128 at C = 256).  A change that keeps the
arithmetic order per accumulator keeps every line; compare two builds of the library with
    MSU_LIB_OVERRIDE=/other/libmsunet_hip.so python tools/mlp_s1_digest.py > a.txt
    python tools/mlp_s1_digest.py > b.txt && diff a.txt b.txt
(the '#' line names the library, by its path from the repository's root, and is the only one allowed
to differ)."""
import hashlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from semantic_segmentation_of_stylegan2_artifacts_amd import _lib, ops  # noqa: E402


def digest(t):
    return hashlib.sha256(t.view(torch.int16).cpu().numpy().tobytes()).hexdigest()[:32]


print(f"# library: {os.path.relpath(_lib.LIB_PATH, ROOT)}")
cus = torch.cuda.get_device_properties(0).multi_processor_count
for C in (128, 192, 256):
    Hd, TT = 4 * C, 128 if C == 256 else 256
    g = torch.Generator().manual_seed(C)
    w1 = torch.randn(Hd, C, generator=g) / C ** 0.5
    b1 = (0.1 * torch.randn(Hd, generator=g)).cuda()
    w2 = torch.randn(C, Hd, generator=g) / Hd ** 0.5
    b2 = (0.1 * torch.randn(C, generator=g)).cuda()
    for M in (1, TT + 1, 8209, TT * (cus + 1) + 5):
        xf = torch.randn(M, C, generator=g)
        for low in (torch.bfloat16, torch.float16):
            x, w1l, w2l = xf.to("cuda", low), w1.to("cuda", low), w2.to("cuda", low)
            for keep in (True, False):
                y = torch.full((M, C), 0x5A5A, device="cuda", dtype=torch.int16).view(low)
                h = torch.full((M, Hd), 0x5A5A, device="cuda", dtype=torch.int16).view(low) if keep else None
                _lib.call("msu_mlp_fused_fwd", ops._dt(x), ops._p(x), ops._p(w1l), ops._p(b1), ops._p(w2l),
                          ops._p(b2), ops._p(y), ops._p(h), M, C, Hd, ops._s(x))
                torch.cuda.synchronize()
                name = "bf16" if low == torch.bfloat16 else "f16"
                print(f"C={C} M={M} {name} H={'yes' if keep else 'no'}: y {digest(y)} "
                      f"H {digest(h) if keep else '-'}")
