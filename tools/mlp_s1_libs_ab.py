"""Builds of the library side by side in ONE process: msu_mlp_fused_fwd (bf16; training form with H
kept, then the no-grad form) called on each build in alternating rounds, HIP events, median / min /
quartiles over 40 rounds x 20 launches per build.  Separate processes differ by several us at these
kernels (tools/mlp_s1_one.py, three processes: 153.9-157.4 us for one build); this does not.
    python tools/mlp_s1_libs_ab.py C M name=/path/libmsunet_hip.so name=/other/libmsunet_hip.so ..."""
import ctypes
import statistics
import sys

import torch

C, M = int(sys.argv[1]), int(sys.argv[2])
libs = []
for a in sys.argv[3:]:
    n, p = a.split("=")
    h = ctypes.CDLL(p)
    h.msu_mlp_fused_fwd.restype = ctypes.c_int
    h.msu_mlp_fused_fwd.argtypes = [ctypes.c_int] + [ctypes.c_void_p] * 7 + [ctypes.c_long, ctypes.c_int, ctypes.c_int,
                                                                             ctypes.c_void_p]
    libs.append((n, h))
Hd = 4 * C
g = torch.Generator().manual_seed(0)
x = torch.randn(M, C, generator=g).to("cuda", torch.bfloat16)
w1 = (torch.randn(Hd, C, generator=g) / C ** 0.5).to("cuda", torch.bfloat16)
b1 = (0.1 * torch.randn(Hd, generator=g)).to("cuda")
w2 = (torch.randn(C, Hd, generator=g) / Hd ** 0.5).to("cuda", torch.bfloat16)
b2 = (0.1 * torch.randn(C, generator=g)).to("cuda")
y = torch.empty(M, C, device="cuda", dtype=torch.bfloat16)
hbuf = torch.empty(M, Hd, device="cuda", dtype=torch.bfloat16)
st = torch.cuda.current_stream().cuda_stream
ROUNDS, REPS = 40, 20
for keep in (True, False):
    res = {n: [] for n, _ in libs}
    hp = hbuf.data_ptr() if keep else None
    for r in range(ROUNDS + 2):
        order = libs if r % 2 == 0 else libs[::-1]
        for n, h in order:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(REPS):
                rc = h.msu_mlp_fused_fwd(1, x.data_ptr(), w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(),
                                         y.data_ptr(), hp, M, C, Hd, st)
                assert rc == 0, rc
            e1.record()
            torch.cuda.synchronize()
            if r >= 2:
                res[n].append(e0.elapsed_time(e1) / REPS * 1e3)
    for n, v in res.items():
        v.sort()
        print(f"C={C} M={M} keep={keep} {n:8s}: median {statistics.median(v):.2f} us, min {v[0]:.2f}, "
              f"quartiles {v[len(v) // 4]:.2f}-{v[3 * len(v) // 4]:.2f} ({len(v)} rounds x {REPS})")
