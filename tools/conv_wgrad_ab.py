"""Builds of the library side by side in ONE process, on the persistent refine-conv weight gradient
(msu_conv3x3_wgrad2 at C = 96 and 128, conv3x3_wgrad_v2_kernel).
Digests: SHA-256 of dW and db on seeded inputs made on the CPU -- both widths, bf16 and f16, in_mode
0-3, overwrite and accumulate, at (1, 8, 8), (1, 20, 36) with nchunk 2 and 7, and (2, 40, 56) with
the default nchunk.  The partial layout and the reduction order are fixed, so two builds that keep
the order of the sums per accumulator print the same digests; the last line counts the cases where
they do not, and the exit status is 1 if there are any.
Timing: the bench shape 8 x 1024 x 1024, bf16 (random, made on the device), in_mode 0 and 2, both
widths; the builds called in rounds that alternate their order, HIP events, median / min / quartiles
over 40 rounds x 5 launches.  Naming one build twice (a=... a2=...) gives the noise of the method.
    python tools/conv_wgrad_ab.py [--digest-only | --time-only] name=/path/libmsunet_hip.so ..."""
import ctypes
import hashlib
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from semantic_segmentation_of_stylegan2_artifacts_amd import switches  # noqa: E402

NCHUNK = int(switches.get("MSU_CONV_WGRAD_BLOCKS"))
flags = [a for a in sys.argv[1:] if a.startswith("--")]
libs = []
for a in sys.argv[1:]:
    if a.startswith("--"):
        continue
    n, p = a.split("=")
    h = ctypes.CDLL(p)
    h.msu_conv3x3_wgrad_workspace.restype = ctypes.c_long
    h.msu_conv3x3_wgrad_workspace.argtypes = [ctypes.c_int] * 5
    h.msu_conv3x3_wgrad2.restype = ctypes.c_int
    h.msu_conv3x3_wgrad2.argtypes = [ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 5 + [ctypes.c_int] * 7 + [ctypes.c_void_p]
    libs.append((n, h))
st = torch.cuda.current_stream().cuda_stream


def inputs(C, B, H, W, mode, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    xs = (B, H // 4, W // 4, 16 * C) if mode & 2 else (B, H, W, C)
    return torch.randn(xs, generator=g).to(dtype).cuda(), torch.randn(B, H, W, C, generator=g).to(dtype).cuda()


def wgrad(h, C, a, dz, dw, db, ws, mode, nchunk, B, H, W, acc):
    rc = h.msu_conv3x3_wgrad2(1 if a.dtype == torch.bfloat16 else 2, mode, a.data_ptr(), dz.data_ptr(), dw.data_ptr(),
                              db.data_ptr(), ws.data_ptr(), nchunk, B, H, W, C, C, acc, st)
    assert rc == 0, rc


def sha(t):
    return hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()[:32]


def digests():
    cases, differ = 0, 0
    for C in (96, 128):
        for B, H, W, nchunk in ((1, 8, 8, NCHUNK), (1, 20, 36, 2), (1, 20, 36, 7), (2, 40, 56, NCHUNK)):
            for dtype, dn in ((torch.bfloat16, "bf16"), (torch.float16, "f16")):
                for mode in range(4):
                    a, dz = inputs(C, B, H, W, mode, dtype, 1000 * C + 10 * H + mode)
                    g = torch.Generator().manual_seed(C + mode)
                    w0, b0 = torch.randn(C, C, 3, 3, generator=g).cuda(), torch.randn(C, generator=g).cuda()
                    for acc in (0, 1):
                        seen = set()
                        for n, h in libs:
                            ws = torch.full((h.msu_conv3x3_wgrad_workspace(nchunk, C, C, 0, 0),), float("nan"),
                                            device="cuda")
                            dw, db = w0.clone(), b0.clone()
                            wgrad(h, C, a, dz, dw, db, ws, mode, nchunk, B, H, W, acc)
                            torch.cuda.synchronize()
                            seen.add((sha(dw), sha(db)))
                            print(f"C={C} {B}x{H}x{W} nchunk={nchunk} {dn} mode={mode} "
                                  f"{'accumulate' if acc else 'overwrite'} {n:8s}: dW {sha(dw)} db {sha(db)}", flush=True)
                        cases += 1
                        differ += len(seen) > 1
    print(f"# {cases} cases x {len(libs)} libraries: {differ} cases with differing digests", flush=True)
    return differ


def timing():
    B, H, W, ROUNDS, REPS = 8, 1024, 1024, 40, 5
    for C in (96, 128):
        ws = torch.empty(max(h.msu_conv3x3_wgrad_workspace(NCHUNK, C, C, 0, 0) for _, h in libs), device="cuda")
        dw, db = torch.empty(C, C, 3, 3, device="cuda"), torch.empty(C, device="cuda")
        for mode in (0, 2):
            xs = (B, H // 4, W // 4, 16 * C) if mode & 2 else (B, H, W, C)
            a = torch.randn(xs, device="cuda").to(torch.bfloat16)
            dz = torch.randn(B, H, W, C, device="cuda").to(torch.bfloat16)
            res = {n: [] for n, _ in libs}
            for r in range(ROUNDS + 2):
                for n, h in (libs if r % 2 == 0 else libs[::-1]):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(REPS):
                        wgrad(h, C, a, dz, dw, db, ws, mode, NCHUNK, B, H, W, 0)
                    e1.record()
                    torch.cuda.synchronize()
                    if r >= 2:
                        res[n].append(e0.elapsed_time(e1) / REPS * 1e3)
            for n, v in res.items():
                v.sort()
                print(f"C={C} {B}x{H}x{W} bf16 mode={mode} nchunk={NCHUNK} {n:8s}: median {statistics.median(v):.1f} us, "
                      f"min {v[0]:.1f}, quartiles {v[len(v) // 4]:.1f}-{v[3 * len(v) // 4]:.1f} "
                      f"({len(v)} rounds x {REPS})", flush=True)
            del a, dz


differ = digests() if "--time-only" not in flags else 0
if "--digest-only" not in flags:
    timing()
sys.exit(1 if differ else 0)
