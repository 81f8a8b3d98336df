"""GPU: the persistent refine-conv kernel at C = 128 (Swin-B decoder head) against fp32 conv2d on
the CPU of the same 16-bit activations, with the tolerances of the C = 96 tests in
test_gpu_ops.py (relative to max |ref|: 2e-2 bf16 / 5e-3 f16 forward, 3e-2 / 7.5e-3 gradients;
they are set by the 16-bit rounding of the outputs, the accumulation is f32 at both widths).

Every output of the C-ABI launches lives inside a larger NaN-filled buffer: the bands before and
after it must stay NaN (nothing written past a ragged tile edge or before the tensor), and the
tensor itself must be fully written.  The same launches are repeated (bitwise equal), run with
the static schedule instead of the tile queue (bitwise equal) and on the generic kernels
(msu_conv_mode bit 1; same tolerances).

Shapes: smaller than a tile; whole 8 x 32 tiles; ragged in both directions; two images; and
"wrap", 33 x 9 = 297 tiles -- more than the 256 workgroups of a launch, so workgroups take a
second tile through the queue -- with both edges ragged."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
C = 128
GUARD = 4096  # elements of each NaN band (a multiple of 8: the outputs stay 16-B aligned)
SHAPES = [(1, 8, 8), (1, 16, 32), (1, 20, 36), (2, 40, 56), (1, 260, 264)]
IDS = ["sub_tile", "whole_tiles", "ragged", "two_images", "wrap"]


def _ops():
    from semantic_segmentation_of_stylegan2_artifacts_amd import ops
    return ops


def _lib():
    from semantic_segmentation_of_stylegan2_artifacts_amd import _lib
    return _lib


def _close(a, b, rtol, atol, what=""):
    a = a.detach().float().cpu()
    b = b.detach().float().cpu()
    assert torch.isfinite(a).all(), f"{what}: non-finite values (unwritten output?)"
    err = (a - b).abs().max().item()
    scale = b.abs().max().item()
    print(f"{what}: max err {err:.3e}, scale {scale:.3e}, bound {atol + rtol * scale:.3e}")
    assert err <= atol + rtol * scale, f"{what}: max err {err:.3e} vs scale {scale:.3e}"


def _tol(dtype, bf16):
    return bf16 if dtype == torch.bfloat16 else bf16 / 4


def _d2s(t):
    from einops import rearrange
    return rearrange(t, "b h w (p1 p2 c) -> b (h p1) (w p2) c", p1=4, p2=4, c=C)


class Case:
    """Inputs of one (shape, d2s, dtype) and the fp32 CPU reference, computed once."""

    def __init__(self, B, H, W, d2s, dtype):
        g = torch.Generator().manual_seed(1000 * H + W + 7 * d2s)
        self.B, self.H, self.W, self.d2s, self.dtype = B, H, W, d2s, dtype
        xs = (B, H // 4, W // 4, 16 * C) if d2s else (B, H, W, C)
        x = torch.randn(xs, generator=g).to(dtype)                      # pre-activation S
        a = F.gelu(x.float()).to(dtype)                                 # the producer's GELU(S)
        w = torch.randn(C, C, 3, 3, generator=g) / math.sqrt(9 * C)
        b = 0.1 * torch.randn(C, generator=g)
        dz = torch.randn(B, H, W, C, generator=g).to(dtype)
        # forward: fp32 conv2d of the 16-bit activation
        af = _d2s(a.float()) if d2s else a.float()
        self.z = F.conv2d(af.permute(0, 3, 1, 2), w, b, padding=1).permute(0, 2, 3, 1).contiguous()
        # gradients: autograd through GELU -> (d2s) -> conv2d in fp32 from the 16-bit S and dz
        xr, wr, br = x.float().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
        ar = F.gelu(xr)
        ar = _d2s(ar) if d2s else ar
        zr = F.conv2d(ar.permute(0, 3, 1, 2), wr, br, padding=1).permute(0, 2, 3, 1)
        zr.backward(dz.float())
        self.dx, self.dw, self.db = xr.grad, wr.grad, br.grad
        self.x, self.a, self.dzd = x.to(DEV), a.to(DEV), dz.to(DEV)
        self.w, self.b = w.to(DEV), b.to(DEV)


_cases = {}


def _case(B, H, W, d2s, dtype):
    key = (B, H, W, d2s, dtype)
    if key not in _cases:
        _cases[key] = Case(B, H, W, d2s, dtype)
    return _cases[key]


def _banded(n, dtype):
    buf = torch.full((n + 2 * GUARD,), float("nan"), device=DEV, dtype=dtype)
    return buf, buf[GUARD:GUARD + n]


def _launch(c):
    """The four launch forms of this case through the C ABI, outputs inside NaN bands:
    (z of the plain forward, z and GELU(z) of the dual forward, dx of the GELU'(S) dgrad)."""
    ops, lib = _ops(), _lib()
    B, H, W = c.B, c.H, c.W
    wt, wf = ops._conv_weight(c.w, c.dtype, 0), ops._conv_weight(c.w, c.dtype, 1)
    n = B * H * W * C
    mode = 2 if c.d2s else 0
    bufs, outs = [], []
    for _ in range(4):
        buf, out = _banded(n, c.dtype)
        bufs.append(buf)
        outs.append(out)
    z1, z, z2, dx = outs
    st = ops._s(c.a)
    lib.call("msu_conv3x3_fwd2", ops._dt(c.a), mode, ops._p(c.a), ops._p(wt), ops._p(c.b), ops._p(z1), None,
             B, H, W, C, C, st)
    lib.call("msu_conv3x3_fwd2", ops._dt(c.a), mode, ops._p(c.a), ops._p(wt), ops._p(c.b), ops._p(z), ops._p(z2),
             B, H, W, C, C, st)
    lib.call("msu_conv3x3_dgrad", ops._dt(c.a), 1 | mode, ops._p(c.dzd), ops._p(wf), ops._p(c.x), ops._p(dx),
             B, H, W, C, C, st)
    torch.cuda.synchronize()
    for buf, name in zip(bufs, ("z (plain)", "z", "GELU(z)", "dx")):
        assert torch.isnan(buf[:GUARD]).all(), f"{name}: the band before the output was written"
        assert torch.isnan(buf[GUARD + n:]).all(), f"{name}: the band after the output was written"
        assert not torch.isnan(buf[GUARD:GUARD + n]).any(), f"{name}: output elements left unwritten"
    shape = (B, H, W, C)
    return z1.view(shape), z.view(shape), z2.view(shape), dx.view(c.x.shape)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("d2s", [False, True], ids=["plain", "d2s"])
@pytest.mark.parametrize("B,H,W", SHAPES, ids=IDS)
def test_c128_fwd_dgrad_match_fp32(B, H, W, d2s, dtype):
    lib = _lib().lib()
    assert lib.msu_conv3x3_route(1 if dtype == torch.bfloat16 else 2, C, C) & 1
    c = _case(B, H, W, d2s, dtype)
    tz, tg = _tol(dtype, 2e-2), _tol(dtype, 3e-2)
    prev = lib.msu_conv_mode(1)
    try:
        z1, z, z2, dx = _launch(c)
        again = _launch(c)
        lib.msu_conv_mode(0)   # static schedule
        static = _launch(c)
        lib.msu_conv_mode(3)   # generic kernels at 128: the route before the persistent kernel
        generic = _launch(c)
    finally:
        lib.msu_conv_mode(prev)
    _close(z1, c.z, tz, tz, "z (plain forward)")
    _close(z, c.z, tz, tz, "z (dual forward)")
    assert torch.equal(z1, z), "the plain and the dual forward store the same z"
    _close(z2, F.gelu(z.float()), tz, tz, "GELU(z)")
    _close(dx, c.dx, tg, tg, "dx")
    names = ("z (plain)", "z", "GELU(z)", "dx")
    for u, r, name in zip(again, (z1, z, z2, dx), names):
        assert torch.equal(u, r), f"{name}: two launches differ"
    for u, r, name in zip(static, (z1, z, z2, dx), names):
        assert torch.equal(u, r), f"{name}: tile queue and static schedule differ"
    for u, r, name in zip(generic, (z1, z, z2, dx), names):
        t = tg if name == "dx" else tz
        _close(r, u, t, t, f"{name}: persistent against generic kernel")


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("d2s", [False, True], ids=["plain", "d2s"])
@pytest.mark.parametrize("B,H,W", SHAPES[:4], ids=IDS[:4])
def test_c128_refine_conv_act_backward(B, H, W, d2s, dtype):
    """The op the model calls: z, GELU(z), dx, dW and db of ops.refine_conv_act at 128."""
    ops = _ops()
    c = _case(B, H, W, d2s, dtype)
    xg = c.x.clone().requires_grad_(True)
    wg, bg = c.w.clone().requires_grad_(True), c.b.clone().requires_grad_(True)
    with torch.autocast("cuda", dtype=dtype):
        z, z2 = ops.refine_conv_act(xg, c.a, wg, bg, d2s, (H, W), dual=True)
    z.backward(c.dzd)
    torch.cuda.synchronize()
    tz, tg = _tol(dtype, 2e-2), _tol(dtype, 3e-2)
    _close(z, c.z, tz, tz, "z")
    _close(z2, F.gelu(z.float()), tz, tz, "GELU(z)")
    _close(xg.grad, c.dx, tg, tg, "dx")
    _close(wg.grad, c.dw, tg, tg, "dW")
    _close(bg.grad, c.db, tg, tg, "db")


def test_c128_second_stream_has_its_own_queue_slot():
    """The wrap shape on a side stream (its own tile-queue slot) equals the current stream's."""
    c = _case(1, 260, 264, True, torch.bfloat16)
    ref = _launch(c)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        outs = _launch(c)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for u, r, name in zip(outs, ref, ("z (plain)", "z", "GELU(z)", "dx")):
        assert torch.equal(u, r), name
