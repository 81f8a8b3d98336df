"""GPU: the refine-conv weight gradient at C = 128 (conv3x3_wgrad_v2h_kernel: one workgroup per
pixel share and output-channel half) against fp32 conv2d autograd on the CPU of the same 16-bit
operands, with the gradient tolerance of the C = 96 tests (3e-2 bf16 / 7.5e-3 f16 of max |ref|),
against the generic kernel (msu_conv_mode bit 1), with `accumulate` against overwrite + f32 add
(bitwise), and with more workgroups than tiles (the idle blocks' partials are zero)."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
C = 128
SHAPES = [(1, 8, 8), (1, 16, 32), (1, 20, 36), (2, 40, 56), (1, 260, 264)]
IDS = ["sub_tile", "whole_tiles", "ragged", "two_images", "wrap"]


def _ops():
    from semantic_segmentation_of_stylegan2_artifacts_amd import ops
    return ops


def _lib():
    from semantic_segmentation_of_stylegan2_artifacts_amd import _lib
    return _lib


def _close(a, b, tol, what):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    assert torch.isfinite(a).all(), f"{what}: non-finite values"
    err, scale = (a - b).abs().max().item(), b.abs().max().item()
    print(f"{what}: max err {err:.3e}, scale {scale:.3e}, bound {tol + tol * scale:.3e}")
    assert err <= tol + tol * scale, f"{what}: max err {err:.3e} vs scale {scale:.3e}"


def _tol(dtype):
    return 3e-2 if dtype == torch.bfloat16 else 7.5e-3


def _d2s(t):
    from einops import rearrange
    return rearrange(t, "b h w (p1 p2 c) -> b (h p1) (w p2) c", p1=4, p2=4, c=C)


def _inputs(B, H, W, d2s, dtype):
    g = torch.Generator().manual_seed(100 * H + W + 3 * d2s)
    xs = (B, H // 4, W // 4, 16 * C) if d2s else (B, H, W, C)
    a = torch.randn(xs, generator=g).to(dtype)       # the conv's input activation, as stored
    dz = torch.randn(B, H, W, C, generator=g).to(dtype)
    return a, dz


def _reference(a, dz, d2s):
    """dW, db of z = conv2d(map(a), w) + b in fp32 (independent of w and b)."""
    w = torch.zeros(C, C, 3, 3, requires_grad=True)
    b = torch.zeros(C, requires_grad=True)
    af = _d2s(a.float()) if d2s else a.float()
    z = F.conv2d(af.permute(0, 3, 1, 2), w, b, padding=1).permute(0, 2, 3, 1)
    z.backward(dz.float())
    return w.grad, b.grad


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("d2s", [False, True], ids=["plain", "d2s"])
@pytest.mark.parametrize("B,H,W", SHAPES, ids=IDS)
def test_c128_wgrad_matches_fp32_and_generic(B, H, W, d2s, dtype):
    ops, lib = _ops(), _lib().lib()
    assert lib.msu_conv3x3_route(1 if dtype == torch.bfloat16 else 2, C, C) & 2
    a, dz = _inputs(B, H, W, d2s, dtype)
    dwr, dbr = _reference(a, dz, d2s)
    ad, dzd = a.to(DEV), dz.to(DEV)
    mode = 2 if d2s else 0
    dw, db = ops._conv_wgrad(ad, dzd, mode, B, H, W, C, C)
    dw2, db2 = ops._conv_wgrad(ad, dzd, mode, B, H, W, C, C)
    prev = lib.msu_conv_mode(0)
    try:
        lib.msu_conv_mode(prev | 2)
        dwg, dbg = ops._conv_wgrad(ad, dzd, mode, B, H, W, C, C)
    finally:
        lib.msu_conv_mode(prev)
    torch.cuda.synchronize()
    t = _tol(dtype)
    _close(dw, dwr, t, "dW")
    _close(db, dbr, t, "db")
    assert torch.equal(dw, dw2) and torch.equal(db, db2), "two launches differ"
    _close(dw, dwg, t, "dW: persistent against generic kernel")
    _close(db, dbg, t, "db: persistent against generic kernel")


@pytest.mark.parametrize("mode", [0, 2], ids=["plain", "d2s"])
def test_c128_wgrad_accumulate_equals_add(mode):
    """accumulate: dW / db added into existing f32 gradients, bitwise equal to the overwrite form
    followed by an f32 add."""
    ops = _ops()
    g = torch.Generator().manual_seed(C + mode)
    B, H, W = 2, 32, 32
    xs = (B, H // 4, W // 4, 16 * C) if mode == 2 else (B, H, W, C)
    a = torch.randn(xs, generator=g).to(DEV, torch.bfloat16)
    dz = torch.randn(B, H, W, C, generator=g).to(DEV, torch.bfloat16)
    w0 = torch.randn(C, C, 3, 3, generator=g).to(DEV)
    b0 = torch.randn(C, generator=g).to(DEV)
    dw, db = ops._conv_wgrad(a, dz, mode, B, H, W, C, C)
    w, b = torch.nn.Parameter(w0.clone()), torch.nn.Parameter(b0.clone())
    w.grad, b.grad = w0.clone(), b0.clone()
    ops._conv_wgrad(a, dz, mode, B, H, W, C, C, into=(w, b))
    torch.cuda.synchronize()
    assert torch.equal(w.grad, w0 + dw)
    assert torch.equal(b.grad, b0 + db)


@pytest.mark.parametrize("nchunk", [1, 2, 7, 16])
def test_c128_wgrad_idle_blocks_write_zero_partials(nchunk):
    """(1, 8, 8) is two 4-row tiles: with more pixel shares than tiles the idle workgroups'
    partial slabs are zero, the sum is right, and nothing past the shares in use is touched."""
    ops, lib = _ops(), _lib()
    B, H, W = 1, 8, 8
    a, dz = _inputs(B, H, W, False, torch.bfloat16)
    dwr, dbr = _reference(a, dz, False)
    ad, dzd = a.to(DEV), dz.to(DEV)
    n = lib.lib().msu_conv3x3_wgrad_workspace(nchunk, C, C, 0, 0)
    ws = torch.full((n + 1024,), float("nan"), device=DEV)
    dw = torch.empty(C, C, 3, 3, device=DEV)
    db = torch.empty(C, device=DEV)
    lib.call("msu_conv3x3_wgrad2", 1, 0, ad.data_ptr(), dzd.data_ptr(), dw.data_ptr(), db.data_ptr(), ws.data_ptr(),
             nchunk, B, H, W, C, C, 0, ops._s(ad))
    torch.cuda.synchronize()
    _close(dw, dwr, 3e-2, "dW")
    _close(db, dbr, 3e-2, "db")
    assert torch.isnan(ws[n:]).all(), "written past the workspace"
    nshare = max(1, nchunk // 2)
    slab = 3 * C * 3 * C
    part = ws[:nshare * slab].view(nshare, slab)
    dbpart = ws[nchunk * slab:nchunk * slab + nshare * C].view(nshare, C)
    assert torch.isfinite(part).all() and torch.isfinite(dbpart).all(), "a share's partials left unwritten"
    for s in range(2, nshare):  # shares beyond the two tiles
        assert not part[s].any() and not dbpart[s].any(), f"idle share {s} wrote non-zero partials"
