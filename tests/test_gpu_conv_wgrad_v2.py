"""GPU: the persistent refine-conv weight gradient (conv3x3_wgrad_v2_kernel) at both of its widths,
C = 96 (one workgroup per pixel share) and C = 128 (one per pixel share and output-channel half),
against fp32 conv2d autograd on the CPU of the same 16-bit operands -- GELU on load (in_mode bit 0)
as F.gelu in fp32 of the stored input -- with the gradient tolerance of the refine-conv tests
(3e-2 bf16 / 7.5e-3 f16 of max |ref|); at 128 against the generic kernel (msu_conv_mode bit 1, which
does nothing at 96); with `accumulate` against overwrite + f32 add (bitwise); with several tiles per
workgroup; and with more workgroups than tiles (the idle blocks' partials are zero)."""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
WIDTHS = [96, 128]
SHAPES = [(1, 8, 8), (1, 16, 32), (1, 20, 36), (2, 40, 56), (1, 260, 264)]
IDS = ["sub_tile", "whole_tiles", "ragged", "two_images", "wrap"]
# in_mode: bit 0 GELU on load, bit 1 d2s input.  The GELU modes on the three small shapes only.
CASES = [pytest.param(*s, m, id=f"{i}-{n}") for m, n in ((0, "plain"), (2, "d2s")) for s, i in zip(SHAPES, IDS)]
CASES += [pytest.param(*s, m, id=f"{i}-{n}") for m, n in ((1, "gelu"), (3, "d2s_gelu"))
          for s, i in zip(SHAPES[:3], IDS[:3])]


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


def _d2s(t, C):
    from einops import rearrange
    return rearrange(t, "b h w (p1 p2 c) -> b (h p1) (w p2) c", p1=4, p2=4, c=C)


@functools.lru_cache(maxsize=None)
def _case(C, B, H, W, mode, dtype):
    """Seeded 16-bit operands (a: the conv's input as stored, dz) and dW, db of
    z = conv2d(act(map(a)), w) + b in fp32 (independent of w and b).  Shared, never written to."""
    d2s, gelu = bool(mode & 2), bool(mode & 1)
    g = torch.Generator().manual_seed(100 * H + W + 3 * d2s)
    xs = (B, H // 4, W // 4, 16 * C) if d2s else (B, H, W, C)
    a = torch.randn(xs, generator=g).to(dtype)
    dz = torch.randn(B, H, W, C, generator=g).to(dtype)
    w = torch.zeros(C, C, 3, 3, requires_grad=True)
    b = torch.zeros(C, requires_grad=True)
    af = _d2s(a.float(), C) if d2s else a.float()
    if gelu:
        af = F.gelu(af)
    z = F.conv2d(af.permute(0, 3, 1, 2), w, b, padding=1).permute(0, 2, 3, 1)
    z.backward(dz.float())
    return a, dz, w.grad, b.grad


def _direct(C, ad, dzd, mode, nchunk, B, H, W):
    """msu_conv3x3_wgrad2 (bf16, overwrite) on a NaN-filled workspace with a band behind it."""
    ops, lib = _ops(), _lib()
    n = lib.lib().msu_conv3x3_wgrad_workspace(nchunk, C, C, 0, 0)
    ws = torch.full((n + 1024,), float("nan"), device=DEV)
    dw = torch.empty(C, C, 3, 3, device=DEV)
    db = torch.empty(C, device=DEV)
    lib.call("msu_conv3x3_wgrad2", 1, mode, ad.data_ptr(), dzd.data_ptr(), dw.data_ptr(), db.data_ptr(), ws.data_ptr(),
             nchunk, B, H, W, C, C, 0, ops._s(ad))
    torch.cuda.synchronize()
    assert torch.isnan(ws[n:]).all(), "written past the workspace"
    return dw, db, ws


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("B,H,W,mode", CASES)
@pytest.mark.parametrize("C", WIDTHS)
def test_wgrad_v2_matches_fp32_and_generic(C, B, H, W, mode, dtype):
    ops, lib = _ops(), _lib().lib()
    assert lib.msu_conv3x3_route(1 if dtype == torch.bfloat16 else 2, C, C) & 2
    a, dz, dwr, dbr = _case(C, B, H, W, mode, dtype)
    ad, dzd = a.to(DEV), dz.to(DEV)
    dw, db = ops._conv_wgrad(ad, dzd, mode, B, H, W, C, C)
    dw2, db2 = ops._conv_wgrad(ad, dzd, mode, B, H, W, C, C)
    if C == 128:
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
    if C == 128:
        _close(dw, dwg, t, "dW: persistent against generic kernel")
        _close(db, dbg, t, "db: persistent against generic kernel")


@pytest.mark.parametrize("mode", [0, 2], ids=["plain", "d2s"])
@pytest.mark.parametrize("C", WIDTHS)
def test_wgrad_v2_accumulate_equals_add(C, mode):
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


@pytest.mark.parametrize("mode", [0, 3], ids=["plain", "d2s_gelu"])
@pytest.mark.parametrize("C", WIDTHS)
def test_wgrad_v2_several_tiles_per_workgroup(C, mode):
    """(1, 20, 36) is ten 4-row x 32-pixel tiles; nchunk = 2 is two pixel shares of five tiles at
    96 and one share of ten at 128, so the two LDS buffers change over more than once."""
    B, H, W = 1, 20, 36
    a, dz, dwr, dbr = _case(C, B, H, W, mode, torch.bfloat16)
    ad, dzd = a.to(DEV), dz.to(DEV)
    dw, db, _ = _direct(C, ad, dzd, mode, 2, B, H, W)
    dw2, db2, _ = _direct(C, ad, dzd, mode, 2, B, H, W)
    _close(dw, dwr, 3e-2, "dW")
    _close(db, dbr, 3e-2, "db")
    assert torch.equal(dw, dw2) and torch.equal(db, db2), "two launches differ"


@pytest.mark.parametrize("nchunk", [1, 2, 7, 16])
@pytest.mark.parametrize("C", WIDTHS)
def test_wgrad_v2_idle_blocks_write_zero_partials(C, nchunk):
    """(1, 8, 8) is two 4-row tiles: with more pixel shares than tiles the idle workgroups'
    partial slabs are zero, the sum is right, and nothing past the shares in use is touched."""
    B, H, W = 1, 8, 8
    a, dz, dwr, dbr = _case(C, B, H, W, 0, torch.bfloat16)
    dw, db, ws = _direct(C, a.to(DEV), dz.to(DEV), 0, nchunk, B, H, W)
    _close(dw, dwr, 3e-2, "dW")
    _close(db, dbr, 3e-2, "db")
    nshare = nchunk if C == 96 else max(1, nchunk // 2)
    slab = 3 * C * 3 * C
    part = ws[:nshare * slab].view(nshare, slab)
    dbpart = ws[nchunk * slab:nchunk * slab + nshare * C].view(nshare, C)
    assert torch.isfinite(part).all() and torch.isfinite(dbpart).all(), "a share's partials left unwritten"
    for s in range(2, nshare):  # shares beyond the two tiles
        assert not part[s].any() and not dbpart[s].any(), f"idle share {s} wrote non-zero partials"
