"""GPU: the Swin-B widths of the streamed-weight fused MLP (csrc/mlp_s1.hip, C = 128 -> 512)
against plain fp32 PyTorch and against the GEMM pair: the inference form, the training form under
autograd, and the routing of a Swin-B model.

Reference and tolerances as tests/test_gpu_mlp_infer.py: fp32 of the same 16-bit operands with
the kernel's two roundings (H and GELU(H) in 16 bits), |y - ref| <= 1e-2 |ref| + 4e-3 max|ref|;
gradients within 3e-2 of the reference's largest entry; fused against pair rel. L2 <= 2e-3.
Every case runs for both 16-bit formats and for every shipped width of the family.
"""
import pytest
import torch
import torch.nn.functional as F

from semantic_segmentation_of_stylegan2_artifacts_amd import ops

pytestmark = pytest.mark.gpu

DEV = "cuda"
# the widths this family adds (hidden 4 C); one that is not shipped is absent from
# MLP_KERNEL_SHAPES altogether, (128, 512) is required
WIDTHS = [C for C in (128, 256) if (C, 4 * C) in ops.MLP_KERNEL_SHAPES]


@pytest.fixture(params=[torch.bfloat16, torch.float16], ids=["bf16", "f16"])
def low(request):
    return request.param


def _params(seed, C):
    g = torch.Generator().manual_seed(seed)
    Hd = 4 * C
    w1 = torch.nn.Parameter((torch.randn(Hd, C, generator=g) / C ** 0.5).to(DEV))
    b1 = torch.nn.Parameter((torch.randn(Hd, generator=g) * 0.1).to(DEV))
    w2 = torch.nn.Parameter((torch.randn(C, Hd, generator=g) / Hd ** 0.5).to(DEV))
    b2 = torch.nn.Parameter((torch.randn(C, generator=g) * 0.1).to(DEV))
    return w1, b1, w2, b2


def _ref(x, w1, b1, w2, b2, low):
    h = (x.float() @ w1.detach().to(low).float().t() + b1.detach()).to(low).float()
    g = F.gelu(h).to(low).float()
    return g @ w2.detach().to(low).float().t() + b2.detach()


def _within(name, a, r):
    r = r.detach()
    scale = r.abs().max().item()
    err = ((a.float() - r).abs() - 1e-2 * r.abs()).max().item()
    print(f"{name}: excess err {err:.3e}, bound {4e-3 * scale:.3e}")
    assert err <= 4e-3 * scale, f"{name}: excess err {err:.3e} vs scale {scale:.3e}"


def test_required_width_is_shipped():
    assert 128 in WIDTHS, ops.MLP_KERNEL_SHAPES


# M: one token; one wave tile + a row; one workgroup tile + a row; ragged; several tiles per
# workgroup slot; "wrap": 256 (CUs + 1) + 5, the smallest M at which a workgroup walks a second
# token tile (the ring continues across the tile boundary, the next tile's x is loaded behind
# the last fc1)
@pytest.mark.parametrize("M", [1, 33, 257, 1000, 8209, "wrap"])
@pytest.mark.parametrize("C", WIDTHS)
def test_mlp_wide_infer_matches_fp32(M, C, low):
    if M == "wrap":
        M = 256 * (torch.cuda.get_device_properties(0).multi_processor_count + 1) + 5
    w1, b1, w2, b2 = _params(M + C, C)
    x = torch.randn(M, C, generator=torch.Generator().manual_seed(M + 1)).to(DEV, low)
    n0 = ops.mlp_infer_calls
    with torch.no_grad(), torch.autocast("cuda", dtype=low):
        y = ops.mlp(x, w1, b1, w2, b2)
    assert ops.mlp_infer_calls == n0 + 1, "the no-grad MLP did not take the fused kernel"
    assert y.dtype == low and y.shape == (M, C)
    _within(f"y C={C} M={M}", y, _ref(x, w1, b1, w2, b2, low))


@pytest.mark.parametrize("M", [33, 8209])
@pytest.mark.parametrize("C", WIDTHS)
def test_mlp_wide_train_matches_fp32(M, C, low, monkeypatch):
    """Trainer-style parameters (flat .grad, 16-bit shadows, direct accumulation), as
    tests/test_gpu_mlp_infer.py::test_mlp_train_matches_fp32: the backward takes the two-kernel
    route, mlp.3's weight gradient on GELU(H) re-derived from H on the side stream."""
    monkeypatch.setattr(ops, "_MLP_TRAIN", True)
    w1, b1, w2, b2 = _params(M + 3, C)
    Hd = 4 * C
    for p_ in (w1, b1, w2, b2):
        p_.grad = torch.zeros_like(p_)
        p_._msu_direct = True
        p_._msu_shadow = p_.detach().to(low)
        if p_.dim() == 2:
            p_._msu_shadow_t = p_.detach().t().contiguous().to(low)
        p_._msu_shadow_ver = p_._version
    g = torch.Generator().manual_seed(M + 4)
    x = torch.randn(M, C, generator=g).to(DEV, low)
    dy = torch.randn(M, C, generator=g).to(DEV, low)
    xr = x.float().requires_grad_(True)
    pr = [t.detach().to(low).float().requires_grad_(True) if t.dim() == 2 else t.detach().clone().requires_grad_(True)
          for t in (w1, b1, w2, b2)]
    hr = F.linear(xr, pr[0], pr[1])
    yr = F.linear(F.gelu(hr), pr[2], pr[3])
    yr.backward(dy.float())
    xg = x.clone().requires_grad_(True)
    t0 = ops.mlp_train_calls
    with torch.autocast("cuda", dtype=low):
        y, h, gg = torch.ops.msunet.mlp(xg, w1, b1, w2, b2, True)
    assert ops.mlp_train_calls == t0 + 1, "the training MLP did not take the fused kernel"
    assert gg.numel() == 0 and h.shape == (M, Hd) and h.dtype == low
    y.backward(dy)
    torch.cuda.synchronize()
    _within(f"y C={C} M={M}", y, yr)
    _within(f"H C={C} M={M}", h, hr)
    for name, a, r in (("dx", xg.grad, xr.grad), ("dw1", w1.grad, pr[0].grad), ("db1", b1.grad, pr[1].grad),
                       ("dw2", w2.grad, pr[2].grad), ("db2", b2.grad, pr[3].grad)):
        err = (a.float() - r).abs().max().item()
        print(f"{name} C={C} M={M}: {err:.3e} vs {r.abs().max().item():.3e}")
        assert err <= 3e-2 * r.abs().max().item(), f"{name} M={M}: {err:.3e} vs {r.abs().max().item():.3e}"


@pytest.mark.parametrize("C", WIDTHS)
def test_mlp_wide_fused_matches_pair(C, low, monkeypatch):
    """The pair (MSU_MLP_TRAIN=0: H and GELU(H) kept) against the fused training form (y and the
    stored H) and against the fused no-grad form (y)."""
    w1, b1, w2, b2 = _params(7, C)
    x = torch.randn(2, 64, 64, C, generator=torch.Generator().manual_seed(8)).to(DEV, low)
    monkeypatch.setattr(ops, "_MLP_TRAIN", False)
    t0 = ops.mlp_train_calls
    with torch.autocast("cuda", dtype=low):
        y_pair, h_pair, g_pair = torch.ops.msunet.mlp(x.clone().requires_grad_(True), w1, b1, w2, b2, True)
    assert ops.mlp_train_calls == t0 and g_pair.numel() == h_pair.numel(), "the pair arm took the fused kernel"
    n0 = ops.mlp_infer_calls
    with torch.no_grad(), torch.autocast("cuda", dtype=low):
        y_inf = ops.mlp(x, w1, b1, w2, b2)
    assert ops.mlp_infer_calls == n0 + 1
    monkeypatch.setattr(ops, "_MLP_TRAIN", True)
    with torch.autocast("cuda", dtype=low):
        y_tr, h_tr, g_tr = torch.ops.msunet.mlp(x.clone().requires_grad_(True), w1, b1, w2, b2, True)
    assert ops.mlp_train_calls == t0 + 1 and g_tr.numel() == 0 and h_tr.shape == h_pair.shape
    for name, a, b in (("y no-grad", y_inf, y_pair), ("y", y_tr, y_pair), ("H", h_tr, h_pair)):
        rel = ((a.float() - b.float()).norm() / b.float().norm()).item()
        print(f"{name} C={C}: rel. L2 {rel:.3e}")
        assert rel <= 2e-3, (name, rel)


def test_swin_b_blocks_take_the_fused_mlp():
    """One bf16 training-mode forward of a Swin-B MS-UNet at 224^2 (4 . 8 . 7: every stage a
    whole number of windows): the no-grad blocks of the discarded branches take the inference
    form, every other block at a shipped width the training form."""
    from semantic_segmentation_of_stylegan2_artifacts_amd import load_config
    from semantic_segmentation_of_stylegan2_artifacts_amd.network import MSUNet
    from semantic_segmentation_of_stylegan2_artifacts_amd.network.model_parts import SwinTransformerBlock
    cfg = load_config(None, "swin_b", **{"DATA.IMG_SIZE": 224, "DATA.BATCH_SIZE": 1})
    torch.manual_seed(0)
    model = MSUNet(cfg, img_size=224, num_classes=1).to(DEV).train()
    net = model.ms_unet

    def shipped(blocks):
        return [b for b in blocks if isinstance(b, SwinTransformerBlock) and
                (b.mlp[0].in_features, b.mlp[0].out_features) in ops.MLP_FUSED_SHAPES]

    dead = [b for m in net.dead_modules() for b in shipped(m.modules())]
    live = [b for b in shipped(net.modules()) if not any(b is d for d in dead)]
    assert len(dead) == 4 and all(b.mlp[0].in_features == 128 for b in dead), len(dead)
    assert live and all(b.dropout == 0 for b in dead + live)
    x = torch.randn(1, 3, 224, 224, device=DEV)
    n0, t0 = ops.mlp_infer_calls, ops.mlp_train_calls
    with torch.autocast("cuda", dtype=torch.bfloat16):
        y = model(x)
    torch.cuda.synchronize()
    assert torch.isfinite(y.float()).all()
    assert ops.mlp_infer_calls - n0 == len(dead), (ops.mlp_infer_calls - n0, len(dead))
    assert ops.mlp_train_calls - t0 == len(live), (ops.mlp_train_calls - t0, len(live))
