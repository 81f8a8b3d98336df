"""GPU: the Swin-B stage-1 width of the streamed-weight fused MLP (256 -> 1024, csrc/mlp_s1.hip
``mlp_s1_kernel_pc``): what tests/test_gpu_mlp_wide.py does not reach for a kernel with 128-token
workgroup tiles whose two waves per SIMD hand GELU(H) over through LDS.

Reference and tolerances are those of tests/test_gpu_mlp_wide.py: fp32 of the same 16-bit operands
with the kernel's two roundings (H and GELU(H) in 16 bits), |y - ref| <= 1e-2 |ref| + 4e-3 max|ref|,
H held to the same bound; gradients within 3e-2 of the reference's largest entry.  Both 16-bit
formats.  "wrap" is M = 128 (CUs + 1) + 5, the smallest M at which a workgroup walks a second
128-token tile: the weight ring and the hand-over parity continue across the tile boundary, the
next tile's x is loaded behind the last fc1, and the last tile is ragged.

The last three properties (exact H and equal y rows, nothing written past M, two launches bit for
bit) guard code that both kernels of csrc/mlp_s1.hip share (the phases of ``S1Wave``, the ring
bookkeeping of ``S1Ring``), so the ``*_one_role`` tests hold the one-role widths (128 -> 512 and
192 -> 768, ``mlp_s1_kernel``, 256-token workgroup tiles) to them too, at the same M relative to
the tile: TT + 1 and the wrap TT (CUs + 1) + 5.
"""
import pytest
import torch
import torch.nn.functional as F

from semantic_segmentation_of_stylegan2_artifacts_amd import _lib, ops

pytestmark = pytest.mark.gpu

DEV = "cuda"
C, HD = 256, 1024
# one token; a wave tile (32) and its edges; three full wave pairs plus a row; the workgroup
# tile's (128) edges; two tiles less a row; the wrap
MS = [1, 31, 32, 33, 97, 127, 129, 255, "wrap"]


@pytest.fixture(params=[torch.bfloat16, torch.float16], ids=["bf16", "f16"])
def low(request):
    return request.param


ONE_ROLE = [128, 192]  # the widths of mlp_s1_kernel; their workgroup tile:
TT1 = 256


def _m(M, TT=128):
    if M == "wrap":
        return TT * (torch.cuda.get_device_properties(0).multi_processor_count + 1) + 5
    return M


_PARAMS = {}


def _params(seed=11, C=C):
    """f32 master parameters, made once per seed and width and never modified."""
    HD = 4 * C
    if (seed, C) not in _PARAMS:
        g = torch.Generator().manual_seed(seed)
        _PARAMS[seed, C] = ((torch.randn(HD, C, generator=g) / C ** 0.5).to(DEV),
                            (torch.randn(HD, generator=g) * 0.1).to(DEV),
                            (torch.randn(C, HD, generator=g) / HD ** 0.5).to(DEV),
                            (torch.randn(C, generator=g) * 0.1).to(DEV))
    return _PARAMS[seed, C]


def _x(M, low, seed=1, C=C):
    return torch.randn(M, C, generator=torch.Generator().manual_seed(M + seed)).to(DEV, low)


def _ref(x, w1, b1, w2, b2, low):
    """(y, H) in fp32 from the 16-bit operands with the kernel's two roundings."""
    h = (x.float() @ w1.to(low).float().t() + b1).to(low).float()
    g = F.gelu(h).to(low).float()
    return g @ w2.to(low).float().t() + b2, h


def _within(name, a, r):
    scale = r.abs().max().item()
    err = ((a.float() - r).abs() - 1e-2 * r.abs()).max().item()
    print(f"{name}: excess err {err:.3e}, bound {4e-3 * scale:.3e}")
    assert err <= 4e-3 * scale, f"{name}: excess err {err:.3e} vs scale {scale:.3e}"


def _fwd_raw(x, w1l, b1, w2l, b2, y, h, M):
    """msu_mlp_fused_fwd itself on the given buffers (h may be None)."""
    C = x.shape[1]
    _lib.call("msu_mlp_fused_fwd", ops._dt(x), ops._p(x), ops._p(w1l), ops._p(b1), ops._p(w2l), ops._p(b2),
              ops._p(y), ops._p(h), M, C, 4 * C, ops._s(x))


def test_width_is_shipped_and_routed():
    assert (C, HD) in ops.MLP_FUSED_SHAPES, ops.MLP_FUSED_SHAPES
    assert _lib.lib().msu_mlp_fused_supported(C, HD) == 1


@pytest.mark.parametrize("M", MS)
def test_values_match_fp32(M, low, monkeypatch):
    monkeypatch.setattr(ops, "_MLP_TRAIN", True)
    monkeypatch.setattr(ops, "_MLP_INFER", True)
    M = _m(M)
    w1, b1, w2, b2 = _params()
    x = _x(M, low)
    yr, hr = _ref(x, w1, b1, w2, b2, low)
    n0, t0 = ops.mlp_infer_calls, ops.mlp_train_calls
    with torch.no_grad(), torch.autocast("cuda", dtype=low):
        y = ops.mlp(x, w1, b1, w2, b2)
    assert (ops.mlp_infer_calls, ops.mlp_train_calls) == (n0 + 1, t0), "the no-grad MLP did not take the fused kernel"
    with torch.autocast("cuda", dtype=low):
        yt, h, g = torch.ops.msunet.mlp(x, w1, b1, w2, b2, True)
    assert (ops.mlp_infer_calls, ops.mlp_train_calls) == (n0 + 1, t0 + 1), "the training MLP did not take the fused kernel"
    assert y.shape == (M, C) and y.dtype == low and yt.shape == (M, C) and h.shape == (M, HD) and h.dtype == low
    assert g.numel() == 0
    _within(f"y no-grad M={M}", y, yr)
    _within(f"y M={M}", yt, yr)
    _within(f"H M={M}", h, hr)


@pytest.mark.parametrize("M", [129, "wrap"])
def test_gradients_match_fp32(M, low, monkeypatch):
    """Trainer-style parameters (flat .grad, 16-bit shadows, direct accumulation), as
    tests/test_gpu_mlp_wide.py::test_mlp_wide_train_matches_fp32, at sizes where the 128-token
    tile ends ragged and where a workgroup walks a second tile."""
    monkeypatch.setattr(ops, "_MLP_TRAIN", True)
    M = _m(M)
    w1, b1, w2, b2 = (torch.nn.Parameter(t.clone()) for t in _params(5))
    for p_ in (w1, b1, w2, b2):
        p_.grad = torch.zeros_like(p_)
        p_._msu_direct = True
        p_._msu_shadow = p_.detach().to(low)
        if p_.dim() == 2:
            p_._msu_shadow_t = p_.detach().t().contiguous().to(low)
        p_._msu_shadow_ver = p_._version
    x = _x(M, low, seed=3)
    dy = _x(M, low, seed=4)
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
    assert gg.numel() == 0 and h.shape == (M, HD)
    y.backward(dy)
    torch.cuda.synchronize()
    _within(f"y M={M}", y, yr.detach())
    _within(f"H M={M}", h, hr.detach())
    for name, a, r in (("dx", xg.grad, xr.grad), ("dw1", w1.grad, pr[0].grad), ("db1", b1.grad, pr[1].grad),
                       ("dw2", w2.grad, pr[2].grad), ("db2", b2.grad, pr[3].grad)):
        err = (a.float() - r).abs().max().item()
        print(f"{name} M={M}: {err:.3e} vs {r.abs().max().item():.3e}")
        assert err <= 3e-2 * r.abs().max().item(), f"{name} M={M}: {err:.3e} vs {r.abs().max().item():.3e}"


def _distinct_b1(low, HD=HD):
    """HD distinct values exactly representable in `low`, 2^-7 .. 2, alternating sign."""
    base, step = (0x3C00, 1) if low == torch.bfloat16 else (0x2000, 8)
    bits = (base + step * torch.arange(HD, dtype=torch.int32)).to(torch.int16)
    v = bits.view(low).float()
    v[1::2] = -v[1::2]
    assert v.to(low).unique().numel() == HD
    return v.to(DEV)


def _check_h_is_exact(M, low, C):
    """x = 0: fc1 adds nothing, so every stored H row is round16(b1) = b1 bit for bit, whatever
    the MFMA numerics: a wrong hidden-unit permutation or chunk order shows.  With W1 = 0 and
    b2 = 0 too, every token sees the same GELU(H) row: all y rows are bitwise equal and match
    the reference's row, which a stale or swapped hand-over buffer (wrong parity) breaks."""
    HD = 4 * C
    w1, _, w2, _ = _params(C=C)
    b1 = _distinct_b1(low, HD)
    x = torch.zeros(M, C, device=DEV, dtype=low)
    w1l, w2l = w1.to(low).contiguous(), w2.to(low).contiguous()
    b2z = torch.zeros(C, device=DEV)
    y = torch.empty(M, C, device=DEV, dtype=low)
    h = torch.empty(M, HD, device=DEV, dtype=low)
    _fwd_raw(x, w1l, b1, w2l, b2z, y, h, M)
    want = b1.to(low).view(torch.int16)
    assert torch.equal(h.view(torch.int16), want.expand(M, HD)), "H rows differ from round16(b1)"
    _fwd_raw(x, torch.zeros_like(w1l), b1, w2l, b2z, y, h, M)
    assert torch.equal(h.view(torch.int16), want.expand(M, HD))
    assert torch.equal(y.view(torch.int16), y[:1].view(torch.int16).expand(M, C)), "y rows differ from each other"
    yr, _ = _ref(x[:1], torch.zeros_like(w1), b1, w2, b2z, low)
    _within(f"y row C={C} M={M}", y[:1], yr)


@pytest.mark.parametrize("M", [129, "wrap"])
def test_hand_over_is_exact(M, low):
    _check_h_is_exact(_m(M), low, C)


@pytest.mark.parametrize("M", [TT1 + 1, "wrap"])
@pytest.mark.parametrize("width", ONE_ROLE)
def test_h_is_exact_one_role(width, M, low):
    _check_h_is_exact(_m(M, TT1), low, width)


def _check_nothing_is_written_past_m(M, low, C):
    """y and h are the first M rows of larger buffers filled with a sentinel bit pattern: the
    160 rows from M on are untouched, with and without H."""
    HD = 4 * C
    w1, b1, w2, b2 = _params(C=C)
    w1l, w2l = w1.to(low).contiguous(), w2.to(low).contiguous()
    x = _x(M, low, C=C)
    extra, sentinel = 160, 0x5A5A
    ybuf = torch.full((M + extra, C), sentinel, device=DEV, dtype=torch.int16)
    hbuf = torch.full((M + extra, HD), sentinel, device=DEV, dtype=torch.int16)
    _fwd_raw(x, w1l, b1, w2l, b2, ybuf.view(low), hbuf.view(low), M)
    torch.cuda.synchronize()
    assert (ybuf[M:] == sentinel).all() and (hbuf[M:] == sentinel).all()
    yr, hr = _ref(x, w1, b1, w2, b2, low)
    _within(f"y M={M}", ybuf[:M].view(low), yr)
    _within(f"H M={M}", hbuf[:M].view(low), hr)
    ybuf.fill_(sentinel)
    _fwd_raw(x, w1l, b1, w2l, b2, ybuf.view(low), None, M)
    assert (ybuf[M:] == sentinel).all()
    _within(f"y no-H M={M}", ybuf[:M].view(low), yr)


@pytest.mark.parametrize("M", [1, 33, 129, 1000])
def test_nothing_is_written_past_m(M, low):
    _check_nothing_is_written_past_m(M, low, C)


@pytest.mark.parametrize("M", [1, 33, TT1 + 1, 1000])
@pytest.mark.parametrize("width", ONE_ROLE)
def test_nothing_is_written_past_m_one_role(width, M, low):
    _check_nothing_is_written_past_m(M, low, width)


def _check_two_launches_agree_bitwise(M, low, C):
    """The same inputs twice at the wrap M: y and H bit for bit (a hand-over race, a read ahead
    of its DMA or a slot refilled under a reader would differ)."""
    HD = 4 * C
    w1, b1, w2, b2 = _params(C=C)
    w1l, w2l = w1.to(low).contiguous(), w2.to(low).contiguous()
    x = _x(M, low, C=C)
    out = []
    for _ in range(2):
        y = torch.empty(M, C, device=DEV, dtype=low)
        h = torch.empty(M, HD, device=DEV, dtype=low)
        _fwd_raw(x, w1l, b1, w2l, b2, y, h, M)
        out.append((y, h))
    torch.cuda.synchronize()
    assert torch.equal(out[0][0].view(torch.int16), out[1][0].view(torch.int16))
    assert torch.equal(out[0][1].view(torch.int16), out[1][1].view(torch.int16))


def test_two_launches_agree_bitwise(low):
    _check_two_launches_agree_bitwise(_m("wrap"), low, C)


@pytest.mark.parametrize("width", ONE_ROLE)
def test_two_launches_agree_bitwise_one_role(width, low):
    _check_two_launches_agree_bitwise(_m("wrap", TT1), low, width)
