"""GPU: attention dropout pinned to the host restatement of its mask streams.

Every other attention test with dropout on takes its mask from the kernel's own stored keep
bits.  Here the mask comes from tests/_attn_mask_ref.py (numpy, restated from csrc/common.h),
and the numerical reference is ``attn_ref_from_qkv`` in float64 on the operands the kernels
receive (qkv / dy rounded to the storage type, qkv bias and table f32), with that host mask.

a. the 16-bit forward's stored keep bits (csrc/window_attention_mfma.hip, unfused and fused
   stage-0 kernels) equal the host mask exactly, also with a device counter (``seed_dev``) mixed
   into the seed, before and after the counter is bumped in place;
b. under a counter the 16-bit backward that reads the stored bits, the one that re-hashes and
   the op's own autograd backward agree bit for bit;
c. the f32 parity kernels (csrc/window_attention.hip), which always re-hash, forward and
   backward against float64 at every shape of test_gpu_ops.ATTN_CASES, at 81 windows x 32 heads
   (more windows than the 2048 / nh = 64 backward blocks) and through ``seed_dev``;
d. the 16-bit kernels at the production head counts 4 / 8 / 12 / 16 / 24 / 32 with dropout 0.05
   (and p = 0 at 16 and 32 heads), forward and backward, whole tensors and head by head.

Tolerances are the project's own: 16-bit ``_check`` of test_gpu_production_parity.py (max error
<= t max|ref| and relative L2 <= t / 4, t = 3e-2 bf16 / 7.5e-3 f16); f32 ``_close(1e-4, 1e-5)``
of test_gpu_ops.test_window_attention_fp32.
"""
import functools

import pytest
import torch

from _attn_mask_ref import keep_mask
from _parity_refs import attn_ref_from_qkv, decode_keep_bits
from test_gpu_ops import ATTN_CASES, _close
from test_gpu_production_parity import TOL, _check

pytestmark = pytest.mark.gpu

DEV = "cuda"
BIG_SEED = (5 << 40) + 77
BF16, F16 = torch.bfloat16, torch.float16
DT_ID = {BF16: "bf16", F16: "f16"}


def _ops():
    from semantic_segmentation_of_stylegan2_artifacts_amd import ops
    return ops


def _nwin(B, H, W):
    return B * ((H + 6) // 7) * ((W + 6) // 7)


@functools.lru_cache(maxsize=None)
def _host_mask_cpu(n_items, seed, p, counter):
    return torch.from_numpy(keep_mask(n_items, seed, p, counter))


def host_mask(n_items, seed, p, counter=None):
    """The host restatement's mask, bool [n_items, 49, 49] on the device (built once per key)."""
    return _host_mask_cpu(n_items, seed, p, counter).to(DEV)


def _assert_mask(keep, n_items, seed, p, counter=None):
    assert keep.numel() == n_items * 128
    got = decode_keep_bits(keep, n_items)
    want = host_mask(n_items, seed, p, counter)
    if not torch.equal(got, want):
        bad = (got != want)
        first = bad.nonzero()[0].tolist()
        raise AssertionError(f"stored keep bits != host mask: {bad.sum().item()} of {bad.numel()} bits differ, "
                             f"{bad.flatten(1).any(1).sum().item()} of {n_items} items, first (item, i, j) = {first}")
    return want


def _inputs(B, H, W, nh, dtype, seed):
    """randn as in the existing attention tests; qkv / dy already in the storage type."""
    C = 32 * nh
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B, H, W, 3 * C, generator=g).to(DEV, dtype)
    qb = (0.3 * torch.randn(3 * C, generator=g)).to(DEV)
    table = torch.randn(169, nh, generator=g).to(DEV)
    dy = torch.randn(B, H, W, C, generator=g).to(DEV, dtype)
    return qkv, qb, table, dy


def _ref64(qkv, qb, table, dy, nh, shift, mask, p):
    """float64 attn_ref_from_qkv with the given mask -> out, dqkv, d qkv-bias, d table."""
    q, b, t = (x.detach().double().requires_grad_(True) for x in (qkv, qb, table))
    y = attn_ref_from_qkv(q, b, t, nh, shift, keep=mask, p_drop=p)
    dq, db, dt = torch.autograd.grad((y * dy.double()).sum(), (q, b, t))
    return y.detach(), dq, db, dt


def _run(qkv, qb, table, dy, nh, shift, p, seed, seed_dev=None):
    """ops.window_attention forward + backward on leaves of the given tensors."""
    _ops()  # registers torch.ops.msunet
    q, b, t = (x.clone().requires_grad_(True) for x in (qkv, qb, table))
    low = qkv.dtype != torch.float32
    with torch.autocast("cuda", dtype=qkv.dtype if low else BF16, enabled=low):
        y, keep, _ = torch.ops.msunet.window_attention(q, b, t, nh, shift, p, seed, seed_dev)
    assert y.dtype == qkv.dtype
    y.backward(dy)
    torch.cuda.synchronize()
    return y.detach(), q.grad, b.grad, t.grad, keep


# ------------------------------------------------------------------------------------------
# a. stored keep bits == host mask
S1, S2, S3, S4 = (2, 8, 8, 1), (1, 10, 12, 2), (2, 30, 33, 3), (1, 58, 58, 32)
# dtype, shift, p, seed, (B, H, W, nh): every value of every axis at least once, each shape with
# both seeds and both shifts, the 32-head shape with the seed above 2^32
KEEP_CASES = [
    (BF16, 0, 0.05, 4321, S1),
    (F16, 3, 0.25, BIG_SEED, S1),
    (BF16, 3, 0.5, 4321, S2),
    (F16, 0, 0.05, BIG_SEED, S2),
    (BF16, 3, 0.25, BIG_SEED, S3),
    (F16, 0, 0.5, 4321, S3),
    (F16, 3, 0.05, 4321, S3),
    (BF16, 3, 0.05, BIG_SEED, S4),
    (F16, 0, 0.5, BIG_SEED, S4),
    (BF16, 0, 0.25, 4321, S4),
]


@pytest.mark.parametrize("low,shift,p,seed,shape", KEEP_CASES,
                         ids=[f"{DT_ID[c[0]]}-s{c[1]}-p{c[2]}-seed{c[3]}-{'x'.join(map(str, c[4]))}"
                              for c in KEEP_CASES])
def test_keep_bits_equal_host_mask(low, shift, p, seed, shape):
    _ops()
    B, H, W, nh = shape
    qkv, qb, table, _ = _inputs(B, H, W, nh, low, 11 + H)
    with torch.no_grad(), torch.autocast("cuda", dtype=low):
        _, keep, _ = torch.ops.msunet.window_attention(qkv, qb, table, nh, shift, p, seed, None)
    _assert_mask(keep, _nwin(B, H, W) * nh, seed, p)


def _fused_inputs(B, H, W, low, proj):
    C = 96
    g = torch.Generator().manual_seed(5 + H)
    x = torch.randn(B, H, W, C, generator=g).to(DEV, low)
    w = (torch.randn(3 * C, C, generator=g) / C ** 0.5).to(DEV)
    b = (0.3 * torch.randn(3 * C, generator=g)).to(DEV)
    table = torch.randn(169, 3, generator=g).to(DEV)
    wp = (torch.randn(C, C, generator=g) / C ** 0.5).to(DEV) if proj else None
    bp = (0.1 * torch.randn(C, generator=g)).to(DEV) if proj else None
    return x, w, b, table, wp, bp


@pytest.mark.parametrize("proj", [False, True], ids=["attn", "attn_proj"])
@pytest.mark.parametrize("low", [BF16, F16], ids=["bf16", "f16"])
@pytest.mark.parametrize("p,seed", [(0.05, BIG_SEED), (0.5, 4321)])
def test_fused_stage0_keep_bits_equal_host_mask(p, seed, low, proj):
    ops = _ops()
    B, H, W, shift = 2, 28, 28, 3
    x, w, b, table, wp, bp = _fused_inputs(B, H, W, low, proj)
    with torch.no_grad(), torch.autocast("cuda", dtype=low):
        assert ops.window_attention_qkv_fusable(x, 3, b)
        keep = torch.ops.msunet.window_attention_qkv(x, w, b, table, wp, bp, 3, shift, p, seed, None, True)[3]
    _assert_mask(keep, _nwin(B, H, W) * 3, seed, p)


@pytest.mark.parametrize("op", ["attn", "fused", "fused_proj"])
@pytest.mark.parametrize("low", [BF16, F16], ids=["bf16", "f16"])
@pytest.mark.parametrize("k", [0, 7])
def test_keep_bits_with_device_counter(k, low, op):
    """seed_dev: the mask is that of launch_seed(seed, counter), read from the device at launch
    time (an in-place bump changes the next launch), and differs from the counter-less mask."""
    _ops()
    p, seed, shift = 0.25, 4321, 3
    if op == "attn":
        B, H, W, nh = S3
        qkv, qb, table, _ = _inputs(B, H, W, nh, low, 3)

        def fwd(c):
            return torch.ops.msunet.window_attention(qkv, qb, table, nh, shift, p, seed, c)[1]
    else:
        B, H, W, nh = 2, 28, 28, 3
        x, w, b, table, wp, bp = _fused_inputs(B, H, W, low, op == "fused_proj")

        def fwd(c):
            return torch.ops.msunet.window_attention_qkv(x, w, b, table, wp, bp, nh, shift, p, seed, c, True)[3]
    n = _nwin(B, H, W) * nh
    c = torch.tensor([k], dtype=torch.int64, device=DEV)
    with torch.no_grad(), torch.autocast("cuda", dtype=low):
        keep0 = fwd(c)
        c.add_(1)
        keep1 = fwd(c)
    m0 = _assert_mask(keep0, n, seed, p, counter=k)
    m1 = _assert_mask(keep1, n, seed, p, counter=k + 1)
    plain = host_mask(n, seed, p)
    assert not torch.equal(m0, plain) and not torch.equal(m1, plain) and not torch.equal(m0, m1)


# ------------------------------------------------------------------------------------------
# b. 16-bit backward under a counter: stored bits == re-hash == the op's autograd backward
@pytest.mark.parametrize("low", [BF16, F16], ids=["bf16", "f16"])
def test_backward_keep_bits_equal_rehash_with_device_counter(low):
    from semantic_segmentation_of_stylegan2_artifacts_amd import _lib
    ops = _ops()
    B, H, W, nh = S3
    C, shift, p, seed, k = 32 * nh, 3, 0.3, 4321, 5
    qkv, qb, table, dout = _inputs(B, H, W, nh, low, 17)
    c = torch.tensor([k], dtype=torch.int64, device=DEV)
    y, keep, _ = torch.ops.msunet.window_attention(qkv, qb, table, nh, shift, p, seed, c)
    _assert_mask(keep, _nwin(B, H, W) * nh, seed, p, counter=k)
    L = _lib.lib()
    dt = ops._dt(qkv)
    outs = []
    for kp in (keep.data_ptr(), None):
        ws = torch.empty(L.msu_win_attn_bwd_workspace(dt, B, H, W, C, nh), device=DEV)
        dqkv = torch.empty_like(qkv)
        dtab = torch.empty_like(table)
        dbias = torch.empty(3 * C, device=DEV)
        _lib.call("msu_win_attn_bwd", dt, qkv.data_ptr(), qb.data_ptr(), table.data_ptr(), dout.data_ptr(),
                  dqkv.data_ptr(), dtab.data_ptr(), dbias.data_ptr(), ws.data_ptr(), B, H, W, C, nh, shift, p,
                  seed, c.data_ptr(), kp, torch.cuda.current_stream().cuda_stream)
        outs.append((dqkv, dtab, dbias))
    torch.cuda.synchronize()
    for what, a, b in zip(("dqkv", "dtable", "dbias"), *outs):
        assert torch.equal(a, b), what
    q = qkv.clone().requires_grad_(True)
    with torch.autocast("cuda", dtype=low):
        y2 = ops.window_attention(q, qb, table, nh, shift, p, seed, c)
    assert torch.equal(y2, y)
    y2.backward(dout)
    assert torch.equal(q.grad, outs[0][0])


# ------------------------------------------------------------------------------------------
# c. f32 kernels with dropout against float64
def _f32_case(B, H, W, nh, shift, p, seed, counter=None):
    """Measured on an MI355X over the cases below: max error <= 8.3e-7 max|ref| (d table; out,
    dqkv and d qkv bias <= 3.9e-7) against the 1e-4 of test_window_attention_fp32."""
    qkv, qb, table, dy = _inputs(B, H, W, nh, torch.float32, B * H * W + nh)
    c = None if counter is None else torch.tensor([counter], dtype=torch.int64, device=DEV)
    y, dq, db, dt, keep = _run(qkv, qb, table, dy, nh, shift, p, seed, c)
    assert keep.numel() == 0  # the f32 kernels store no bits: forward and backward re-hash
    mask = host_mask(_nwin(B, H, W) * nh, seed, p, counter)
    yr, dqr, dbr, dtr = _ref64(qkv, qb, table, dy, nh, shift, mask, p)
    for what, a, r in (("out", y, yr), ("dqkv", dq, dqr), ("d qkv bias", db, dbr), ("d table", dt, dtr)):
        scale = r.abs().max().item()
        print(f"f32 {what}: max err {(a.double() - r).abs().max().item():.3e}, scale {scale:.3e}")
    _close(y, yr, 1e-4, 1e-5, "out")
    _close(dq, dqr, 1e-4, 1e-5, "dqkv")
    _close(db, dbr, 1e-4, 1e-5, "d qkv bias (padded tokens)")
    _close(dt, dtr, 1e-4, 1e-5, "d relative_position_bias_table")


@pytest.mark.parametrize("B,H,W,nh,shift", ATTN_CASES)
def test_f32_dropout_matches_fp64(B, H, W, nh, shift):
    _f32_case(B, H, W, nh, shift, 0.3, 77)


def test_f32_dropout_matches_fp64_block_loop():
    """81 windows on 2048 / 32 = 64 backward blocks: the block loop and its carried partials."""
    _f32_case(1, 58, 58, 32, 3, 0.05, 77)


def test_f32_dropout_matches_fp64_device_counter():
    _f32_case(1, 10, 12, 2, 3, 0.3, 77, counter=3)


# ------------------------------------------------------------------------------------------
# d. 16-bit kernels at the production head counts
def _head_blocks(need, cap):
    """csrc/window_attention_mfma.hip head_blocks restated: min(need, cap) up to a multiple of 8."""
    cap = max(8, cap // 8 * 8)
    return (min(need, cap) + 7) // 8 * 8


def _capacities(nwin, nh):
    """Windows the persistent grids hold at once: forward waves 4 head_blocks(ceil(nwin / 4),
    512 / nh), backward workgroups head_blocks(nwin, 1024 / nh)."""
    return 4 * _head_blocks((nwin + 3) // 4, 512 // nh), _head_blocks(nwin, 1024 // nh)


# nh: (B, H, W), windows, forward waves, backward workgroups.  Each map is padded (H % 7 != 0) and
# has more windows than both capacities, so the next-window prefetch and the register-carried
# table gradient run:
#    4: 23^2 = 529 > 4 * 128 = 512 (cap 512 / 4 = 128), 1024 / 4 = 256
#    8: 17^2 = 289 > 4 *  64 = 256,                      1024 / 8 = 128
#   12: 13^2 = 169 > 4 *  40 = 160 (42 -> 40),           85 -> 80
#   16: 12^2 = 144 > 4 *  32 = 128,                      64
#   24:  9^2 =  81 > 4 *  16 =  64 (21 -> 16),           42 -> 40
#   32:  9^2 =  81 > 4 *  16 =  64,                      32
# No side is 7 k + 3: with shift 3 the 4 padded rows / columns of such a map are exactly the
# shift mask's middle region, only padded queries attend to padded keys, and the qkv-bias gradient
# is identically zero (80 x 80 at 16 heads, also 12 x 12 windows, gave max|ref| = 1e-13 in
# float64 and exact zeros from the kernel): nothing to scale the error with, hence 81.
PROD_HEADS = {
    4: ((1, 160, 160), 529, 512, 256),
    8: ((1, 114, 114), 289, 256, 128),
    12: ((1, 90, 90), 169, 160, 80),
    16: ((1, 81, 81), 144, 128, 64),
    24: ((1, 58, 58), 81, 64, 40),
    32: ((1, 58, 58), 81, 64, 32),
}
# nh, shift, p: shift 3 everywhere, shift 0 for the first and last rows, p = 0 (the DROP = false
# instantiation) at 32 and 16 heads
PROD_CASES = [(4, 3, 0.05), (4, 0, 0.05), (8, 3, 0.05), (12, 3, 0.05), (16, 3, 0.05), (24, 3, 0.05),
              (32, 3, 0.05), (32, 0, 0.05), (32, 3, 0.0), (16, 3, 0.0)]


def _stats(y, ref, dim):
    """max error / max|ref| and relative L2 per slice along ``dim`` (printed before the asserts)."""
    d = (y.double() - ref).movedim(dim, 0).flatten(1)
    r = ref.movedim(dim, 0).flatten(1)
    return (d.abs().amax(1) / r.abs().amax(1)).max().item(), (d.norm(dim=1) / r.norm(dim=1)).max().item()


@pytest.mark.parametrize("low", [BF16, F16], ids=["bf16", "f16"])
@pytest.mark.parametrize("nh,shift,p", PROD_CASES)
def test_production_heads_match_fp64(nh, shift, p, low):
    """Stored keep bits == host mask first, then out / dqkv / d table / d qkv bias against float64
    with that mask, whole and head by head.  Measured on an MI355X (max error / max|ref|,
    relative L2; the per-head worst in brackets): bf16 out and dqkv <= 4.5e-3 (6.2e-3), 2.36e-3
    (2.38e-3) against 3e-2, 7.5e-3; f16 <= 6.0e-4 (7.9e-4), 2.95e-4 (2.98e-4) against 7.5e-3,
    1.9e-3; d table <= 1.3e-4 (3.1e-4); d qkv bias <= 1.5e-3."""
    (B, H, W), nwin, fwd_waves, bwd_blocks = PROD_HEADS[nh]
    assert _nwin(B, H, W) == nwin and H % 7 not in (0, 3) and W % 7 not in (0, 3)
    assert _capacities(nwin, nh) == (fwd_waves, bwd_blocks) and nwin > max(fwd_waves, bwd_blocks)
    seed = 4321 + nh
    qkv, qb, table, dy = _inputs(B, H, W, nh, low, 100 * nh + shift + int(p * 100))
    y, dq, db, dt, keep = _run(qkv, qb, table, dy, nh, shift, p, seed)
    mask = _assert_mask(keep, nwin * nh, seed, p) if p > 0 else None
    yr, dqr, dbr, dtr = _ref64(qkv, qb, table, dy, nh, shift, mask, p)

    t = TOL[low]
    yh, yrh = y.view(B, H, W, nh, 32), yr.view(B, H, W, nh, 32)
    dqh, dqrh = dq.view(B, H, W, 3, nh, 32), dqr.view(B, H, W, 3, nh, 32)
    for what, a, r, dim in (("out", yh, yrh, 3), ("dqkv", dqh, dqrh, 4), ("d table", dt, dtr, 1)):
        whole = _stats(a.reshape(1, -1), r.reshape(1, -1), 0)
        head = _stats(a, r, dim)
        print(f"{what}: max err / scale {whole[0]:.3e} (worst head {head[0]:.3e}), relative L2 {whole[1]:.3e} "
              f"(worst head {head[1]:.3e}); bounds {t:.1e}, {t / 4:.1e}")
    print("d qkv bias: max err / scale %.3e, relative L2 %.3e" % _stats(db.reshape(1, -1), dbr.reshape(1, -1), 0))

    _check(y, yr, t, "out")
    _check(dq, dqr, t, "dqkv")
    _check(dt, dtr, t, "d relative_position_bias_table")
    _check(db, dbr, t, "d qkv bias (padded tokens)")
    for h in range(nh):
        _check(yh[..., h, :], yrh[..., h, :], t, f"out, head {h}")
        _check(dqh[..., h, :], dqrh[..., h, :], t, f"dqkv, head {h}")
        _check(dt[:, h], dtr[:, h], t, f"d table, head {h}")
