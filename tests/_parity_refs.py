"""Plain fp32 PyTorch references shared by the GPU parity tests (test infrastructure only).

* ``attn_ref_from_qkv``: torchvision v1 ``shifted_window_attention`` (restated in
  oracle/swin_block.py, which cites it) driven by the post-Linear qkv of the real tokens, with
  an optional dropout keep mask on the softmax probabilities (``F.dropout`` after the softmax,
  kept values scaled by 1 / (1 - p)).
* ``decode_keep_bits``: the 16-bit attention forward's stored keep bits
  (csrc/window_attention_mfma.hip, ``[window x head][query tile][lane]`` words; bit jt*16 + r of
  lane l in tile it <-> query 32 it + (l & 31), key 32 jt + crow(r, l >> 5)) -> [items, 49, 49].
  What those bits should be is restated on the host in ``tests/_attn_mask_ref.py``
  (``keep_mask``: the dropout streams of csrc/common.h in numpy, same [items, 49, 49] layout);
  tests/test_gpu_attn_dropout.py compares the two and evaluates ``attn_ref_from_qkv`` in float64
  with the host mask.
* ``conv3x3_ref``: ``conv2d(a, W, b, padding=1)`` on NHWC tensors as nine shifted fp32
  matmuls (autograd gives dA, dW, db), so the 1024^2 references need neither the CPU nor a
  library convolution.
* ``conv3x3_ref64`` / ``conv3x3_abs64`` / ``conv3x3_wgrad_ref64`` / ``conv3x3_wgrad_abs64`` /
  ``gelu64`` / ``gelu_grad64``: the refine-conv family in float64 with its condition terms
  (tests/test_gpu_conv_matrix.py judges every kernel of csrc/conv3x3.h against them).
* ``gemm_ref64`` / ``gemm_abs64``: a . w^T + b in float64 and its condition term (with ``gelu64`` /
  ``gelu_grad64``: what tests/test_gpu_gemm_matrix.py judges the token GEMM, the NT GEMM and the
  one-pass Linear backward against).
* ``ln_plain_ref`` / ``ln_add_ref`` / ``ln_merge_ref`` / ``ln_d2s2_ref`` / ``ln_head_ref``: the
  four input modes of csrc/layernorm.hip and its 1-channel head in float64 (the one exception to
  "fp32" above: tests/test_gpu_ln_matrix.py judges f32 kernels against them).
"""
import math

import torch
import torch.nn.functional as F

from oracle import swin_block as osb


def gelu_grad(h):
    return 0.5 * (1.0 + torch.erf(h / math.sqrt(2.0))) + h * torch.exp(-0.5 * h * h) / math.sqrt(2.0 * math.pi)


def decode_keep_bits(keep, n_items):
    """[n_items * 128] int32 keep words -> bool [n_items, 49, 49] (query, key)."""
    dev = keep.device
    it, lane, b = torch.meshgrid(torch.arange(2), torch.arange(64), torch.arange(32), indexing="ij")
    r = b & 15
    i = (32 * it + (lane & 31)).reshape(-1).to(dev)
    j = (32 * (b >> 4) + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)).reshape(-1).to(dev)
    bits = ((keep.view(n_items, 2, 64, 1) >> torch.arange(32, device=dev, dtype=torch.int32)) & 1).bool()
    full = torch.zeros(n_items, 64, 64, dtype=torch.bool, device=dev)
    full[:, i, j] = bits.reshape(n_items, -1)
    return full[:, :49, :49]


def attn_ref_from_qkv(qkv, qkv_bias, table, nh, shift, keep=None, p_drop=0.0):
    """torchvision semantics given the post-Linear qkv of real tokens; padded tokens take
    qkv_bias (= Linear of the zero pad).  keep: bool [windows * nh, 49, 49] dropout mask in the
    kernels' (window, head) item order, or None."""
    B, H, W, C3 = qkv.shape
    C = C3 // 3
    ws = 7
    pad_r, pad_b = (ws - W % ws) % ws, (ws - H % ws) % ws
    x = F.pad(qkv - qkv_bias, (0, 0, 0, pad_r, 0, pad_b)) + qkv_bias
    _, pH, pW, _ = x.shape
    _, _, sh = osb.effective_shift(H, W, ws, shift)
    if sum(sh) > 0:
        x = torch.roll(x, shifts=(-sh[0], -sh[1]), dims=(1, 2))
    nW = (pH // ws) * (pW // ws)
    x = x.view(B, pH // ws, ws, pW // ws, ws, C3).permute(0, 1, 3, 2, 4, 5).reshape(B * nW, ws * ws, C3)
    qkv_ = x.reshape(x.size(0), x.size(1), 3, nh, C // nh).permute(2, 0, 3, 1, 4)
    q, k, v = qkv_[0] * (C // nh) ** -0.5, qkv_[1], qkv_[2]
    attn = q.matmul(k.transpose(-2, -1)) + osb.relative_position_bias(table, index_for(table.device), ws)
    if sum(sh) > 0:
        mask = osb.shift_mask(pH, pW, ws, sh).to(attn.device)
        attn = attn.view(B, nW, nh, ws * ws, ws * ws) + mask.unsqueeze(1).unsqueeze(0)
        attn = attn.view(-1, nh, ws * ws, ws * ws)
    attn = torch.softmax(attn, -1)
    if keep is not None:
        attn = attn * keep.view(attn.shape).to(attn.dtype) * (1.0 / (1.0 - p_drop))
    o = attn.matmul(v).transpose(1, 2).reshape(B * nW, ws * ws, C)
    o = o.view(B, pH // ws, pW // ws, ws, ws, C).permute(0, 1, 3, 2, 4, 5).reshape(B, pH, pW, C)
    if sum(sh) > 0:
        o = torch.roll(o, shifts=(sh[0], sh[1]), dims=(1, 2))
    return o[:, :H, :W, :]


_INDEX = {}


def index_for(device):
    key = str(device)
    if key not in _INDEX:
        _INDEX[key] = osb.relative_position_index(7).to(device)
    return _INDEX[key]


def conv3x3_ref(a, w, b):
    """a: [B, H, W, Cin] f32, w: [Cout, Cin, 3, 3], b: [Cout] -> [B, H, W, Cout] (padding 1)."""
    B, H, W, _ = a.shape
    ap = F.pad(a, (0, 0, 1, 1, 1, 1))
    z = b.view(1, 1, 1, -1).expand(B, H, W, -1)
    for dy in range(3):
        for dx in range(3):
            z = z + ap[:, dy:dy + H, dx:dx + W, :].matmul(w[:, :, dy, dx].t())
    return z


def d2s4(x, C):
    """FinalPatchExpand_X4_V2's rearrange 'b h w (p1 p2 c) -> b (h p1) (w p2) c' (p = 4)."""
    B, h, w, _ = x.shape
    return x.view(B, h, w, 4, 4, C).permute(0, 1, 3, 2, 4, 5).reshape(B, 4 * h, 4 * w, C)


# ----------------------------------------------------------------------------- refine-conv family
# fp64 references of csrc/conv3x3.h (tests/test_gpu_conv_matrix.py), evaluated on the operands'
# device and fed exactly the stored operands.  No library convolution: nine shifted, zero-padded
# slices, one torch.matmul each.
def d2s4_rearrange(x, C):
    """The pre-depth-to-space tensor [B, H/4, W/4, 16 C] as the image [B, H, W, C], through the
    rearrange the conv tests use."""
    from einops import rearrange
    return rearrange(x, "b h w (p1 p2 c) -> b (h p1) (w p2) c", p1=4, p2=4, c=C)


def gelu64(x):
    x = x.double()
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def gelu_grad64(x):
    x = x.double()
    return 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def _shifted(a):
    """The nine zero-padded shifts of a [B, H, W, C]: ((dy, dx), a[:, y + dy - 1, x + dx - 1, :])."""
    B, H, W, _ = a.shape
    ap = F.pad(a, (0, 0, 1, 1, 1, 1))
    for dy in range(3):
        for dx in range(3):
            yield (dy, dx), ap[:, dy:dy + H, dx:dx + W, :]


def conv3x3_ref64(a, w, b=None, d2s=False):
    """conv2d(a, w, b, padding=1) in float64.  a: [B, H, W, Cin] (d2s: the pre-depth-to-space
    [B, H/4, W/4, 16 Cin]), w: [Cout, Cin, 3, 3], b: [Cout] or None -> [B, H, W, Cout]."""
    w = w.double()
    a = a.double()
    if d2s:
        a = d2s4_rearrange(a, w.shape[1])
    z = torch.zeros(a.shape[:3] + (w.shape[0],), dtype=torch.float64, device=a.device)
    for (dy, dx), s in _shifted(a):
        z += torch.matmul(s, w[:, :, dy, dx].t())
    return z if b is None else z + b.double()


def conv3x3_abs64(a, w, b=None, d2s=False):
    """The same sum over absolute values: the condition term A = sum |a| |w| + |b| of every output."""
    return conv3x3_ref64(a.double().abs(), w.double().abs(), None if b is None else b.double().abs(), d2s)


def conv3x3_dgrad_weight(w):
    """The weight whose conv3x3 of dz is the input gradient: [Cin, Cout, 3, 3], taps flipped."""
    return w.flip(2, 3).transpose(0, 1).contiguous()


def conv3x3_wgrad_ref64(a, dz, dtype=torch.float64):
    """(dW [Cout, Cin, 3, 3], db [Cout]) of z = conv3x3(a, W) + b: the nine a_shifted^T @ dz
    products over all pixels.  a: the conv's input image [B, H, W, Cin] (already float64), dz:
    [B, H, W, Cout].  dtype = float32 evaluates the same products with the float64 operands cast
    to f32 (the figure the sum tolerance of the conv matrix is derived from)."""
    Cin, Cout = a.shape[-1], dz.shape[-1]
    d = dz.double().to(dtype).reshape(-1, Cout)
    dw = torch.empty(Cout, Cin, 3, 3, dtype=dtype, device=a.device)
    for (dy, dx), s in _shifted(a.double().to(dtype)):
        dw[:, :, dy, dx] = torch.matmul(s.reshape(-1, Cin).t(), d).t()
    return dw, d.sum(0)


def conv3x3_wgrad_abs64(a, dz):
    """sum_pixels |a| |dz| per weight element and sum_pixels |dz| per bias element."""
    return conv3x3_wgrad_ref64(a.double().abs(), dz.double().abs())


# ----------------------------------------------------------------------------- GEMM family
# fp64 references of csrc/gemm_tok.h, gemm_nt.hip, gemm_pp.h and gemm_linbwd.hip
# (tests/test_gpu_gemm_matrix.py), evaluated on the operands' device on exactly the stored operands.
def gemm_ref64(a, w, b=None, dtype=torch.float64):
    """a [M, K] . w [N, K]^T (+ b [N]) -> [M, N] in float64.  dtype = float32 evaluates the same
    matmul with the float64 operands cast to f32 (the figure the GEMM matrix derives kappa from)."""
    y = torch.matmul(a.double().to(dtype), w.double().to(dtype).t())
    return y if b is None else y + b.double().to(dtype)


def gemm_abs64(a, w, b=None):
    """The same over absolute values: the condition term sum |a| |w| + |b| of every output."""
    return gemm_ref64(a.double().abs(), w.double().abs(), None if b is None else b.double().abs())


# ----------------------------------------------------------------------------- LayerNorm family
# fp64 references of csrc/layernorm.hip, one per input mode, evaluated on the tensors' device.
# Each takes what the kernel takes, already rounded to the storage type, and returns a dict of
# fp64 tensors: y, mean, rstd, the LayerNorm input rows ``xr`` [rows, C] (for the error bounds)
# and, through autograd, dx (in the source layout), dgamma, dbeta (+ db / s in add mode).
def _ln64(xr, gamma, beta, eps):
    mean = xr.mean(-1, keepdim=True)
    var = ((xr - mean) ** 2).mean(-1, keepdim=True)
    rstd = (var + eps).rsqrt()
    return (xr - mean) * rstd * gamma + beta, mean.squeeze(-1), rstd.squeeze(-1)


def _ln_mode_ref(build_rows, srcs, gamma, beta, dy, eps, extra=None):
    """build_rows(*fp64 leaves) -> (LayerNorm input rows [rows, C], dict of extra outputs)."""
    leaves = [s.detach().double().requires_grad_(True) for s in srcs]
    g = gamma.detach().double().requires_grad_(True)
    b = beta.detach().double().requires_grad_(True)
    xr, out = build_rows(*leaves)
    y, mean, rstd = _ln64(xr, g, b, eps)
    out.update(y=y.detach(), mean=mean.detach(), rstd=rstd.detach(), xr=xr.detach())
    if dy is not None:
        loss = (y * dy.detach().double().reshape(y.shape)).sum()
        if extra is not None:
            loss = loss + extra(xr)
        grads = torch.autograd.grad(loss, leaves + [g, b])
        out.update(grads=[t.detach() for t in grads[:-2]], dgamma=grads[-2].detach(), dbeta=grads[-1].detach())
    return out


def ln_plain_ref(x, gamma, beta, dy=None, eps=1e-5, dres=()):
    """LayerNorm over the last dim; dres: further gradients of x (summed into dx)."""
    C = x.shape[-1]
    extra = (lambda xr: sum((xr * r.detach().double().reshape(-1, C)).sum() for r in dres)) if dres else None
    out = _ln_mode_ref(lambda xs: (xs.reshape(-1, C), {}), [x], gamma, beta, dy, eps, extra)
    if dy is not None:
        out["dx"] = out.pop("grads")[0]
    return out


def ln_add_ref(a, b, scale, rows_per_sample, gamma, beta, dy=None, eps=1e-5, dres=(), s=None):
    """s = a + scale[row // rows_per_sample] * b, y = LN(s).  The kernel rounds s to the storage
    type and normalises that rounded value: given the kernel's own ``s``, y and the backward are
    evaluated at it (its gradient still flows to a and b), while ``s`` of the result stays the
    exact fp64 sum.  b / scale may be None (s = a / scale 1)."""
    C = a.shape[-1]
    rows = a.numel() // C
    sc = None
    if scale is not None:
        idx = torch.arange(rows, device=a.device) // rows_per_sample
        sc = scale.detach().double()[idx].unsqueeze(-1)
    srcs = [a] if b is None else [a, b]

    def build(a64, b64=None):
        s64 = a64.reshape(-1, C)
        if b64 is not None:
            s64 = s64 + (b64.reshape(-1, C) if sc is None else sc * b64.reshape(-1, C))
        used = s64 if s is None else s64 + (s.detach().double().reshape(-1, C) - s64).detach()
        return used, {"s": s64.detach()}

    extra = (lambda xr: sum((xr * r.detach().double().reshape(-1, C)).sum() for r in dres)) if dres else None
    out = _ln_mode_ref(build, srcs, gamma, beta, dy, eps, extra)
    out["scale_rows"] = sc
    if dy is not None:
        grads = out.pop("grads")
        out["dx"] = grads[0]
        out["db"] = grads[1] if b is not None else (grads[0] if sc is None else grads[0].reshape(-1, C) * sc)
    return out


def merge_rows(x):
    """PatchMerging's gather: [B, H, W, Cin] -> [B * H/2 * W/2, 4 Cin] in x0, x1, x2, x3 order."""
    B, H, W, Cin = x.shape
    assert H % 2 == 0 and W % 2 == 0
    x0, x1, x2, x3 = x[:, 0::2, 0::2], x[:, 1::2, 0::2], x[:, 0::2, 1::2], x[:, 1::2, 1::2]
    return torch.cat([x0, x1, x2, x3], -1).reshape(-1, 4 * Cin)


def d2s2_rows(x):
    """PatchExpand's rearrange 'b h w (p1 p2 c) -> b (h p1) (w p2) c' (p = 2) as view / permute:
    [B, H, W, 4c] -> [B * 2H * 2W, c]."""
    B, H, W, C4 = x.shape
    c = C4 // 4
    return x.reshape(B, H, W, 2, 2, c).permute(0, 1, 3, 2, 4, 5).reshape(-1, c)


def ln_merge_ref(x, gamma, beta, dy=None, eps=1e-5):
    out = _ln_mode_ref(lambda xs: (merge_rows(xs), {}), [x], gamma, beta, dy, eps)
    if dy is not None:
        out["dx"] = out.pop("grads")[0]
    return out


def ln_d2s2_ref(x, gamma, beta, dy=None, eps=1e-5):
    out = _ln_mode_ref(lambda xs: (d2s2_rows(xs), {}), [x], gamma, beta, dy, eps)
    if dy is not None:
        out["dx"] = out.pop("grads")[0]
    return out


def ln_head_ref(z, gamma, beta, w, dlogit=None, eps=1e-5):
    """logit[r] = <LN(z[r]), w> (the 1-channel output head); dz, dgamma, dbeta, dw by autograd."""
    C = z.shape[-1]
    z64 = z.detach().double().reshape(-1, C).requires_grad_(True)
    g, b, w64 = (t.detach().double().reshape(-1).requires_grad_(True) for t in (gamma, beta, w))
    y, mean, rstd = _ln64(z64, g, b, eps)
    logit = (y * w64).sum(-1)
    out = dict(logit=logit.detach(), mean=mean.detach(), rstd=rstd.detach(), xr=z64.detach(), y=y.detach())
    if dlogit is not None:
        dz, dg, db, dw = torch.autograd.grad((logit * dlogit.detach().double().reshape(-1)).sum(), (z64, g, b, w64))
        out.update(dz=dz, dgamma=dg, dbeta=db, dw=dw)
    return out
