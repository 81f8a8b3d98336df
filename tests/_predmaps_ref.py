"""Float64 numpy restatement of what ``msu_pred_maps`` computes (TEST INFRASTRUCTURE ONLY),
and the seeded inputs of the prediction-map tests.

Inputs: logits are multiples of 1/8 in [-8, 8] without 0 (exact in bf16 and f16).  For every
such logit p = sigmoid(logit) lies >= 7e-3 from the mask threshold 0.4, >= 3e-2 from 0.5,
>= 3e-3 levels from a rounding boundary of ``heat`` and >= 1e-2 from a colormap-index boundary,
so an f32 fast-exp sigmoid cannot flip a byte (``test_logit_grid_margins`` re-checks this).
Images are uniform random bytes / 255, as the dataset makes them.
"""
import functools

import numpy as np
import torch

from oracle.dynamic_loss import dynamic_loss

COLOR = (255, 0, 255)
LOSS = dict(alpha=0.2, beta=0.8, mix=0.45)


def lut64():
    """Closed form of matplotlib's table for from_list("g2r", [(0, green), (.5, yellow), (1, red)])."""
    t = np.arange(256, dtype=np.float64) / 255.0
    g0 = 128.0 / 255.0
    lo = t <= 0.5
    return np.stack([np.where(lo, 2 * t, 1.0), np.where(lo, g0 + (1 - g0) * 2 * t, 2 - 2 * t), np.zeros(256)], 1)


def outline_band(M):
    """Pixels of M [B, H, W] (bool) whose 3x3 neighbourhood holds a true and a false M (false
    outside the image)."""
    B, H, W = M.shape
    pad = np.zeros((B, H + 2, W + 2), dtype=bool)
    pad[:, 1:-1, 1:-1] = M
    any_ = np.zeros_like(M)
    all_ = np.ones_like(M)
    for dy in range(3):
        for dx in range(3):
            v = pad[:, dy:dy + H, dx:dx + W]
            any_ |= v
            all_ &= v
    return any_ & ~all_


def reference(logits, image=None, label=None, sig_threshold=0.5, mask_threshold=0.4, heat_alpha=0.45,
              mask_alpha=0.25, color=COLOR, outline=True, loss=LOSS):
    """logits [B, 1, H, W] (torch, any float dtype), image [B, 3, H, W], label [B, H, W] ->
    dict of numpy arrays; ``heat_rgb_real`` is v * 255 + 0.5 before the floor."""
    x = logits.float().double().numpy()[:, 0]
    B, H, W = x.shape
    p = 1.0 / (1.0 + np.exp(-x))
    out = {"prob": p, "heat": np.floor(np.clip(p, 0, 1) * 255 + 0.5).astype(np.uint8)}
    M = p > mask_threshold
    out["mask"] = np.where(M, 255, 0).astype(np.uint8)
    if image is not None:
        img = image.double().numpy().transpose(0, 2, 3, 1)  # [B, H, W, 3]
        u = np.floor(img * 255 + 0.5)
        idx = np.minimum((p * 256).astype(np.int64), 255)
        v = np.clip((1 - heat_alpha) * img + heat_alpha * lut64()[idx], 0, 1)
        out["heat_rgb_real"] = v * 255 + 0.5
        out["heat_rgb"] = np.floor(out["heat_rgb_real"]).astype(np.uint8)
        col = np.array(color, dtype=np.float64)
        blend = (u * (1 - mask_alpha) + col * mask_alpha).astype(np.uint8)  # truncation
        m = np.where(M[..., None], blend, u.astype(np.uint8))
        if outline:
            m = np.where(outline_band(M)[..., None], col.astype(np.uint8), m)
        out["mask_rgb"] = m.astype(np.uint8)
    pb = p > sig_threshold
    sums = np.zeros((B, 12))
    sums[:, 1] = (p * p).sum((1, 2))
    sums[:, 3] = p.sum((1, 2))
    if label is None:
        sums[:, 8] = pb.sum((1, 2))
    else:
        gb = label.reshape(B, H, W).numpy() > 0
        g = gb.astype(np.float64)
        cols = [p * g, p * p, g, p, (1 - g) * p, g * (1 - p), (1 - p) * (1 - g), pb & gb, pb & ~gb, ~pb & gb,
                ~pb & ~gb, np.maximum(x, 0) - x * g + np.log1p(np.exp(-np.abs(x)))]
        for k, c in enumerate(cols):
            sums[:, k] = c.sum((1, 2), dtype=np.float64)
        out["loss"] = np.array([float(dynamic_loss(logits[b:b + 1].float(), label.reshape(B, H, W)[b:b + 1].float(),
                                                   loss["alpha"], loss["beta"], loss["mix"])) for b in range(B)])
    out["sums"] = sums
    return out


def grid_logits(shape, g):
    """Multiples of 1/8 in [-8, 8], 0 excluded."""
    k = torch.randint(1, 65, shape, generator=g).float()
    s = torch.randint(0, 2, shape, generator=g).float() * 2 - 1
    return k * s / 8.0


def byte_image(B, H, W, g):
    return torch.randint(0, 256, (B, 3, H, W), generator=g).float() / 255.0


@functools.lru_cache(maxsize=None)
def random_case(B, H, W, seed=3):
    """(logits f32 [B, 1, H, W], image, label) of a seeded case: image 0 has an empty label
    ('real'), the others ~30 % positives.  The heat_rgb check needs >= 90 % of the oracle's
    values >= 1e-3 from a rounding boundary: a property of the inputs alone (expected share
    95.4 %), which a case of a few pixels can miss by chance; seed 3 meets it at every shape the
    tests use (worst 93.3 %, seeds 0-5 tried on the CPU)."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * B + 131 * H + W)
    logits = grid_logits((B, 1, H, W), g)
    image = byte_image(B, H, W, g)
    label = (torch.rand(B, H, W, generator=g) < 0.3).float()
    if B > 1:
        label[0] = 0
    return logits, image, label


MASK_KINDS = ("empty", "full", "corners", "seam_lines", "hole", "checkerboard", "edge_blobs")


def structured_mask(kind, H, W, tile=(16, 64)):
    M = np.zeros((H, W), dtype=bool)
    th, tw = tile
    if kind == "full":
        M[:] = True
    elif kind == "corners":
        M[0, 0] = M[0, W - 1] = M[H - 1, 0] = M[H - 1, W - 1] = True
    elif kind == "seam_lines":  # one-pixel lines on both sides of every tile seam
        for y in range(th, H, th):
            M[y - 1, ::3] = True
            M[y, 1::3] = True
        for x in range(tw, W, tw):
            M[::3, x - 1] = True
            M[2::3, x] = True
    elif kind == "hole":
        M[2:H - 2, 2:W - 2] = True
        M[H // 2, W // 2] = False
        M[min(16, H - 3), min(64, W - 3)] = False  # and one on a tile corner
    elif kind == "checkerboard":
        M[::2, ::2] = True
        M[1::2, 1::2] = True
    elif kind == "edge_blobs":  # a blob touching each image edge
        M[0:3, W // 2 - 2:W // 2 + 3] = True
        M[H - 3:H, W // 3:W // 3 + 4] = True
        M[H // 2 - 2:H // 2 + 2, 0:3] = True
        M[H // 3:H // 3 + 5, W - 2:W] = True
    elif kind != "empty":
        raise ValueError(kind)
    return M


@functools.lru_cache(maxsize=None)
def structured_case(kind, H, W):
    """Grid logits whose mask (p > 0.4) is ``structured_mask(kind)``: a positive multiple of 1/8
    inside, at most -5/8 outside (sigmoid(-5/8) = 0.349 < 0.4)."""
    g = torch.Generator().manual_seed(len(kind) * 977 + H * 31 + W)
    M = torch.from_numpy(structured_mask(kind, H, W))
    mag = torch.randint(1, 60, (H, W), generator=g).float() / 8.0
    logits = torch.where(M, mag, -(mag + 0.5)).reshape(1, 1, H, W)
    image = byte_image(1, H, W, g)
    label = (torch.rand(1, H, W, generator=g) < 0.3).float()
    return logits, image, label
