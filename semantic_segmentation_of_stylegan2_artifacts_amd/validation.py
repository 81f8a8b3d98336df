"""Validation metrics of ``scripts/validation_functions.py`` computed on the GPU.

The reference loops over single images, moves every prediction to the host and calls medpy
(``calculate_metrics`` :37-178, ``calculate_metrics_real`` :214-244, ``calculate_metrics_fake``
:247-309).  Here one HIP pass (``msu_seg_metrics``) reduces a whole batch of logits to per-image
sums; only ``[B, 12]`` doubles come back, and the formulas below are the reference's:

* an image is "real" when its ground truth is empty (``:111``), else "fake";
* fake: binary Dice / IoU / recall / precision with medpy's published definitions
  (``dc`` = 2|A&B| / (|A| + |B|), 0 when both are empty; ``jc`` = |A&B| / |A|B|; recall /
  precision 0 on an empty denominator), ``bin_f1`` with smooth 1e-8 (``:264``), soft Dice
  (``:300-301``) and soft IoU (``:304``) with smooth 1e-8;
* real: FPR = fp / (fp + tn) (``:235``);
* both: binary accuracy and the binary / soft confusion matrices;
* ``Score = mean_soft_dice - 10 * mean_FPR`` (``:180``).

Every binary metric above is tied to one threshold.  ``threshold_histogram`` (``msu_seg_sweep``)
counts, in one more pass over the same logits, how many of K ascending thresholds each pixel's
probability exceeds; ``sweep_counts`` turns that into the (tp, fp, fn, tn) of every threshold,
``summarize_sweep`` into the epoch means per threshold and the pooled pixel ROC / PR curves, and
``select_threshold`` picks an operating point.  ``evaluate(..., sweep=thresholds)`` does all of it.
"""
import math

import numpy as np
import torch

from . import _lib, ops

SMOOTH = 1e-8

# column order of msu_seg_metrics' output rows
COLS = ("inter", "sum_p2", "sum_g", "sum_p", "soft_fp", "soft_fn", "soft_tn", "tp", "fp", "fn", "tn")


def image_sums(logits, labels, threshold=0.5):
    """Per-image metric sums on the GPU: logits [B, 1, H, W] (f32 / bf16 / f16), labels [B, H, W]
    or [B, 1, H, W] -> float64 tensor [B, 12] (host)."""
    ops._need_cuda(logits, labels)
    B = logits.shape[0]
    if labels.shape[0] != B:
        raise ValueError(f"batch mismatch: logits {B}, labels {labels.shape[0]}")
    x = logits.contiguous()
    if x.dtype not in (torch.float32, torch.bfloat16, torch.float16):
        x = x.float()
    lab = ops._f32(labels)
    N = x[0].numel()
    if lab[0].numel() != N:
        raise ValueError(f"label size {tuple(labels.shape)} does not match logits {tuple(logits.shape)}")
    L = _lib.lib()
    nblk = L.msu_metrics_nblk(N)
    part = torch.empty(B * nblk * 12, device=x.device, dtype=torch.float32)
    out = torch.empty(B, 12, device=x.device, dtype=torch.float64)
    _lib.call("msu_seg_metrics", ops._dt(x), ops._p(x), ops._p(lab), B, N, float(threshold), ops._p(part), nblk,
              ops._p(out), ops._s(x))
    return out.cpu()


def binary_metrics(tp, fp, fn, tn):
    """The threshold-dependent half of an image's metrics from its confusion counts (reference
    formulas, see module doc): ``accuracy`` and ``real`` for every image, ``fpr`` for a real one
    (no positive ground-truth pixel), ``bin_dice``, ``bin_iou``, ``recall``, ``precision`` and
    ``bin_f1`` for a fake one."""
    tp, fp, fn, tn = int(tp), int(fp), int(fn), int(tn)
    total = tp + fp + fn + tn
    if total <= 0:
        raise ValueError(f"metric calculation failed because total = {total}")
    m = {"accuracy": (tp + tn) / total, "real": tp + fn == 0}
    if m["real"]:
        m["fpr"] = fp / (fp + tn)
        return m
    m["bin_dice"] = 2.0 * tp / (2 * tp + fp + fn) if (2 * tp + fp + fn) > 0 else 0.0
    m["bin_iou"] = tp / (tp + fp + fn)
    m["recall"] = tp / (tp + fn) if (tp + fn) > 0 else 0.0
    m["precision"] = tp / (tp + fp) if (tp + fp) > 0 else 0.0
    m["bin_f1"] = 2 * (m["precision"] * m["recall"]) / (m["precision"] + m["recall"] + SMOOTH)
    return m


def metrics_from_sums(row):
    """One image's metrics from its ``image_sums`` row (reference formulas, see module doc)."""
    c = {k: float(v) for k, v in zip(COLS, row.tolist())}
    tp, fp, fn, tn = (int(round(c[k])) for k in ("tp", "fp", "fn", "tn"))
    total = tp + fp + fn + tn
    if total <= 0:
        raise ValueError(f"metric calculation failed because total = {total}")
    m = {"tp": tp, "fp": fp, "fn": fn, "tn": tn, "accuracy": (tp + tn) / total,
         "confusion_matrix_bin": [[tp, fp], [fn, tn]],
         "confusion_matrix_soft": [[c["inter"], c["soft_fp"]], [c["soft_fn"], c["soft_tn"]]],
         "real": c["sum_g"] == 0.0}
    if m["real"]:
        m["fpr"] = fp / (fp + tn)
        return m
    m["bin_dice"] = 2.0 * tp / (2 * tp + fp + fn) if (2 * tp + fp + fn) > 0 else 0.0
    m["bin_iou"] = tp / (tp + fp + fn)
    m["recall"] = tp / (tp + fn) if (tp + fn) > 0 else 0.0
    m["precision"] = tp / (tp + fp) if (tp + fp) > 0 else 0.0
    m["bin_f1"] = 2 * (m["precision"] * m["recall"]) / (m["precision"] + m["recall"] + SMOOTH)
    # sum(g^2) == sum(g) for a binary ground truth
    m["soft_dice"] = (2.0 * c["inter"] + SMOOTH) / (c["sum_p2"] + c["sum_g"] + SMOOTH)
    m["soft_iou"] = (c["inter"] + SMOOTH) / (c["sum_p"] + c["sum_g"] - c["inter"] + SMOOTH)
    return m


def batch_metrics(logits, labels, threshold=0.5):
    """List of per-image metric dicts for a batch (one GPU pass)."""
    return [metrics_from_sums(r) for r in image_sums(logits, labels, threshold)]


def summarize(per_image):
    """Epoch summary of ``calculate_metrics`` (:152-180): mean soft Dice / IoU and binary
    metrics over fake images, mean FPR over real images, Score = soft Dice - 10 * FPR."""
    fake = [m for m in per_image if not m["real"]]
    real = [m for m in per_image if m["real"]]

    def mean(ms, k):
        return sum(m[k] for m in ms) / len(ms) if ms else float("nan")

    out = {k: mean(fake, k) for k in ("soft_dice", "soft_iou", "bin_dice", "bin_iou", "recall", "precision",
                                      "bin_f1", "accuracy")}
    out["mean_fpr"] = mean(real, "fpr")
    out["accuracy_all"] = mean(per_image, "accuracy")
    out["score"] = out["soft_dice"] - 10.0 * out["mean_fpr"]
    out["n_fake"], out["n_real"] = len(fake), len(real)
    return out


# ----------------------------------------------------------------------------- threshold sweep
BINARY_KEYS = ("bin_dice", "bin_iou", "recall", "precision", "bin_f1", "accuracy")
_threshold_cache = {}


def default_thresholds(n=99):
    """The even grid k / (n + 1), k = 1 .. n (99: 0.01 .. 0.99)."""
    n = int(n)
    if n < 1:
        raise ValueError(f"need at least one threshold, got n = {n}")
    return [k / (n + 1) for k in range(1, n + 1)]


def check_thresholds(thresholds):
    """The thresholds as the kernel compares them (float32): finite, strictly ascending after the
    rounding (two doubles that collapse to one float32 are duplicates), 1 <= K <= the kernel's
    maximum.  Returns the float32 array; ValueError otherwise."""
    t = np.asarray([float(v) for v in thresholds], dtype=np.float64)
    kmax = _lib.lib().msu_seg_sweep_max_k()
    if t.ndim != 1 or not 1 <= t.size <= kmax:
        raise ValueError(f"need 1 to {kmax} thresholds, got {t.size}")
    if not np.isfinite(t).all():
        raise ValueError("thresholds must be finite")
    with np.errstate(over="ignore"):
        t32 = t.astype(np.float32)
    if not np.isfinite(t32).all():
        raise ValueError("thresholds must be finite in float32")
    if (t32[1:] <= t32[:-1]).any():
        k = int(np.argmax(t32[1:] <= t32[:-1]))
        raise ValueError(f"thresholds must be strictly ascending in float32: entries {k} and {k + 1} "
                         f"are {t[k]!r} and {t[k + 1]!r}")
    return t32


def _device_thresholds(thresholds, device):
    key = (tuple(float(v) for v in thresholds), str(device))
    t = _threshold_cache.get(key)
    if t is None:
        t = torch.from_numpy(check_thresholds(key[0])).to(device)
        if len(_threshold_cache) >= 16:
            _threshold_cache.clear()
        _threshold_cache[key] = t
    return t


def threshold_histogram(logits, labels, thresholds):
    """Per image and class, how many pixels exceed exactly j of the ``thresholds`` (one GPU pass,
    ``msu_seg_sweep``): logits [B, 1, H, W] (f32 / bf16 / f16), labels [B, H, W] or [B, 1, H, W]
    -> int64 tensor [B, 2, K + 1] (host); class 1 is ``label > 0``, the predicate is
    ``image_sums``' ``p > t`` (a tie is not positive)."""
    t32 = check_thresholds(thresholds)
    ops._need_cuda(logits, labels)
    B = logits.shape[0]
    if labels.shape[0] != B:
        raise ValueError(f"batch mismatch: logits {B}, labels {labels.shape[0]}")
    x = logits.contiguous()
    if x.dtype not in (torch.float32, torch.bfloat16, torch.float16):
        x = x.float()
    lab = ops._f32(labels)
    N = x[0].numel()
    if lab[0].numel() != N:
        raise ValueError(f"label size {tuple(labels.shape)} does not match logits {tuple(logits.shape)}")
    thr = _device_thresholds(thresholds, x.device)
    K = int(t32.size)
    hist = torch.empty(B, 2, K + 1, device=x.device, dtype=torch.int64)
    _lib.call("msu_seg_sweep", ops._dt(x), ops._p(x), ops._p(lab), B, N, ops._p(thr), K, ops._p(hist), ops._s(x))
    return hist.cpu()


def sweep_counts(hist):
    """``threshold_histogram``'s [B, 2, K + 1] -> int64 [B, K, 4] = (tp, fp, fn, tn) of every
    threshold: a pixel is positive at t_k when it exceeds more than k thresholds, so tp_k and
    fp_k are the suffix sums over j > k of the class rows; fn_k = P - tp_k, tn_k = Nn - fp_k."""
    h = np.asarray(hist, dtype=np.int64)
    if h.ndim != 3 or h.shape[1] != 2 or h.shape[2] < 2:
        raise ValueError(f"expected a [B, 2, K + 1] histogram, got {h.shape}")
    above = np.cumsum(h[:, :, ::-1], axis=2)[:, :, ::-1]  # above[..., j] = sum over j' >= j
    total = above[:, :, :1]
    pos = above[:, :, 1:]                                   # [B, 2, K]: sum over j > k
    tp, fp = pos[:, 1], pos[:, 0]
    return np.stack([tp, fp, total[:, 1] - tp, total[:, 0] - fp], axis=2)


def _mean(values):
    return sum(values) / len(values) if values else float("nan")


def summarize_sweep(thresholds, counts):
    """Per-threshold epoch summary from ``sweep_counts`` rows of a whole split ([n, K, 4]).

    Lists of K values: the fake-image means of ``BINARY_KEYS``, ``mean_fpr`` over the real images,
    ``accuracy_all`` and ``bin_score = mean bin_dice - 10 * mean_fpr`` (the reference's Score with
    the Dice taken binary), exactly ``summarize``'s means of ``binary_metrics``; ``n_fake`` /
    ``n_real``.  ``"pooled"``: the pixel-level curves from the counts summed over all images,
    ``tpr``, ``fpr``, ``precision`` (1 where nothing is predicted positive), ``auroc`` (trapezoid
    over the K points and the end points (0, 0) and (1, 1)) and ``average_precision``
    (sum_k (R_k - R_{k+1}) P_k, R_K = 0).  ``tpr``, ``precision`` and ``average_precision`` are NaN
    without a positive pixel, ``fpr`` without a negative one, ``auroc`` in either case."""
    c = np.asarray(counts, dtype=np.int64)
    thresholds = [float(t) for t in thresholds]
    if c.ndim != 3 or c.shape[2] != 4 or c.shape[1] != len(thresholds):
        raise ValueError(f"expected counts [n, {len(thresholds)}, 4], got {c.shape}")
    K = c.shape[1]
    real = [int(r[0, 0] + r[0, 2]) == 0 for r in c]
    out = {"thresholds": thresholds, "n_fake": real.count(False), "n_real": real.count(True)}
    cols = {k: [] for k in BINARY_KEYS + ("mean_fpr", "accuracy_all", "bin_score")}
    for k in range(K):
        ms = [binary_metrics(*row[k].tolist()) for row in c]
        fake = [m for m in ms if not m["real"]]
        for key in BINARY_KEYS:
            cols[key].append(_mean([m[key] for m in fake]))
        cols["mean_fpr"].append(_mean([m["fpr"] for m in ms if m["real"]]))
        cols["accuracy_all"].append(_mean([m["accuracy"] for m in ms]))
        cols["bin_score"].append(cols["bin_dice"][-1] - 10.0 * cols["mean_fpr"][-1])
    out.update(cols)

    nan = float("nan")
    tot = c.sum(axis=0, dtype=np.int64)  # [K, 4]
    tp, fp, fn, tn = (tot[:, i].astype(np.float64) for i in range(4))
    P, Nn = (float(tp[0] + fn[0]), float(fp[0] + tn[0])) if c.shape[0] else (0.0, 0.0)
    tpr = tp / P if P > 0 else np.full(K, nan)
    fpr = fp / Nn if Nn > 0 else np.full(K, nan)
    prec = np.where(tp + fp > 0, tp / np.maximum(tp + fp, 1.0), 1.0) if P > 0 else np.full(K, nan)
    # both curves fall as k grows: (1, 1), the K points, (0, 0)
    x, y = np.concatenate([[1.0], fpr, [0.0]]), np.concatenate([[1.0], tpr, [0.0]])
    auroc = float(np.sum((x[:-1] - x[1:]) * (y[:-1] + y[1:]) * 0.5)) if P > 0 and Nn > 0 else nan
    ap = float(np.sum((tpr - np.concatenate([tpr[1:], [0.0]])) * prec)) if P > 0 else nan
    out["pooled"] = {"tpr": tpr.tolist(), "fpr": fpr.tolist(), "precision": prec.tolist(), "auroc": auroc,
                     "average_precision": ap, "n_pos": int(P), "n_neg": int(Nn)}
    return out


def select_threshold(sweep, key="bin_dice", max_fpr=None):
    """The threshold of a ``summarize_sweep`` dict with the largest ``key`` among those whose
    ``mean_fpr`` is at most ``max_fpr`` (None: all); ties go to the lowest threshold.  ValueError
    when nothing qualifies (every candidate's ``key`` NaN included) or when ``max_fpr`` is given
    and the split has no real image."""
    if key not in sweep or not isinstance(sweep[key], list):
        raise ValueError(f"unknown sweep column {key!r}")
    if max_fpr is not None and sweep["n_real"] == 0:
        raise ValueError("max_fpr needs at least one real image in the split")
    best = None
    for k, v in enumerate(sweep[key]):
        if math.isnan(v) or (max_fpr is not None and not sweep["mean_fpr"][k] <= max_fpr):
            continue
        if best is None or v > sweep[key][best]:
            best = k
    if best is None:
        raise ValueError(f"no threshold qualifies (key {key!r}, max_fpr {max_fpr})")
    return sweep["thresholds"][best]


@torch.no_grad()
def evaluate(model, batches, threshold=0.5, amp_dtype=torch.bfloat16, sweep=None):
    """Run ``model`` in eval mode over ``(images, labels)`` batches on the GPU and summarise
    (the metric part of ``calculate_metrics``; no CSV / checkpoint side effects).  ``sweep``: a
    threshold sequence; the same logits then also go through ``threshold_histogram`` and the
    summary gains ``"sweep"`` (``summarize_sweep``).  None: nothing else is launched."""
    if sweep is not None:
        sweep = [float(t) for t in sweep]
        check_thresholds(sweep)
    model.eval()
    per_image, hists = [], []
    for images, labels in batches:
        with torch.autocast("cuda", dtype=amp_dtype, enabled=amp_dtype != torch.float32):
            logits = model(images)
        per_image += batch_metrics(logits, labels, threshold)
        if sweep is not None:
            hists.append(threshold_histogram(logits, labels, sweep).numpy())
    out = summarize(per_image)
    if sweep is not None:
        counts = sweep_counts(np.concatenate(hists)) if hists else np.zeros((0, len(sweep), 4), np.int64)
        out["sweep"] = summarize_sweep(sweep, counts)
    return out
