"""Float64 numpy restatement of the threshold sweep (TEST INFRASTRUCTURE ONLY): the histogram
``msu_seg_sweep`` fills and the counts by direct comparison, the summary formulas of
``validation.summarize_sweep``, a Mann-Whitney AUROC, and the "margin inputs" on which a float32
sigmoid cannot land on the other side of a threshold.

Margin inputs: thresholds k / (K + 1); logits drawn from the midpoints, in logit space, between
neighbouring thresholds, plus +-12, +-40 and +-inf, rounded to the logits' dtype; a candidate
stays only if its float64 probability keeps ``MARGIN`` = 1e-4 from every threshold, ten times the
rtol 1e-5 / atol 1e-6 the suite grants a float32 probability.  (In f32 and f16 every midpoint
stays, the densest set K = 1024 keeping 4.9e-4 in the middle and 4.0e-4 at its ends; bf16's
8-bit mantissa moves some midpoints of the dense sets too close and those drop out.)  Labels
come from {0, 0.3, 1, 255}."""
import numpy as np
import torch

MARGIN = 1e-4
SMOOTH = 1e-8
BINARY_KEYS = ("bin_dice", "bin_iou", "recall", "precision", "bin_f1", "accuracy")


# The (dtype, B, N, K) cases of the GPU comparison, crossed sparsely: N covers one pixel, ragged
# tails, sizes around the block (256) and around a block's share (4096), vector (N % 8 == 0) and
# scalar paths; K covers the search depths around 64 and 256, one threshold and the maximum.
# Every N meets every dtype, every K meets every dtype, each N meets three Ks.
NS = (1, 3, 255, 256, 257, 4095, 4096, 4097, 37 * 70)
KS = (1, 2, 63, 64, 65, 255, 256, 257, 1024)
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
GPU_CASES = [(tuple(DTYPES)[(i + j) % 3], (1, 3)[(i + j) % 2], N, KS[(i + 3 * j) % 9])
             for i, N in enumerate(NS) for j in range(3)]


def thresholds(K):
    return [k / (K + 1) for k in range(1, K + 1)]


def sigmoid64(x):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-np.asarray(x, dtype=np.float64)))


def f32_thresholds(ts):
    return np.asarray(ts, dtype=np.float64).astype(np.float32).astype(np.float64)


def margin(values, ts):
    """min |p64 - t| over logit values and (float32-rounded) thresholds; NaN logits are skipped."""
    v = np.asarray(values, dtype=np.float64).ravel()
    p = sigmoid64(v[~np.isnan(v)])
    return float(np.abs(p[:, None] - f32_thresholds(ts)[None, :]).min())


def candidates(K, dtype):
    """The logit values of the margin set for K thresholds in ``dtype`` (float64 array)."""
    t = np.asarray(thresholds(K), dtype=np.float64)
    lg = np.log(t / (1.0 - t))
    mid = (lg[:-1] + lg[1:]) / 2
    c = np.concatenate([mid, [12.0, -12.0, 40.0, -40.0, np.inf, -np.inf]])
    c = np.unique(torch.from_numpy(c).to(dtype).double().numpy())
    p = sigmoid64(c)
    keep = np.abs(p[:, None] - f32_thresholds(thresholds(K))[None, :]).min(axis=1) >= MARGIN
    return c[keep]


def margin_case(B, N, K, dtype, seed=0):
    """(logits [B, N] in ``dtype``, label [B, N] f32, thresholds list) of the margin set."""
    rng = np.random.default_rng(seed + 1000003 * K + 7 * N + B)
    c = candidates(K, dtype)
    logits = torch.from_numpy(c[rng.integers(0, len(c), (B, N))]).to(dtype)
    label = torch.from_numpy(np.array([0.0, 0.3, 1.0, 255.0], dtype=np.float32)[rng.integers(0, 4, (B, N))])
    return logits, label, thresholds(K)


def histogram(logits, label, ts):
    """int64 [B, 2, K + 1]: per image and class (label > 0), the pixels whose float64 probability
    exceeds exactly j thresholds, by direct comparison (a NaN compares false: bin 0)."""
    x = torch.as_tensor(logits).double().numpy()
    g = (torch.as_tensor(label).double().numpy() > 0).reshape(x.shape[0], -1)
    x = x.reshape(x.shape[0], -1)
    t = f32_thresholds(ts)
    out = np.zeros((x.shape[0], 2, len(t) + 1), dtype=np.int64)
    for b in range(x.shape[0]):
        p = sigmoid64(x[b])
        n = np.zeros(p.shape, dtype=np.int64)
        for tk in t:
            n += tk < p
        for cls in (0, 1):
            out[b, cls] = np.bincount(n[g[b] == bool(cls)], minlength=len(t) + 1)
    return out


def counts_direct(logits, label, ts):
    """int64 [B, K, 4] = (tp, fp, fn, tn) at every threshold, each by its own comparison."""
    x = torch.as_tensor(logits).double().numpy()
    g = (torch.as_tensor(label).double().numpy() > 0).reshape(x.shape[0], -1)
    p = sigmoid64(x.reshape(x.shape[0], -1))
    out = np.zeros((x.shape[0], len(ts), 4), dtype=np.int64)
    for k, tk in enumerate(f32_thresholds(ts)):
        pos = p > tk
        out[:, k] = np.stack([(pos & g).sum(1), (pos & ~g).sum(1), (~pos & g).sum(1), (~pos & ~g).sum(1)], axis=1)
    return out


def counts_from_hist(hist):
    """(tp, fp, fn, tn) from a histogram, element by element (no cumulative sum)."""
    h = np.asarray(hist, dtype=np.int64)
    B, _, K1 = h.shape
    out = np.zeros((B, K1 - 1, 4), dtype=np.int64)
    for b in range(B):
        for k in range(K1 - 1):
            tp, fp = int(h[b, 1, k + 1:].sum()), int(h[b, 0, k + 1:].sum())
            out[b, k] = (tp, fp, int(h[b, 1].sum()) - tp, int(h[b, 0].sum()) - fp)
    return out


def image_metrics(tp, fp, fn, tn):
    """The binary metrics of one image (medpy's definitions as validation.py states them)."""
    tp, fp, fn, tn = float(tp), float(fp), float(fn), float(tn)
    m = {"accuracy": (tp + tn) / (tp + fp + fn + tn), "real": tp + fn == 0}
    if m["real"]:
        m["fpr"] = fp / (fp + tn)
        return m
    m["bin_dice"] = 2 * tp / (2 * tp + fp + fn)
    m["bin_iou"] = tp / (tp + fp + fn)
    m["recall"] = tp / (tp + fn)
    m["precision"] = tp / (tp + fp) if tp + fp > 0 else 0.0
    m["bin_f1"] = 2 * m["precision"] * m["recall"] / (m["precision"] + m["recall"] + SMOOTH)
    return m


def summary(ts, counts):
    """What validation.summarize_sweep returns, restated."""
    c = np.asarray(counts, dtype=np.float64)
    n, K = c.shape[0], c.shape[1]
    nan = float("nan")
    out = {"thresholds": [float(t) for t in ts]}
    for key in BINARY_KEYS + ("mean_fpr", "accuracy_all", "bin_score"):
        out[key] = []
    is_real = [c[i, 0, 0] + c[i, 0, 2] == 0 for i in range(n)]
    out["n_real"], out["n_fake"] = sum(is_real), n - sum(is_real)
    for k in range(K):
        ms = [image_metrics(*c[i, k]) for i in range(n)]
        for key in BINARY_KEYS:
            v = [m[key] for m in ms if not m["real"]]
            out[key].append(float(np.mean(v)) if v else nan)
        v = [m["fpr"] for m in ms if m["real"]]
        out["mean_fpr"].append(float(np.mean(v)) if v else nan)
        out["accuracy_all"].append(float(np.mean([m["accuracy"] for m in ms])) if ms else nan)
        out["bin_score"].append(out["bin_dice"][-1] - 10 * out["mean_fpr"][-1])
    tp, fp, fn, tn = c.sum(axis=0).T if n else np.zeros((4, K))
    P, Nn = tp[0] + fn[0], fp[0] + tn[0]
    tpr = tp / P if P > 0 else np.full(K, nan)
    fpr = fp / Nn if Nn > 0 else np.full(K, nan)
    prec = np.array([nan if P == 0 else (tp[k] / (tp[k] + fp[k]) if tp[k] + fp[k] > 0 else 1.0) for k in range(K)])
    auroc = nan
    if P > 0 and Nn > 0:
        xs, ys = [1.0] + list(fpr) + [0.0], [1.0] + list(tpr) + [0.0]
        auroc = sum((xs[i] - xs[i + 1]) * (ys[i] + ys[i + 1]) / 2 for i in range(K + 1))
    ap = nan
    if P > 0:
        r = list(tpr) + [0.0]
        ap = sum((r[k] - r[k + 1]) * prec[k] for k in range(K))
    out["pooled"] = {"tpr": list(tpr), "fpr": list(fpr), "precision": list(prec), "auroc": auroc,
                     "average_precision": ap}
    return out


def mann_whitney_auroc(pos, neg):
    """P(score of a positive > score of a negative) + half P(equal), from the scores."""
    pos, neg = np.sort(np.asarray(pos, dtype=np.float64)), np.sort(np.asarray(neg, dtype=np.float64))
    below = np.searchsorted(neg, pos, side="left")
    equal = np.searchsorted(neg, pos, side="right") - below
    return float((below.sum() + 0.5 * equal.sum()) / (len(pos) * len(neg)))
