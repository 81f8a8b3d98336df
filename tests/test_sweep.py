"""CPU: the host side of the threshold sweep (validation.sweep_counts / binary_metrics /
summarize_sweep / select_threshold / threshold validation), the margins of the inputs the GPU
tests use, and the argument guards of the C entry.  The float64 restatement is
tests/_sweep_ref.py."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import _sweep_ref as ref
from semantic_segmentation_of_stylegan2_artifacts_amd import _lib, validation


def _same(a, b, tol=1e-12):
    """Nested dict / list / number equality, NaN == NaN, floats to ``tol`` absolute."""
    if isinstance(a, dict):
        assert set(a) >= set(b)
        for k in b:
            _same(a[k], b[k], tol)
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b)
        for x, y in zip(a, b):
            _same(x, y, tol)
    elif isinstance(b, float) and math.isnan(b):
        assert math.isnan(a)
    else:
        assert abs(a - b) <= tol, (a, b)


def test_margin_sets_keep_their_margin():
    """Every (dtype, K) the GPU comparison uses: min |p64 - t| >= 1e-4 over the set's logit
    values, the set still spans the thresholds, and f32 / f16 drop no midpoint."""
    seen = set()
    for name, B, N, K in ref.GPU_CASES:
        if (name, K) in seen:
            continue
        seen.add((name, K))
        c = ref.candidates(K, ref.DTYPES[name])
        m = ref.margin(c, ref.thresholds(K))
        print(f"{name} K={K}: {len(c)} values, margin {m:.3e}")
        assert m >= ref.MARGIN
        assert np.isinf(c).sum() == 2 and len(c) >= 6
        if name != "bf16":
            assert len(c) == K - 1 + 6
        else:
            assert len(c) >= min(K - 1, 32) + 6  # bf16 keeps a spread of interior bins
    assert {k for _, k in seen} == set(ref.KS) and {n for _, _, n, _ in ref.GPU_CASES} == set(ref.NS)
    # the densest set: half a threshold step (4.9e-4) in the middle, (sqrt(2) - 1) of a step (4.0e-4)
    # at the two ends, where the logit-space midpoint of t and 2 t is their geometric mean
    c = ref.candidates(1024, torch.float32)
    assert ref.margin(c, ref.thresholds(1024)) == pytest.approx((2 ** 0.5 - 1) / 1025, rel=0.01)
    assert ref.margin(c[np.abs(c) < 1], ref.thresholds(1024)) == pytest.approx(0.5 / 1025, rel=0.01)
    # a drawn case is made of the set's values
    lg, lab, ts = ref.margin_case(3, 257, 65, torch.bfloat16)
    assert lg.dtype == torch.bfloat16 and lab.dtype == torch.float32 and len(ts) == 65
    assert ref.margin(lg.double().numpy(), ts) >= ref.MARGIN
    assert set(np.unique(lab.numpy()).tolist()) <= {0.0, np.float32(0.3).item(), 1.0, 255.0}


def test_sweep_counts_equal_direct_counts():
    rng = np.random.default_rng(0)
    for B, K in ((1, 1), (4, 2), (3, 17), (2, 1024)):
        h = rng.integers(0, 1000, (B, 2, K + 1))
        h[0, 1] = 0                      # a real image
        h[-1, :, 1:-1] = 0               # saturated: end bins only
        c = validation.sweep_counts(h)
        assert c.dtype == np.int64 and c.shape == (B, K, 4)
        assert np.array_equal(c, ref.counts_from_hist(h))
        assert (np.diff(c[:, :, 0], axis=1) <= 0).all() and (np.diff(c[:, :, 1], axis=1) <= 0).all()
        assert (np.diff(c[:, :, 2], axis=1) >= 0).all() and (np.diff(c[:, :, 3], axis=1) >= 0).all()
        assert (c[:, :, 0] + c[:, :, 2] == h[:, 1].sum(1, keepdims=True)).all()
        assert (c[:, :, 1] + c[:, :, 3] == h[:, 0].sum(1, keepdims=True)).all()
    assert np.array_equal(validation.sweep_counts(torch.from_numpy(h)), c)  # a host tensor works too
    big = np.zeros((1, 2, 3), dtype=np.int64)
    big[0, 0] = (2**40, 5, 2**33)  # no 32-bit arithmetic anywhere
    assert validation.sweep_counts(big)[0].tolist() == [[0, 5 + 2**33, 0, 2**40], [0, 2**33, 0, 2**40 + 5]]
    with pytest.raises(ValueError):
        validation.sweep_counts(np.zeros((2, 3, 4)))


def test_histogram_restatement_is_consistent():
    """The two direct statements in _sweep_ref agree (histogram -> counts == per-threshold counts),
    ties and NaN included."""
    lg, lab, ts = ref.margin_case(2, 500, 9, torch.float32)
    lg[0, :5] = 0.0          # p == 0.5 == t_4: not positive at t_4
    lg[1, :3] = float("nan")
    h = ref.histogram(lg, lab, ts)
    assert h.sum() == 1000
    assert np.array_equal(validation.sweep_counts(h), ref.counts_direct(lg, lab, ts))


def test_binary_metrics_equal_metrics_from_sums():
    rng = np.random.default_rng(1)
    rows = [tuple(int(v) for v in rng.integers(0, 50, 4)) for _ in range(200)]
    rows += [(0, 0, 7, 9), (0, 3, 7, 0), (5, 0, 0, 0), (0, 0, 0, 4), (0, 6, 0, 0), (0, 2, 0, 3), (3, 1, 0, 0)]
    for tp, fp, fn, tn in rows:
        if tp + fp + fn + tn == 0:
            continue
        full = validation.metrics_from_sums(torch.tensor([0.0, 0, tp + fn, 0, 0, 0, 0, tp, fp, fn, tn], dtype=torch.float64))
        got = validation.binary_metrics(tp, fp, fn, tn)
        keys = ("fpr",) if full["real"] else ("bin_dice", "bin_iou", "recall", "precision", "bin_f1")
        assert set(got) == set(keys) | {"accuracy", "real"}
        for k in keys + ("accuracy", "real"):
            assert got[k] == full[k], (k, tp, fp, fn, tn)
        _same(got, {k: v for k, v in ref.image_metrics(tp, fp, fn, tn).items()})
    with pytest.raises(ValueError):
        validation.binary_metrics(0, 0, 0, 0)


@pytest.mark.parametrize("kind", ["mixed", "no_real", "no_fake", "one_class", "empty_positive_class"])
def test_summarize_sweep_equals_restatement(kind):
    rng = np.random.default_rng(2)
    K = 7
    h = rng.integers(0, 40, (5, 2, K + 1))
    if kind == "mixed":
        h[1, 1] = h[3, 1] = 0
    elif kind == "no_fake":
        h[:, 1] = 0
    elif kind == "one_class":
        h[:, 0] = 0
    elif kind == "empty_positive_class":
        h[:, :, -3:] = 0  # nothing predicted positive at the high thresholds
    ts = ref.thresholds(K)
    c = validation.sweep_counts(h)
    got, want = validation.summarize_sweep(ts, c), ref.summary(ts, c)
    _same(got, want)
    assert (got["n_fake"], got["n_real"]) == {"mixed": (3, 2), "no_fake": (0, 5)}.get(kind, (5, 0))
    p = got["pooled"]
    if kind == "no_fake":
        assert math.isnan(p["auroc"]) and math.isnan(p["average_precision"]) and math.isnan(p["tpr"][0])
        assert all(math.isnan(v) for v in got["bin_dice"]) and not math.isnan(got["mean_fpr"][0])
    if kind == "one_class":
        assert math.isnan(p["auroc"]) and math.isnan(p["fpr"][0]) and not math.isnan(p["average_precision"])
    if kind == "no_real":
        assert all(math.isnan(v) for v in got["mean_fpr"]) and all(math.isnan(v) for v in got["bin_score"])
    if kind == "empty_positive_class":
        assert p["precision"][-1] == 1.0 and got["precision"][-1] == 0.0  # pooled: 1; per image: medpy's 0
    # the epoch means are summarize's of the per-image binary metrics
    for k in range(K):
        s = validation.summarize([dict(validation.binary_metrics(*r[k]), soft_dice=0.0, soft_iou=0.0) for r in c])
        for key in validation.BINARY_KEYS + ("mean_fpr", "accuracy_all"):
            a, b = got[key][k], s[key]
            assert a == b or (math.isnan(a) and math.isnan(b)), (key, k)
    with pytest.raises(ValueError):
        validation.summarize_sweep(ts[:-1], c)


@pytest.mark.parametrize("K,dtype", [(9, torch.float32), (255, torch.float32), (64, torch.bfloat16)])
def test_pooled_auroc_is_mann_whitney_when_thresholds_separate(K, dtype):
    """The trapezoid over the K points is the Mann-Whitney AUROC (half credit for ties) of the
    bin index, always; and of the probabilities themselves when every distinct probability has a
    bin of its own.  A margin set's midpoints do; its three values beyond each end (12, 40, inf)
    share an outer bin, so for the second statement +-40 and +-inf are folded onto +-12."""
    lg, lab, ts = ref.margin_case(3, 2000, K, dtype, seed=4)
    g = (lab.numpy() > 0).ravel()
    h = ref.histogram(lg, lab, ts)
    sweep = validation.summarize_sweep(ts, validation.sweep_counts(h))
    bins = (ref.sigmoid64(lg.double().numpy()).ravel()[:, None] > ref.f32_thresholds(ts)[None, :]).sum(1)
    assert len(np.unique(bins)) >= min(K + 1, 30)
    assert abs(sweep["pooled"]["auroc"] - ref.mann_whitney_auroc(bins[g], bins[~g])) <= 1e-12
    lg = lg.clamp(-12, 12)
    p = ref.sigmoid64(lg.double().numpy()).ravel()
    assert len(np.unique(p)) == len(np.unique(bins))
    sweep = validation.summarize_sweep(ts, validation.sweep_counts(ref.histogram(lg, lab, ts)))
    assert abs(sweep["pooled"]["auroc"] - ref.mann_whitney_auroc(p[g], p[~g])) <= 1e-12
    # by hand: 0.9 beats three negatives, 0.5 beats two and ties one
    assert ref.mann_whitney_auroc([0.9, 0.5], [0.5, 0.1, 0.2]) == pytest.approx((3 + 2.5) / 6)


def _sweep(bin_dice, mean_fpr, n_real=1):
    return {"thresholds": [0.1 * (k + 1) for k in range(len(bin_dice))], "bin_dice": bin_dice,
            "mean_fpr": mean_fpr, "n_real": n_real, "n_fake": 1}


def test_select_threshold():
    s = _sweep([0.2, 0.7, 0.7, 0.9, 0.5], [0.5, 0.3, 0.2, 0.1, 0.0])
    assert validation.select_threshold(s) == s["thresholds"][3]
    assert validation.select_threshold(s, "bin_dice", 0.05) == s["thresholds"][4]
    assert validation.select_threshold(s, max_fpr=0.1) == s["thresholds"][3]          # the bound is inclusive
    s = _sweep([0.7, 0.7, 0.7], [0.3, 0.2, 0.1])
    assert validation.select_threshold(s) == s["thresholds"][0]                       # ties: lowest index
    assert validation.select_threshold(s, max_fpr=0.25) == s["thresholds"][1]
    assert validation.select_threshold(s, "mean_fpr") == s["thresholds"][0]
    with pytest.raises(ValueError, match="no threshold qualifies"):
        validation.select_threshold(s, max_fpr=0.05)
    nan = float("nan")
    with pytest.raises(ValueError, match="no threshold qualifies"):
        validation.select_threshold(_sweep([nan, nan], [0.1, 0.1]))
    with pytest.raises(ValueError, match="real image"):
        validation.select_threshold(_sweep([0.5, 0.6], [nan, nan], n_real=0), max_fpr=0.5)
    assert validation.select_threshold(_sweep([0.5, 0.6], [nan, nan], n_real=0)) == pytest.approx(0.2)
    with pytest.raises(ValueError, match="unknown"):
        validation.select_threshold(s, "soft_dice")


def test_default_thresholds():
    t = validation.default_thresholds()
    assert len(t) == 99 and t[0] == 0.01 and t[49] == 0.5 and t[-1] == 0.99
    assert validation.default_thresholds(9) == [k / 10 for k in range(1, 10)]
    with pytest.raises(ValueError):
        validation.default_thresholds(0)


def _need_lib():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built")
    return _lib.lib()


def test_threshold_validation():
    """Checked on the host before anything touches a device (the tensors here are CPU tensors:
    a valid list gets as far as the device check and fails there)."""
    _need_lib()
    lg, lab = torch.zeros(2, 1, 4, 4), torch.zeros(2, 4, 4)
    tiny = float(np.nextafter(np.float32(0.5), np.float32(1))) - 1e-9  # rounds to a float32 of its own
    assert np.array_equal(validation.check_thresholds([0.25, 0.5, tiny]),
                          np.array([0.25, 0.5, np.nextafter(np.float32(0.5), np.float32(1))], dtype=np.float32))
    for bad, what in (([0.5, 0.4], "ascending"), ([0.5, 0.5], "ascending"), ([0.5, 0.5 + 1e-12], "ascending"),
                      ([0.1, float("nan")], "finite"), ([0.1, float("inf")], "finite"), ([0.1, 1e300], "finite"),
                      ([], "thresholds"), (ref.thresholds(1025), "thresholds")):
        with pytest.raises(ValueError, match=what):
            validation.threshold_histogram(lg, lab, bad)
        with pytest.raises(ValueError, match=what):
            validation.check_thresholds(bad)
    with pytest.raises(RuntimeError):  # CPU tensors have no kernel
        validation.threshold_histogram(lg, lab, [0.5])
    with pytest.raises(ValueError, match="ascending"):
        validation.evaluate(None, [], sweep=[0.6, 0.5])


def test_sweep_argument_codes():
    """The C entry refuses bad sizes and null pointers with -2 before touching the device."""
    L = _need_lib()
    assert L.msu_seg_sweep_max_k() == 1024
    max_n = L.msu_seg_sweep_max_n()
    assert max_n >= 2**31  # far beyond any image; a block's u32 bins cannot wrap below it
    buf = ctypes.create_string_buffer(64)  # never dereferenced: every call below is refused
    p = ctypes.addressof(buf)
    for dtype, lg, lab, B, N, thr, K, hist in (
            (0, p, p, 0, 16, p, 1, p), (0, p, p, -1, 16, p, 1, p), (0, p, p, 1, 0, p, 1, p),
            (0, p, p, 1, -5, p, 1, p), (0, p, p, 1, max_n + 1, p, 1, p), (0, p, p, 1, 16, p, 0, p),
            (0, p, p, 1, 16, p, -3, p), (0, p, p, 1, 16, p, 1025, p), (0, None, p, 1, 16, p, 1, p),
            (1, p, None, 1, 16, p, 1, p), (2, p, p, 1, 16, None, 1, p), (0, p, p, 1, 16, p, 1, None),
            (3, p, p, 1, 16, p, 1, p), (0, None, None, 1, 16, None, 1024, None)):
        assert L.msu_seg_sweep(dtype, lg, lab, B, N, thr, K, hist, None) == -2, (dtype, B, N, K)
