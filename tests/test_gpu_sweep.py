"""GPU: msu_seg_sweep / validation.threshold_histogram against the float64 restatement in
tests/_sweep_ref.py (element for element, on inputs that keep every probability 1e-4 from every
threshold), against msu_seg_metrics on random inputs (exact: same sigmoid, same predicate), and
evaluate / predict end to end."""
import csv
import json
import os

import numpy as np
import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu

import cases  # noqa: E402
import _sweep_ref as ref  # noqa: E402
from oracle.msunet import make_cfg  # noqa: E402

DEV = "cuda"


def _hist(logits, label, ts):
    from semantic_segmentation_of_stylegan2_artifacts_amd import validation
    h = validation.threshold_histogram(logits.to(DEV), label.to(DEV), ts)
    assert h.dtype == torch.int64 and tuple(h.shape) == (logits.shape[0], 2, len(ts) + 1) and not h.is_cuda
    return h.numpy()


@pytest.mark.parametrize("name,B,N,K", ref.GPU_CASES, ids=lambda v: str(v))
def test_histogram_equals_fp64_reference(name, B, N, K):
    logits, label, ts = ref.margin_case(B, N, K, ref.DTYPES[name])
    got, want = _hist(logits, label, ts), ref.histogram(logits, label, ts)
    bad = np.argwhere(got != want)
    assert bad.size == 0, (len(bad), bad[:5].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])
    assert got.sum() == B * N


def _random_case(dtype):
    g = torch.Generator().manual_seed(3)
    logits = (torch.randn(4, 1, 96, 160, generator=g) * 3).to(dtype)
    label = (torch.rand(4, 96, 160, generator=g) < 0.05).float()
    label[1] = 0
    return logits, label


@pytest.mark.parametrize("special", ["ties", "nonfinite"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_counts_equal_image_sums(dtype, special):
    """The (tp, fp, fn, tn) of every threshold are msu_seg_metrics' at that threshold, exactly, on
    random normal logits: with exact zeros and 0.5 in the list (a tie is not positive), and with
    NaN (positive nowhere) and +-inf logits."""
    from semantic_segmentation_of_stylegan2_artifacts_amd import validation
    logits, label = _random_case(dtype)
    flat = logits.view(4, -1)
    if special == "ties":
        flat[:, ::7] = 0.0
    else:
        flat[0, 5], flat[2, 11], flat[3, 100] = float("nan"), float("nan"), float("nan")
        flat[0, 9], flat[1, 3], flat[2, 77] = float("inf"), float("-inf"), float("inf")
        flat[3, 4000], flat[2, 15359] = float("-inf"), float("nan")
    ts = [0.02, 0.1, 0.35, 0.5, 0.62, 0.9, 0.995]
    counts = validation.sweep_counts(_hist(logits, label, ts))
    for k, t in enumerate(ts):
        base = validation.image_sums(logits.to(DEV), label.to(DEV), t).numpy()[:, 7:11]
        assert np.array_equal(counts[:, k], base), (t, counts[:, k].tolist(), base.tolist())
    if special == "ties":  # the zeros are negative at 0.5 and positive just below it
        zeros = (flat.float() == 0).sum(1).numpy()
        assert (zeros >= 15360 // 7).all()
        h = _hist(logits, label, [float(np.nextafter(np.float32(0.5), np.float32(0))), 0.5])
        assert np.array_equal(h[:, :, 1].sum(1), zeros)


@pytest.mark.parametrize("kind", ["background", "foreground", "half"])
def test_saturated_images_at_the_workload_size(kind):
    """1 x 1024^2, every pixel in an end bin (the per-thread register path; a block's share is
    4096 pixels, a wave's 1024)."""
    N, K = 1024 * 1024, 99
    logits = torch.full((1, N), -40.0, dtype=torch.bfloat16)
    label = torch.zeros(1, N)
    want = np.zeros((1, 2, K + 1), dtype=np.int64)
    if kind == "background":
        want[0, 0, 0] = N
    elif kind == "foreground":
        logits[:], label[:] = 40.0, 1.0
        want[0, 1, K] = N
    else:  # the second half confident foreground, 1000 pixels of it unlabelled
        logits[0, N // 2:], label[0, N // 2 + 1000:] = 40.0, 1.0
        want[0, 0, 0], want[0, 0, K], want[0, 1, K] = N // 2, 1000, N // 2 - 1000
    got = _hist(logits, label, ref.thresholds(K))
    assert np.array_equal(got, want), np.argwhere(got != want)[:5].tolist()


def test_guard_bands_and_no_dependence_on_previous_contents():
    """hist sits in the middle of a 0xA5-filled buffer: the guards stay, every inside element is
    overwritten, on two consecutive calls with different inputs into the same buffer."""
    from semantic_segmentation_of_stylegan2_artifacts_amd import _lib, ops
    B, N, K, guard = 3, 37 * 70, 65, 512
    n = B * 2 * (K + 1)
    buf = torch.full(((n + 2 * guard) * 8,), 0xA5, dtype=torch.uint8, device=DEV).view(torch.int64)
    sentinel = int(np.frombuffer(b"\xa5" * 8, dtype=np.int64)[0])
    thr = torch.tensor(ref.thresholds(K), dtype=torch.float32, device=DEV)
    for seed in (0, 1):
        logits, label, ts = ref.margin_case(B, N, K, torch.float32, seed=seed)
        lg, lb = logits.to(DEV), label.to(DEV)
        _lib.call("msu_seg_sweep", 0, lg.data_ptr(), lb.data_ptr(), B, N, thr.data_ptr(), K,
                  buf.data_ptr() + guard * 8, ops._s(lg))
        torch.cuda.synchronize()
        host = buf.cpu().numpy()
        assert (host[:guard] == sentinel).all() and (host[guard + n:] == sentinel).all()
        assert np.array_equal(host[guard:guard + n].reshape(B, 2, K + 1), ref.histogram(logits, label, ts))


def test_two_calls_are_bitwise_equal():
    logits, label = _random_case(torch.bfloat16)
    ts = ref.thresholds(255)
    a, b = _hist(logits, label, ts), _hist(logits, label, ts)
    assert a.tobytes() == b.tobytes() and a.sum() == 4 * 96 * 160
    assert (a[:, :, 1:-1] > 0).sum() > 400  # the interior (LDS atomic) path did the work


def _write_split(root, n):
    """Three synthetic n^2 PNGs with masks (the second one 'real': empty mask) and test.txt."""
    g = torch.Generator().manual_seed(21)
    names = ["0900001", "0000002", "0900003"]
    masks = cases.blob_masks(3, n, n, 5, fake=[True, False, True]).numpy()
    for d in ("fake_images", "fake_labels", "real_images", "real_labels", "lists"):
        os.makedirs(os.path.join(root, d))
    for name, m in zip(names, masks):
        kind = "fake" if name.startswith("09") else "real"
        img = torch.randint(0, 256, (n, n, 3), generator=g, dtype=torch.uint8).numpy()
        Image.fromarray(img).save(os.path.join(root, f"{kind}_images", name + ".png"))
        Image.fromarray((m * 255).astype(np.uint8)).save(os.path.join(root, f"{kind}_labels", name + "_mask.png"))
    with open(os.path.join(root, "lists", "test.txt"), "w") as f:
        f.write("\n".join(names) + "\n")
    return names


def _same(a, b):
    return a == b or (isinstance(a, float) and np.isnan(a) and np.isnan(b))


def test_evaluate_and_test_split_with_sweep(tmp_path):
    """evaluate(sweep=T): the entry at t = 0.5 is evaluate(threshold=0.5) for every shared key,
    sweep=None returns what it returned before; test_split(sweep=T) reports the same sweep and
    leaves its other fields alone."""
    from semantic_segmentation_of_stylegan2_artifacts_amd import predict, validation
    from semantic_segmentation_of_stylegan2_artifacts_amd.dataset.dataset import SegArtifact_dataset
    from semantic_segmentation_of_stylegan2_artifacts_amd.network.model_parts import MSUNetSys
    spec = cases.model_cases()["tiny224"]
    cfg = make_cfg(**spec["cfg"])
    model = MSUNetSys(img_size=cfg["img_size"], embed_dim=cfg["embed_dim"], depths=cfg["depths"],
                      num_heads=cfg["num_heads"], drop_path_rate=0.0)
    model.load_state_dict(cases.model_params(cfg, spec["seed"]), strict=True)
    model = model.to(DEV)
    root = str(tmp_path / "data")
    _write_split(root, cfg["img_size"])
    db = SegArtifact_dataset(base_dir=root, list_dir=os.path.join(root, "lists"), split="test", transform=None)
    batches = list(predict.dataset_batches(db, 2, torch.device(DEV)))
    pairs = [(b[0], b[1]) for b in batches]
    T = validation.default_thresholds(9)
    assert T[4] == 0.5
    base = validation.evaluate(model, pairs, threshold=0.5, amp_dtype=torch.bfloat16)
    assert "sweep" not in base and set(base) == {
        "soft_dice", "soft_iou", "bin_dice", "bin_iou", "recall", "precision", "bin_f1", "accuracy", "mean_fpr",
        "accuracy_all", "score", "n_fake", "n_real"}
    full = validation.evaluate(model, pairs, threshold=0.5, amp_dtype=torch.bfloat16, sweep=T)
    sweep = full.pop("sweep")
    assert full == base or all(_same(full[k], base[k]) for k in base)
    assert sweep["thresholds"] == T and (sweep["n_fake"], sweep["n_real"]) == (2, 1)
    shared = [k for k in base if k in sweep and isinstance(sweep[k], list)]
    assert set(shared) == {"bin_dice", "bin_iou", "recall", "precision", "bin_f1", "accuracy", "mean_fpr",
                           "accuracy_all"}
    for k in shared:
        assert sweep[k][4] == base[k], k
    # and at another threshold, through the other reduction
    other = validation.evaluate(model, pairs, threshold=T[2], amp_dtype=torch.bfloat16)
    for k in shared:
        assert sweep[k][2] == other[k], k
    assert 0.0 <= sweep["pooled"]["auroc"] <= 1.0 and 0.0 <= sweep["pooled"]["average_precision"] <= 1.0
    assert sweep["pooled"]["n_pos"] + sweep["pooled"]["n_neg"] == 3 * cfg["img_size"] ** 2

    plain = predict.test_split(model, batches, (0.2, 0.8, 0.45), threshold=0.5, keep_maps=False)
    swept = predict.test_split(model, batches, (0.2, 0.8, 0.45), threshold=0.5, keep_maps=False, sweep=T)
    assert "sweep" not in plain.summary and swept._fields == plain._fields
    assert swept.summary.pop("sweep") == sweep
    assert json.dumps(predict._jsonable(swept.summary)) == json.dumps(predict._jsonable(plain.summary))
    assert json.dumps(predict._jsonable(swept.per_image)) == json.dumps(predict._jsonable(plain.per_image))
    assert swept[:4] == plain[:4] or all(_same(a, b) for a, b in zip(swept[:4], plain[:4]))
    # unlabelled batches: maps only, nothing to sweep
    res = predict.test_split(model, [(b[0], None, b[2]) for b in batches], (0.2, 0.8, 0.45), keep_maps=False, sweep=T)
    assert res.summary is None


def test_command_line_sweep(tmp_path, capsys):
    """predict --sweep 9 --select bin_dice: threshold_sweep.csv with one row per threshold,
    summary.sweep and selected_threshold in metrics.json; the maps are written as without it."""
    import yaml
    from semantic_segmentation_of_stylegan2_artifacts_amd import checkpoint, load_config, predict, validation
    from semantic_segmentation_of_stylegan2_artifacts_amd.network import MSUNet
    root = str(tmp_path / "data")
    names = _write_split(root, 224)
    cfg_path = str(tmp_path / "config.yaml")
    with open(cfg_path, "w") as f:
        yaml.safe_dump({"DATA": {"IMG_SIZE": 224, "DATA_PATH": root, "BATCH_SIZE": 2},
                        "LIST_DIR": os.path.join(root, "lists"),
                        "MODEL": {"SWIN": {"EMBED_DIM": 32, "DEPTHS": [2, 2, 2, 2], "NUM_HEADS": [1, 2, 4, 8]}}}, f)
    config = load_config(cfg_path)
    torch.manual_seed(0)
    checkpoint.save_best(MSUNet(config, img_size=224, num_classes=1), 3, 0.5, str(tmp_path))
    out_dir = str(tmp_path / "out")
    stamp = predict.main(["--cfg", cfg_path, "--check_point_dir", str(tmp_path), "--out_dir", out_dir,
                          "--sweep", "9", "--select", "bin_dice"])
    assert capsys.readouterr().out.strip().splitlines()[-1] == stamp
    run = os.path.join(out_dir, "test_" + stamp)
    assert sorted(os.listdir(run)) == ["config_used.yaml", "metrics.json", "predictions", "threshold_sweep.csv"]
    assert sorted(os.listdir(os.path.join(run, "predictions"))) == \
           sorted(p.format(n) for n in names for _, p in predict.MAP_FILES)
    with open(os.path.join(run, "metrics.json")) as f:
        m = json.load(f)
    sweep = m["summary"]["sweep"]
    assert sweep["thresholds"] == validation.default_thresholds(9) and len(sweep["bin_dice"]) == 9
    assert m["selected_threshold"] == sweep["thresholds"][int(np.argmax(sweep["bin_dice"]))]
    assert m["selection"] == {"key": "bin_dice", "max_fpr": None}
    with open(os.path.join(run, "threshold_sweep.csv")) as f:
        rows = list(csv.DictReader(f))
    assert len(rows) == 9
    assert [float(r["threshold"]) for r in rows] == sweep["thresholds"]
    assert [float(r["bin_dice"]) for r in rows] == sweep["bin_dice"]
    assert [float(r["mean_fpr"]) for r in rows] == sweep["mean_fpr"]
    # an explicit list and a bound on the mean FPR
    out2 = str(tmp_path / "out2")
    stamp = predict.main(["--cfg", cfg_path, "--check_point_dir", str(tmp_path), "--out_dir", out2,
                          "--sweep_thresholds", "0.3,0.5", "--select", "bin_dice:1.0"])
    with open(os.path.join(out2, "test_" + stamp, "metrics.json")) as f:
        m2 = json.load(f)
    assert m2["summary"]["sweep"]["thresholds"] == [0.3, 0.5] and m2["selected_threshold"] in (0.3, 0.5)
    assert m2["selection"] == {"key": "bin_dice", "max_fpr": 1.0}
    assert m2["summary"]["sweep"]["bin_dice"][1] == sweep["bin_dice"][4]
    # the argument errors come before anything is loaded
    for bad in (["--select", "bin_dice"], ["--sweep", "9", "--no_labels"], ["--sweep", "3", "--sweep_thresholds", "0.5"],
                ["--sweep", "9", "--select", "soft_dice"], ["--sweep", "9", "--select", "bin_dice:low"]):
        with pytest.raises(SystemExit):
            predict.main(["--cfg", cfg_path, "--check_point_dir", str(tmp_path), "--out_dir", out_dir] + bad)
    capsys.readouterr()
