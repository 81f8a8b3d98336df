"""Test-split evaluation with prediction maps: the reference's ``test.py``.

``test.py`` loads ``best_model.pth``, runs ``calculate_metrics`` over the test split one image
at a time (``scripts/validation_functions.py:37-211``: per-image DynamicLoss and metrics, the
f32 probability map of every image copied to the host) and renders each map on the CPU
(``create_bin_heat_mask_from_list``, ``save_color_heatmap`` and ``overlay_mask_on_image`` of
``scripts/map_generator.py``).  Here the forwards are batched and one HIP pass per batch
(``ops.prediction_maps`` / ``msu_pred_maps``) turns the logits into the per-image metric sums,
the BCE sum and the finished byte images; only ``[B, 12]`` doubles and bytes reach the host.

    python -m semantic_segmentation_of_stylegan2_artifacts_amd.predict --cfg FILE \\
        --check_point_dir DIR --out_dir DIR [--batch_size N] [--no_labels] [--ema] [--cache]
        [--sweep N | --sweep_thresholds a,b,c] [--select KEY[:MAX_FPR]]

(``--ema``: the averaged weights a checkpoint saved with ``ema_state=`` holds under ``"model_ema"``.)
``--sweep`` / ``--sweep_thresholds``: the binary metrics at every threshold of a list from the same
forwards (``validation.threshold_histogram``), written to ``threshold_sweep.csv`` and
``summary.sweep``; ``--select`` adds the chosen operating point (``validation.select_threshold``).

Not ported: the matplotlib figure with a colour bar that ``save_color_heatmap`` draws around
the overlay (``{case}_heatmap.png`` holds the overlay array itself), tensorboard, tqdm, csv.
``overlay_mask_on_image`` traces external contours with cv2 and draws them two pixels thick;
the outline here is the two-pixel band along every edge of the mask, holes included.
"""
import argparse
import csv
import json
import math
import os
import shutil
import sys
from collections import namedtuple
from datetime import datetime

import numpy as np
import torch
from PIL import Image

from . import ops, validation

MASK_THRESHOLD = 0.4   # create_bin_heat_mask_from_list: binmsk = heat > 0.4
HEAT_ALPHA = 0.45      # save_color_heatmap(alpha=0.45)
MASK_ALPHA = 0.25      # overlay_mask_on_image(alpha=0.25)
MASK_COLOR = (255, 0, 255)
SMOOTH = 1e-6          # TverskyLoss smooth (loss/DynamicLoss.py:22-52)

MAP_FILES = (("heat", "{}_grey_heats.png"), ("mask", "{}_bin_mask.png"), ("image", "{}.png"),
             ("heat_rgb", "{}_heatmap.png"), ("mask_rgb", "{}_overlay_color.png"))

# calculate_metrics' return value (mean_soft_dice, output_list, Score, mean_FPR), then the
# per-image rows and the epoch summary
TestResult = namedtuple("TestResult", "mean_soft_dice output_list score mean_fpr per_image summary")


def colormap_lut():
    """matplotlib's 256-entry table of ``LinearSegmentedColormap.from_list("g2r", [(0, "green"),
    (.5, "yellow"), (1, "red")])`` in closed form, float64 [256, 3] (the kernel evaluates the
    same expressions in f32)."""
    t = np.arange(256, dtype=np.float64) / 255.0
    g0 = 128.0 / 255.0
    lo = t <= 0.5
    return np.stack([np.where(lo, 2 * t, 1.0), np.where(lo, g0 + (1 - g0) * 2 * t, 2 - 2 * t),
                     np.zeros(256)], axis=1)


def per_image_loss(row, alpha, beta, mix):
    """The reference's DynamicLoss of a batch of one (``loss/DynamicLoss.py:82-111``) from the
    image's ``prediction_maps`` sums row, in double: BCE mean, mixed with the Tversky loss when
    the mask is non-empty.  For a {0, 1} label the Tversky sums are the soft confusion sums."""
    c = [float(v) for v in row]
    inter, sum_g, soft_fp, soft_fn = c[0], c[2], c[4], c[5]
    n = c[7] + c[8] + c[9] + c[10]
    if n <= 0:
        raise ValueError(f"loss calculation failed because the image has {n} pixels")
    bce = c[11] / n
    if sum_g > 0:
        tversky = 1.0 - (inter + SMOOTH) / (inter + alpha * soft_fp + beta * soft_fn + SMOOTH)
        return (1.0 - mix) * bce + mix * tversky
    return bce


def _mean_matrix(ms, key):
    if not ms:
        return None
    return np.mean(np.array([m[key] for m in ms], dtype=float), axis=0).flatten().tolist()


def summarize_test(per_image):
    """``validation.summarize`` plus the means ``calculate_metrics`` logs (``:157-192``): mean
    val loss over all / fake / real images and the mean binary and soft confusion matrices,
    flattened [tp, fp, fn, tn] as the reference writes them (None for an empty group)."""
    out = validation.summarize(per_image)
    groups = {"": per_image, "_fake": [m for m in per_image if not m["real"]],
              "_real": [m for m in per_image if m["real"]]}
    for tag, ms in groups.items():
        out["mean_val_loss" + tag] = sum(m["val_loss"] for m in ms) / len(ms) if ms else float("nan")
        out["mean_confusion_matrix_bin" + tag] = _mean_matrix(ms, "confusion_matrix_bin")
        out["mean_confusion_matrix_soft" + tag] = _mean_matrix(ms, "confusion_matrix_soft")
    return out


def _loss_cfg(loss_cfg):
    if isinstance(loss_cfg, dict):
        return float(loss_cfg["alpha"]), float(loss_cfg["beta"]), float(loss_cfg["mix"])
    alpha, beta, mix = loss_cfg
    return float(alpha), float(beta), float(mix)


@torch.no_grad()
def test_split(model, batches, loss_cfg, *, threshold=0.5, amp_dtype=torch.bfloat16, keep_maps=True, sweep=None):
    """Run ``model`` in eval mode over the test split and return a ``TestResult``.

    ``batches`` yields ``(images, labels, case_names)``: images f32 [B, 3, H, W] in [0, 1] on
    the GPU, labels [B, H, W] / [B, 1, H, W] or None (``atrifact_prediction``: maps only),
    case_names a list of B strings (or None: running numbers).  ``loss_cfg``: (alpha, beta, mix)
    of DynamicLoss, or a dict with those keys.  ``keep_maps``: True keeps every image's maps
    (u8 numpy: heat, mask, heat_rgb, mask_rgb and the source image) in ``output_list`` as
    ``(case_name, maps)``; a callable receives ``(case_name, maps)`` instead and nothing is kept;
    False renders nothing.

    Per-image rows are ``validation.metrics_from_sums`` plus ``val_loss`` and ``case_name``
    (unlabelled: ``case_name`` only); the summary is ``summarize_test`` (None unlabelled).
    ``sweep``: a threshold sequence; the logits of every labelled batch then also go through
    ``validation.threshold_histogram`` and the summary gains ``"sweep"``
    (``validation.summarize_sweep``); the maps and every other field stay at ``threshold``."""
    alpha, beta, mix = _loss_cfg(loss_cfg)
    if sweep is not None:
        sweep = [float(t) for t in sweep]
        validation.check_thresholds(sweep)
    model.eval()
    per_image, output_list, hists = [], [], []
    count = 0
    for batch in batches:
        images, labels = batch[0], batch[1]
        names = batch[2] if len(batch) > 2 and batch[2] is not None else None
        B = images.shape[0]
        names = [str(n) for n in names] if names is not None else [str(count + i) for i in range(B)]
        if len(names) != B:
            raise ValueError(f"batch mismatch: images {B}, case names {len(names)}")
        count += B
        with torch.autocast("cuda", dtype=amp_dtype, enabled=amp_dtype != torch.float32):
            logits = model(images)
        if logits.shape[1] != 1:
            raise ValueError(f"Binary task expected 1 logit channel, got {logits.shape[1]}")
        if sweep is not None and labels is not None:
            hists.append(validation.threshold_histogram(logits, labels, sweep).numpy())
        want = (("sums",) if labels is not None else ()) + \
               (("heat", "mask", "heat_rgb", "mask_rgb") if keep_maps else ())
        if not want:
            continue
        out = ops.prediction_maps(logits, images if keep_maps else None, labels, sig_threshold=threshold,
                                  mask_threshold=MASK_THRESHOLD, heat_alpha=HEAT_ALPHA, mask_alpha=MASK_ALPHA,
                                  color=MASK_COLOR, outline=True, want=want)
        if keep_maps:
            # the dataset makes image = u8 / 255: the source bytes back, HWC
            out["image"] = (images.float() * 255.0 + 0.5).clamp_(0, 255).to(torch.uint8).permute(0, 2, 3, 1)
        host = {k: v.cpu() for k, v in out.items()}
        for i, name in enumerate(names):
            if labels is not None:
                row = host["sums"][i]
                m = validation.metrics_from_sums(row[:len(validation.COLS)])
                m["val_loss"] = per_image_loss(row.tolist(), alpha, beta, mix)
                m["case_name"] = name
                per_image.append(m)
            else:
                per_image.append({"case_name": name})
            if keep_maps:
                maps = {k: host[k][i].numpy() for k in ("heat", "mask", "heat_rgb", "mask_rgb", "image")}
                if callable(keep_maps):
                    keep_maps(name, maps)
                else:
                    output_list.append((name, maps))
    if count == 0:
        raise ValueError("Expected at least one test cases")
    labelled = [m for m in per_image if "real" in m]
    if not labelled:
        nan = float("nan")
        return TestResult(nan, output_list, nan, nan, per_image, None)
    if len(labelled) != len(per_image):
        raise ValueError("labelled and unlabelled batches cannot be mixed in one split")
    summary = summarize_test(per_image)
    if sweep is not None:
        summary["sweep"] = validation.summarize_sweep(sweep, validation.sweep_counts(np.concatenate(hists)))
    return TestResult(summary["soft_dice"], output_list, summary["score"], summary["mean_fpr"], per_image, summary)


def save_maps(case_name, maps, out_dir, image_u8=None):
    """Write one image's maps as PNGs under the reference's names: ``{case}_grey_heats.png`` and
    ``{case}_bin_mask.png`` (mode L), ``{case}.png`` (the source image: ``image_u8`` or
    ``maps["image"]``, [H, W, 3]), ``{case}_heatmap.png`` and ``{case}_overlay_color.png`` (RGB).
    Entries that are absent are not written.  Returns the paths."""
    os.makedirs(out_dir, exist_ok=True)
    maps = dict(maps)
    if image_u8 is not None:
        maps["image"] = image_u8
    paths = []
    for key, pattern in MAP_FILES:
        if maps.get(key) is None:
            continue
        a = np.ascontiguousarray(np.asarray(maps[key]))
        rgb = key in ("image", "heat_rgb", "mask_rgb")
        if a.dtype != np.uint8 or a.ndim != (3 if rgb else 2) or (rgb and a.shape[2] != 3):
            raise ValueError(f"{key} must be uint8 {'[H, W, 3]' if rgb else '[H, W]'}, got {a.shape} {a.dtype}")
        path = os.path.join(out_dir, pattern.format(case_name))
        Image.fromarray(a).save(path)  # uint8 [H, W] -> mode L, [H, W, 3] -> RGB
        paths.append(path)
    return paths


def _cached_batches(dataset, batch_size, device, cache):
    """``dataset_batches`` through a ``DeviceSampleCache``: a file is decoded the first time it
    is met (every time once the cache is full) and later passes gather its row on the device.
    Fills and gathers run on the cache's stream; the caller's stream waits for each batch."""
    from .dataset.dataset import augment_gather
    n = len(dataset)
    stream = cache.attach()
    pin = torch.empty(batch_size, cache.H, cache.W, 3, dtype=torch.uint8).pin_memory()
    pin_l = torch.empty(batch_size, cache.H, cache.W, dtype=torch.uint8).pin_memory() if cache.labels else None
    uploaded = None
    for i0 in range(0, n, batch_size):
        idx = range(i0, min(n, i0 + batch_size))
        if uploaded is not None:
            uploaded.synchronize()  # the pinned rows are free again
        with torch.cuda.device(device), torch.cuda.stream(stream):
            rows = cache.load([(dataset, i) for i in idx], pin, pin_l, staging_count=min(cache.staging, batch_size))
            uploaded = torch.cuda.Event()
            uploaded.record(stream)
            x, y = augment_gather(cache.img, cache.lbl, rows)
        cur = torch.cuda.current_stream(device)
        cur.wait_stream(stream)
        x.record_stream(cur)
        if y is not None:
            y.record_stream(cur)
        yield x, y, [dataset.sample_list[i].strip("\n") for i in idx]


def dataset_batches(dataset, batch_size, device, cache=None):
    """``(images, labels, case_names)`` batches of a ``SegArtifact_dataset`` /
    ``SegArtifact_no_label_dataset`` in list order, no augmentation: PIL decode on the host,
    /255, label threshold and HWC -> CHW in ``msu_augment_batch`` on the GPU.  ``cache``: a
    ``dataset.DeviceSampleCache``; the split is then decoded once and later passes (validation
    after every epoch) gather it from the device with ``msu_augment_gather``, same bytes."""
    if cache is not None:
        yield from _cached_batches(dataset, batch_size, device, cache)
        return
    from .dataset.dataset import augment_batch
    n = len(dataset)
    for i0 in range(0, n, batch_size):
        idx = range(i0, min(n, i0 + batch_size))
        raw = [dataset.read_raw(i) for i in idx]
        img = torch.from_numpy(np.stack([r[0] for r in raw])).to(device)
        lbl = None
        if dataset.with_labels:
            lbl = torch.from_numpy(np.stack([r[1] for r in raw])).to(device)
        x, y = augment_batch(img, lbl)
        yield x, y, [dataset.sample_list[i].strip("\n") for i in idx]


SWEEP_COLUMNS = validation.BINARY_KEYS + ("mean_fpr", "accuracy_all", "bin_score")


def write_sweep_csv(path, sweep):
    """One row per threshold of a ``validation.summarize_sweep`` dict: the per-threshold means and
    the pooled pixel-level tpr / fpr / precision (empty cells for NaN)."""
    pooled = ("tpr", "fpr", "precision")
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(("threshold",) + SWEEP_COLUMNS + tuple("pooled_" + k for k in pooled))
        for k, t in enumerate(sweep["thresholds"]):
            row = [sweep[c][k] for c in SWEEP_COLUMNS] + [sweep["pooled"][c][k] for c in pooled]
            w.writerow([repr(t)] + ["" if math.isnan(v) else repr(v) for v in row])


def _parse_select(text):
    key, _, bound = text.partition(":")
    if key not in SWEEP_COLUMNS:
        raise ValueError(f"--select: unknown key {key!r} (known: {', '.join(SWEEP_COLUMNS)})")
    return key, (float(bound) if bound else None)


def _jsonable(v):
    if isinstance(v, dict):
        return {k: _jsonable(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [_jsonable(x) for x in v]
    if isinstance(v, float) and not math.isfinite(v):
        return None
    if isinstance(v, (np.floating, np.integer)):
        return _jsonable(v.item())
    return v


def main(argv=None):
    from . import checkpoint, load_config
    from .dataset.dataset import SegArtifact_dataset, SegArtifact_no_label_dataset
    from .network.MSUNet import MSUNet

    parser = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    parser.add_argument("--cfg", type=str, required=True, metavar="FILE", help="path to config file")
    parser.add_argument("--check_point_dir", type=str, required=True, metavar="DIR",
                        help="path to directory with best_model.pth")
    parser.add_argument("--out_dir", type=str, required=True, metavar="DIR", help="path to the out dir")
    parser.add_argument("--batch_size", type=int, default=None, help="images per forward (default DATA.BATCH_SIZE)")
    parser.add_argument("--no_labels", action="store_true", help="unlabelled split: maps only")
    parser.add_argument("--ema", action="store_true",
                        help="load the checkpoint's averaged weights ('model_ema') instead of 'model'")
    parser.add_argument("--cache", action="store_true",
                        help="keep the decoded split on the device (DeviceSampleCache, 4 B / pixel): the path "
                             "a training loop's per-epoch validation takes; one pass here decodes as much")
    parser.add_argument("--sweep", type=int, default=None, metavar="N",
                        help="also report the binary metrics at the N thresholds k / (N + 1)")
    parser.add_argument("--sweep_thresholds", type=str, default=None, metavar="a,b,c",
                        help="as --sweep with an explicit ascending threshold list")
    parser.add_argument("--select", type=str, default=None, metavar="KEY[:MAX_FPR]",
                        help="with a sweep: write the threshold with the largest KEY (e.g. bin_dice) among those "
                             "with mean FPR <= MAX_FPR to metrics.json as selected_threshold")
    args = parser.parse_args(argv)
    sweep = select = None
    if args.sweep is not None and args.sweep_thresholds is not None:
        parser.error("--sweep and --sweep_thresholds exclude each other")
    if args.sweep is not None:
        sweep = validation.default_thresholds(args.sweep)
    elif args.sweep_thresholds is not None:
        sweep = [float(t) for t in args.sweep_thresholds.split(",") if t.strip()]
    if sweep is not None and args.no_labels:
        parser.error("a threshold sweep needs labels")
    if args.select is not None:
        if sweep is None:
            parser.error("--select needs --sweep or --sweep_thresholds")
        try:
            select = _parse_select(args.select)
        except ValueError as e:
            parser.error(str(e))
    config = load_config(args.cfg)
    if not torch.cuda.is_available():
        raise RuntimeError("predict needs a HIP device (no CPU fallback)")
    device = torch.device("cuda", torch.cuda.current_device())
    torch.manual_seed(int(config.SEED))

    timestamp_str = datetime.now().strftime("%d%m%y_%H%M")
    output_dir = os.path.join(os.path.abspath(args.out_dir), f"test_{timestamp_str}")
    pred_dir = os.path.join(output_dir, "predictions")
    os.makedirs(pred_dir, exist_ok=True)
    shutil.copy(args.cfg, os.path.join(output_dir, "config_used.yaml"))

    model = MSUNet(config, img_size=config.DATA.IMG_SIZE, num_classes=config.MODEL.NUM_CLASSES)
    msg = checkpoint.load_checkpoint(model, os.path.join(args.check_point_dir, "best_model.pth"), strict=True,
                                     use_ema=args.ema)
    print("loaded checkpoint", msg)
    model.to(device)

    cls = SegArtifact_no_label_dataset if args.no_labels else SegArtifact_dataset
    db_test = cls(base_dir=config.DATA.DATA_PATH, list_dir=config.get("LIST_DIR", "./lists"), split="test",
                  transform=None)
    batch_size = int(args.batch_size or config.DATA.BATCH_SIZE)
    cache = None
    if args.cache:
        from .dataset import DeviceSampleCache
        cache = DeviceSampleCache(config.DATA.IMG_SIZE, config.DATA.IMG_SIZE, labels=not args.no_labels,
                                  device=device, max_samples=len(db_test))
    res = test_split(model, dataset_batches(db_test, batch_size, device, cache=cache),
                     (config.TRAIN.TVERSKY_LOSS_ALPHA, config.TRAIN.TVERSKY_LOSS_BETA,
                      config.TRAIN.LOSS_TVERSKY_BCE_MIX),
                     threshold=config.TRAIN.SIG_THRESHOLD, amp_dtype=torch.float16,
                     keep_maps=lambda name, maps: save_maps(name, maps, pred_dir), sweep=sweep)
    report = {"date": timestamp_str, "summary": res.summary, "per_image": res.per_image}
    if sweep is not None:
        write_sweep_csv(os.path.join(output_dir, "threshold_sweep.csv"), res.summary["sweep"])
    if select is not None:
        report["selected_threshold"] = validation.select_threshold(res.summary["sweep"], *select)
        report["selection"] = {"key": select[0], "max_fpr": select[1]}
    with open(os.path.join(output_dir, "metrics.json"), "w") as f:
        json.dump(_jsonable(report), f, indent=1)
    if res.summary is not None:
        print(f"mean_dice_test: {res.mean_soft_dice:.6f}, Score: {res.score:.6f}, FPR: {res.mean_fpr:.6f}")
    print(timestamp_str, file=sys.stdout)
    return timestamp_str


if __name__ == "__main__":
    main()
