"""What the device sample cache buys the loader-fed training step: four arms in one process.

Workload: the Swin-T 1024^2 bs 8 bf16 training step of ``bench.py`` (same config, model, Trainer
arguments and seed as its single-GPU main; the PNG set is its ``_write_png_set``), fed by

* ``resident``  -- batches that already sit on the device (``data.batch_pool``), the bench's figure;
* ``uncached``  -- ``GpuBatchLoader`` as ``bench.py``'s ``loader_fed`` leg runs it: every file decoded;
* ``cache_fill`` -- ``GpuBatchLoader(cache=...)`` with a fresh ``DeviceSampleCache``: the epoch that
  decodes every file once and fills the rows;
* ``cache_warm`` -- the next epoch through the same cache: nothing to decode, a few KB uploaded.

An "epoch" is one pass of ``epoch_plan`` over the PNG set (``--fake`` + ``--real`` files, every one
used every epoch, so the warm epoch has no miss); the resident arm runs as many steps.  Whole epochs
are timed between synchronises, so a loader arm includes starting its producer and the first,
unoverlapped batch.  After a warm-up (resident steps, one uncached epoch) the arms alternate for
``--repeats`` rounds, the order rotating by one each round (``cache_warm`` always follows its
``cache_fill``).  Decode threads as in ``bench.py``: ``min(16, CPUs in the affinity mask)``.

Prints, and writes to ``--out`` (default ``profiles/loader_cache_ab.txt``), per arm: img/s and
ms/step by round with median, min and max, the files decoded per epoch, and the two gaps to the
resident arm with the spread of each.

    python tools/loader_cache_ab.py [--repeats 5] [--fake 144] [--real 96] [--out FILE]
"""
import argparse
import os
import shutil
import statistics
import sys
import tempfile
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import bench  # noqa: E402  (the PNG writer; importing runs nothing)
from semantic_segmentation_of_stylegan2_artifacts_amd import load_config  # noqa: E402
from semantic_segmentation_of_stylegan2_artifacts_amd.data import batch_pool  # noqa: E402
from semantic_segmentation_of_stylegan2_artifacts_amd.dataset import (DeviceSampleCache, GpuBatchLoader,  # noqa: E402
                                                                      RandomGenerator, SegArtifact_dataset, epoch_plan)
from semantic_segmentation_of_stylegan2_artifacts_amd.network import MSUNet  # noqa: E402
from semantic_segmentation_of_stylegan2_artifacts_amd.trainer import Trainer  # noqa: E402


class CountingDataset(SegArtifact_dataset):
    decodes = 0

    def read_raw(self, idx):
        CountingDataset.decodes += 1  # a statistic: a lost update under threads would show below
        return super().read_raw(idx)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--fake", type=int, default=144)
    ap.add_argument("--real", type=int, default=96)
    ap.add_argument("--img", type=int, default=1024)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "loader_cache_ab.txt"))
    a = ap.parse_args()
    if a.repeats < 3:
        raise SystemExit("loader_cache_ab: at least three repeats per arm")
    if not torch.cuda.is_available():
        raise SystemExit("loader_cache_ab: needs a HIP device (timings are not taken on a CPU)")
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    # bench.py's single-GPU trainer set-up
    cfg = load_config(None, "swin_t", **{"DATA.IMG_SIZE": a.img, "DATA.BATCH_SIZE": a.batch})
    torch.manual_seed(cfg.SEED)
    model = MSUNet(cfg, img_size=a.img, num_classes=1).to(device)
    model.ms_unet.skip_dead_branches = False  # the bench default (no --skip-dead)
    trainer = Trainer(model, cfg, device, world_size=1, process_group=None, rank=0, seed=cfg.SEED,
                      grad_wire_dtype=None)
    pool = batch_pool(2, a.batch, a.img, device, cfg.SEED)
    threads = max(1, min(16, len(os.sched_getaffinity(0))))
    root = tempfile.mkdtemp(prefix="msu_png_")
    try:
        bench._write_png_set(root, a.fake, a.real, a.img, cfg.SEED)
        tf = RandomGenerator(output_size=[a.img, a.img], random_flip_flag=True, transform=True)
        db_fake = CountingDataset(root, root, "fake", transform=tf)
        db_real = CountingDataset(root, root, "real", transform=tf)
        epoch_no = [0]

        def loader(cache):
            e = epoch_no[0]
            epoch_no[0] += 1
            mixed, sampler, _, _ = epoch_plan(db_fake, db_real, epoch_num=e, seed=cfg.SEED)
            return GpuBatchLoader(mixed, sampler, device=device, num_threads=threads, slots=3, seed=cfg.SEED,
                                  epoch=e, batches_per_step=a.batch // 2, cache=cache)

        n_steps = len(loader(None))
        if n_steps < 10:
            raise SystemExit(f"loader_cache_ab: an epoch of {n_steps} steps is too short to time")

        def timed(run):
            torch.cuda.synchronize()
            d0 = CountingDataset.decodes
            t0 = time.perf_counter()
            k = run()
            torch.cuda.synchronize()
            return time.perf_counter() - t0, k, CountingDataset.decodes - d0

        def run_resident():
            for i in range(n_steps):
                trainer.step(*pool[i % len(pool)])
            return n_steps

        def run_loader(cache):
            k = 0
            for b in loader(cache):
                trainer.step(b["image"], b["label"])
                k += 1
            return k

        for i in range(a.warmup):
            trainer.step(*pool[i % len(pool)])
        timed(lambda: run_loader(None))

        arms = ("resident", "uncached", "cache_fill", "cache_warm")
        res = {arm: [] for arm in arms}
        units = ["resident", "uncached", "cache"]
        caches = []
        for r in range(a.repeats):
            for unit in units[r % 3:] + units[:r % 3]:
                if unit == "resident":
                    res["resident"].append(timed(run_resident))
                elif unit == "uncached":
                    res["uncached"].append(timed(lambda: run_loader(None)))
                else:
                    caches[:] = []  # the previous round's rows go back to the allocator first
                    cache = DeviceSampleCache(a.img, a.img, device=device, max_samples=a.fake + a.real)
                    caches.append(cache)
                    res["cache_fill"].append(timed(lambda: run_loader(cache)))
                    res["cache_warm"].append(timed(lambda: run_loader(cache)))
        stats = caches[-1].stats()

        say(f"loader_cache_ab: Swin-T {a.img}^2 bs {a.batch} bf16 training step, "
            f"{'graph replay' if trainer._graph is not None else 'eager'}, {torch.cuda.get_device_name(device)}")
        say(f"PNG set {a.fake} fake + {a.real} real (compress_level 1), {n_steps} steps per epoch, "
            f"{threads} decode threads, {a.repeats} alternating rounds, warm-up {a.warmup} resident steps + 1 uncached epoch")
        say(f"cache: {stats['rows_used']} rows of {stats['capacity']}, {stats['nbytes'] / 2**20:.0f} MiB "
            f"({stats['nbytes'] / max(1, stats['capacity']) / 2**20:.0f} MiB per sample)")
        say()
        say(f"{'arm':<11} {'img/s med':>9} {'min':>7} {'max':>7}   {'ms/step med':>11} {'min':>7} {'max':>7}   decodes/epoch   img/s by round")
        rate = {}
        for arm in arms:
            ips = [k * a.batch / t for t, k, _ in res[arm]]
            ms = [t / k * 1e3 for t, k, _ in res[arm]]
            dec = sorted({d for _, _, d in res[arm]})
            rate[arm] = ips
            say(f"{arm:<11} {statistics.median(ips):9.2f} {min(ips):7.2f} {max(ips):7.2f}   "
                f"{statistics.median(ms):11.3f} {min(ms):7.3f} {max(ms):7.3f}   {'/'.join(map(str, dec)):>13}   "
                + " ".join(f"{v:.2f}" for v in ips))
        say()
        med = {arm: statistics.median(v) for arm, v in rate.items()}
        for arm in ("uncached", "cache_fill", "cache_warm"):
            gaps = [(1 - v / med["resident"]) * 100 for v in rate[arm]]
            say(f"gap {arm:<10} vs resident (median {med['resident']:.2f} img/s): "
                f"{(1 - med[arm] / med['resident']) * 100:+.2f} % at the medians, by round {min(gaps):+.2f} .. {max(gaps):+.2f} %")
        rs = rate["resident"]
        say(f"spread of the resident arm itself: {(max(rs) - min(rs)) / med['resident'] * 100:.2f} % (max - min over median)")
        lo_w, hi_u = min(rate["cache_warm"]), max(rate["uncached"])
        say("cache_warm vs uncached: " + (
            f"faster outside the spread (slowest warm round {lo_w:.2f} > fastest uncached round {hi_u:.2f} img/s)"
            if lo_w > hi_u else
            f"NOT faster outside the spread (slowest warm round {lo_w:.2f}, fastest uncached round {hi_u:.2f} img/s)"))
    finally:
        shutil.rmtree(root, ignore_errors=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
