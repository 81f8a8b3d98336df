"""Device-resident sample cache: every PNG is decoded once per run, its uint8 pixels stay in
HBM, and each step's batch is gathered from there by the augmentation kernel itself
(``msu_augment_gather``: ``augment_kernel`` reading source row ``rows[b]`` instead of ``b``).

Memory: a sample is ``H * W * 3`` image bytes plus ``H * W`` label bytes, 4 MiB at 1024^2; the
reference's training lists (800 fake + 1157 real) are 7.6 GiB of the card's 288 GB.

Rows: the storage holds ``capacity + staging`` rows.  A sample's key is ``(dataset.data_dir,
sample name)``, so two dataset objects or splits that name the same file share one row.  Rows
are handed out first come, first cached, and never taken back: an epoch touches every fake
sample and a fresh random subset of the real ones, so any sample is as likely to be wanted
again as any other and an eviction policy would only move the decodes around.  When the cache
is full, further samples are *overflow*: decoded every time they are used and passed through
one of the ``staging`` rows at the end of the storage.  Files are assumed not to change during
a run; a row is never refreshed.

Streams: a cache is owned by ONE stream.  Every fill and every gather that reads the cache
runs on that stream, and stream order is what makes a row that was written once safe to read
in every later launch (and a staging row safe to overwrite after the launch that read it).
The first user sets the owner (``attach``); a user that brings a different stream is refused.
For the same reason only one user issues work at a time: ``prefetch``, an iterating loader and
``predict.dataset_batches`` do not run concurrently on one cache.
"""
import threading
from concurrent.futures import ThreadPoolExecutor

import torch


class DeviceSampleCache:
    """``DeviceSampleCache(H, W, *, labels=True, device=None, max_samples=None, max_bytes=None,
    staging=0)``: uint8 rows ``img [capacity + staging, H, W, 3]`` and, with ``labels``,
    ``lbl [capacity + staging, H, W]`` on ``device`` (default: the current HIP device; ``"cpu"``
    keeps the row table usable without one).  ``capacity`` is the smaller of ``max_samples`` and
    ``max_bytes // bytes_per_sample``; at least one of the two is required.  The last ``staging``
    rows carry overflow samples; a ``GpuBatchLoader`` with ``slots`` slots of ``B`` samples needs
    ``slots * B`` of them once the cache can fill up."""

    def __init__(self, H, W, *, labels=True, device=None, max_samples=None, max_bytes=None, staging=0):
        H, W, staging = int(H), int(W), int(staging)
        if H <= 0 or W <= 0 or staging < 0:
            raise ValueError(f"DeviceSampleCache: bad geometry H {H}, W {W}, staging {staging}")
        if max_samples is None and max_bytes is None:
            raise ValueError("DeviceSampleCache: give max_samples, max_bytes or both")
        self.H, self.W, self.labels, self.staging = H, W, bool(labels), staging
        self.bytes_per_sample = H * W * (4 if self.labels else 3)
        caps = [int(max_samples)] if max_samples is not None else []
        if max_bytes is not None:
            caps.append(int(max_bytes) // self.bytes_per_sample)
        self.capacity = min(caps)
        if self.capacity < 0 or self.capacity + staging <= 0:
            raise ValueError(f"DeviceSampleCache: no rows (capacity {self.capacity}, staging {staging})")
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device())
        self.device = torch.device(device)
        n = self.capacity + staging
        self.img = torch.empty(n, H, W, 3, dtype=torch.uint8, device=self.device)
        self.lbl = torch.empty(n, H, W, dtype=torch.uint8, device=self.device) if self.labels else None
        self._rows = {}      # key -> row
        self._free = []      # rows given back by discard()
        self._next = 0       # first row never handed out
        self._stream = None
        self._lock = threading.Lock()
        self._hits = self._misses = self._overflow = 0

    # -------------------------------------------------------------- row table (host only)
    def key(self, dataset, idx):
        """``(data_dir, sample name)`` of sample ``idx`` of a list dataset."""
        if bool(dataset.with_labels) != self.labels:
            raise ValueError("DeviceSampleCache: a labelled dataset needs a cache with labels and an "
                             f"unlabelled one a cache without (dataset {bool(dataset.with_labels)}, "
                             f"cache {self.labels})")
        return (dataset.data_dir, dataset.sample_list[idx].strip("\n"))

    def plan(self, keys, staging_offset=0, staging_count=None):
        """Rows for ``keys``: ``(rows, misses)``.  ``rows[j]`` is the storage row that holds (or
        is about to hold) ``keys[j]``; ``misses`` lists ``(j, row)`` for every sample the caller
        has to decode and ``fill`` before it gathers, ``j`` the key's first position.  A key seen
        before is a hit; a new key takes the next free row; with no free row it is overflow and
        takes the next of the caller's staging rows ``[staging_offset, staging_offset +
        staging_count)`` (relative to ``capacity``; default: all that follow the offset), again a
        miss the next time.  A key repeated within the call gets one row and one decode."""
        if staging_count is None:
            staging_count = self.staging - staging_offset
        if staging_offset < 0 or staging_count < 0 or staging_offset + staging_count > self.staging:
            raise ValueError(f"staging rows [{staging_offset}, {staging_offset + staging_count}) are outside "
                             f"the cache's {self.staging}")
        rows, misses, local, hits = [], [], {}, 0
        with self._lock:
            for j, k in enumerate(keys):
                row = self._rows.get(k)
                if row is None:
                    row = local.get(k)
                if row is not None:
                    hits += 1
                    rows.append(row)
                    continue
                if self._free or self._next < self.capacity:
                    if self._free:
                        row = self._free.pop()
                    else:
                        row = self._next
                        self._next += 1
                    self._rows[k] = row
                elif len(local) < staging_count:
                    row = self.capacity + staging_offset + len(local)
                    local[k] = row
                else:
                    for j_, row_ in misses:  # nothing of a refused call stays planned
                        if row_ < self.capacity:
                            self._free.append(self._rows.pop(keys[j_]))
                    raise RuntimeError(
                        f"DeviceSampleCache is full ({self.capacity} rows) and this call has "
                        f"{staging_count} staging rows for its overflow samples: construct the cache "
                        "with staging >= slots * batch size")
                rows.append(row)
                misses.append((j, row))
            self._hits += hits
            self._overflow += len(local)
            self._misses += len(misses) - len(local)
        return rows, misses

    def discard(self, keys):
        """Give back the rows of ``keys`` whose fill never happened (a decode failed)."""
        with self._lock:
            for k in keys:
                row = self._rows.pop(k, None)
                if row is not None:
                    self._free.append(row)

    def __contains__(self, key):
        return key in self._rows

    @property
    def rows_used(self):
        return len(self._rows)

    @property
    def nbytes(self):
        return (self.capacity + self.staging) * self.bytes_per_sample

    def stats(self):
        """Counters since construction: ``hits`` (samples served from a row filled earlier),
        ``misses`` (decodes that filled a cache row), ``overflow_decodes`` (decodes that went
        through a staging row), ``rows_used``, ``capacity``, ``staging`` and ``nbytes``."""
        return {"hits": self._hits, "misses": self._misses, "overflow_decodes": self._overflow,
                "rows_used": self.rows_used, "capacity": self.capacity, "staging": self.staging,
                "nbytes": self.nbytes}

    # -------------------------------------------------------------- stream ownership
    def attach(self, stream=None):
        """The owning stream.  ``stream`` None: the owner, created on first use.  Otherwise the
        first caller's stream becomes the owner and any other stream raises ``RuntimeError``."""
        with self._lock:
            if stream is None:
                if self._stream is None:
                    self._stream = torch.cuda.Stream(self.device)
                return self._stream
            if self._stream is None:
                self._stream = stream
            elif self._stream != stream:
                raise RuntimeError("DeviceSampleCache is owned by one stream: every fill and gather runs "
                                   "there (stream order keeps a filled row readable); a second user "
                                   "must not bring a stream of its own")
            return self._stream

    # -------------------------------------------------------------- device side
    def fill(self, row, img_u8, lbl_u8=None):
        """Copy one decoded sample from pinned host memory into ``row``, asynchronously on the
        current stream (the owning one)."""
        if not 0 <= row < self.capacity + self.staging:
            raise ValueError(f"row {row} outside the cache's {self.capacity + self.staging}")
        if (lbl_u8 is None) == self.labels:
            raise ValueError("fill: label given to a label-less cache, or missing for a labelled one")
        self.img[row].copy_(img_u8, non_blocking=True)
        if self.labels:
            self.lbl[row].copy_(lbl_u8, non_blocking=True)

    def load(self, refs, img_pin, lbl_pin, *, staging_offset=0, staging_count=None, pool=None, check=None):
        """Rows for the samples ``refs = [(dataset, index), ...]``: plans them, decodes the
        misses (on ``pool`` when given) into ``img_pin[j]`` / ``lbl_pin[j]`` (pinned uint8, ``j``
        the sample's position) and fills their rows on the current stream.  The caller must not
        touch the pinned rows again before those copies are done.  ``check(image)``: the
        transform's own validation.  Returns the row list for ``augment_gather``."""
        keys = [self.key(ds, i) for ds, i in refs]
        rows, misses = self.plan(keys, staging_offset, staging_count)
        img_np = img_pin.numpy()
        lbl_np = None if lbl_pin is None else lbl_pin.numpy()
        want = (self.H, self.W, 3)

        def decode(m):
            j = m[0]
            ds, i = refs[j]
            im, lb = ds.read_raw(i)
            if check is not None:
                check(im)
            if im.shape != want:
                raise ValueError(f"sample {keys[j][1]}: image {im.shape} differs from the batch's {want}")
            img_np[j] = im
            if lbl_np is not None:
                lbl_np[j] = lb

        try:
            if pool is not None:
                list(pool.map(decode, misses))
            else:
                for m in misses:
                    decode(m)
        except BaseException:
            self.discard(keys[j] for j, _ in misses)
            raise
        for j, row in misses:
            self.fill(row, img_pin[j], None if lbl_pin is None else lbl_pin[j])
        return rows

    def prefetch(self, dataset, indices=None, num_threads=8, chunk=8):
        """Decode and fill samples of ``dataset`` (``indices``: default all, in order) ahead of
        training, ``chunk`` at a time on ``num_threads`` threads, until the cache is full; samples
        already cached are skipped.  Must not run while a loader iterates this cache.  Returns
        the number of samples decoded."""
        from .loader import resolve
        todo, seen = [], set()
        room = self.capacity - self.rows_used
        for i in (range(len(dataset)) if indices is None else indices):
            if len(todo) >= room:
                break
            ds, r = resolve(dataset, int(i))
            k = self.key(ds, r)
            if k not in self._rows and k not in seen:
                seen.add(k)
                todo.append((ds, r))
        if not todo:
            return 0
        stream = self.attach()
        bufs = [(torch.empty(chunk, self.H, self.W, 3, dtype=torch.uint8).pin_memory(),
                 torch.empty(chunk, self.H, self.W, dtype=torch.uint8).pin_memory() if self.labels else None,
                 [None]) for _ in range(2)]
        with ThreadPoolExecutor(num_threads) as pool, torch.cuda.device(self.device), torch.cuda.stream(stream):
            for n, c0 in enumerate(range(0, len(todo), chunk)):
                img_pin, lbl_pin, ev = bufs[n % 2]
                if ev[0] is not None:
                    ev[0].synchronize()
                self.load(todo[c0:c0 + chunk], img_pin, lbl_pin, staging_count=0, pool=pool)
                ev[0] = torch.cuda.Event()
                ev[0].record(stream)
        stream.synchronize()
        return len(todo)
