"""CPU: the device sample cache's row table (``DeviceSampleCache.plan`` on a ``device="cpu"``
table: first come first cached, one row per key, shared rows across dataset objects, capacity
never exceeded, overflow through staging rows, the ``stats()`` counters), ``msu_augment_gather``
refusing bad arguments before any launch (null buffers, no device needed) and ``augment_gather``'s
host-side validation (a bad index never reaches the device)."""
import ctypes
import os
from types import SimpleNamespace

import pytest
import torch

from semantic_segmentation_of_stylegan2_artifacts_amd import _lib
from semantic_segmentation_of_stylegan2_artifacts_amd.dataset import DeviceSampleCache, augment_gather

needs_lib = pytest.mark.skipif(not os.path.exists(_lib.LIB_PATH), reason="library not built")


def _ds(data_dir, names, with_labels=True):
    return SimpleNamespace(data_dir=data_dir, sample_list=list(names), with_labels=with_labels)


def _cache(**kw):
    kw.setdefault("device", "cpu")
    return DeviceSampleCache(4, 6, **kw)


# ------------------------------------------------------------------ geometry
def test_capacity_is_the_smaller_bound_and_storage_has_the_staging_rows():
    c = _cache(max_samples=10, max_bytes=7 * 4 * 6 * 4 + 5, staging=3)
    assert c.bytes_per_sample == 4 * 6 * 4 and c.capacity == 7
    assert tuple(c.img.shape) == (10, 4, 6, 3) and tuple(c.lbl.shape) == (10, 4, 6)
    assert c.img.dtype == c.lbl.dtype == torch.uint8
    assert c.nbytes == 10 * 96 == c.stats()["nbytes"]
    c = _cache(max_samples=2, max_bytes=10**9, labels=False)
    assert c.capacity == 2 and c.lbl is None and c.bytes_per_sample == 4 * 6 * 3
    assert _cache(max_bytes=96 * 5).capacity == 5
    with pytest.raises(ValueError):
        _cache()
    with pytest.raises(ValueError):
        DeviceSampleCache(0, 6, device="cpu", max_samples=1)
    # 4 MiB per labelled 1024^2 sample
    assert 1024 * 1024 * 4 == 4 << 20


# ------------------------------------------------------------------ plan
def test_first_come_assignment_and_hits():
    c = _cache(max_samples=8)
    keys = [("d", n) for n in "abcd"]
    rows, misses = c.plan(keys)
    assert rows == [0, 1, 2, 3] and misses == [(0, 0), (1, 1), (2, 2), (3, 3)]
    rows, misses = c.plan([("d", "c"), ("d", "e"), ("d", "a")])
    assert rows == [2, 4, 0] and misses == [(1, 4)]
    assert ("d", "e") in c and ("d", "z") not in c
    s = c.stats()
    assert (s["hits"], s["misses"], s["overflow_decodes"], s["rows_used"], s["capacity"]) == (2, 5, 0, 5, 8)


def test_repeated_key_in_one_call_gets_one_row_and_one_decode():
    c = _cache(max_samples=4)
    rows, misses = c.plan([("d", "a"), ("d", "b"), ("d", "a"), ("d", "a")])
    assert rows == [0, 1, 0, 0] and misses == [(0, 0), (1, 1)]
    s = c.stats()
    assert s["misses"] == 2 and s["hits"] == 2 and s["rows_used"] == 2


def test_same_name_through_two_dataset_objects_shares_a_row():
    c = _cache(max_samples=4)
    train = _ds("/data", ["x", "y"])
    again = _ds("/data", ["y", "z\n"])
    other = _ds("/elsewhere", ["y"])
    assert c.key(train, 1) == c.key(again, 0) == ("/data", "y")
    assert c.key(again, 1) == ("/data", "z")
    rows, _ = c.plan([c.key(train, 0), c.key(train, 1)])
    rows2, misses2 = c.plan([c.key(again, 0), c.key(again, 1), c.key(other, 0)])
    assert rows == [0, 1] and rows2 == [1, 2, 3]
    assert [j for j, _ in misses2] == [1, 2]  # "y" of /data was there; "y" of /elsewhere is another file


def test_capacity_is_never_exceeded_and_overflow_goes_through_staging_every_time():
    c = _cache(max_samples=3, staging=4)
    keys = [("d", str(i)) for i in range(6)]
    rows, misses = c.plan(keys)
    assert rows == [0, 1, 2, 3, 4, 5]          # staging rows follow the capacity rows
    assert [j for j, _ in misses] == list(range(6))
    assert c.rows_used == 3 and all(k in c for k in keys[:3]) and not any(k in c for k in keys[3:])
    # cached keys hit; overflow keys are misses again, in the caller's share of the staging rows
    rows, misses = c.plan([keys[4], keys[1], keys[5], keys[4]], staging_offset=2, staging_count=2)
    assert rows == [5, 1, 6, 5] and misses == [(0, 5), (2, 6)]
    s = c.stats()
    assert s["rows_used"] == 3 == s["capacity"] and s["staging"] == 4
    assert s["misses"] == 3 and s["overflow_decodes"] == 5 and s["hits"] == 2
    assert max(c._rows.values()) < c.capacity


def test_a_call_with_more_overflow_than_staging_rows_is_refused_whole():
    c = _cache(max_samples=2, staging=2)
    c.plan([("d", "a")])
    with pytest.raises(RuntimeError, match="staging"):
        c.plan([("d", "b"), ("d", "c"), ("d", "e")], staging_count=1)
    assert c.rows_used == 1 and ("d", "b") not in c     # the refused call took nothing
    rows, misses = c.plan([("d", "b"), ("d", "c")], staging_count=1)
    assert rows == [1, 2] and len(misses) == 2
    with pytest.raises(ValueError):
        c.plan([("d", "q")], staging_offset=1, staging_count=2)


def test_discard_gives_rows_back():
    c = _cache(max_samples=2)
    c.plan([("d", "a"), ("d", "b")])
    c.discard([("d", "a")])
    assert ("d", "a") not in c and c.rows_used == 1
    rows, misses = c.plan([("d", "c")])
    assert rows == [0] and misses == [(0, 0)]


def test_label_mismatch_is_refused():
    with pytest.raises(ValueError, match="label"):
        _cache(max_samples=2, labels=False).key(_ds("/d", ["a"], with_labels=True), 0)
    with pytest.raises(ValueError, match="label"):
        _cache(max_samples=2, labels=True).key(_ds("/d", ["a"], with_labels=False), 0)


def test_fill_and_load_on_a_cpu_table():
    """The planning / decode / fill path with plain host tensors standing in for the storage."""
    import numpy as np

    class DS(SimpleNamespace):
        def read_raw(self, i):
            self.decoded.append(i)
            return np.full((4, 6, 3), 10 + i, np.uint8), np.full((4, 6), 100 + i, np.uint8)

    ds = DS(data_dir="/d", sample_list=["a", "b", "c"], with_labels=True, decoded=[])
    c = _cache(max_samples=2, staging=1)
    pin, pin_l = torch.empty(3, 4, 6, 3, dtype=torch.uint8), torch.empty(3, 4, 6, dtype=torch.uint8)
    rows = c.load([(ds, 0), (ds, 1), (ds, 2)], pin, pin_l)
    assert rows == [0, 1, 2] and ds.decoded == [0, 1, 2]
    rows = c.load([(ds, 2), (ds, 0)], pin, pin_l)
    assert rows == [2, 0] and ds.decoded == [0, 1, 2, 2]   # the overflow sample again, the cached one not
    assert int(c.img[0, 0, 0, 0]) == 10 and int(c.img[1, 0, 0, 0]) == 11 and int(c.img[2, 0, 0, 0]) == 12
    assert int(c.lbl[0, 0, 0]) == 100 and int(c.lbl[2, 0, 0]) == 102
    bad = DS(data_dir="/d", sample_list=["w"], with_labels=True, decoded=[])
    bad.read_raw = lambda i: (np.zeros((5, 6, 3), np.uint8), np.zeros((5, 6), np.uint8))
    c2 = _cache(max_samples=2)
    with pytest.raises(ValueError, match="differs from the batch's"):
        c2.load([(bad, 0)], pin, pin_l)
    assert c2.rows_used == 0                                 # a failed decode keeps no row
    with pytest.raises(ValueError):
        c.fill(3, pin[0], pin_l[0])
    with pytest.raises(ValueError):
        c.fill(0, pin[0], None)


# ------------------------------------------------------------------ C ABI guards
def _gather(img=1, lbl=None, rows=1, n_rows=4, ops=None, luts=None, out=1, out_l=None, B=2, H=8, W=8):
    buf = ctypes.create_string_buffer(64)  # never read: a refused call touches nothing
    a = ctypes.addressof(buf)

    def p(v):
        return a if v == 1 else None
    return _lib.lib().msu_augment_gather(p(img), p(lbl), p(rows), n_rows, p(ops), p(luts), p(out), p(out_l),
                                         B, H, W, None)


@needs_lib
@pytest.mark.parametrize("kw", [
    dict(B=0), dict(B=-1), dict(H=0), dict(W=0), dict(W=-5), dict(n_rows=0), dict(n_rows=-3),
    dict(img=None), dict(rows=None), dict(out=None),
    dict(lbl=1, out_l=None), dict(lbl=None, out_l=1),
    dict(ops=1, luts=None),
    dict(B=65536, H=1, W=1),                       # grid.z
    dict(B=1, H=16 * 65536, W=1, n_rows=1),        # grid.y
    dict(B=1, H=1024, W=1024, n_rows=349526),      # n_rows * H * W * 3 = 2^40 + 2^21
    dict(B=1, H=1 << 20, W=349526, n_rows=1),      # one sample >= 2^40
    dict(B=1, H=(1 << 31) - 1, W=(1 << 31) - 1, n_rows=(1 << 31) - 1),  # no overflow in the check itself
], ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_gather_refuses_bad_arguments_before_any_launch(kw):
    assert _gather(**kw) == -2


@needs_lib
def test_gather_guard_reaches_call_as_an_error():
    with pytest.raises(_lib.HipLibraryError):
        _lib.call("msu_augment_gather", None, None, None, 4, None, None, None, None, 2, 8, 8, None)


# ------------------------------------------------------------------ wrapper validation (host side)
def _store(n=4, H=5, W=7):
    return torch.zeros(n, H, W, 3, dtype=torch.uint8), torch.zeros(n, H, W, dtype=torch.uint8)


@pytest.mark.parametrize("rows", [[0, 4], [-1, 2], [3, 2, 7], torch.tensor([0, 4]), torch.tensor([-1], dtype=torch.int32)])
def test_augment_gather_refuses_a_bad_index(rows):
    img, lbl = _store()
    with pytest.raises(ValueError, match="outside the store"):
        augment_gather(img, lbl, rows)


def test_augment_gather_refuses_wrong_dtypes_and_shapes():
    img, lbl = _store()
    ops = torch.zeros(2, 2, dtype=torch.int32)
    luts = torch.zeros(2, 5, 256, dtype=torch.uint8)
    bad = [
        (img.float(), lbl, [0, 1], None, None),
        (img[..., :2], lbl, [0, 1], None, None),
        (img[0], lbl, [0, 1], None, None),
        (img, lbl.float(), [0, 1], None, None),
        (img, lbl[:3], [0, 1], None, None),
        (img, lbl[:, :4], [0, 1], None, None),
        (img[:, ::2], None, [0, 1], None, None),                       # not contiguous
        (img, lbl, [], None, None),
        (img, lbl, [0.5, 1.0], None, None),
        (img, lbl, torch.tensor([[0, 1]]), None, None),
        (img, lbl, torch.tensor([0.0, 1.0]), None, None),
        (img, lbl, [0, 1], ops, None),                                 # ops without luts
        (img, lbl, [0, 1], None, luts),
        (img, lbl, [0, 1], ops.long(), luts),
        (img, lbl, [0, 1], ops[:1], luts),
        (img, lbl, [0, 1], ops, luts[:, :4]),
        (img, lbl, [0, 1], ops, luts.int()),
    ]
    for k, args in enumerate(bad):
        with pytest.raises(ValueError):
            augment_gather(*args)
            pytest.fail(f"case {k} accepted")


def test_augment_gather_has_no_cpu_fallback():
    img, lbl = _store()
    with pytest.raises(RuntimeError, match="HIP device"):
        augment_gather(img, lbl, [0, 1])
