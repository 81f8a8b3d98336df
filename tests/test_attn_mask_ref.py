"""CPU: properties of tests/_attn_mask_ref.py alone (the host restatement of the attention
dropout streams of csrc/common.h), so that the yardstick of tests/test_gpu_attn_dropout.py is
sound before a GPU is involved.

The statistical caps are far outside the sampling noise: over the 81 x 32 items x 49 x 49 =
6.2 M bits used here the sd of a fraction is ~1.2e-4 (equal-bits fraction) / ~1.8e-4 (kept
fraction at p = 0.3); the restatement gives kept fractions 0.949981 (p = 0.05) and 0.699663
(p = 0.3) at seed 1234, and equal-bits deviations <= 1.9e-4.
"""
import numpy as np
import pytest

import _attn_mask_ref as mr

N_ITEMS = 81 * 32
SEED = 1234
_CACHE = {}


def _mask(p, seed=SEED, counter=None):
    key = (p, seed, counter)
    if key not in _CACHE:
        m = mr.keep_mask(N_ITEMS, seed, p, counter)
        m.setflags(write=False)
        _CACHE[key] = m
    return _CACHE[key]


def test_words_cover_every_key_once():
    keys = [j for hh in range(2) for n in range(mr.WORDS) for j in mr.word_keys(n, hh)]
    assert sorted(keys) == list(range(64))


def test_fmix32_known_values():
    # murmur3's finaliser maps 0 to 0; idx = 0 leaves the seed as its input
    assert int(mr.fmix32_hash(0, 0)) == 0
    assert int(mr.fmix32_hash(1, 0)) == 0x514E28B7  # fmix32(1), murmur3's published avalanche
    assert int(mr.fmix32_hash(0, 1)) == int(mr.fmix32_hash(0x9E3779B9, 0))


@pytest.mark.parametrize("p,thr", [(0.05, 3277), (0.25, 16384), (0.5, 32768), (0.3, 19661)])
def test_drop_thresh16(p, thr):
    assert mr.drop_thresh16(p) == thr


def test_seed_above_32_bits_folds():
    big = (5 << 40) + 77
    folded = 77 ^ (5 << 8)
    assert mr.drop_seed32(big) == folded
    assert np.array_equal(mr.keep_mask(7, big, 0.25), mr.keep_mask(7, folded, 0.25))
    assert not np.array_equal(mr.keep_mask(7, big, 0.25), mr.keep_mask(7, 77, 0.25))


def test_launch_seed():
    assert mr.launch_seed(99) == 99
    assert mr.launch_seed(99, None) == 99
    assert mr.launch_seed(99, 0) != 99
    assert len({mr.launch_seed(99, c) for c in range(64)}) == 64
    assert all(0 <= mr.launch_seed((1 << 63) - 1, c) < (1 << 64) for c in (0, 1, (1 << 63) - 1))


def test_no_counter_differs_from_counter_zero():
    assert not np.array_equal(mr.keep_mask(7, SEED, 0.25), mr.keep_mask(7, SEED, 0.25, counter=0))


def test_shape_and_determinism():
    a = mr.keep_mask(5, SEED, 0.3)
    assert a.shape == (5, 49, 49) and a.dtype == np.bool_
    assert np.array_equal(a, mr.keep_mask(5, SEED, 0.3))
    # an item's mask does not depend on how many items are built with it
    assert np.array_equal(a[:3], mr.keep_mask(3, SEED, 0.3))


@pytest.mark.parametrize("p", [0.05, 0.3])
def test_kept_fraction(p):
    kept = _mask(p).mean()
    want = 1.0 - mr.drop_thresh16(p) / 65536.0
    print(f"p {p}: kept {kept:.6f}, expected {want:.6f}")
    assert abs(kept - want) <= 5e-4, kept


def _equal_fraction(a, b):
    return (a == b).mean()


@pytest.mark.parametrize("p", [0.05, 0.3])
def test_independence(p):
    """Equal-bits fraction of two independent Bernoulli(1 - p) masks: (1 - p)^2 + p^2."""
    want = (1 - p) ** 2 + p ** 2
    m = _mask(p)
    pairs = {
        "adjacent items": (m[:-1], m[1:]),
        "adjacent query rows": (m[:, :-1], m[:, 1:]),
        "adjacent keys": (m[:, :, :-1], m[:, :, 1:]),
        "seeds s, s + 1": (m, _mask(p, SEED + 1)),
    }
    for c in range(4):
        pairs[f"counters {c}, {c + 1}"] = (_mask(p, SEED, c), _mask(p, SEED, c + 1))
    for what, (a, b) in pairs.items():
        f = _equal_fraction(a, b)
        print(f"p {p} {what}: equal {f:.6f}, expected {want:.6f}")
        assert abs(f - want) <= 1e-3, (what, f)
