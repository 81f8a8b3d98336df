"""Host restatement of the window-attention dropout mask streams (test infrastructure only).

csrc/common.h documents how the keep decisions of an item (window, head) are drawn; this file
says the same thing again in numpy integer arithmetic, independently of the library (it neither
imports it nor reads the .hip sources), so the GPU tests can compare the kernels' masks with
something other than themselves.

* ``fmix32_hash(seed, idx)``: murmur3's 32-bit finaliser of ``idx * 0x9E3779B9 + seed``.
* ``drop_thresh16(p)``: ``ceil`` of the float32 product ``p * 65536``.
* ``drop_seed32(seed)``: low half XOR high half of the 64-bit launch seed.
* ``launch_seed(seed, counter)``: the host seed, or with a device counter
  ``z = seed ^ (counter * 0x9E3779B97F4A7C15); z = (z ^ (z >> 31)) * 0xBF58476D1CE4E5B9;
  z ^ (z >> 29)`` (all mod 2^64).
* stream (item, i, hh): ``h = fmix32_hash(seed32, (item * 64 + i) * 2 + hh)``, state ``x = h | 1``,
  ``d = h``; each step is xorshift 13 / 17 / 5 on x, ``d += 362437``, word ``x + d``; the low and
  the high 16-bit half of the word are kept when ``>= thr``.
* word n of stream (item, i, hh) covers keys j0 (low half), j0 + 1 (high half) with
  ``j0 = 32 (n >> 3) + crow(2 (n & 7), hh)``, ``crow(r, h) = (r & 3) + 8 (r >> 2) + 4 h``.

``item = window * nh + head`` with the windows in (b, wy, wx) order, as
``_parity_refs.attn_ref_from_qkv`` partitions them.
"""
import numpy as np

M32 = np.uint64(0xFFFFFFFF)
M64 = (1 << 64) - 1
WORDS = 16  # words per stream: 2 x 16 halves = the 32 keys of one half of each 32-key tile pair


def _u64(a):
    return np.asarray(a, dtype=np.uint64)


def fmix32_hash(seed, idx):
    """uint32 arrays (held in uint64, every step reduced mod 2^32)."""
    x = (_u64(idx) * np.uint64(0x9E3779B9) + _u64(seed)) & M32
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x85EBCA6B)) & M32
    x ^= x >> np.uint64(13)
    x = (x * np.uint64(0xC2B2AE35)) & M32
    return x ^ (x >> np.uint64(16))


def drop_thresh16(p):
    return int(np.ceil(np.float32(p) * np.float32(65536.0)))


def drop_seed32(seed):
    seed = int(seed) & M64
    return (seed ^ (seed >> 32)) & 0xFFFFFFFF


def launch_seed(seed, counter=None):
    seed = int(seed) & M64
    if counter is None:
        return seed
    z = seed ^ (((int(counter) & M64) * 0x9E3779B97F4A7C15) & M64)
    z = ((z ^ (z >> 31)) * 0xBF58476D1CE4E5B9) & M64
    return z ^ (z >> 29)


def crow(r, h):
    return (r & 3) + 8 * (r >> 2) + 4 * h


def word_keys(n, hh):
    """Keys of the low and the high half of word n of a key-half-hh stream."""
    j0 = 32 * (n >> 3) + crow(2 * (n & 7), hh)
    return j0, j0 + 1


def drop_stream(seed32, item, i, hh):
    h = fmix32_hash(seed32, ((_u64(item) * np.uint64(64) + _u64(i)) * np.uint64(2) + _u64(hh)) & M32)
    return h | np.uint64(1), h.copy()


def drop_next2(x, d, thr):
    """One step of the streams (x, d), in place -> (keep of the low half, keep of the high half)."""
    x ^= (x << np.uint64(13)) & M32
    x ^= x >> np.uint64(17)
    x ^= (x << np.uint64(5)) & M32
    d += np.uint64(362437)
    d &= M32
    w = (x + d) & M32
    t = np.uint64(thr)
    return (w & np.uint64(0xFFFF)) >= t, (w >> np.uint64(16)) >= t


def keep_mask(n_items, seed, p, counter=None):
    """bool [n_items, 49, 49] (query, key): True where the probability is kept."""
    seed32 = drop_seed32(launch_seed(seed, counter))
    thr = drop_thresh16(p)
    item = np.arange(n_items, dtype=np.uint64).reshape(-1, 1, 1)
    i = np.arange(49, dtype=np.uint64).reshape(1, -1, 1)
    hh = np.arange(2, dtype=np.uint64).reshape(1, 1, -1)
    x, d = drop_stream(seed32, item, i, hh)  # [n_items, 49, 2]
    full = np.zeros((n_items, 49, 64), dtype=bool)
    for n in range(WORDS):
        lo, hi = drop_next2(x, d, thr)
        for h in range(2):
            j0, j1 = word_keys(n, h)
            full[:, :, j0] = lo[:, :, h]
            full[:, :, j1] = hi[:, :, h]
    return np.ascontiguousarray(full[:, :, :49])
