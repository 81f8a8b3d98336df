"""CPU: the Linear weight-gradient launcher's plan (csrc/gemm_wgrad.hip) through
``msu_linear_wgrad_plan``, which runs the launcher's own ``wave_plan`` / ``pick_splits`` /
``split_rows`` arithmetic without a HIP call, and the argument guards of ``msu_linear_wgrad_ld``.

* every 16-bit plan that names the wave kernel names one of its sixteen instantiations
  (``MSU_WAVE`` in ``run_wave``; anything else would return -3 at run time), its splits cover M in
  whole stages, and ``msu_wgrad_workspace`` holds its partial slabs;
* which of the eight (waves along N, waves along K) splits the model's Linears and the shapes of
  tests/test_gpu_wgrad.py reach at wave tile 96 and 128 -- see ``test_reachability``.
"""
import ctypes
import os

import pytest

from semantic_segmentation_of_stylegan2_artifacts_amd import _lib

pytestmark = pytest.mark.skipif(not os.path.exists(_lib.LIB_PATH), reason="library not built")

F32, BF16, F16 = 0, 1, 2
SPLITS = [(1, 1), (2, 1), (4, 1), (1, 2), (2, 2), (1, 4), (3, 1), (1, 3)]
WAVE_INSTANCES = {(ntw, wn, wk) for ntw in (6, 8) for wn, wk in SPLITS}  # MSU_WAVE list in run_wave
MS = [1, 31, 1000, 4099, 65549, 524288]


def plan(dtype, M, N, K):
    out = (ctypes.c_int * 6)()
    rc = _lib.lib().msu_linear_wgrad_plan(dtype, M, N, K, out)
    assert rc == 0, (rc, dtype, M, N, K)
    return tuple(out)


def _wgrad_ld(dtype, M, N, K, ldw):
    return _lib.lib().msu_linear_wgrad_ld(dtype, None, None, None, ldw, None, None, M, N, K, 0, None)


# ------------------------------------------------------------------ argument guards
BAD_ARGS = {
    "N-not-8": (4, 100, 96, 96),
    "N-4": (4, 4, 96, 96),
    "K-not-8": (4, 96, 100, 100),
    "K-12": (4, 96, 12, 12),
    "M-negative": (-1, 96, 96, 96),
    "ldw-below-K": (4, 96, 96, 88),
    "ldw-zero": (4, 96, 192, 0),
    "M-zero-N-not-8": (0, 100, 96, 96),     # ahead of the M == 0 early return too
    "M-zero-ldw-below-K": (0, 96, 96, 95),
}


@pytest.mark.parametrize("dtype", [F32, BF16, F16], ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("case", sorted(BAD_ARGS))
def test_bad_arguments_are_refused_before_any_hip_call(case, dtype):
    """Null pointers, M > 0, no device: a refused call returns -2 and touches nothing."""
    M, N, K, ldw = BAD_ARGS[case]
    assert _wgrad_ld(dtype, M, N, K, ldw) == -2


@pytest.mark.parametrize("dtype", [F32, BF16, F16], ids=["f32", "bf16", "f16"])
def test_plan_query_refuses_what_the_launcher_refuses(dtype):
    out = (ctypes.c_int * 6)()
    q = _lib.lib().msu_linear_wgrad_plan
    assert q(dtype, 4, 100, 96, out) == -2
    assert q(dtype, 4, 96, 100, out) == -2
    assert q(dtype, -1, 96, 96, out) == -2
    assert q(dtype, 0, 96, 96, out) == 0


# ------------------------------------------------------------------ launchable plans
WIDTHS = sorted(set(range(96, 1537, 96)) | set(range(128, 1537, 128)))


@pytest.mark.parametrize("N", WIDTHS)
def test_every_plan_is_launchable(N):
    ws = _lib.lib().msu_wgrad_workspace
    for K in WIDTHS:
        for M in MS:
            for dtype in (F32, BF16, F16):
                ntw, wn, wk, rows, S, mchunk = plan(dtype, M, N, K)
                what = (dtype, M, N, K, (ntw, wn, wk, rows, S, mchunk))
                if dtype == F32:
                    assert ntw == 0, what
                if ntw:
                    assert (ntw, wn, wk) in WAVE_INSTANCES, what
                    wt = 16 * ntw
                    assert N % (wn * wt) == 0 and K % (wk * wt) == 0, what  # whole workgroup tiles
                    nw = 3 if wn * wk == 3 else 4
                    assert rows == 32 * (nw // (wn * wk)), what
                else:
                    assert (wn, wk, rows) == (1, 1, 64), what
                assert S >= 1 and S * mchunk >= M, what
                assert mchunk % rows == 0, what
                assert ws(M, N, K) >= S * (N * K + N), what
            assert plan(BF16, M, N, K) == plan(F16, M, N, K)


# ------------------------------------------------------------------ reachability
def _linears(C):
    """(N, K) = (out, in) features of every nn.Linear of the model at embed width C: per stage
    width d the block's qkv / proj / mlp.0 / mlp.3, PatchMerging.reduction, PatchExpand.expand and
    the two input halves of concat_back_dim; FinalPatchExpand_X4_V2.expand."""
    out = [(16 * C, C)]
    for d in (C, 2 * C, 4 * C, 8 * C):
        out += [(3 * d, d), (d, d), (4 * d, d), (d, 4 * d), (2 * d, 4 * d), (2 * d, d)]
    return out


# the (N, K) in units of the wave tile that tests/test_gpu_wgrad.py runs for each split
GPU_TEST_SHAPES = {(1, 1): (1, 1), (2, 1): (2, 1), (1, 2): (1, 2), (3, 1): (3, 1), (1, 3): (1, 3),
                   (4, 1): (4, 1), (1, 4): (1, 4), (2, 2): (2, 2)}


def test_reachability():
    """What this build reports, M = 4099 (the split does not depend on M):

    * the model's Linears reach six of the eight splits at tile 96 -- (1,1) (2,1) (3,1) (4,1) (1,4)
      (2,2) -- and five at tile 128: none of them has K = 2 or 3 tiles against one N tile, so (1,2)
      and (1,3) are reached only by other callers' shapes (N, K) = (t, 2t), (t, 3t), which
      tests/test_gpu_wgrad.py runs;
    * (128, 128) is reported as (0, 1, 1): the generic kernel.  With one wave per (N, K) tile all
      four waves split the rows, a stage is 128 rows of dY [128 + 8] and X [128 + 8] = 68 KB, and
      the ring that fits 160 KB is 2 stages deep, below the 3-stage minimum.  The ring depth
      depends only on (tile, wn, wk), so no shape reaches ``MSU_WAVE(8, 1, 1)`` -- the only
      instantiation whose cross-wave reduction takes two passes (HALVES == 2): it is dead code.
      Every other tile-128 split keeps a 3-stage ring.
    """
    for C, ntw in ((96, 6), (128, 8)):
        model = {plan(BF16, 4099, N, K)[:3] for N, K in _linears(C)}
        want = {(ntw, 1, 1), (ntw, 2, 1), (ntw, 3, 1), (ntw, 4, 1), (ntw, 1, 4), (ntw, 2, 2)}
        if C == 128:
            want = (want - {(8, 1, 1)}) | {(0, 1, 1)}
        assert model == want, (C, sorted(model))
        for (wn, wk), (a, b) in GPU_TEST_SHAPES.items():
            got = plan(BF16, 4099, a * C, b * C)[:3]
            if (ntw, wn, wk) == (8, 1, 1):
                assert got == (0, 1, 1)
            else:
                assert got == (ntw, wn, wk), (C, wn, wk, got)
    # (8, 1, 1) at any width: a shape picks (1, 1) when no other split divides its tile counts
    for N in range(128, 4097, 128):
        for K in range(128, 4097, 128):
            assert plan(F16, 4099, N, K)[:3] != (8, 1, 1), (N, K)
    assert plan(BF16, 4099, 128, 128) == (0, 1, 1, 64, 9, 512)
    assert plan(BF16, 4099, 640, 128)[:4] == (0, 1, 1, 64)  # 5 x 1 tiles: (1, 1) again
    assert plan(BF16, 4099, 96, 96) == (6, 1, 1, 128, 5, 896)
    assert plan(BF16, 4099, 480, 96)[:4] == (6, 1, 1, 128)
