"""CPU: the Swin-B stage-1 width of the streamed-weight fused MLP (256 -> 1024, csrc/mlp_s1.hip
``mlp_s1_kernel_pc``) is listed and dispatched: ops.MLP_KERNEL_SHAPES and the library agree, the
wider Swin-B stages stay on the GEMM pair, and msu_mlp_fused_fwd's argument checks cover the new
shape.  Those checks sit ahead of every HIP call, so the entry point is called with fake 16-B
aligned pointers and M = 0 on a machine without a device: nothing is touched."""
import os

import pytest

from semantic_segmentation_of_stylegan2_artifacts_amd import _lib, ops

F32, BF16, F16 = 0, 1, 2
needs_lib = pytest.mark.skipif(not os.path.exists(_lib.LIB_PATH), reason="library not built")


def test_stage1_width_is_listed_and_wider_stages_are_not():
    assert (256, 1024) in ops.MLP_KERNEL_SHAPES
    assert ops.MLP_KERNEL_SHAPES[0] == (96, 384), "MSU_MLP_S1=0 keeps the first shape only"
    assert (384, 1536) not in ops.MLP_KERNEL_SHAPES and (512, 2048) not in ops.MLP_KERNEL_SHAPES


@needs_lib
def test_library_reports_the_width():
    L = _lib.lib()
    assert L.msu_mlp_fused_supported(256, 1024) == 1
    assert L.msu_mlp_fused_supported(256, 512) == 0
    assert L.msu_mlp_fused_supported(256, 768) == 0


def _fwd(dtype, C, Hd, M=0, off=None):
    """msu_mlp_fused_fwd on fake pointers (never dereferenced: every case returns before a HIP
    call); ``off``: index of the pointer moved 8 bytes off its 16-B alignment."""
    p = [0x10000 * (i + 1) for i in range(7)]  # x, w1, b1, w2, b2, y, h
    if off is not None:
        p[off] += 8
    return _lib.lib().msu_mlp_fused_fwd(dtype, *p, M, C, Hd, None)


@needs_lib
def test_empty_call_is_accepted_and_bad_arguments_are_refused():
    assert _fwd(BF16, 256, 1024) == 0
    assert _fwd(F16, 256, 1024) == 0
    for off in range(7):
        assert _fwd(BF16, 256, 1024, off=off) == -2, off
    assert _fwd(F32, 256, 1024) == -2
    assert _fwd(BF16, 256, 512) == -2
    assert _fwd(BF16, 256, 1024, M=-1) == -2
