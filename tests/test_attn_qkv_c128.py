"""CPU: the Swin-B stage-0 width of the fused qkv -> window attention -> proj unit
(csrc/window_attention_mfma.hip attn_qkv_fwd_mfma<T, 128, ...>): which (C, heads) the library says
it covers, what msu_win_attn_qkv_fwd2 refuses with -2 before any launch, and that no
instantiation of the kernel in the built library uses scratch or more than a CU's LDS."""
import ctypes
import os
import re
import shutil
import subprocess
import sys
import tempfile

import pytest

from semantic_segmentation_of_stylegan2_artifacts_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
READELF = "/opt/rocm/llvm/bin/llvm-readelf"
BF16, F16, F32 = 1, 2, 0

COVERED = ((96, 3), (128, 4))
NEAR_MISSES = ((128, 3), (96, 4), (128, 8), (192, 6), (256, 8), (64, 2))


def _library():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built")
    return _lib.lib()


def test_dtype_codes_are_the_librarys():
    """The codes this file passes as `dtype` are the ones ops passes."""
    import torch
    from semantic_segmentation_of_stylegan2_artifacts_amd import ops
    assert ops._DT[torch.float32] == F32 and ops._DT[torch.bfloat16] == BF16 and ops._DT[torch.float16] == F16


def test_supported_widths():
    L = _library()
    for C, nh in COVERED:
        assert L.msu_win_attn_qkv_supported(C, nh) == 1, (C, nh)
    for C, nh in NEAR_MISSES:
        assert L.msu_win_attn_qkv_supported(C, nh) == 0, (C, nh)


def _fwd2_null(L, dtype, B, H, W, C, nh):
    null = ctypes.c_void_p(None)
    return L.msu_win_attn_qkv_fwd2(dtype, null, null, null, null, null, null, null, null, null, null, null, B, H, W, C,
                                   nh, 3, 0.0, 0, null, null)


def test_fwd2_refuses_before_any_launch():
    """Null buffers everywhere: a call that got as far as a launch would not return -2."""
    L = _library()
    assert L.msu_win_attn_qkv_supported(128, 4) == 1
    assert _fwd2_null(L, F32, 1, 14, 14, 128, 4) == -2  # f32 at a covered width
    assert _fwd2_null(L, BF16, 1, 14, 14, 128, 3) == -2  # head count
    assert _fwd2_null(L, F16, 1, 14, 14, 128, 3) == -2
    assert 64 * 512 * 512 * 3 * 128 >= 2 ** 32
    assert _fwd2_null(L, BF16, 64, 512, 512, 128, 4) == -2  # B H W 3C >= 2^32: 32-bit row offsets


def _kernel_metadata(lib):
    """{kernel symbol: {field: value}} from the code-object notes of the gfx950 code in lib."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import lds_hazard_check as chk
    finally:
        sys.path.pop(0)
    work = tempfile.mkdtemp(prefix="msu_meta_")
    out = {}
    try:
        for obj in chk.extract_code_objects(lib, work):
            notes = subprocess.run([READELF, "--notes", obj], check=True, capture_output=True, text=True).stdout
            for block in re.split(r"\n\s*- \.", notes):
                name = re.search(r"\.name:\s+(\S+)", block)
                if name is None or ".vgpr_count:" not in block:
                    continue
                out[name.group(1)] = {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\s*(?:\n|$)", block)}
    finally:
        shutil.rmtree(work, ignore_errors=True)
    return out


def test_fused_unit_instantiations_have_no_scratch():
    """Both widths x bf16 / f16 x DROP x STORE_QKV x PROJ = 32 kernels; the 128 ones hold their
    q operand and W_proj fragments in registers for a whole window, so a spill is a slow kernel."""
    if not os.path.exists(_lib.LIB_PATH) or not os.path.exists(READELF):
        pytest.skip("library not built / llvm-readelf missing")
    meta = {k: v for k, v in _kernel_metadata(_lib.LIB_PATH).items() if "attn_qkv_fwd_mfma" in k}
    assert len(meta) == 32, sorted(meta)
    for C in (96, 128):  # the width is the second template argument
        mine = {k: v for k, v in meta.items() if re.search(rf"attn_qkv_fwd_mfmaI(t|DF16_)Li{C}E", k)}
        assert len(mine) == 16, (C, sorted(meta))
        for name, m in mine.items():
            assert m["private_segment_fixed_size"] == 0, (name, m["private_segment_fixed_size"])
            assert m["vgpr_spill_count"] == 0, (name, m["vgpr_spill_count"])
            assert m["vgpr_count"] <= 256, (name, m["vgpr_count"])
            assert m["max_flat_workgroup_size"] == 64 * 2 * (C // 32), (name, m["max_flat_workgroup_size"])
            # the images are dynamic LDS (sized at launch): nothing static beside them
            assert m["group_segment_fixed_size"] == 0, (name, m["group_segment_fixed_size"])
