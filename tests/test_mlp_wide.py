"""CPU: the Swin-B widths of the streamed-weight fused MLP (csrc/mlp_s1.hip): the library and
ops.MLP_KERNEL_SHAPES agree on which shapes are built, msunet::mlp's fake kernel reports the fused
route's outputs for them, and every instantiation of the kernel in the built library is free of
scratch (these kernels read LDS through untracked inline asm: a spilled fragment register ahead
of its wait is the failure tests/test_lds_hazards.py exists to catch)."""
import os
import re
import shutil
import subprocess
import sys
import tempfile

import pytest
import torch

from semantic_segmentation_of_stylegan2_artifacts_amd import _lib, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
READELF = "/opt/rocm/llvm/bin/llvm-readelf"

# the widths this family adds (hidden 4 C); a width without a shipped kernel is absent from
# MLP_KERNEL_SHAPES altogether
WIDE = tuple(s for s in ((128, 512), (256, 1024)) if s in ops.MLP_KERNEL_SHAPES)
NEAR_MISSES = ((128, 256), (128, 1024), (256, 512), (512, 2048))


def test_swin_b_stage0_width_is_a_kernel_shape():
    assert (128, 512) in ops.MLP_KERNEL_SHAPES
    assert ops.MLP_KERNEL_SHAPES[0] == (96, 384), "MSU_MLP_S1=0 keeps the first shape only"


def test_supported_shapes_agree_with_the_library():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built")
    L = _lib.lib()
    assert L.msu_mlp_fused_supported(128, 512) == 1
    for C, Hd in ((128, 512), (256, 1024)) + NEAR_MISSES:
        assert ((C, Hd) in ops.MLP_KERNEL_SHAPES) == bool(L.msu_mlp_fused_supported(C, Hd)), (C, Hd)
    for C, Hd in NEAR_MISSES:
        assert not L.msu_mlp_fused_supported(C, Hd), (C, Hd)


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("C,Hd", WIDE)
def test_mlp_fake_reports_the_fused_route(C, Hd, dt, monkeypatch):
    from torch._subclasses.fake_tensor import FakeTensorMode
    monkeypatch.setattr(ops, "_MLP_TRAIN", True)
    monkeypatch.setattr(ops, "_MLP_INFER", True)
    monkeypatch.setattr(ops, "MLP_FUSED_SHAPES", ops.MLP_KERNEL_SHAPES)
    with FakeTensorMode():
        x = torch.empty(4, 7, C, device="cuda", dtype=dt)
        w1, w2 = torch.empty(Hd, C, device="cuda"), torch.empty(C, Hd, device="cuda")
        b1, b2 = torch.empty(Hd, device="cuda"), torch.empty(C, device="cuda")
        y, h, g = torch.ops.msunet.mlp(x, w1, b1, w2, b2, True)
        assert y.shape == (4, 7, C) and y.dtype == dt
        assert h.shape == (4, 7, Hd) and h.dtype == dt and g.numel() == 0
        y, h, g = torch.ops.msunet.mlp(x, w1, b1, w2, b2, False)
        assert y.shape == (4, 7, C) and h.numel() == 0 and g.numel() == 0


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
            # one YAML map per kernel under amdhsa.kernels: "- .agpr_count: ..." opens it
            for block in re.split(r"\n\s*- \.", notes):
                name = re.search(r"\.name:\s+(\S+)", block)
                if name is None or ".vgpr_count:" not in block:
                    continue
                out[name.group(1)] = {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\s*(?:\n|$)", block)}
    finally:
        shutil.rmtree(work, ignore_errors=True)
    return out


def test_mlp_s1_instantiations_have_no_scratch():
    if not os.path.exists(_lib.LIB_PATH) or not os.path.exists(READELF):
        pytest.skip("library not built / llvm-readelf missing")
    meta = {k: v for k, v in _kernel_metadata(_lib.LIB_PATH).items() if "mlp_s1_kernel" in k}
    # per shipped streamed width: bf16 / f16, with and without the H store
    widths = [s[0] for s in ops.MLP_KERNEL_SHAPES if s != (96, 384)]
    assert len(meta) == 4 * len(widths), sorted(meta)
    for C in widths:  # the width is the kernel's last template argument: ...ELi<C>EEEv... mangled
        assert len([k for k in meta if f"ELi{C}EEE" in k]) == 4, (C, sorted(meta))
    for name, m in meta.items():
        # every field indexed directly: a renamed key is an error, not a pass
        assert m["private_segment_fixed_size"] == 0, (name, m["private_segment_fixed_size"])
        assert m["vgpr_count"] <= 256, (name, m["vgpr_count"])
        assert m["vgpr_spill_count"] == 0, (name, m["vgpr_spill_count"])
