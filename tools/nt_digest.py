"""SHA-256 digests of what csrc/gemm_nt.hip writes on seeded operands, through the C ABI: for
every (form, layout, epilogue, bias, split A) of tests/test_gpu_gemm_matrix.py's NT table (tables,
operands and the banded launch imported from it), bf16 and f16, nk = K / 64 in {1, 2, 3, 5}, at the
matrix's three shapes per column group, a digest of Y (and of Y2 under the GELU dual epilogue).
Only msu_nt_gemm / _kn / _cat and the forced tile form of msu_nt_gemm_mode (bits 1-2) are called,
and the CU count comes from torch, so the same script runs on any build of the library.  A change
that keeps the summation order and the waits of every form keeps every line; compare two builds with
    MSU_LIB_OVERRIDE=/other/libmsunet_hip.so python tools/nt_digest.py > a.txt
    python tools/nt_digest.py > b.txt && diff a.txt b.txt
(the '#' line names the library, by its path from the repository's root, and is the only one allowed
to differ)."""
import hashlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_gpu_gemm_matrix as M  # noqa: E402
from semantic_segmentation_of_stylegan2_artifacts_amd import _lib  # noqa: E402


def digest(t):
    return hashlib.sha256(t.contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()[:24]


def shape(grp, sh, cus):
    """(M, N) of the matrix's shape names (its _nt_shape, without the plan call)."""
    if grp == "n128":
        return {"one": (1, 32), "ragged": (100, 160), "large": (128 * -(-9 * 2 * cus // 8) + 37, 160)}[sh]
    return {"one": (1, 192), "ragged": (100, 384), "large": (256 * (2 * cus + 2) + 37, 192)}[sh]


lib = _lib.lib()
cus = torch.cuda.get_device_properties(0).multi_processor_count
print(f"# library: {os.path.relpath(_lib.LIB_PATH, ROOT)}")
prev = lib.msu_nt_gemm_mode(0)
try:
    for grp, sh, dt, nk in M.NT_CASES:
        Mr, N = shape(grp, sh, cus)
        K = 64 * nk
        o, wk = M._nt_operands(dt, Mr, N, K, False, sorted({64, K - 64}) if nk >= 2 and grp == "n128" else ())
        for form in dict(M.NT_SHAPES[grp])[sh]:
            lib.msu_nt_gemm_mode(M.NT_FORMS[form][0])
            for layout, epi, bias, K1 in M._nt_variants(form, nk):
                tag = f"{form} {layout} epi{epi}{'+b' if bias else ''}{' cat%d' % K1 if K1 else ''} {M.DTNAME[dt]} {Mr}x{N}x{K}"
                y, y2 = M._nt_launch(o, tag, layout, epi, bias, K1, wk)
                print(f"{tag}: Y {digest(y)}" + (f" Y2 {digest(y2)}" if y2 is not None else ""))
        del o, wk
        torch.cuda.empty_cache()
finally:
    lib.msu_nt_gemm_mode(prev)
