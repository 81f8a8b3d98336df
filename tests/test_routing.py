"""CPU: every 16-bit Linear GEMM of the benchmarked step routes to a hand-written kernel.

SURVEY 8(a) row 8 (torchvision's block: qkv / proj / mlp.0 / mlp.3, model_parts.py:143-151) and
the Linears around it (PatchMerging.reduction :87-95, PatchExpand.expand, concat_back_dim
:792-824, FinalPatchExpand_X4_V2.expand :458): forward and input-gradient GEMMs at the Swin-T /
Swin-S / Swin-B widths for 8 x 1024^2 (and 8 x 512^2) go to the token GEMM (csrc/gemm_tok.h) or
the persistent tiled NT GEMM (csrc/gemm_nt.hip), never to the library GEMM, unless the
MSU_GEMM_ROUTE=lib A/B switch asks for it.  The routing queries are host functions of the C-ABI
library (no GPU needed).
"""
import ctypes

import pytest

from semantic_segmentation_of_stylegan2_artifacts_amd import _lib, ops


def _shapes(C, B, img):
    """(M, N, K, epi) of every Linear forward and input gradient of the step."""
    out = []
    res = img // 4
    for s in range(4):
        c = C * 2 ** s
        M = B * (res // 2 ** s) ** 2
        for n, k in ((3 * c, c), (c, c), (c, 2 * c), (2 * c, c)):  # qkv, proj, concat, expand
            out += [(M, n, k, ops.TOK_PLAIN), (M, k, n, ops.TOK_PLAIN)]
        out += [(M, 4 * c, c, ops.TOK_GELU_DUAL), (M, c, 4 * c, ops.TOK_PLAIN),   # mlp.0 / mlp.3 fwd
                (M, 4 * c, c, ops.TOK_GELU_GRAD), (M, c, 4 * c, ops.TOK_PLAIN)]   # mlp.3 / mlp.0 dgrad
        if s < 3:  # PatchMerging reduction 4c -> 2c at the next stage's token count
            out += [(M // 4, 2 * c, 4 * c, ops.TOK_PLAIN), (M // 4, 4 * c, 2 * c, ops.TOK_PLAIN)]
    M0 = B * res * res
    out += [(M0, 16 * C, C, ops.TOK_GELU_DUAL), (M0, C, 16 * C, ops.TOK_PLAIN),  # x4 expand
            (M0, C, 48, ops.TOK_PLAIN)]  # patch embed (im2col K = 3 * 4 * 4)
    return out


@pytest.mark.parametrize("C,img", [(96, 1024), (96, 512), (128, 1024)])
def test_every_step_gemm_is_hand_written(C, img, monkeypatch):
    monkeypatch.setattr(ops, "_ROUTE_FORCE", "")
    monkeypatch.setattr(ops, "_tok_cache", {})
    lib = [(M, N, K, e) for M, N, K, e in _shapes(C, 8, img) if ops.gemm_route(M, N, K, e) == "lib"]
    assert not lib, lib


def test_lib_switch_still_reaches_the_library(monkeypatch):
    monkeypatch.setattr(ops, "_ROUTE_FORCE", "lib")
    monkeypatch.setattr(ops, "_tok_cache", {})
    assert ops.gemm_route(8 * 64 ** 2, 3 * 384, 384) == "lib"


def test_the_48_deep_token_stage_takes_the_plain_epilogue_only(monkeypatch):
    """gemm_tok_k48.hip is built for the plain epilogue without split A: at K % 48 == 0 with K a
    multiple of neither 96 nor 128 the token GEMM still takes a plain Linear, while a GELU epilogue
    and the skip fusion are routed elsewhere (they used to be promised here and refused at launch)."""
    monkeypatch.setattr(ops, "_ROUTE_FORCE", "")
    monkeypatch.setattr(ops, "_tok_cache", {})
    M = 8 * 256 ** 2
    for K in (48, 144, 240):
        assert ops.tok_supported_epi(M, 96, K, ops.TOK_PLAIN)
        assert not ops.tok_supported_epi(M, 96, K, ops.TOK_GELU_DUAL)
        assert not ops.tok_supported_epi(M, 96, K, ops.TOK_GELU_GRAD)
        assert not ops.tok_supported_cat(M, 96, K)
        assert ops.gemm_route(M, 96, K) == "tok"
        assert ops.gemm_route(M, 96, K, ops.TOK_GELU_DUAL) != "tok"
        assert ops._cat_route(M, 96, K, K // 2) != "tok"
    assert ops.tok_supported_cat(M, 96, 192) and ops._cat_route(M, 96, 192, 96) == "tok"


# (M, N, wkn) -> (tile rows, tile columns, ring depth, tiles, grid) of the NT GEMM on 256 CUs (the
# MI355X's count, and the library's fallback where no device answers): what the cost model and the
# grid sizing of csrc/gemm_nt.hip gave at 5a430d0, before the kernel's A3W2 ring and tile queue
# were removed, at mode 0.  The 18 production shapes of tools/nt_shapes.py, SHAPES + BIG (both weight
# layouts) and WIDE of tests/test_gpu_nt_gemm.py, and its three underfilled shapes.
NT_PLANS = [
    ((131072, 576, 0), (256, 192, 2, 1536, 256)),
    ((131072, 192, 0), (256, 192, 2, 512, 256)),
    ((131072, 768, 0), (256, 192, 2, 2048, 256)),
    ((32768, 1152, 0), (256, 192, 2, 768, 256)),
    ((32768, 384, 0), (256, 192, 2, 256, 256)),
    ((32768, 1536, 0), (256, 192, 2, 1024, 256)),
    ((32768, 768, 0), (256, 192, 2, 512, 256)),
    ((8192, 2304, 0), (256, 192, 2, 384, 256)),
    ((8192, 768, 0), (128, 192, 2, 256, 256)),
    ((8192, 3072, 0), (256, 192, 2, 512, 256)),
    ((32768, 384, 1), (256, 128, 3, 384, 256)),
    ((131072, 192, 1), (256, 128, 3, 1024, 256)),
    ((4096, 1152, 0), (128, 192, 2, 192, 192)),
    ((4096, 1152, 1), (256, 128, 3, 144, 144)),
    ((4096, 384, 0), (128, 128, 2, 96, 96)),
    ((4096, 384, 1), (128, 128, 2, 96, 96)),
    ((1000, 384, 0), (128, 128, 2, 24, 24)),
    ((1000, 384, 1), (128, 128, 2, 24, 24)),
    ((2048, 768, 0), (128, 128, 2, 96, 96)),
    ((2048, 768, 1), (128, 128, 2, 96, 96)),
    ((777, 192, 0), (128, 128, 2, 14, 14)),
    ((777, 192, 1), (128, 128, 2, 14, 14)),
    ((300, 2304, 0), (128, 128, 2, 54, 54)),
    ((300, 2304, 1), (128, 128, 2, 54, 54)),
    ((128, 768, 0), (128, 128, 2, 6, 6)),
    ((128, 768, 1), (128, 128, 2, 6, 6)),
    ((513, 96, 0), (128, 128, 2, 5, 5)),
    ((513, 96, 1), (128, 128, 2, 5, 5)),
    ((64, 160, 0), (128, 128, 2, 2, 2)),
    ((64, 160, 1), (128, 128, 2, 2, 2)),
    ((1, 32, 0), (128, 128, 2, 1, 1)),
    ((1, 32, 1), (128, 128, 2, 1, 1)),
    ((32768, 1152, 1), (256, 128, 3, 1152, 256)),
    ((32077, 416, 0), (256, 128, 3, 504, 256)),
    ((32077, 416, 1), (256, 128, 3, 504, 256)),
    ((65536, 640, 0), (256, 128, 3, 1280, 256)),
    ((65536, 640, 1), (256, 128, 3, 1280, 256)),
    ((32077, 384, 0), (256, 192, 2, 252, 252)),
    ((32077, 384, 1), (256, 128, 3, 378, 256)),
    ((8187, 576, 0), (128, 192, 2, 192, 192)),
]


def _nt_plan(M, N, K, wkn, epi=0):
    """(rc, (rows, columns, ring, tiles, grid), ping-pong kernel, tile-queue field, CU count) of msu_nt_gemm_plan2."""
    out = (ctypes.c_long * 8)()
    rc = _lib.lib().msu_nt_gemm_plan2(M, N, K, epi, wkn, out)
    return rc, (out[0], out[1], out[2], out[4], out[5]), out[3], out[6], out[7]


def test_nt_plan_table_is_unchanged():
    """nt_cfg's cost model and the grid sizing, pinned shape by shape; at mode 0 neither K nor the
    epilogue enters, and the field that reported the tile queue is 0."""
    lib = _lib.lib()
    prev = lib.msu_nt_gemm_mode(0)
    try:
        for (M, N, wkn), want in NT_PLANS:
            for K, epi in ((64, 0), (384, 1), (3072, 2)):
                got = _nt_plan(M, N, K, wkn, epi)
                assert got == (0, want, 0, 0, 256), ((M, N, K, wkn, epi), got, want)
    finally:
        lib.msu_nt_gemm_mode(prev)
    assert _nt_plan(4096, 100, 384, 0)[0] == -2  # N % 32
    assert _nt_plan(4096, 384, 96, 1)[0] == -2   # K % 64
    assert _lib.plan_nt(8192, 768) == (128, 192, False) and _lib.plan_nt(32768, 1152) == (256, 192, False)


def test_nt_mode_ignores_the_removed_bits():
    """msu_nt_gemm_mode: bit 0 (the ping-pong kernel) and bits 1-2 (the forced tile form) are kept;
    bits 3 and 4 (once the A3W2 ring and the tile queue) are ignored and read back 0."""
    lib = _lib.lib()
    prev = lib.msu_nt_gemm_mode(0x18)
    try:
        assert lib.msu_nt_gemm_mode(6) == 0
        assert lib.msu_nt_gemm_mode(0x1f) == 6
        assert lib.msu_nt_gemm_mode(0x18) == 7
        # with the stale bits set a launch is planned as at mode 0
        assert _nt_plan(32768, 384, 384, 0) == (0, (256, 192, 2, 256, 256), 0, 0, 256)
        # forced forms, as the tests and tools reach them: 1 -> 128 x 192, 2 -> 256 x 128, 3 -> 128 x 128
        for mode, want in ((2, (128, 192, 2)), (4, (256, 128, 3)), (6, (128, 128, 2)), (0, (256, 192, 2))):
            lib.msu_nt_gemm_mode(mode)
            assert _nt_plan(32768, 384, 384, 0)[1][:3] == want, mode
    finally:
        lib.msu_nt_gemm_mode(prev)
    assert lib.msu_nt_gemm_mode(prev) == prev
