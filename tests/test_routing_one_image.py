"""CPU: test_routing.py's rule at the smallest production shape, one 1024^2 image (and 4 x 512^2).

Stage 0 then has 65 536 tokens, ``_LINBWD_MIN_M``: the one-pass Linear backward, the fused units
and the persistent convs all run, and so must every GEMM -- the x4 expand + GELU (96 -> 1536,
which the NT GEMM does not cover at K = 96) used to fall through to the library GEMM there.
Below that M the routing is as it was."""
import pytest

from semantic_segmentation_of_stylegan2_artifacts_amd import ops
from test_routing import _shapes


@pytest.mark.parametrize("C,B,img", [(96, 1, 1024), (96, 4, 512), (128, 1, 1024)])
def test_every_gemm_of_a_one_image_step_is_hand_written(C, B, img, monkeypatch):
    monkeypatch.setattr(ops, "_ROUTE_FORCE", "")
    monkeypatch.setattr(ops, "_tok_cache", {})
    lib = [s for s in _shapes(C, B, img) if ops.gemm_route(*s) == "lib"]
    assert not lib, lib
    assert ops.gemm_route(65536, 16 * 96, 96, ops.TOK_GELU_DUAL) == "tok"


def test_smaller_shapes_and_the_switches_route_as_before(monkeypatch):
    monkeypatch.setattr(ops, "_tok_cache", {})
    monkeypatch.setattr(ops, "_ROUTE_FORCE", "")
    assert ops.gemm_route(16384, 16 * 96, 96, ops.TOK_GELU_DUAL) == "lib"
    assert ops.gemm_route(2 * 56 * 56, 16 * 96, 96, ops.TOK_GELU_DUAL) == "lib"
    monkeypatch.setattr(ops, "_tok_cache", {})
    monkeypatch.setattr(ops, "_ROUTE_FORCE", "lib")
    assert ops.gemm_route(65536, 16 * 96, 96, ops.TOK_GELU_DUAL) == "lib"
