"""CPU: the LayerNorm entry points refuse shapes no kernel can address, before any launch.

The checks in csrc/layernorm.hip sit ahead of the ``rows == 0`` early return and of every HIP
call, so the three entry points are called here with null buffers and ``rows > 0`` on a machine
without a device: a refused call returns its code and touches nothing.

* ``-2``: ``C % VW != 0`` (VW = 8 for 16-bit storage, 4 for f32: rows of whole 16-byte chunks),
  ``C > 2048``, and in merge mode ``Cin % VW != 0`` (a chunk would straddle two of the four
  gathered quadrants and the last row would read past the tensor), ``C != 4 * Cin``, odd ``H`` or
  ``W`` (PatchMerging asserts both even; ``H >> 1`` would drop the last line).
* ``-3``: ``msu_layernorm_bwd3``'s rule for the extra residual gradients (``dres2`` needs
  ``dres``, ``dres3`` needs ``dres2``, neither exists in merge / d2s mode).
"""
import ctypes
import os

import pytest

from semantic_segmentation_of_stylegan2_artifacts_amd import _lib

pytestmark = pytest.mark.skipif(not os.path.exists(_lib.LIB_PATH), reason="library not built")

F32, BF16, F16 = 0, 1, 2
PLAIN, ADD, MERGE, D2S2 = 0, 1, 2, 3


def _fwd(dtype, mode, rows, C, H=0, W=0, Cin=0):
    return _lib.lib().msu_layernorm_fwd(dtype, mode, None, None, None, 1, None, None, None, None, None, None,
                                        rows, C, H, W, Cin, 1e-5, None)


def _bwd(dtype, mode, rows, C, H=0, W=0, Cin=0):
    return _lib.lib().msu_layernorm_bwd(dtype, mode, None, None, None, None, None, None, None, None, None, 1,
                                        None, 1, None, None, rows, C, H, W, Cin, 0, None)


def _bwd3(dtype, mode, rows, C, H=0, W=0, Cin=0, dres=None, dres2=None, dres3=None):
    return _lib.lib().msu_layernorm_bwd3(dtype, mode, None, None, dres, dres2, dres3, None, None, None, None, None,
                                         None, 1, None, 1, None, None, rows, C, H, W, Cin, 0, None)


ENTRY = [_fwd, _bwd, _bwd3]

# (dtype, mode, rows, C, H, W, Cin)
BAD_SHAPES = {
    "merge-bf16-Cin12": (BF16, MERGE, 4, 48, 4, 4, 12),   # C % 8 == 0 but a chunk straddles quadrants
    "merge-f16-Cin12": (F16, MERGE, 4, 48, 4, 4, 12),
    "merge-f32-Cin6": (F32, MERGE, 4, 24, 4, 4, 6),        # C % 4 == 0, Cin % 4 != 0
    "merge-C-not-4Cin": (F32, MERGE, 4, 64, 4, 4, 32),
    "merge-odd-H": (BF16, MERGE, 4, 64, 5, 4, 16),
    "merge-odd-W": (BF16, MERGE, 4, 64, 4, 5, 16),
    "merge-odd-H-f32": (F32, MERGE, 4, 64, 3, 4, 16),
    "merge-odd-W-f32": (F32, MERGE, 4, 64, 4, 7, 16),
    "plain-bf16-C100": (BF16, PLAIN, 4, 100, 0, 0, 0),     # 100 % 8 != 0
    "plain-f16-C12": (F16, PLAIN, 4, 12, 0, 0, 0),
    "plain-f32-C6": (F32, PLAIN, 4, 6, 0, 0, 0),
    "add-f32-C98": (F32, ADD, 4, 98, 0, 0, 0),
    "d2s-bf16-C20": (BF16, D2S2, 16, 20, 2, 2, 0),
    "merge-f32-C18": (F32, MERGE, 4, 18, 4, 4, 4),
    "plain-f32-C2052": (F32, PLAIN, 4, 2052, 0, 0, 0),
    "plain-bf16-C2056": (BF16, PLAIN, 4, 2056, 0, 0, 0),
    "add-f16-C4096": (F16, ADD, 4, 4096, 0, 0, 0),
    "d2s-f32-C2304": (F32, D2S2, 16, 2304, 2, 2, 0),
    "merge-bf16-C2080": (BF16, MERGE, 4, 2080, 4, 4, 520),
}


@pytest.mark.parametrize("entry", ENTRY, ids=["fwd", "bwd", "bwd3"])
@pytest.mark.parametrize("case", sorted(BAD_SHAPES))
def test_unaddressable_shape_is_refused(entry, case):
    dtype, mode, rows, C, H, W, Cin = BAD_SHAPES[case]
    assert entry(dtype, mode, rows, C, H, W, Cin) == -2


def test_guards_sit_before_the_empty_early_return():
    """rows == 0 is a no-op only for a shape that could run."""
    for entry in ENTRY:
        assert entry(BF16, MERGE, 0, 48, 4, 4, 12) == -2
        assert entry(F32, MERGE, 0, 64, 5, 4, 16) == -2
        assert entry(BF16, MERGE, 0, 64, 4, 4, 16) == 0
        assert entry(F32, PLAIN, 0, 96) == 0
        assert entry(F16, D2S2, 0, 96, 3, 5, 0) == 0


def test_bwd3_residual_rule():
    """dres2 / dres3 are never read on a refused call: any non-null address will do."""
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    for mode in (PLAIN, ADD):
        assert _bwd3(BF16, mode, 4, 96, dres=None, dres2=p) == -3            # dres2 without dres
        assert _bwd3(BF16, mode, 4, 96, dres=None, dres2=p, dres3=p) == -3
        assert _bwd3(F32, mode, 4, 96, dres=p, dres2=None, dres3=p) == -3     # dres3 without dres2
        assert _bwd3(F32, mode, 4, 96, dres=None, dres2=None, dres3=p) == -3
    assert _bwd3(BF16, MERGE, 4, 64, 4, 4, 16, dres=p, dres2=p) == -3         # merge / d2s have no residual
    assert _bwd3(BF16, D2S2, 16, 96, 2, 2, 0, dres=p, dres2=p) == -3
    assert _bwd3(F32, D2S2, 16, 96, 2, 2, 0, dres=p, dres2=p, dres3=p) == -3


def test_call_raises_for_a_refused_merge_width():
    """ops.merge_layer_norm reaches the library through _lib.call: a refused width is an error
    (HipLibraryError), never a result."""
    with pytest.raises(_lib.HipLibraryError):
        _lib.call("msu_layernorm_fwd", BF16, MERGE, None, None, None, 1, None, None, None, None, None, None,
                  4, 48, 4, 4, 12, 1e-5, None)
    with pytest.raises(_lib.HipLibraryError):
        _lib.call("msu_layernorm_bwd", F32, MERGE, None, None, None, None, None, None, None, None, None, 1,
                  None, 1, None, None, 4, 24, 4, 4, 6, 0, None)
