"""CPU: gradient accumulation over micro-batches (``Trainer(accum_steps=k)``) -- what needs no device.

* ``trainer.accum_split`` is the window's cut: ``torch.tensor_split``'s sizes and the f32 shares
  ``B_i / n`` the loss kernels are handed.
* The constructor's argument rule and its default, ``config.TRAIN.ACCUMULATION_STEPS``.
* ``msu_dynloss_fwd4`` refuses a weight or a ``first`` it cannot honour before any launch: called
  here with null buffers on a machine without a device, as tests/test_capi_ln_guards.py calls the
  LayerNorm entries.
* ``GradBucketer.hold`` on two gloo ranks: a held backward neither counts nor launches, the
  window's last backward learns the accumulation counts of a single backward, overlaps its buckets
  from the second window on, and the one all-reduce per window leaves both ranks with the gradient
  of the global batch of all four micro-batches.
"""
import os

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from semantic_segmentation_of_stylegan2_artifacts_amd import _lib
from semantic_segmentation_of_stylegan2_artifacts_amd.trainer import FlatGroup, GradBucketer, is_no_decay

from test_dp_gloo import _data, _free_port, _model

needs_lib = pytest.mark.skipif(not os.path.exists(_lib.LIB_PATH), reason="library not built")


# ----------------------------------------------------------------------------- the split rule
@pytest.mark.parametrize("n,k,sizes", [(4, 2, [2, 2]), (5, 3, [2, 2, 1]), (7, 7, [1] * 7), (8, 1, [8])])
def test_accum_split_sizes_and_weights(n, k, sizes):
    from semantic_segmentation_of_stylegan2_artifacts_amd.trainer import accum_split
    parts = accum_split(n, k)
    assert [b - a for a, b, _ in parts] == sizes
    assert sizes == [t.numel() for t in torch.tensor_split(torch.arange(n), k)]
    assert parts[0][0] == 0 and parts[-1][1] == n
    assert all(parts[i][1] == parts[i + 1][0] for i in range(k - 1))
    for (a, b, w), size in zip(parts, sizes):
        assert isinstance(w, float)
        assert w == torch.tensor(size / n, dtype=torch.float64).to(torch.float32).item()  # one rounding
    assert abs(sum(w for _, _, w in parts) - 1.0) <= k * 2.0 ** -24
    if k == 1:
        assert parts == [(0, n, 1.0)]


def test_accum_split_refuses_what_it_cannot_cut():
    from semantic_segmentation_of_stylegan2_artifacts_amd.trainer import accum_split
    for n, k in ((1, 2), (0, 1), (6, 7), (4, 0), (4, -2), (4, 2.0), (4, True), (4, "2"), (4, None)):
        with pytest.raises(ValueError):
            accum_split(n, k)


# ----------------------------------------------------------------------------- the constructor
def _trainer(conf=None, **kw):
    from semantic_segmentation_of_stylegan2_artifacts_amd import load_config
    from semantic_segmentation_of_stylegan2_artifacts_amd.trainer import Trainer
    conf = load_config(None, "swin_t") if conf is None else conf
    return Trainer(torch.nn.Linear(8, 8), conf, "cpu", use_graph=False, **kw)


@pytest.mark.parametrize("bad", [True, False, 2.0, 0, -1, "2"])
def test_constructor_refuses_bad_accum_steps(bad):
    with pytest.raises(ValueError, match="accum_steps"):
        _trainer(accum_steps=bad)


def test_accum_steps_defaults_to_the_config_key():
    from semantic_segmentation_of_stylegan2_artifacts_amd import load_config
    assert _trainer().accum_steps == 1  # the reference's default
    assert _trainer(load_config(None, "swin_t", **{"TRAIN.ACCUMULATION_STEPS": 4})).accum_steps == 4
    assert _trainer(load_config(None, "swin_t", **{"TRAIN.ACCUMULATION_STEPS": 4}), accum_steps=2).accum_steps == 2
    conf = load_config(None, "swin_t")
    del conf.TRAIN["ACCUMULATION_STEPS"]
    assert _trainer(conf).accum_steps == 1
    assert _trainer(conf, accum_steps=3).accum_steps == 3
    with pytest.raises(ValueError, match="accum_steps"):
        _trainer(load_config(None, "swin_t", **{"TRAIN.ACCUMULATION_STEPS": 0}))
    # the window-loss buffer exists only for a window
    assert _trainer()._window_loss is None and _trainer(accum_steps=2)._window_loss is not None


def test_grad_bucketer_hold_is_off_by_default():
    m = _model()
    red = GradBucketer([FlatGroup(list(m.named_parameters())[::-1], 0.0, "cpu")], 1 << 20)
    assert red.hold is False


# ----------------------------------------------------------------------------- the C-ABI guards
F32, BF16 = 0, 1


def _fwd4(w, first, B=2, dtype=F32):
    return _lib.lib().msu_dynloss_fwd4(dtype, None, None, B, 1000, 0.2, 0.8, 0.45, None, 1, None, None, None,
                                       None, None, w, first, None)


@needs_lib
@pytest.mark.parametrize("w", [0.0, -0.5, float("inf"), float("-inf"), float("nan")])
def test_fwd4_refuses_a_weight_that_is_no_share(w):
    for first in (0, 1):
        assert _fwd4(w, first) == -2
        assert _fwd4(w, first, dtype=BF16) == -2


@needs_lib
@pytest.mark.parametrize("first", [-1, 2, 255])
def test_fwd4_refuses_first_outside_0_1(first):
    assert _fwd4(0.5, first) == -2
    assert _fwd4(1.0, first) == -2


@needs_lib
def test_fwd4_refuses_more_samples_than_the_final_kernel_holds():
    """fwd3 notices B > 64 after its first launch; fwd4 before it."""
    assert _fwd4(0.5, 1, B=65) == -2
    assert _fwd4(0.5, 0, B=0) == -2


@needs_lib
def test_call_raises_for_a_refused_window_weight():
    with pytest.raises(_lib.HipLibraryError):
        _lib.call("msu_dynloss_fwd4", F32, None, None, 2, 1000, 0.2, 0.8, 0.45, None, 1, None, None, None,
                  None, None, float("nan"), 1, None)


def test_loss_window_registration_round_trip():
    """ops.set_loss_window mirrors set_step_flag: registered, reported unused until a launch, cleared."""
    from semantic_segmentation_of_stylegan2_artifacts_amd import ops
    acc = torch.zeros(())
    try:
        ops.set_loss_window(acc, 0.25, False)
        assert ops._loss_window[:3] == [acc, 0.25, False] and ops.loss_window_used() is False
        assert ops._window_for(torch.zeros(2)) is ops._loss_window
    finally:
        ops.set_loss_window(None)
    assert ops._loss_window[0] is None and ops._window_for(torch.zeros(2)) is None


# ----------------------------------------------------------------------------- the held reducer
WINDOWS, MICRO, CHUNK = 3, 2, 3


def _chunk(window, rank, j):
    return _data(10 * window + MICRO * rank + j, n=CHUNK)


def _groups(m):
    named = list(m.named_parameters())
    decay = [(n, p) for n, p in named if not is_no_decay(n, p)][::-1]
    nodecay = [(n, p) for n, p in named if is_no_decay(n, p)][::-1]
    return [FlatGroup(decay, 0.01, "cpu"), FlatGroup(nodecay, 0.0, "cpu")]


def _window_worker(rank, world, port, bucket_bytes, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    m = _model()
    groups = _groups(m)
    red = GradBucketer(groups, bucket_bytes)
    for window in range(WINDOWS):
        held = None
        for j in range(MICRO):
            last = j == MICRO - 1
            red.hold = not last
            x, y = _chunk(window, rank, j)
            # this micro-batch's share of the global mean: 1 / (MICRO * world) of equal chunks
            (((m(x) - y) ** 2).mean() / (MICRO * world)).backward()
            if not last:
                held = (list(red.launches), list(red.pending), len(red.works))
        overlapped = list(red.launches)  # issued by the last backward itself, before finish()
        red.finish()
        grads = torch.cat([p.grad.reshape(-1).clone() for g in groups for p in g.params])
        out[(rank, window)] = {"grads": grads, "held": held, "overlapped": [(b, via) for b, _, via, _ in overlapped],
                               "launches": [(b, via) for b, _, via, _ in red.last_launches],
                               "expected": list(red.expected), "buckets": len(red.buckets)}
        for g in groups:
            g.grad.zero_()
    dist.destroy_process_group()


@pytest.mark.parametrize("bucket_bytes", [64, 1 << 20])
def test_held_micro_batches_leave_one_allreduce_per_window(bucket_bytes):
    world = 2
    out = mp.Manager().dict()
    mp.spawn(_window_worker, args=(world, _free_port(), bucket_bytes, out), nprocs=world, join=True)
    # the accumulation counts of ONE backward, from a bucketer that never reduces
    m = _model()
    single = GradBucketer(_groups(m), bucket_bytes)
    x, y = _chunk(0, 0, 0)
    ((m(x) - y) ** 2).mean().backward()
    counts = list(single.pending)
    assert max(counts) > 1  # the shared layer accumulates twice: a held backward that counted would show
    for window in range(WINDOWS):
        for rank in range(world):
            r = out[(rank, window)]
            nb = r["buckets"]
            assert r["held"] == ([], [0] * nb, 0), "the held backward counted or launched"
            assert r["expected"] == counts
            assert sorted(b for b, _ in r["launches"]) == list(range(nb))  # each bucket exactly once
            if window == 0:  # the counts are learned here: everything from finish()
                assert r["overlapped"] == [] and all(via == "finish" for _, via in r["launches"])
            else:  # the last micro-batch's backward overlaps its buckets
                assert r["overlapped"] == r["launches"] and all(via == "hook" for _, via in r["launches"])
        m = _model()
        named = list(m.named_parameters())
        xs, ys = zip(*[_chunk(window, rank, j) for rank in range(world) for j in range(MICRO)])
        ((m(torch.cat(xs)) - torch.cat(ys)) ** 2).mean().backward()
        decay = [p for n, p in named if not is_no_decay(n, p)][::-1]
        nodecay = [p for n, p in named if is_no_decay(n, p)][::-1]
        ref = torch.cat([p.grad.reshape(-1) for p in decay + nodecay])
        g0, g1 = out[(0, window)]["grads"], out[(1, window)]["grads"]
        assert torch.equal(g0, g1), "ranks disagree"
        torch.testing.assert_close(g0, ref, rtol=1e-5, atol=1e-6)
