"""CPU: the per-backward state of ``ops`` (side-stream keep list and event guards, the residual
handoff mailbox, pending LayerNorm partials) belongs to one backward and cannot outlive it.
The autograd engine drops its queued end-of-backward callbacks when a node raises; the next
backward must then discard what the failed one parked, queue its own callback and run it once
(the failed-backward rule).  No kernel is involved: the nodes are test-local
``autograd.Function``s on CPU tensors that park the way the ops' backwards do."""
import pytest
import torch

from semantic_segmentation_of_stylegan2_artifacts_amd import _lib, ops


class _Node(torch.autograd.Function):
    """Backward: queue the end-of-backward work, park the gradient under a handoff key and in
    the keep list, then raise if told to."""

    @staticmethod
    def forward(ctx, x, key, fail):
        ctx.key, ctx.fail = key, fail
        return x.clone()

    @staticmethod
    def backward(ctx, g):
        ops._join_at_end_of_backward()
        assert ops._park(ctx.key, g)
        ops._side_keep.append(g)
        if ctx.fail:
            raise RuntimeError("backward node failed")
        return g, None, None


def _backward(key, fail):
    x = torch.ones(3, requires_grad=True)
    _Node.apply(x, key, fail).sum().backward()
    return x.grad


@pytest.fixture(autouse=True)
def _clean_state():
    ops.reset_backward_state()
    yield
    ops.reset_backward_state()


@pytest.fixture
def callbacks(monkeypatch):
    """Calls of ops._end_of_backward (the engine's queued callback), counted."""
    ran = []
    inner = ops._end_of_backward

    def counted():
        ran.append(1)
        inner()

    monkeypatch.setattr(ops, "_end_of_backward", counted)
    return ran


def test_backward_after_a_raising_backward_runs_its_end_once(callbacks):
    with pytest.raises(RuntimeError, match="backward node failed"):
        _backward(101, fail=True)
    assert not callbacks  # the engine dropped the failed backward's callback
    assert len(ops._res_handoff) == 1 and len(ops._side_keep) == 1  # ... and its state is still here
    discards = ops.backward_discards
    dropped = ops.res_dropped
    assert torch.equal(_backward(102, fail=False), torch.ones(3))
    assert len(callbacks) == 1
    assert not ops._res_handoff and not ops._side_keep
    assert ops.backward_discards == discards + 1
    assert ops.res_dropped == dropped + 1  # the good backward's own parked gradient, not the stale one
    # and the one after that is an ordinary backward again
    _backward(103, fail=False)
    assert len(callbacks) == 2 and ops.backward_discards == discards + 1
    assert not ops._res_handoff and not ops._side_keep


def test_stale_layernorm_partials_are_discarded_not_flushed(callbacks, monkeypatch):
    calls = []
    monkeypatch.setattr(_lib, "call", lambda name, *args: calls.append((name, args)))
    w = torch.nn.Parameter(torch.ones(8))
    b = torch.nn.Parameter(torch.zeros(8))
    w.grad, b.grad = torch.zeros(8), torch.zeros(8)
    stale = (torch.full((2 * 16,), 7.0), 2, 8, w, b)  # (part, nparts, C, gamma, beta)
    ops._ln_pending.append(stale)  # as a failed backward's LayerNorm node left it
    discards = ops.backward_discards
    with pytest.raises(RuntimeError, match="backward node failed"):
        _backward(201, fail=True)
    _backward(202, fail=False)
    assert len(callbacks) == 1
    assert not [c for c in calls if c[0] == "msu_colsum_batch"], "stale partials reached a reduction"
    assert not ops._ln_pending
    assert ops.backward_discards == discards + 1
    assert not w.grad.any() and not b.grad.any()


def test_reset_backward_state_is_idempotent(callbacks):
    discards = ops.backward_discards
    for _ in range(2):
        ops.reset_backward_state()  # nothing parked: changes nothing, raises nothing
        assert not (ops._side_keep or ops._res_handoff or ops._res_closed or ops._ln_pending)
        assert ops._bwd_task == -1
    _backward(301, fail=False)  # queues its callback as the first backward of a process does
    assert len(callbacks) == 1
    assert ops.backward_discards == discards
    assert ops._bwd_task == -1 and not ops._side_keep and not ops._res_handoff


def test_reset_backward_state_drops_parked_state_and_event_guards():
    with pytest.raises(RuntimeError, match="backward node failed"):
        _backward(401, fail=True)
    p = torch.nn.Parameter(torch.zeros(2))
    p._msu_side_event = object()  # as _guard_side_write leaves it
    ops._side_event_params.append(p)
    ops._res_closed.add(401)
    ops.reset_backward_state()
    assert not (ops._side_keep or ops._res_handoff or ops._res_closed or ops._ln_pending)
    assert p._msu_side_event is None and ops._bwd_task == -1
