"""GPU: ``Trainer(max_grad_norm=...)`` -- global-norm clipping inside the device-side step.

The sum of squares rides in the step's non-finite check (``msu_grad_sumsq2``), and
``msu_grad_clip_scale`` folds ``clip_grad_norm_``'s coefficient into the one factor AdamW
multiplies every gradient by, so the norm is the norm of exactly what AdamW consumes (unscaled
under a loss scale) and no extra pass reads the gradients.  On the swinT224 fixture of
test_gpu_trainer.py (batch 2): the readout and the factor against an f64 recomputation from the
raw flat gradients AdamW was handed, the first moment the clipped step leaves, the unscale under
a static f16 loss scale, the skip rule, and all of it live inside a replayed HIP graph.

Data parallelism is covered on the host (test_grad_clip.py, two gloo ranks): the launch sits
after the reducer's finish(), every rank sums identical reduced buffers in the same order."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from test_gpu_trainer import _setup  # noqa: E402

DEV = "cuda"
ULP = 2.0 ** -23  # one f32 ulp, relative, at most


class _Spy:
    """Snapshots what every AdamW launch of a step is handed: the raw flat gradient buffer (by
    group) and the inv_scale factor."""

    def __init__(self, tr):
        from semantic_segmentation_of_stylegan2_artifacts_amd import ops
        self.ops, self.tr = ops, tr
        self.grads, self.inv = [], []

    def __enter__(self):
        self.adamw = self.ops.adamw_dev_

        def snap(param, grad, *a, **kw):
            assert grad is self.tr.groups[len(self.grads)].grad
            self.grads.append(grad.clone())
            self.inv.append(kw["inv_scale"].clone())
            return self.adamw(param, grad, *a, **kw)

        self.ops.adamw_dev_ = snap
        return self

    def __exit__(self, *exc):
        self.ops.adamw_dev_ = self.adamw

    def sumsq(self):
        return sum((g.double() ** 2).sum().item() for g in self.grads)


def _trainer(**kw):
    from semantic_segmentation_of_stylegan2_artifacts_amd.trainer import Trainer
    model, x, target, conf = _setup()
    return Trainer(model, conf, DEV, **kw), x, target


def _close(a, b, ulps=1):
    return abs(a - b) <= ulps * ULP * abs(b)


def test_eager_bf16_step_clips_by_the_norm_of_what_adamw_consumes():
    from semantic_segmentation_of_stylegan2_artifacts_amd.trainer import grad_clip_rule
    tr, x, target = _trainer(use_graph=False, max_grad_norm=float("inf"))
    with _Spy(tr) as spy:
        tr.step(x, target)
    N = tr.grad_norm()
    assert math.isfinite(N) and N > 0
    assert _close(N, math.sqrt(spy.sumsq()))
    # measuring alone changes nothing: AdamW's factor is exactly 1
    assert len(spy.inv) == 2 and all(i.item() == 1.0 for i in spy.inv)
    assert tr.grad_norm_dev.item() == N and tr.max_grad_norm == float("inf")

    tr, x, target = _trainer(use_graph=False, max_grad_norm=N / 2)
    with _Spy(tr) as spy:
        tr.step(x, target)
    S = spy.sumsq()
    want_norm, want_factor = grad_clip_rule(S, None, N / 2)
    got = tr.grad_norm()
    factor = spy.inv[0].item()
    print({"N": N, "norm": got, "f64_norm": math.sqrt(S), "factor": factor, "rule": (want_norm, want_factor)})
    assert _close(got, math.sqrt(S))
    assert spy.inv[1].item() == factor and _close(factor, want_factor)
    assert 0.4 < factor < 0.6 and tr.clip_inv.item() == factor
    # the first step's first moment: (1 - beta1) x (gradient x factor), in AdamW's order
    w1 = torch.tensor(1.0 - tr.betas[0], dtype=torch.float64).float().item()
    for g, raw, inv in zip(tr.groups, spy.grads, spy.inv):
        torch.testing.assert_close(g.exp_avg, (raw * inv) * w1, rtol=4e-7, atol=2e-8)
        assert g.exp_avg.abs().max().item() > 0 and not g.grad.any()
    assert tr.optimizer_steps() == 1


def test_f16_static_scale_reports_the_unscaled_norm():
    tr, x, target = _trainer(use_graph=False, amp_dtype=torch.float16, loss_scale=1024.0,
                             max_grad_norm=float("inf"))
    with _Spy(tr) as spy:
        tr.step(x, target)
    got, want = tr.grad_norm(), math.sqrt(spy.sumsq()) * 2.0 ** -10
    print({"norm": got, "f64_norm_unscaled": want})
    assert _close(got, want)
    assert all(i.item() == 2.0 ** -10 for i in spy.inv)  # inv_out handed on, never clipped
    assert tr.inv_out.item() == 2.0 ** -10 and tr.optimizer_steps() == 1


def test_nonfinite_gradient_skips_the_clipped_step():
    tr, x, target = _trainer(use_graph=False, max_grad_norm=1.0)
    tr.step(x, target)
    assert tr.optimizer_steps() == 1 and math.isfinite(tr.grad_norm())
    snap = [(g.data.clone(), g.exp_avg.clone(), g.exp_avg_sq.clone()) for g in tr.groups]
    bad = x.clone()
    bad[0, 0, 5, 7] = float("nan")  # -> NaN logits -> NaN gradients everywhere
    loss = tr.step(bad, target)
    torch.cuda.synchronize()
    assert not torch.isfinite(loss).item() and tr.found_inf.item() == 1.0
    for g, (d, m, v) in zip(tr.groups, snap):
        assert torch.equal(g.data, d) and torch.equal(g.exp_avg, m) and torch.equal(g.exp_avg_sq, v)
        assert not g.grad.any()
    assert tr.optimizer_steps() == 1 and not math.isfinite(tr.grad_norm())
    tr.step(x, target)
    assert tr.optimizer_steps() == 2 and math.isfinite(tr.grad_norm())
    assert not torch.equal(tr.groups[0].data, snap[0][0])


def test_norm_and_factor_are_live_inside_the_replayed_step():
    from semantic_segmentation_of_stylegan2_artifacts_amd.trainer import grad_clip_rule
    # a small learning rate: the four steps see about the same model, so their norms differ by
    # the input alone and stay far above the max_grad_norm chosen from the first one
    tr, x, target = _trainer(use_graph=True, graph_warmup=2, max_grad_norm=float("inf"), lr=1e-6)
    inputs = [x, 0.5 * x]
    norms = []
    for k in range(4):
        tr.step(inputs[k % 2], target)
        assert (tr._graph is not None) == (k >= 2)
        want = grad_clip_rule(math.fsum(tr.part.cpu().tolist()), None, tr.max_grad_norm)
        got = (tr.grad_norm_dev.item(), tr.clip_inv.item())
        print({"step": k, "replayed": tr._graph is not None, "got": got, "rule": want, "max": tr.max_grad_norm})
        assert _close(got[0], want[0]) and _close(got[1], want[1]), (k, got, want)
        assert (got[1] < 1.0) == (k >= 1)
        norms.append(got[0])
        if k == 0:  # from here on the step clips (before the capture: nothing to drop yet)
            tr.max_grad_norm = 1e-3 * got[0]
    assert norms[2] != norms[3] and tr.optimizer_steps() == 4
    snap = [(g.data.clone(), g.exp_avg.clone(), g.exp_avg_sq.clone()) for g in tr.groups]
    bad = x.clone()
    bad[0, 1, 3, 3] = float("inf")
    tr.step(bad, target)
    torch.cuda.synchronize()
    assert tr.found_inf.item() == 1.0 and tr.optimizer_steps() == 4 and not math.isfinite(tr.grad_norm())
    for g, (d, m, v) in zip(tr.groups, snap):
        assert torch.equal(g.data, d) and torch.equal(g.exp_avg, m) and torch.equal(g.exp_avg_sq, v)
        assert not g.grad.any()
    tr.step(x, target)
    assert tr.optimizer_steps() == 5 and math.isfinite(tr.grad_norm())
    # max_grad_norm is a launch argument of the captured step
    assert tr._graph is not None
    tr.max_grad_norm = tr.max_grad_norm
    assert tr._graph is not None
    tr.max_grad_norm = 2.0 * tr.max_grad_norm
    assert tr._graph is None
    with pytest.raises(ValueError):
        tr.max_grad_norm = None
