"""CPU: the host restatement of global-norm gradient clipping and the Trainer's arguments.

``trainer.grad_clip_rule(sumsq, inv, max_norm)`` restates ``msu_grad_clip_scale`` (the kernel
is pinned to it bitwise in test_gpu_grad_norm.py): here it is pinned to
``torch.nn.utils.clip_grad_norm_`` itself, to its fixed points, and to the data-parallel
semantics -- every rank derives the same factor from its own reduced flat buffers, equal to the
one of the single-process global batch."""
import math

import pytest
import torch
import torch.multiprocessing as mp

from semantic_segmentation_of_stylegan2_artifacts_amd.trainer import grad_clip_rule, is_no_decay

from test_dp_gloo import _data, _free_port, _model, _worker


def _f32(v):
    return torch.tensor(v, dtype=torch.float64).to(torch.float32).item()


def test_rule_matches_torch_clip_grad_norm():
    """n = 10007, gradients randn x (1, 3, 0.5), max_norm 150: the norms are about 100, 302 and
    50, so exactly the middle one clips.  The reference's own arithmetic is f32: the factor
    rounds once (2^-24), torch's f32 coefficient and product once each -- 3 x 2^-24 on the
    clipped gradient; its f32 total_norm carries the f32 reduction's error, within 2^-22."""
    g = torch.Generator().manual_seed(7)
    n, max_norm = 10007, 150.0
    torch.randn(n, generator=g)  # the parameter draw of test_adamw_dev_skip_matches_torch_adamw
    clipped = []
    for s in (1.0, 3.0, 0.5):
        grad = torch.randn(n, generator=g) * s
        p = torch.zeros(n, requires_grad=True)
        p.grad = grad.clone()
        total = torch.nn.utils.clip_grad_norm_([p], max_norm)
        sumsq = math.fsum(float(v) ** 2 for v in grad.double().tolist())
        norm, factor = grad_clip_rule(sumsq, None, max_norm)
        mine = (grad.double() * factor).float()
        err = ((mine - p.grad).abs() / p.grad.abs().clamp_min(1e-30)).max().item()
        print({"scale": s, "norm": norm, "torch_norm": total.item(), "factor": factor, "max_rel_err": err})
        assert abs(norm - total.item()) <= 2.0 ** -22 * total.item()
        assert err <= 3 * 2.0 ** -24, err
        clipped.append(factor < 1.0)
        if factor == 1.0:
            assert torch.equal(p.grad, grad)
    assert clipped == [False, True, False]


@pytest.mark.parametrize("inv", [None, 0.5, 2.0 ** -16])
def test_rule_fixed_points(inv):
    i = 1.0 if inv is None else inv
    # S = 25: norm 5 x inv; max 2.5 clips by 2.5 / (5 inv + 1e-6) where that is below 1
    norm, factor = grad_clip_rule(25.0, inv, 2.5)
    assert norm == _f32(5.0 * i)
    coef = 2.5 / (5.0 * i + 1e-6)
    assert factor == _f32(i * min(coef, 1.0))
    if inv is None:
        assert factor == _f32(2.5 / (5.0 + 1e-6)) and factor < 0.5
    # inf never clips: the factor is f32(inv) exactly
    norm, factor = grad_clip_rule(25.0, inv, float("inf"))
    assert norm == _f32(5.0 * i) and factor == _f32(i)
    # S = 0: norm 0, no clipping
    assert grad_clip_rule(0.0, inv, 2.5) == (0.0, _f32(i))
    # S = inf: norm inf, coefficient 0
    norm, factor = grad_clip_rule(float("inf"), inv, 2.5)
    assert norm == float("inf") and factor == 0.0
    # S = nan: a NaN coefficient leaves the factor as it is
    norm, factor = grad_clip_rule(float("nan"), inv, 2.5)
    assert math.isnan(norm) and factor == _f32(i)


def _trainer(**kw):
    from semantic_segmentation_of_stylegan2_artifacts_amd import load_config
    from semantic_segmentation_of_stylegan2_artifacts_amd.trainer import Trainer
    return Trainer(torch.nn.Linear(8, 8), load_config(None, "swin_t"), "cpu", use_graph=False, **kw)


@pytest.mark.parametrize("bad", [0, -1.0, float("nan"), True, "5"])
def test_trainer_refuses_unusable_max_grad_norm(bad):
    with pytest.raises(ValueError):
        _trainer(max_grad_norm=bad)


def test_trainer_clipping_needs_the_skip_rule_and_is_off_by_default():
    with pytest.raises(ValueError):
        _trainer(max_grad_norm=1.0, skip_nonfinite=False)
    with pytest.raises(ValueError):
        _trainer(max_grad_norm=float("inf"), skip_nonfinite=False)
    tr = _trainer()
    assert tr.max_grad_norm is None and tr.grad_norm() is None and tr.grad_norm_dev is None
    assert tr.part is None and tr.clip_inv is None
    tr = _trainer(max_grad_norm=None)
    assert tr.grad_norm() is None
    for ok in (1.0, 5, float("inf")):
        tr = _trainer(max_grad_norm=ok)
        assert tr.max_grad_norm == float(ok)
        assert tr.part.dtype == torch.float64 and tr.grad_norm_dev.shape == (1,) and tr.clip_inv.shape == (1,)
        with pytest.raises(ValueError):
            tr.max_grad_norm = -2.0
        assert tr.max_grad_norm == float(ok)


def test_two_gloo_ranks_clip_like_the_global_batch():
    """After GradBucketer.finish() each rank's flat buffers hold the global-batch gradient
    (test_dp_gloo.py; the alignment gaps are zero, asserted by its worker): the rule applied to
    each rank's own sum of squares gives the same (norm, factor) on both ranks, equal to the rule
    on the single-process global-batch gradient; max_norm is half that gradient's norm."""
    world = 2
    out = mp.Manager().dict()
    mp.spawn(_worker, args=(world, _free_port(), 256, out), nprocs=world, join=True)

    def sumsq(t):
        return math.fsum(float(v) ** 2 for v in t.double().tolist())

    for step in range(3):
        m = _model()
        named = list(m.named_parameters())
        xs, ys = zip(*[_data(r + 10 * step) for r in range(world)])
        ((m(torch.cat(xs)) - torch.cat(ys)) ** 2).mean().backward()
        decay = [p for n, p in named if not is_no_decay(n, p)][::-1]
        nodecay = [p for n, p in named if is_no_decay(n, p)][::-1]
        ref = torch.cat([p.grad.reshape(-1) for p in decay + nodecay])
        max_norm = 0.5 * math.sqrt(sumsq(ref))
        want = grad_clip_rule(sumsq(ref), None, max_norm)
        got = [grad_clip_rule(sumsq(out[(r, step)]), None, max_norm) for r in range(world)]
        assert got[0] == got[1], (step, got)
        # the ranks' f32 sum of two half-batch gradients against the global batch's own: 1e-5
        # relative per element (test_dp_gloo.py), so at most that on the norm and the factor
        assert got[0][0] == pytest.approx(want[0], rel=1e-5) and got[0][1] == pytest.approx(want[1], rel=1e-5)
        assert 0.49 < got[0][1] <= 0.5  # 0.5 N / (N + 1e-6)
