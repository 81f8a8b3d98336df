"""GPU: ``Trainer(ema_decay=...)`` -- the weights' moving average inside the device-side step.

On the swinT224 fixture of test_gpu_trainer.py (batch 2): after every applied step both groups'
averages are bitwise ``ema_rule(ema before, weights after, decay)`` -- eagerly, inside a replayed
HIP graph and after the decay changed; the average never feeds back into training; a skipped step
leaves it alone; and ``ema_scope()`` swaps it in for an evaluation (weights, 16-bit shadow and
transposed shadow) and restores every buffer bitwise."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from test_gpu_trainer import _setup  # noqa: E402

DEV = "cuda"


def _trainer(**kw):
    from semantic_segmentation_of_stylegan2_artifacts_amd.trainer import Trainer
    model, x, target, conf = _setup()
    return Trainer(model, conf, DEV, **kw), x, target


def _bits(t):
    return t.view({4: torch.int32, 2: torch.int16}[t.element_size()])


def _same(a, b):
    if a is None or b is None:  # the no-decay group has no 2-D weights: no transposed shadow
        return a is None and b is None
    return torch.equal(_bits(a), _bits(b))


def _clone(t):
    return None if t is None else t.clone()


def _obeys(tr, before, decay):
    """Both groups' averages are bitwise the rule applied to the weights as they are now."""
    from semantic_segmentation_of_stylegan2_artifacts_amd.trainer import ema_rule
    for g, e0 in zip(tr.groups, before):
        want = ema_rule(e0, g.data, decay)
        got = g.ema.cpu().numpy()
        if not np.array_equal(got.view(np.uint32), want.view(np.uint32)):
            return False
        if not (got != e0.cpu().numpy()).any():  # the average did move
            return False
    return True


def _emas(tr):
    return [g.ema.clone() for g in tr.groups]


@pytest.fixture(scope="module")
def ema_run():
    """Three eager bf16 steps with ema_decay=0.9: the rule per step, and what the steps left."""
    tr, x, target = _trainer(use_graph=False, ema_decay=0.9, seed=0)
    start_equal = all(_same(g.ema, g.data) and g.ema.data_ptr() != g.data.data_ptr() for g in tr.groups)
    obeyed, losses = [], []
    for _ in range(3):
        before = _emas(tr)
        losses.append(tr.step(x, target).clone())
        obeyed.append(_obeys(tr, before, 0.9))
    torch.cuda.synchronize()
    return {"start_equal": start_equal, "obeyed": obeyed, "losses": losses, "steps": tr.optimizer_steps(),
            "state": [(g.data.clone(), g.exp_avg.clone(), g.exp_avg_sq.clone()) for g in tr.groups],
            "moved": [not _same(g.ema, g.data) for g in tr.groups]}


def test_eager_bf16_average_follows_the_rule(ema_run):
    assert ema_run["start_equal"]
    assert ema_run["obeyed"] == [True, True, True]
    assert ema_run["steps"] == 3 and all(ema_run["moved"])


def test_the_average_never_feeds_back(ema_run):
    tr, x, target = _trainer(use_graph=False, seed=0)
    assert tr.ema_decay is None and all(g.ema is None for g in tr.groups)
    losses = [tr.step(x, target).clone() for _ in range(3)]
    torch.cuda.synchronize()
    for a, b in zip(losses, ema_run["losses"]):
        assert _same(a.reshape(1), b.reshape(1))
    for g, (d, m, v) in zip(tr.groups, ema_run["state"]):
        assert _same(g.data, d) and _same(g.exp_avg, m) and _same(g.exp_avg_sq, v)


def test_skipped_step_leaves_the_average_alone():
    tr, x, target = _trainer(use_graph=False, lr=1e-4, amp_dtype=torch.float16, loss_scale="dynamic",
                             init_scale=2.0 ** 40, ema_decay=0.9)
    for g in tr.groups:  # an average away from the weights: a wrongly applied lerp would show
        g.ema.mul_(0.5)
    snap = [(g.data.clone(), g.ema.clone()) for g in tr.groups]
    tr.step(x, target)  # overflows in f16 at this scale
    torch.cuda.synchronize()
    assert tr.found_inf.item() == 1.0 and tr.optimizer_steps() == 0 and tr.skipped_steps() == 1
    for g, (d, e) in zip(tr.groups, snap):
        assert _same(g.data, d) and _same(g.ema, e) and not g.grad.any()
    tr.scale.fill_(1024.0)
    before = _emas(tr)
    tr.step(x, target)
    assert tr.optimizer_steps() == 1 and tr.skipped_steps() == 1
    assert _obeys(tr, before, 0.9)


def test_replayed_graph_advances_the_average_and_takes_a_new_decay():
    tr, x, target = _trainer(use_graph=True, graph_warmup=2, ema_decay=0.9)
    for k in range(4):
        before = _emas(tr)
        tr.step(x, target)
        assert (tr._graph is not None) == (k >= 2)
        assert _obeys(tr, before, 0.9), k
    tr.ema_decay = 0.9
    assert tr._graph is not None
    tr.ema_decay = 0.5  # a launch argument of the captured step
    assert tr._graph is None and tr.ema_decay == 0.5
    for k in range(2):
        before = _emas(tr)
        tr.step(x, target)
        assert tr._graph is not None
        assert _obeys(tr, before, 0.5), k
    assert tr.optimizer_steps() == 6


def _eval_logits(model, x):
    model.eval()
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        return model(x).clone()


def _transposed_ok(g):
    if g.ttable is None:
        return True
    for off, toff, N, K, _ in g.ttable.tolist():
        if not _same(g.tshadow[toff:toff + N * K].view(K, N), g.shadow[off:off + N * K].view(N, K).t().contiguous()):
            return False
    return True


def test_ema_scope_swaps_in_the_average_and_restores():
    from semantic_segmentation_of_stylegan2_artifacts_amd.trainer import Trainer
    tr, x, target = _trainer(use_graph=False, ema_decay=0.9)
    for _ in range(2):
        tr.step(x, target)
    snap = [(g.data.clone(), g.ema.clone(), g.shadow.clone(), _clone(g.tshadow)) for g in tr.groups]
    versions = tr._param_versions()

    def restored():
        return all(_same(g.data, d) and _same(g.ema, e) and _same(g.shadow, s) and _same(g.tshadow, t)
                   for g, (d, e, s, t) in zip(tr.groups, snap))

    with tr.ema_scope() as inside:
        assert inside is tr
        for g, (d, e, s, t) in zip(tr.groups, snap):
            assert _same(g.data, e) and _same(g.ema, d)
            assert _same(g.shadow, e.to(torch.bfloat16)) and not _same(g.shadow, s)
            assert _transposed_ok(g)
        assert tr.groups[0].ttable is not None and len(tr.groups[0].ttable) > 10
        assert tr._param_versions() == versions
        assert all(p._msu_shadow_ver == p._version for g in tr.groups for p in g.params)
        logits = _eval_logits(tr.model, x)
        with pytest.raises(RuntimeError):
            tr.ema_scope()
        with pytest.raises(RuntimeError):
            tr.ema_state_dict()
    assert restored()
    ema_sd = tr.ema_state_dict()
    plain = _eval_logits(tr.model, x)
    assert not torch.equal(plain, logits)  # the average is another model
    # an exception inside still restores; step() is refused there
    with pytest.raises(RuntimeError, match="ema_scope"):
        with tr.ema_scope():
            tr.step(x, target)
    assert restored() and tr.optimizer_steps() == 2
    before = _emas(tr)
    tr.step(x, target)
    assert _obeys(tr, before, 0.9) and tr.optimizer_steps() == 3
    del tr, snap

    # a second model given the EMA state and a trainer of its own, without an EMA
    model2, _, _, conf = _setup()
    model2.load_state_dict(ema_sd, strict=True)
    tr2 = Trainer(model2, conf, DEV, use_graph=False)
    for g in tr2.groups:
        g.refresh_shadow()
    logits2 = _eval_logits(model2, x)
    assert torch.isfinite(logits).all()
    assert _same(logits, logits2)


def test_f32_trainer_swaps_without_a_shadow():
    tr, x, target = _trainer(use_graph=False, amp_dtype=torch.float32, ema_decay=0.5)
    before = _emas(tr)
    tr.step(x, target)
    assert _obeys(tr, before, 0.5)
    snap = [(g.data.clone(), g.ema.clone(), g.shadow.clone()) for g in tr.groups]
    with tr.ema_scope():
        for g, (d, e, s) in zip(tr.groups, snap):
            assert _same(g.data, e) and _same(g.ema, d)
            assert _same(g.shadow, s)  # not written: the f32 path reads no shadow
    for g, (d, e, s) in zip(tr.groups, snap):
        assert _same(g.data, d) and _same(g.ema, e) and _same(g.shadow, s)
