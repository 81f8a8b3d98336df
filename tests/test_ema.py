"""CPU: the weight EMA of ``Trainer(ema_decay=...)`` -- everything that needs no device.

The host rule ``trainer.ema_rule`` (what ``msu_adamw_dev3`` computes per element, pinned bitwise
to the kernel in test_gpu_ema.py) against ``torch.lerp``, constructor / setter validation and the
buffers on a CPU-device Trainer, the EMA's state dict, the ``"model_ema"`` checkpoint key, and
the argument errors ``ops.adamw_dev_`` / ``ops.swap_cast_`` raise before any library call."""
import numpy as np
import pytest
import torch

import cases
from oracle.msunet import make_cfg

DECAYS = [0.0, 0.5, 0.9, 0.999, 0.9999]


def _rule_inputs():
    g = torch.Generator().manual_seed(11)
    e = torch.randn(4096, generator=g)
    p = e + 1e-2 * torch.randn(4096, generator=g)  # an average next to its weights
    wide = torch.randn(1024, generator=g) * 10.0 ** torch.randint(-6, 6, (1024,), generator=g).float()
    den = torch.tensor([1e-45, -1e-45, 3e-39, -7e-40, 1.1754942e-38, 0.0, -0.0, 2e-41])
    same = torch.randn(64, generator=g)
    ema = torch.cat([e, wide, torch.zeros(8), den, torch.zeros(8), den, same])
    par = torch.cat([p, wide.flip(0), den, torch.zeros(8), torch.zeros(8), den.flip(0), same])
    return ema, par


@pytest.mark.parametrize("decay", DECAYS)
def test_ema_rule_is_aten_lerp(decay):
    """ema_rule == torch.lerp(ema, p, 1 - decay) on CPU f32.  ATen's vectorised CPU lerp forms
    base + coeff * diff with one fused multiply-add where the host has one, ema_rule (like the
    kernel, compiled with fp contract off) rounds the product first: bitwise equality where torch
    did not fuse, otherwise at most 1 f32 ulp of max(|ema|, |p|) -- the printed line says which."""
    from semantic_segmentation_of_stylegan2_artifacts_amd.trainer import ema_rule
    ema, p = _rule_inputs()
    got = ema_rule(ema, p, decay)
    assert got.dtype == np.float32 and got.shape == (ema.numel(),)
    want = torch.lerp(ema, p, 1.0 - decay).numpy()
    exact = np.array_equal(got.view(np.uint32), want.view(np.uint32)) or np.array_equal(got, want)
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    ulp = np.maximum(np.maximum(np.abs(ema.numpy()), np.abs(p.numpy())).astype(np.float64) * 2.0 ** -23, 2.0 ** -149)
    print({"decay": decay, "torch_cpu_lerp": "unfused (bitwise)" if exact else "fused (<= 1 ulp)",
           "differing": int((got != want).sum()), "max_err_ulps": float((err / ulp).max())})
    assert exact or (err <= ulp).all()
    # ema == p stays put, and decay 0 hands the parameters over bitwise
    assert np.array_equal(got[-64:], p.numpy()[-64:])
    if decay == 0.0:
        # (p - (p - e) * 0: a parameter that is -0.0 may come out +0.0, lerp's own behaviour)
        pn = p.numpy()
        assert np.array_equal(got[pn != 0].view(np.uint32), pn[pn != 0].view(np.uint32)) and not got[pn == 0].any()


def test_ema_rule_rounds_like_f32_not_like_double():
    from semantic_segmentation_of_stylegan2_artifacts_amd.trainer import ema_rule
    e, p = np.float32(1.0), np.float32(1.0 + 2.0 ** -23)
    w = np.float32(1.0 - 0.9)
    assert ema_rule([e], [p], 0.9)[0] == np.float32(e + np.float32(w * np.float32(p - e)))
    assert ema_rule(torch.tensor([2.0]), torch.tensor([4.0]), 0.25)[0] == np.float32(3.5)  # w = 0.75: the high branch


def _build(ema_decay=None, **kw):
    from semantic_segmentation_of_stylegan2_artifacts_amd import load_config
    from semantic_segmentation_of_stylegan2_artifacts_amd.network.model_parts import MSUNetSys
    from semantic_segmentation_of_stylegan2_artifacts_amd.trainer import Trainer
    spec = cases.model_cases()["tiny224"]
    m = MSUNetSys(img_size=224, embed_dim=32, depths=[2, 2, 2, 2], num_heads=[1, 2, 4, 8])
    m.load_state_dict(cases.model_params(make_cfg(**spec["cfg"]), spec["seed"]), strict=True)
    return m, Trainer(m, load_config(None, "swin_t"), "cpu", ema_decay=ema_decay, **kw)


@pytest.mark.parametrize("bad", [True, False, float("nan"), -0.1, 1.0, 1.5, "0.9", float("inf")])
def test_bad_decays_raise(bad):
    with pytest.raises(ValueError):
        _build(ema_decay=bad)
    _, tr = _build(ema_decay=0.9)
    with pytest.raises(ValueError):
        tr.ema_decay = bad
    assert tr.ema_decay == 0.9


def test_default_allocates_nothing_and_a_decay_clones_the_weights():
    _, tr = _build()
    assert tr.ema_decay is None and all(g.ema is None for g in tr.groups)
    with pytest.raises(RuntimeError):
        tr.ema_scope()
    with pytest.raises(RuntimeError):
        tr.ema_state_dict()
    with pytest.raises(RuntimeError):
        tr.reset_ema()
    with pytest.raises(ValueError):  # the buffers are a construction-time decision
        tr.ema_decay = 0.9
    tr.ema_decay = None

    _, tr = _build(ema_decay=0)
    assert tr.ema_decay == 0.0 and isinstance(tr.ema_decay, float)
    _, tr = _build(ema_decay=0.999)
    for g in tr.groups:
        assert g.ema.dtype == torch.float32 and g.ema.data_ptr() != g.data.data_ptr()
        assert torch.equal(g.ema.view(torch.int32), g.data.view(torch.int32))  # gaps included
        used = torch.zeros(g.numel, dtype=torch.bool)
        for p, off in zip(g.params, g.offsets):
            used[off:off + p.numel()] = True
        assert not g.ema[~used].any()
    # the setter: a launch argument (drops a captured step), never a switch
    tr._graph = object()
    tr.ema_decay = 0.999
    assert tr._graph is not None
    tr.ema_decay = 0.5
    assert tr._graph is None and tr.ema_decay == 0.5
    with pytest.raises(ValueError):
        tr.ema_decay = None


def test_ema_state_dict_round_trip_and_reset():
    m, tr = _build(ema_decay=0.9)
    g = torch.Generator().manual_seed(5)
    for grp in tr.groups:  # an average that differs from the weights, gaps left zero
        for p, off in zip(grp.params, grp.offsets):
            grp.ema[off:off + p.numel()].copy_(torch.randn(p.numel(), generator=g))
    sd = tr.ema_state_dict()
    model_sd = m.state_dict()
    assert list(sd) == list(model_sd)
    owned = {n for grp in tr.groups for n in grp.names}
    assert owned and owned < set(sd)
    for grp in tr.groups:
        for n, p, off in zip(grp.names, grp.params, grp.offsets):
            assert sd[n].shape == p.shape and sd[n].device.type == "cpu"
            assert torch.equal(sd[n].reshape(-1), grp.ema[off:off + p.numel()])
            assert not torch.equal(sd[n], model_sd[n])
    for k in set(sd) - owned:  # dead-branch parameters and buffers: as the model has them
        assert torch.equal(sd[k], model_sd[k]) and sd[k].data_ptr() != model_sd[k].data_ptr()

    m2, tr2 = _build(ema_decay=0.9)
    before = [grp.data.clone() for grp in tr2.groups]
    tr2.load_ema_state_dict(sd)
    for a, b, d in zip(tr.groups, tr2.groups, before):
        assert torch.equal(a.ema, b.ema) and torch.equal(b.data, d)  # the weights did not move
    # strict among the owned parameters
    name = tr.groups[0].names[0]
    with pytest.raises(KeyError):
        tr2.load_ema_state_dict({k: v for k, v in sd.items() if k != name})
    with pytest.raises(ValueError):
        tr2.load_ema_state_dict(dict(sd, **{name: sd[name].reshape(-1)[:-1]}))
    tr2.load_ema_state_dict({k: v for k, v in sd.items() if k in owned})  # the rest is not needed
    # a model loaded with the EMA state carries it in its owned parameters
    m3, _ = _build()
    m3.load_state_dict(sd, strict=True)
    assert torch.equal(dict(m3.named_parameters())[name], sd[name])

    tr2.reset_ema()
    for grp in tr2.groups:
        assert torch.equal(grp.ema, grp.data) and grp.ema.data_ptr() != grp.data.data_ptr()


def test_checkpoints_carry_model_ema_only_when_given(tmp_path):
    from semantic_segmentation_of_stylegan2_artifacts_amd import checkpoint
    m, tr = _build(ema_decay=0.9)
    for grp in tr.groups:
        grp.ema.mul_(0.5)
    ema = tr.ema_state_dict()
    name = tr.groups[0].names[0]
    plain, with_ema = tmp_path / "plain", tmp_path / "ema"
    plain.mkdir()
    with_ema.mkdir()

    def same(a, b):
        if isinstance(a, dict):
            return isinstance(b, dict) and list(a) == list(b) and all(same(a[k], b[k]) for k in a)
        return torch.equal(a, b) if torch.is_tensor(a) else a == b

    opt = tr.optimizer_state_dict()
    for save, keys in ((lambda d, **kw: checkpoint.save_best(m, 3, 0.25, str(d), **kw), ["model", "epoch", "best_score"]),
                       (lambda d, **kw: checkpoint.save_last(m, opt, 3, 17, 0.5, str(d), **kw),
                        ["epoch", "model", "optimizer", "iter_num", "dice"])):
        a = torch.load(save(plain), weights_only=True)
        b = torch.load(save(plain, ema_state=None), weights_only=True)
        c = torch.load(save(with_ema, ema_state=ema), weights_only=True)
        assert list(a) == list(b) == keys and same(a, b)  # the payloads of before, key for key
        assert list(c) == keys + ["model_ema"] and same({k: c[k] for k in keys}, a)
        assert same(c["model_ema"], ema) and not torch.equal(c["model_ema"][name], c["model"][name])

    m2, _ = _build()
    msg = checkpoint.load_checkpoint(m2, str(with_ema / "best_model.pth"), use_ema=True)
    assert not msg.missing_keys and not msg.unexpected_keys
    assert same({k: v.detach() for k, v in m2.state_dict().items()}, ema)
    checkpoint.load_checkpoint(m2, str(with_ema / "epoch_3.pth"), use_ema=True)
    checkpoint.load_checkpoint(m2, str(with_ema / "best_model.pth"))  # default: the weights themselves
    assert same({k: v.detach() for k, v in m2.state_dict().items()}, {k: v.detach() for k, v in m.state_dict().items()})
    with pytest.raises(KeyError, match="model_ema"):
        checkpoint.load_checkpoint(m2, str(plain / "best_model.pth"), use_ema=True)
    with pytest.raises(KeyError, match="model_ema"):
        checkpoint.load_checkpoint(m2, str(plain / "epoch_3.pth"), use_ema=True)


def test_ops_argument_errors_come_before_the_library(monkeypatch):
    from semantic_segmentation_of_stylegan2_artifacts_amd import _lib, ops

    def no_call(*a, **kw):
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_lib, "call", no_call)
    n = 64
    p, g, m, v, ema = (torch.zeros(n) for _ in range(5))
    hyper = torch.zeros(2, dtype=torch.float64)
    args = (p, g, m, v, hyper, 0.9, 0.999, 1e-8, 0.05)
    with pytest.raises(ValueError):
        ops.adamw_dev_(*args, ema=ema)
    with pytest.raises(ValueError):
        ops.adamw_dev_(*args, ema_decay=0.9)
    for bad in (1.0, -0.1, float("nan"), True, "0.9"):
        with pytest.raises(ValueError):
            ops.adamw_dev_(*args, ema=ema, ema_decay=bad)
    for bad in (torch.zeros(n + 1), torch.zeros(n, dtype=torch.float64), torch.zeros(2 * n)[::2]):
        with pytest.raises(ValueError):
            ops.adamw_dev_(*args, ema=bad, ema_decay=0.9)
    with pytest.raises(ValueError):
        ops.adamw_dev_(*args, ema=ema, ema_decay=0.9, shadow=torch.zeros(n))
    with pytest.raises(RuntimeError):  # valid arguments on the CPU: no fall-back
        ops.adamw_dev_(*args, ema=ema, ema_decay=0.9)

    a, b = torch.zeros(n), torch.zeros(n)
    both = torch.zeros(2 * n + 8)
    for x, y, sh in ((a, torch.zeros(n + 4), None), (a, torch.zeros(n, dtype=torch.float64), None),
                     (torch.zeros(2 * n)[::2], b, None), (a.view(8, 8), b.view(8, 8), None),
                     (a, b, torch.zeros(n)), (a, b, torch.zeros(n + 4, dtype=torch.bfloat16)),
                     (both[:n], both[n - 4:2 * n - 4], None), (both[:n], both[:n], None)):
        with pytest.raises(ValueError):
            ops.swap_cast_(x, y, sh)
    base = torch.zeros(n + 8)
    lo = (-base.data_ptr() // 4) % 4  # index of a 16-byte aligned element
    with pytest.raises(ValueError, match="aligned"):
        ops.swap_cast_(base[lo + 1:lo + 1 + 32], torch.zeros(32))
    with pytest.raises(RuntimeError):
        ops.swap_cast_(base[lo:lo + 32], base[lo + 32:lo + 64])
