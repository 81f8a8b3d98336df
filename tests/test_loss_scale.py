"""CPU: the f16 loss scale's rule, the Trainer's argument checks and the checkpoint key.

``trainer.loss_scale_rule`` is the host restatement of what ``msu_loss_scale_step`` does to
{scale, growth tracker} on the device; here it is pinned to ``torch._amp_update_scale_`` (the op
``GradScaler.update()`` runs) on CPU tensors, step by step over scripted non-finite flags.  The
GPU kernel is pinned to the same op over the same scripts in ``test_gpu_loss_scale.py``."""
import pytest
import torch

# (init scale, growth interval, the steps' found_inf flags)
SCRIPTS = {
    # growth at steps 3 and 7 (three clean steps in a row; the back-off at step 4 restarts the
    # count), back-offs at 4, 9 and 10, and a tracker left mid-count at the end
    "interval3": (65536.0, 3, (0, 0, 0, 1, 0, 0, 0, 0, 1, 1, 0, 0)),
    # 2^127 x 2 is not a finite f32: the growth is dropped, the tracker still restarts
    "top_of_range": (2.0 ** 127, 3, (0, 0, 0, 1, 0, 0, 0, 0, 1, 1, 0, 0)),
}


def torch_rule(scale, tracker, flags, interval, device="cpu", growth=2.0, backoff=0.5):
    """[(scale, tracker)] after each step, by torch._amp_update_scale_."""
    s = torch.full((1,), scale, dtype=torch.float32, device=device)
    t = torch.full((1,), tracker, dtype=torch.int32, device=device)
    out = []
    for f in flags:
        torch._amp_update_scale_(s, t, torch.full((1,), float(f), device=device), growth, backoff, interval)
        out.append((s.item(), t.item()))
    return out


@pytest.mark.parametrize("name", sorted(SCRIPTS))
def test_host_rule_equals_torch_amp_update_scale(name):
    from semantic_segmentation_of_stylegan2_artifacts_amd.trainer import loss_scale_rule
    scale, interval, flags = SCRIPTS[name]
    ref = torch_rule(scale, 0, flags, interval)
    s, t, got = scale, 0, []
    for f in flags:
        s, t = loss_scale_rule(s, t, bool(f), 2.0, 0.5, interval)
        got.append((s, t))
    assert got == ref, (got, ref)
    if name == "interval3":  # the script reaches both branches
        assert max(g[0] for g in got) == 2 * scale and got[-1] == (scale / 2, 2)
    else:  # never above 2^127: the overflowing growth was refused
        assert max(g[0] for g in got) == scale and got[2] == (scale, 0)


def test_static_scale_is_the_rule_with_unit_factors():
    from semantic_segmentation_of_stylegan2_artifacts_amd.trainer import loss_scale_rule
    s, t = 1024.0, 0
    for f in (0, 1, 0, 0, 0):
        s, t = loss_scale_rule(s, t, bool(f), 1.0, 1.0, 2)
        assert s == 1024.0


def _trainer(**kw):
    from semantic_segmentation_of_stylegan2_artifacts_amd import load_config
    from semantic_segmentation_of_stylegan2_artifacts_amd.trainer import Trainer
    return Trainer(torch.nn.Linear(8, 8), load_config(None, "swin_t"), "cpu", use_graph=False, **kw)


def test_constructor_refuses_a_scale_it_cannot_honour():
    with pytest.raises(ValueError, match="float16"):
        _trainer(amp_dtype=torch.bfloat16, loss_scale="dynamic")
    with pytest.raises(ValueError, match="float16"):
        _trainer(amp_dtype=torch.float32, loss_scale=1024.0)
    with pytest.raises(ValueError, match="skip_nonfinite"):
        _trainer(amp_dtype=torch.float16, loss_scale="dynamic", skip_nonfinite=False)
    with pytest.raises(ValueError, match="loss_scale"):
        _trainer(amp_dtype=torch.float16, loss_scale="static")
    with pytest.raises(ValueError):
        _trainer(amp_dtype=torch.float16, loss_scale=0.0)


def test_constructor_defaults_and_state_dict_format():
    tr = _trainer(amp_dtype=torch.float16)
    assert tr.scale is None and tr.loss_scale() is None and tr.scaler_state_dict() == {}
    assert tr.groups[0].shadow.dtype == torch.float16
    assert _trainer().groups[0].shadow.dtype == torch.bfloat16
    tr = _trainer(amp_dtype=torch.float16, loss_scale="dynamic")
    ref = torch.amp.GradScaler("cpu").state_dict()
    assert tr.scaler_state_dict() == ref  # GradScaler's defaults, key for key
    tr = _trainer(amp_dtype=torch.float16, loss_scale=512, growth_interval=7)
    assert tr.scaler_state_dict() == {"scale": 512.0, "growth_factor": 1.0, "backoff_factor": 1.0,
                                      "growth_interval": 7, "_growth_tracker": 0}
    tr.load_scaler_state_dict(ref)
    assert tr.scaler_state_dict() == ref
    with pytest.raises(RuntimeError):
        _trainer().load_scaler_state_dict(ref)


def test_f16_wire_keeps_its_own_scale_only_without_a_loss_scale():
    """Under a trainer loss scale the buckets arrive scaled (the reference's GradScaler-scaled
    fp16 gradients): the f16 wire casts them as they are, no second scale."""
    plain = _trainer(amp_dtype=torch.float16, grad_wire_dtype=torch.float16, always_reduce=True)
    assert plain.reducer.wire_dtype == torch.float16 and plain.reducer.scale is not None
    scaled = _trainer(amp_dtype=torch.float16, loss_scale="dynamic", grad_wire_dtype=torch.float16,
                      always_reduce=True)
    assert scaled.reducer.wire_dtype == torch.float16 and scaled.reducer.scale is None
    assert scaled.reducer.inv_scale is None and scaled.reducer.growth_tracker is None


def test_save_last_writes_the_scaler_key_only_with_a_state(tmp_path):
    from semantic_segmentation_of_stylegan2_artifacts_amd import checkpoint
    m = torch.nn.Linear(4, 4)
    opt = {"state": {}, "param_groups": []}
    path = checkpoint.save_last(m, opt, 3, 17, 0.5, str(tmp_path))
    assert set(torch.load(path, weights_only=True)) == {"epoch", "model", "optimizer", "iter_num", "dice"}
    path = checkpoint.save_last(m, opt, 4, 17, 0.5, str(tmp_path), scaler_state={})
    assert "scaler" not in torch.load(path, weights_only=True)
    state = torch.amp.GradScaler("cpu").state_dict()
    path = checkpoint.save_last(m, opt, 5, 17, 0.5, str(tmp_path), scaler_state=state)
    got = torch.load(path, weights_only=True)
    assert got["scaler"] == state
    assert set(got) == {"epoch", "model", "optimizer", "iter_num", "dice", "scaler"}
