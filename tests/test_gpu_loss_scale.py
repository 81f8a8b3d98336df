"""GPU: the native f16 training step with a device-side dynamic loss scale.

``Trainer(amp_dtype=torch.float16, loss_scale="dynamic")`` seeds backward with a scale kept in
device memory and runs ``GradScaler.update()``'s rule inside the step (``msu_loss_scale_step``,
the launch that otherwise only advances the step count), so the reference's fp16 autocast +
GradScaler arithmetic (trainer.py:182, :308-316) runs on the flat buffers, the fused AdamW pass,
f16 weight shadows, the bucketer and the HIP-graph replay.  Pinned here:

* the kernel against ``torch._amp_update_scale_`` on the GPU, bitwise, over the scripts of
  ``test_loss_scale.py``;
* one f16 step on the swinT224 fixture against the reference's fp32 golden record, with
  ``test_gpu_reference_step.py``'s bounds, and the f16 shadows the Linear ops then read;
* the overflow path from an absurd scale down to the first applied step, next to a torch
  GradScaler on the reference loop;
* the same inside a replayed HIP graph, on the production routes at 1024^2, across two
  data-parallel ranks, and through the GradScaler-format state dict.
"""
import copy
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import cases  # noqa: E402
from oracle.msunet import make_cfg  # noqa: E402
from test_loss_scale import SCRIPTS  # noqa: E402

DEV = "cuda"
F16 = torch.float16


# ----------------------------------------------------------------------------- 1. the kernel
@pytest.mark.parametrize("inv_world", [None, 0.5])
@pytest.mark.parametrize("name", sorted(SCRIPTS))
def test_kernel_equals_torch_amp_update_scale(name, inv_world):
    from semantic_segmentation_of_stylegan2_artifacts_amd import ops
    init, interval, flags = SCRIPTS[name]
    hyper = torch.tensor([1e-3, 0.0], device=DEV, dtype=torch.float64)
    scale = torch.full((1,), init, device=DEV)
    tracker = torch.zeros(1, device=DEV, dtype=torch.int32)
    inv_out = torch.zeros(1, device=DEV)
    iw = None if inv_world is None else torch.full((1,), inv_world, device=DEV)
    ref_s, ref_t = scale.clone(), tracker.clone()
    for i, f in enumerate(flags):
        found = torch.full((1,), float(f), device=DEV)
        before = scale.item()
        ops.loss_scale_step_(hyper, found, scale, tracker, inv_out, iw, 2.0, 0.5, interval)
        torch._amp_update_scale_(ref_s, ref_t, found, 2.0, 0.5, interval)
        assert torch.equal(scale, ref_s) and torch.equal(tracker, ref_t), (i, scale, ref_s, tracker, ref_t)
        # powers of two throughout: the quotient is exact
        assert inv_out.item() == (1.0 if inv_world is None else inv_world) / before, (i, inv_out, before)
        assert hyper[1].item() == flags[:i + 1].count(0) and hyper[0].item() == 1e-3
    assert found.item() == float(flags[-1])  # read only


def test_kernel_argument_errors_launch_nothing():
    from semantic_segmentation_of_stylegan2_artifacts_amd import _lib, ops
    hyper = torch.tensor([1e-3, 0.0], device=DEV, dtype=torch.float64)
    found, scale, inv_out = torch.zeros(1, device=DEV), torch.full((1,), 4.0, device=DEV), torch.zeros(1, device=DEV)
    tracker = torch.zeros(1, device=DEV, dtype=torch.int32)
    L = _lib.lib()
    s = torch.cuda.current_stream().cuda_stream
    good = [hyper.data_ptr(), found.data_ptr(), scale.data_ptr(), tracker.data_ptr(), None, inv_out.data_ptr(),
            2.0, 0.5, 3, s]
    for idx, bad in ((0, None), (1, None), (2, None), (3, None), (5, None), (8, 0), (6, 0.5), (7, 0.0), (7, 2.0)):
        args = list(good)
        args[idx] = bad
        assert L.msu_loss_scale_step(*args) == -2, (idx, bad)
    torch.cuda.synchronize()
    assert scale.item() == 4.0 and tracker.item() == 0 and hyper[1].item() == 0 and inv_out.item() == 0
    with pytest.raises(ValueError):
        ops.loss_scale_step_(hyper, found, scale, tracker.float(), inv_out)


# ----------------------------------------------------------------------------- the fixture model
def _spec():
    spec = cases.model_cases()["swinT224"]
    return spec, make_cfg(**spec["cfg"])


def _setup(batch=None):
    """The model and inputs of test_gpu_reference_step.py (Swin-T widths, 224^2, no dropout)."""
    from semantic_segmentation_of_stylegan2_artifacts_amd import load_config
    from semantic_segmentation_of_stylegan2_artifacts_amd.network.model_parts import MSUNetSys
    spec, cfg = _spec()
    model = MSUNetSys(img_size=cfg["img_size"], patch_size=cfg["patch_size"], in_chans=cfg["in_chans"],
                      num_classes=cfg["num_classes"], embed_dim=cfg["embed_dim"], depths=cfg["depths"],
                      num_heads=cfg["num_heads"], window_size=cfg["window_size"], mlp_ratio=cfg["mlp_ratio"],
                      drop_rate=0.0, attn_drop_rate=0.0, drop_path_rate=0.0)
    model.load_state_dict(cases.model_params(cfg, spec["seed"]), strict=True)
    x, target = cases.model_inputs(cfg, spec["batch"] if batch is None else batch, spec["seed"])
    conf = load_config(None, "swin_t", **{"TRAIN.BASE_LR": 1e-4})
    return model.to(DEV).train(), x.to(DEV), target.to(DEV), conf


class _Spy:
    """Records what one step hands to the loss (logits) and to AdamW (gradients x inv_scale)."""

    def __init__(self, tr, names):
        from semantic_segmentation_of_stylegan2_artifacts_amd import ops
        self.ops, self.tr, self.names = ops, tr, names
        self.grads, self.logits, self.inv = {}, None, None
        inner = tr.loss_fn
        spy = self

        class _Loss(torch.nn.Module):
            def forward(self, out, lab):
                spy.logits = out.detach().float().clone()
                return inner(out, lab)

        tr.loss_fn = _Loss()

    def __enter__(self):
        self.adamw = self.ops.adamw_dev_

        def snap(param, grad, *a, **kw):
            self.inv = kw["inv_scale"].clone()
            for g in self.tr.groups:
                if g.grad is grad:
                    for p, off in zip(g.params, g.offsets):
                        self.grads[self.names[id(p)]] = grad[off:off + p.numel()].view_as(p) * kw["inv_scale"]
            return self.adamw(param, grad, *a, **kw)

        self.ops.adamw_dev_ = snap
        return self

    def __exit__(self, *exc):
        self.ops.adamw_dev_ = self.adamw


# ----------------------------------------------------------------------------- 2. one f16 step
def test_f16_dynamic_step_matches_the_golden_record_and_refreshes_f16_shadows(golden_dir):
    from semantic_segmentation_of_stylegan2_artifacts_amd import ops
    from semantic_segmentation_of_stylegan2_artifacts_amd.trainer import Trainer
    z = np.load(os.path.join(golden_dir, "msunet_swinT224.npz"))
    model, x, t, conf = _setup()
    names = {id(p): k for k, p in model.named_parameters()}
    before = {k: p.detach().clone() for k, p in model.named_parameters()}
    tr = Trainer(model, conf, DEV, lr=1e-4, amp_dtype=F16, loss_scale="dynamic", use_graph=False)
    assert tr.loss_scale() == 65536.0
    with _Spy(tr, names) as spy:
        loss = tr.step(x, t)
    torch.cuda.synchronize()
    ref = torch.from_numpy(z["logits"])
    rel = ((spy.logits.cpu() - ref).norm() / ref.norm()).item()
    norms = dict(zip(list(z["grad_names"]), z["grad_norm"]))
    gmax = max(norms.values())
    assert set(spy.grads) == set(norms)
    worst = max(abs(spy.grads[k].norm().item() - n) / (5e-2 * n + 1e-3 * gmax) for k, n in norms.items())
    print(json.dumps({"logits_rel_l2": rel, "loss": loss.item(), "loss_golden": float(z["loss"]),
                      "norm_worst_fraction_of_tol": worst, "inv_out": spy.inv.item()}))
    assert rel < 1e-2, rel
    assert abs(loss.item() - float(z["loss"])) <= 1e-2 * abs(float(z["loss"])), (loss.item(), float(z["loss"]))
    assert spy.inv.item() == 1.0 / 65536.0
    assert all(torch.isfinite(g).all() for g in spy.grads.values())
    for k, n in norms.items():
        gn = spy.grads[k].norm().item()
        assert abs(gn - n) <= 5e-2 * n + 1e-3 * gmax, (k, gn, n)
    assert tr.loss_scale() == 65536.0 and tr.growth_tracker.item() == 1
    assert tr.optimizer_steps() == 1 and tr.skipped_steps() == 0
    moved = sum(not torch.equal(before[k], p.detach()) for k, p in model.named_parameters() if k in norms)
    assert moved == len(norms)
    # the shadows the next forward / backward reads: the cast of the updated master weights
    n_t = 0
    for g in tr.groups:
        assert g.shadow.dtype == F16
        for p in g.params:
            assert torch.equal(p._msu_shadow, p.detach().to(F16)), names[id(p)]
            assert ops._shadow(p, F16) is p._msu_shadow, names[id(p)]
            if hasattr(p, "_msu_shadow_t"):
                assert torch.equal(p._msu_shadow_t, p.detach().to(F16).t()), names[id(p)]
                assert ops._shadow_t(p, F16) is p._msu_shadow_t
                n_t += 1
    assert n_t > 50


# ----------------------------------------------------------------------------- 3. overflow
def test_overflowing_scale_backs_off_to_the_first_applied_step():
    from semantic_segmentation_of_stylegan2_artifacts_amd.loss import DynamicLoss
    from semantic_segmentation_of_stylegan2_artifacts_amd.trainer import Trainer
    from test_gpu_reference_step import make_optimizer, reference_step
    model, x, t, conf = _setup()
    twin = copy.deepcopy(model)
    tr = Trainer(model, conf, DEV, lr=1e-4, amp_dtype=F16, loss_scale="dynamic", init_scale=2.0 ** 40,
                 use_graph=False)
    snap = [(g.data.clone(), g.exp_avg.clone(), g.exp_avg_sq.clone()) for g in tr.groups]
    tr.step(x, t)
    torch.cuda.synchronize()
    for g, (d, m, v) in zip(tr.groups, snap):
        assert torch.equal(g.data, d) and torch.equal(g.exp_avg, m) and torch.equal(g.exp_avg_sq, v)
        assert not g.grad.any()
    assert tr.optimizer_steps() == 0 and tr.skipped_steps() == 1 and tr.loss_scale() == 2.0 ** 39
    tr.lr = 0.0
    k = 1
    while tr.optimizer_steps() == 0 and k < 40:
        tr.step(x, t)
        k += tr.optimizer_steps() == 0
        assert tr.loss_scale() == 2.0 ** (40 - k), (k, tr.loss_scale())
    assert tr.optimizer_steps() == 1 and tr.skipped_steps() == k
    # the reference loop with a torch GradScaler from the same scale, on a copy
    t_ = conf.TRAIN
    opt = make_optimizer(twin, 0.0, 1e-3, (0.9, 0.999), 1e-8)
    scaler = torch.amp.GradScaler("cuda", init_scale=2.0 ** 40)
    dl = DynamicLoss(alpha=t_.TVERSKY_LOSS_ALPHA, beta=t_.TVERSKY_LOSS_BETA, tversky_bce_mix=t_.LOSS_TVERSKY_BCE_MIX)
    k_ref = 0
    while k_ref < 40:
        s0 = scaler.get_scale()
        reference_step(twin, dl, opt, scaler, x, t, DEV, lambda *a: None)
        if scaler.get_scale() == s0:
            break
        k_ref += 1
    print(json.dumps({"skips_trainer": k, "skips_gradscaler": k_ref}))
    assert abs(k - k_ref) <= 1, (k, k_ref)


# ----------------------------------------------------------------------------- 4. replay
def test_scale_evolves_inside_the_replayed_step():
    """test_gpu_trainer.py::test_nonfinite_input_skips_replayed_step under a loss scale."""
    from semantic_segmentation_of_stylegan2_artifacts_amd.trainer import Trainer
    model, x, t, conf = _setup(batch=2)
    tr = Trainer(model, conf, DEV, amp_dtype=F16, loss_scale="dynamic", growth_interval=4, use_graph=True,
                 graph_warmup=2)
    for _ in range(3):
        tr.step(x, t)
    assert tr._graph is not None and tr.optimizer_steps() == 3
    assert tr.loss_scale() == 65536.0 and tr.growth_tracker.item() == 3
    snap = [(g.data.clone(), g.exp_avg.clone(), g.exp_avg_sq.clone()) for g in tr.groups]
    bad = x.clone()
    bad[0, 1, 3, 3] = float("inf")
    tr.step(bad, t)
    torch.cuda.synchronize()
    assert tr.found_inf.item() == 1.0 and tr.optimizer_steps() == 3
    assert tr.loss_scale() == 32768.0 and tr.growth_tracker.item() == 0
    for g, (d, m, v) in zip(tr.groups, snap):
        assert torch.equal(g.data, d) and torch.equal(g.exp_avg, m) and torch.equal(g.exp_avg_sq, v)
        assert not g.grad.any()
    tr.step(x, t)
    assert tr.optimizer_steps() == 4 and tr.skipped_steps() == 1
    assert tr.loss_scale() == 32768.0 and tr.growth_tracker.item() == 1
    assert not torch.equal(tr.groups[0].data, snap[0][0])
    for _ in range(3):  # the replayed launch grows the scale too: four clean steps in a row
        tr.step(x, t)
    assert tr.loss_scale() == 65536.0 and tr.growth_tracker.item() == 0 and tr.optimizer_steps() == 7


# ----------------------------------------------------------------------------- 5. production routes
IMG = 1024
FULL = ("ms_unet.up.refine1.weight", "ms_unet.up.refine2.weight",
        "ms_unet.layers.0.blocks.1.attn.relative_position_bias_table")


def _routes_child(outdir):
    fd = os.open(os.path.join(outdir, "child.log"), os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
    os.dup2(fd, 1)
    os.dup2(fd, 2)
    from semantic_segmentation_of_stylegan2_artifacts_amd import load_config, ops
    from semantic_segmentation_of_stylegan2_artifacts_amd.data import synthetic_batch
    from semantic_segmentation_of_stylegan2_artifacts_amd.loss import DynamicLoss
    from semantic_segmentation_of_stylegan2_artifacts_amd.network import MSUNet
    from semantic_segmentation_of_stylegan2_artifacts_amd.trainer import Trainer
    from test_gpu_step_parity import _summary

    torch.cuda.set_device(0)
    cfg = load_config(None, "swin_t", **{"DATA.IMG_SIZE": IMG, "DATA.BATCH_SIZE": 1, "MODEL.DROP_RATE": 0.0,
                                         "MODEL.DROP_PATH_RATE": 0.0, "MODEL.ATTN_DROP_RATE": 0.0})
    torch.manual_seed(cfg.SEED)
    sd = MSUNet(cfg, img_size=IMG, num_classes=1).state_dict()
    x, y = synthetic_batch(1, IMG, DEV, 131)
    t = cfg.TRAIN

    def fresh():
        m = MSUNet(cfg, img_size=IMG, num_classes=1)
        m.load_state_dict(sd, strict=True)
        return m.to(DEV).train()

    m = fresh()
    logits = m(x)
    loss = DynamicLoss(alpha=t.TVERSKY_LOSS_ALPHA, beta=t.TVERSKY_LOSS_BETA,
                       tversky_bce_mix=t.LOSS_TVERSKY_BCE_MIX)(logits, y)
    loss.backward()
    torch.cuda.synchronize()
    out = {"fp32": _summary(logits, loss.item(), {k: p.grad for k, p in m.named_parameters() if p.grad is not None})}
    del m, logits, loss
    torch.cuda.empty_cache()

    m = fresh()
    names = {id(p): k for k, p in m.named_parameters()}
    tr = Trainer(m, cfg, DEV, lr=0.0, amp_dtype=F16, loss_scale="dynamic", use_graph=False)
    counts = {}
    with _Spy(tr, names) as spy:
        for i in range(2):  # the second step reads the shadows AdamW's pass wrote
            lb0, fq0, mt0 = ops.linbwd_calls, ops.fused_qkv_calls, ops.mlp_train_calls
            spy.grads.clear()
            loss = tr.step(x, y)
            torch.cuda.synchronize()
            counts[i] = {"linbwd": ops.linbwd_calls - lb0, "fused_qkv": ops.fused_qkv_calls - fq0,
                         "fused_mlp": ops.mlp_train_calls - mt0}
    out["f16"] = _summary(spy.logits, loss.item(), spy.grads)
    out["f16"]["counts"] = counts
    out["f16"]["lib_routes"] = [list(k) for k, v in ops._tok_cache.items()
                                if isinstance(k, tuple) and k[0] == "route" and v == "lib"]
    out["f16"]["scale"] = tr.loss_scale()
    out["f16"]["steps"] = tr.optimizer_steps()
    torch.save(out, os.path.join(outdir, "arms.pt"))


def test_f16_scaled_step_on_the_production_routes(tmp_path):
    """Swin-T at 1024^2, batch 1: stage 0 has 65 536 tokens, the smallest shape at which the
    one-pass Linear backward (``_LINBWD_MIN_M``), the token GEMM, the fused attention / MLP units
    and the persistent convs all run -- here in f16 under gradients 65 536 x their size.  Against
    the fp32 parity mode with test_gpu_step_parity.py's f16 tolerances, in a child process."""
    import torch.multiprocessing as mp
    from test_gpu_step_parity import TOL, _rel
    p = mp.get_context("spawn").Process(target=_routes_child, args=(str(tmp_path),))
    p.start()
    p.join(600)
    if p.is_alive():
        p.kill()
        p.join()
    f, log = os.path.join(tmp_path, "arms.pt"), os.path.join(tmp_path, "child.log")
    assert os.path.exists(f), (f"child exited with {p.exitcode}; its log ends:\n"
                               + (open(log).read()[-4000:] if os.path.exists(log) else ""))
    arms = torch.load(f, weights_only=True)
    ref, got = arms["fp32"], arms["f16"]
    assert set(got["norms"]) == set(ref["norms"]), sorted(set(got["norms"]) ^ set(ref["norms"]))
    gmax = max(ref["norms"].values())
    frac = {k: abs(got["norms"][k] - n) / (5e-2 * n + 1e-3 * gmax) for k, n in ref["norms"].items()}
    rec = {"logits_rel_l2": _rel(got["logits"], ref["logits"]), "loss": got["loss"], "loss_fp32": ref["loss"],
           "norm_worst_fraction_of_tol": max(frac.values()), "n_params": len(frac),
           "full_rel_l2": {k: _rel(got["full"][k], ref["full"][k]) for k in FULL},
           "counts": got["counts"], "lib_routes": got["lib_routes"], "scale": got["scale"]}
    print(json.dumps(rec))
    assert rec["logits_rel_l2"] <= TOL["f16"]["logits"], rec
    assert abs(got["loss"] - ref["loss"]) <= 1e-2 * abs(ref["loss"]), rec
    assert max(frac.values()) <= 1.0, (sorted(frac.items(), key=lambda kv: -kv[1])[:10], rec)
    assert rec["n_params"] > 300
    for k, r in rec["full_rel_l2"].items():
        assert r <= TOL["f16"]["full"], (k, rec)
    assert got["scale"] == 65536.0 and got["steps"] == 2, rec
    for c in got["counts"].values():
        assert c["linbwd"] > 0 and c["fused_qkv"] > 0 and c["fused_mlp"] > 0, rec
    assert not got["lib_routes"], rec


# ----------------------------------------------------------------------------- 6. two ranks
def _dp_worker(rank, world, port, outdir):
    import torch.distributed as dist
    from semantic_segmentation_of_stylegan2_artifacts_amd import ops
    from semantic_segmentation_of_stylegan2_artifacts_amd.trainer import Trainer
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    model, x, t, conf = _setup(batch=2)
    x, t = x[rank:rank + 1], t[rank:rank + 1]
    tr = Trainer(model, conf, dev, amp_dtype=F16, loss_scale="dynamic", bucket_mb=1 / 16, world_size=world,
                 process_group=dist.group.WORLD, rank=rank, seed=0)
    for step in range(3):
        xs = x
        if step == 1 and rank == 1:
            xs = x.clone()
            xs[0, 0, 5, 7] = float("nan")
        tr.step(xs, t)
    torch.cuda.synchronize()
    out = {"state": torch.cat([torch.cat([g.data, g.exp_avg, g.exp_avg_sq]) for g in tr.groups]).cpu(),
           "scale": tr.scale.cpu(), "tracker": tr.growth_tracker.cpu(), "skipped": tr.skipped_steps(),
           "applied": tr.optimizer_steps(), "own_scale": tr.reducer.scale is not None}
    ops.set_grad_ready_callback(None)
    torch.save(out, os.path.join(outdir, f"rank{rank}.pt"))
    dist.destroy_process_group()


def test_two_ranks_skip_and_back_off_together(tmp_path):
    """Two gloo ranks on one GPU (test_gpu_dp.py): rank 1's second image holds a NaN; its
    gradients reach rank 0 through the all-reduce, both skip that step and halve their scale."""
    import torch.multiprocessing as mp
    from test_gpu_dp import _free_port
    mp.spawn(_dp_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    r = [torch.load(os.path.join(tmp_path, f"rank{k}.pt"), weights_only=True) for k in range(2)]
    for key in ("state", "scale", "tracker"):
        assert torch.equal(r[0][key], r[1][key]), f"ranks disagree on {key}"
    for k in range(2):
        assert r[k]["skipped"] == 1 and r[k]["applied"] == 2, r[k]
        assert r[k]["scale"].item() == 32768.0 and r[k]["tracker"].item() == 1
        assert not r[k]["own_scale"]
        assert torch.isfinite(r[k]["state"]).all()


# ----------------------------------------------------------------------------- 7. state
def test_scaler_state_dict_round_trips_and_takes_a_gradscaler_state():
    from semantic_segmentation_of_stylegan2_artifacts_amd.trainer import Trainer
    model, x, t, conf = _setup()
    tr = Trainer(model, conf, DEV, amp_dtype=F16, loss_scale="dynamic", init_scale=2.0 ** 40, use_graph=False)
    tr.step(x, t)  # overflows: the state now differs from the constructor's
    sd = tr.scaler_state_dict()
    assert sd == {"scale": 2.0 ** 39, "growth_factor": 2.0, "backoff_factor": 0.5, "growth_interval": 2000,
                  "_growth_tracker": 0}
    other = Trainer(_setup()[0], conf, DEV, amp_dtype=F16, loss_scale=8.0, use_graph=False)
    other.load_scaler_state_dict(sd)
    assert other.scaler_state_dict() == sd and other.scale.item() == 2.0 ** 39
    real = torch.amp.GradScaler("cuda", init_scale=1024.0, growth_interval=5).state_dict()
    other.load_scaler_state_dict(real)
    assert other.scaler_state_dict() == real
    assert other.loss_scale() == 1024.0 and other.growth_interval == 5 and other.scale_factors == (2.0, 0.5)
    other.lr = 0.0
    other.step(x, t)  # the loaded state is what the step runs on
    assert other.loss_scale() == 1024.0 and other.growth_tracker.item() == 1 and other.optimizer_steps() == 1
