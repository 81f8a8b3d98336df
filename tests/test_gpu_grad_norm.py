"""GPU: the kernels of global-norm gradient clipping (csrc/grad_norm.hip).

``msu_grad_sumsq2`` is the step's non-finite check that also sums the squares of both flat
gradient buffers, in f64 and in a fixed order; ``msu_grad_clip_scale`` turns the partial sums
into the gradient norm and folds ``clip_grad_norm_``'s coefficient into the factor AdamW unscales
by.  Pinned here: exact integer sums over every load path (scalar head / 16-byte body / scalar
tail of each buffer, one and many workgroups, the unrolled and the remainder loop), bitwise
repeatability, the non-finite flag's contract, the f32 range, the f64 error bound, the scalar
rule bitwise against its host restatement ``trainer.grad_clip_rule``, every refused argument,
and the optimizer step the pieces make together against ``torch.optim.AdamW`` on clipped
gradients."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"

# (n0, n1): single elements, nothing at all, one workgroup with and without tails, two
# buffers whose boundary falls inside a vector, several workgroups, every workgroup looping more
# than once (n > 2 x 1024 x nblk) and enough for the four-loads-in-flight loop (n > 4 x 1024 x nblk)
SIZES = [(1, 0), (0, 1), (0, 0), (255, 0), (256, 1), (257, 255), (12293, 4099), (2000003, 1100001),
         (3000001, 2500003)]


def _ops():
    from semantic_segmentation_of_stylegan2_artifacts_amd import ops
    return ops


def _views(n0, n1, misaligned, fill):
    """x0 / x1 of n0 / n1 elements, 16-byte aligned or 4 and 12 bytes past a boundary."""
    o0, o1 = (1, 3) if misaligned else (0, 0)
    b0, b1 = fill(n0 + o0), fill(n1 + o1)
    x0, x1 = b0[o0:], b1[o1:]
    for x, o in ((x0, o0), (x1, o1)):
        assert x.numel() == 0 or x.data_ptr() % 16 == 4 * o
    return x0, x1


def _ints(n):
    g = torch.Generator().manual_seed(n + 11)
    return torch.randint(-8, 9, (n,), generator=g).float().to(DEV)


def test_block_count_depends_on_n_alone():
    ops = _ops()
    for n in (0, 1, 1024, 1025, 4096, 12293 + 4099, 1024 * 1024, 1024 * 1024 + 1, 3100004, 1 << 33):
        assert ops.grad_sumsq_blocks(n) == min(1024, max(1, -(-n // 1024))), n


@pytest.mark.parametrize("misaligned", [False, True], ids=["aligned", "misaligned"])
@pytest.mark.parametrize("n0,n1", SIZES)
def test_exact_integer_sums(n0, n1, misaligned):
    """Integers in [-8, 8]: every square, partial and total is exact in f64."""
    ops = _ops()
    x0, x1 = _views(n0, n1, misaligned, _ints)
    want = int((x0.double() ** 2).sum().item() + (x1.double() ** 2).sum().item())
    nblk = ops.grad_sumsq_blocks(n0 + n1)
    assert n0 + n1 < 3000000 or n0 + n1 > 2 * 1024 * nblk
    part = torch.full((nblk,), float("nan"), device=DEV, dtype=torch.float64)  # garbage: never cleared
    flag = torch.zeros(1, device=DEV)
    ops.grad_sumsq_(x0, part, flag, x1)
    again = torch.full((nblk,), -7.5, device=DEV, dtype=torch.float64)
    ops.grad_sumsq_(x0, again, flag, x1)
    p = part.cpu()
    assert torch.isfinite(p).all() and torch.equal(p, p.round()) and (p >= 0).all()
    assert int(p.sum().item()) == want, (p.sum().item(), want)
    assert torch.equal(part, again)
    assert flag.item() == 0.0
    if n1 == 0:  # the one-buffer form: x2 = None
        ops.grad_sumsq_(x0, again.fill_(-1.0), flag)
        assert torch.equal(part, again)


@pytest.mark.parametrize("misaligned", [False, True], ids=["aligned", "misaligned"])
@pytest.mark.parametrize("n0,n1", [(2, 3), (257, 255), (12293, 4099)])
def test_nonfinite_flag_contract(n0, n1, misaligned):
    """One non-finite value at a time, at the first and last element of each buffer (the last
    one sits in the scalar tail where the buffer is misaligned): flag 1.  A clean input writes
    nothing: 0 stays 0, 1 stays 1 (the loss's own flag survives).  flag may be null."""
    ops = _ops()
    x0, x1 = _views(n0, n1, misaligned, _ints)
    part = torch.zeros(ops.grad_sumsq_blocks(n0 + n1), device=DEV, dtype=torch.float64)
    flags = []
    for buf, pos in ((x0, 0), (x0, n0 - 1), (x1, 0), (x1, n1 - 1)):
        for bad in (float("nan"), float("inf"), float("-inf")):
            keep = buf[pos].item()
            buf[pos] = bad
            flag = torch.zeros(1, device=DEV)
            ops.grad_sumsq_(x0, part, flag, x1)
            flags.append(flag)
            assert not torch.isfinite(part.sum()).item()
            buf[pos] = keep
    assert torch.cat(flags).tolist() == [1.0] * 12
    for preset in (0.0, 1.0):
        flag = torch.full((1,), preset, device=DEV)
        ops.grad_sumsq_(x0, part, flag, x1)
        assert flag.item() == preset and torch.isfinite(part).all()
    want = part.clone()
    ops.grad_sumsq_(x0, part.fill_(-1.0), None, x1)
    assert torch.equal(part, want)


@pytest.mark.parametrize("value", [1e-30, 1e25])
def test_f32_range(value):
    """1e-30^2 underflows and 1e25^2 overflows in f32; in f64 both squares are exact."""
    ops = _ops()
    x = torch.full((1000,), value, device=DEV)
    sq = float(x[0].item()) ** 2
    ref = math.fsum([sq] * 1000)
    assert (x * x)[0].item() in (0.0, float("inf"))  # what an f32 accumulation would see
    part = torch.zeros(ops.grad_sumsq_blocks(1000), device=DEV, dtype=torch.float64)
    flag = torch.zeros(1, device=DEV)
    ops.grad_sumsq_(x, part, flag)
    got = part.cpu().sum().item()
    assert abs(got - ref) <= 1000 * 2.0 ** -52 * ref, (got, ref)
    assert flag.item() == 0.0  # large, not non-finite
    norm, inv = torch.zeros(1, device=DEV), torch.zeros(1, device=DEV)
    ops.grad_clip_scale_(part, None, 1.0, norm, inv)
    assert norm.item() == pytest.approx(math.sqrt(ref), rel=2.0 ** -23)


def test_accuracy_against_fsum():
    """|sum(part) - S_ref| <= n 2^-52 S_ref: each of the n double additions rounds by at most
    2^-53 of a running sum that never exceeds S (the squares themselves are exact)."""
    ops = _ops()
    n0, n1 = 2000003, 1100001
    g = torch.Generator().manual_seed(5)
    x0, x1 = _views(n0, n1, True, lambda n: torch.randn(n, generator=g).to(DEV))
    ref = math.fsum(v * v for v in torch.cat([x0, x1]).double().cpu().tolist())
    part = torch.zeros(ops.grad_sumsq_blocks(n0 + n1), device=DEV, dtype=torch.float64)
    ops.grad_sumsq_(x0, part, None, x1)
    got = math.fsum(part.cpu().tolist())
    print({"sum": got, "ref": ref, "rel_err": abs(got - ref) / ref, "bound": (n0 + n1) * 2.0 ** -52})
    assert abs(got - ref) <= (n0 + n1) * 2.0 ** -52 * ref


def _same(a, b):
    return a == b or (math.isnan(a) and math.isnan(b))


def test_clip_scale_equals_the_host_rule_bitwise():
    from semantic_segmentation_of_stylegan2_artifacts_amd.trainer import grad_clip_rule
    ops = _ops()
    cases = []
    for inv in (None, 0.5, 2.0 ** -16):
        i = 1.0 if inv is None else inv
        for S, mx in ((25.0, 2.5), (25.0, float("inf")), (0.0, 2.5), (float("inf"), 2.5), (float("nan"), 2.5),
                      (float("inf"), float("inf"))):
            cases.append(([S], inv, mx))
        for S in (1.0, 2.0, 3.0, 7.0, 10.0, 1000.0, 12345.0, 99980001.0, 2.0 ** 40 + 1.0, 2.0 ** 52 + 2.0):
            norm = math.sqrt(S) * i
            for mx in (0.5 * norm, norm, norm * (1 + 1e-7), norm + 2e-6, 2.0 * norm, 1e-3, 1e6):
                cases.append(([S], inv, mx))
    g = torch.Generator().manual_seed(3)
    for nblk in (2, 255, 256, 300, 1024):  # the fixed-order sum: exact on integers, any order
        cases.append((torch.randint(0, 1 << 20, (nblk,), generator=g).double().tolist(), 0.5, 100.0))
    norm_out = torch.full((len(cases),), -1.0, device=DEV)
    inv_out = torch.full((len(cases),), -1.0, device=DEV)
    inv_in = {v: torch.full((1,), v, device=DEV) for v in (0.5, 2.0 ** -16)}
    keep = []
    for k, (part, inv, mx) in enumerate(cases):
        keep.append(torch.tensor(part, device=DEV, dtype=torch.float64))
        ops.grad_clip_scale_(keep[-1], None if inv is None else inv_in[inv], mx, norm_out[k:k + 1], inv_out[k:k + 1])
    norm_out, inv_out = norm_out.cpu().tolist(), inv_out.cpu().tolist()
    wrong = []
    for k, (part, inv, mx) in enumerate(cases):
        S = part[0] if len(part) == 1 else float(sum(int(v) for v in part))
        want = grad_clip_rule(S, inv, mx)
        if not (_same(norm_out[k], want[0]) and _same(inv_out[k], want[1])):
            wrong.append((S, inv, mx, (norm_out[k], inv_out[k]), want))
    assert not wrong, wrong[:10]
    assert all(t.item() in (0.5, 2.0 ** -16) for t in inv_in.values())  # read only


def test_refused_arguments_launch_nothing():
    from semantic_segmentation_of_stylegan2_artifacts_amd import _lib
    ops = _ops()
    L = _lib.lib()
    s = torch.cuda.current_stream().cuda_stream
    x0, x1 = torch.ones(3000, device=DEV), torch.ones(500, device=DEV)
    nblk = ops.grad_sumsq_blocks(3500)
    assert nblk == 4
    part = torch.full((8,), -3.0, device=DEV, dtype=torch.float64)
    flag = torch.zeros(1, device=DEV)
    good = [x0.data_ptr(), 3000, x1.data_ptr(), 500, part.data_ptr(), nblk, flag.data_ptr(), s]
    assert L.msu_grad_sumsq_nblk(-5) == 1
    for idx, bad in ((4, None), (0, None), (2, None), (1, -1), (3, -1), (5, nblk + 1), (5, nblk - 1), (5, 0)):
        args = list(good)
        args[idx] = bad
        assert L.msu_grad_sumsq2(*args) == -2, (idx, bad)
    # a null buffer is fine where it is empty
    assert L.msu_grad_sumsq2(x0.data_ptr(), 3000, None, 0, part.data_ptr(), ops.grad_sumsq_blocks(3000), None, s) == 0
    torch.cuda.synchronize()
    assert part[:3].sum().item() == 3000.0 and (part[3:] == -3.0).all()
    part.fill_(-3.0)
    inv_in = torch.full((1,), 0.5, device=DEV)
    norm_out, inv_out = torch.full((1,), -1.0, device=DEV), torch.full((1,), -2.0, device=DEV)
    good = [part.data_ptr(), 4, inv_in.data_ptr(), 1.0, norm_out.data_ptr(), inv_out.data_ptr(), s]
    for idx, bad in ((0, None), (1, 0), (1, -1), (1, 1025), (4, None), (5, None), (5, inv_in.data_ptr()),
                     (5, norm_out.data_ptr()), (3, 0.0), (3, -1.0), (3, float("nan")), (3, float("-inf"))):
        args = list(good)
        args[idx] = bad
        assert L.msu_grad_clip_scale(*args) == -2, (idx, bad)
    torch.cuda.synchronize()
    assert flag.item() == 0.0 and (part == -3.0).all() and inv_in.item() == 0.5
    assert norm_out.item() == -1.0 and inv_out.item() == -2.0
    # the Python wrappers refuse before the library is called
    p4 = torch.zeros(4, device=DEV, dtype=torch.float64)
    for call in (lambda: ops.grad_sumsq_(x0, p4.float(), flag, x1),
                 lambda: ops.grad_sumsq_(x0, p4[:3], flag, x1),
                 lambda: ops.grad_sumsq_(x0.double(), p4, flag, x1),
                 lambda: ops.grad_sumsq_(x0, p4, flag, x1.half()),
                 lambda: ops.grad_sumsq_(x0[::2], p4[:2], flag),
                 lambda: ops.grad_sumsq_(x0, p4, flag.double(), x1),
                 lambda: ops.grad_clip_scale_(p4.float(), inv_in, 1.0, norm_out, inv_out),
                 lambda: ops.grad_clip_scale_(p4[:0], inv_in, 1.0, norm_out, inv_out),
                 lambda: ops.grad_clip_scale_(p4, inv_in.double(), 1.0, norm_out, inv_out),
                 lambda: ops.grad_clip_scale_(p4, inv_in, 1.0, norm_out.double(), inv_out),
                 lambda: ops.grad_clip_scale_(p4, inv_in, 1.0, norm_out, inv_out.half()),
                 lambda: ops.grad_clip_scale_(p4, inv_in, 0.0, norm_out, inv_out),
                 lambda: ops.grad_clip_scale_(p4, inv_in, float("nan"), norm_out, inv_out),
                 lambda: ops.grad_clip_scale_(p4, inv_in, True, norm_out, inv_out),
                 lambda: ops.grad_clip_scale_(p4, inv_in, "1", norm_out, inv_out),
                 lambda: ops.grad_clip_scale_(p4, inv_in, 1.0, norm_out, inv_in),
                 lambda: ops.grad_clip_scale_(p4, inv_in, 1.0, norm_out, norm_out)):
        with pytest.raises(ValueError):
            call()
    torch.cuda.synchronize()
    assert norm_out.item() == -1.0 and inv_out.item() == -2.0 and inv_in.item() == 0.5


def test_clipped_adamw_dev_matches_torch_adamw_on_clipped_gradients():
    """test_adamw_dev_skip_matches_torch_adamw's three steps (the middle one non-finite) through
    grad_sumsq_ -> step_advance_ -> grad_clip_scale_(max 40) -> adamw_dev_(inv_scale=clip_inv):
    torch.optim.AdamW fed the f64-clipped, f32-rounded gradients of the two finite steps (norms
    about 100 and 50: both clip).  That test's tolerances, widened by the extra roundings: the
    factor rounds to f32 once and the product once, the reference's own rounding once -- 3 x 2^-24
    = 1.8e-7 on the gradient, twice that on its square.  The moments are compared, not only the
    parameters: Adam's first update is nearly invariant to a rescaled gradient."""
    from semantic_segmentation_of_stylegan2_artifacts_amd.trainer import grad_clip_rule
    ops = _ops()
    g = torch.Generator().manual_seed(7)
    n, max_norm = 10007, 40.0
    p0 = torch.randn(n, generator=g)
    grads = [torch.randn(n, generator=g) * s for s in (1.0, 3.0, 0.5)]
    sumsq = [math.fsum(v * v for v in gr.double().tolist()) for gr in grads]
    ref = p0.clone().requires_grad_(True)
    opt = torch.optim.AdamW([ref], lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.05)
    for k in (0, 2):
        coef = max_norm / (math.sqrt(sumsq[k]) + 1e-6)
        assert coef < 1.0
        ref.grad = (grads[k].double() * coef).float()
        opt.step()
    p = p0.to(DEV)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    hyper = torch.tensor([1e-2, 0.0], device=DEV, dtype=torch.float64)
    found = torch.zeros(1, device=DEV)
    part = torch.zeros(ops.grad_sumsq_blocks(n), device=DEV, dtype=torch.float64)
    norm_dev, clip_inv = torch.zeros(1, device=DEV), torch.zeros(1, device=DEV)
    for k in range(3):
        gd = grads[k].to(DEV)
        if k == 1:
            gd[17] = float("inf")
        found.zero_()
        ops.grad_sumsq_(gd, part, found)
        ops.step_advance_(hyper, found)
        ops.grad_clip_scale_(part, None, max_norm, norm_dev, clip_inv)
        ops.adamw_dev_(p, gd, m, v, hyper, 0.9, 0.999, 1e-8, 0.05, inv_scale=clip_inv, found_inf=found)
        want = grad_clip_rule(math.fsum(part.cpu().tolist()), None, max_norm)
        if k == 1:
            assert found.item() == 1.0 and norm_dev.item() == float("inf") and clip_inv.item() == 0.0
        else:
            assert found.item() == 0.0
            assert norm_dev.item() == pytest.approx(math.sqrt(sumsq[k]), rel=2.0 ** -23)
            assert abs(clip_inv.item() - want[1]) <= 2.0 ** -23 * want[1]  # one f32 ulp
    assert hyper[1].item() == 2.0
    torch.testing.assert_close(p.cpu(), ref.detach(), rtol=4e-7, atol=1e-8)
    torch.testing.assert_close(m.cpu(), opt.state[ref]["exp_avg"], rtol=6e-7, atol=2e-8)
    torch.testing.assert_close(v.cpu(), opt.state[ref]["exp_avg_sq"], rtol=8e-7, atol=1e-12)
    # clipping really happened: the unclipped first moment is 2.5x larger
    unclipped = 0.1 * grads[2] + 0.9 * 0.1 * grads[0]
    assert m.cpu().norm().item() < 0.6 * unclipped.norm().item()
