"""Every reachable kernel variant of csrc/layernorm.hip against an fp64 reference, judged per row.

The C API is driven directly (``_lib.call``), so the nullable arguments, ``accumulate`` and
``nparts`` are under the test's control; ``nparts`` is ``msu_ln_part_blocks`` and ``part`` is
sized as ``ops._ln_parts`` sizes it.  The references are tests/_parity_refs.py (plain PyTorch in
float64 on the device), fed the same storage-rounded tensors as the kernel.

Reachable variants ``<TPR lanes per row, KMAX 16-byte chunks per lane>`` (default build, both
directions; nchunk = C / VW, VW = 8 for bf16 / f16 and 4 for f32):

    nchunk <= 16 -> <16,1>    <= 32 -> <32,1>    <= 64 -> <64,1>
           <= 128 -> <32,4>   <= 256 -> <64,4>   <= 512 -> <64,8> (f32 only: C <= 2048)

For 16-bit storage the three KMAX = 1 rows take the software-prefetched row loop.  The widths
below sit on both edges of every boundary; ``_assert_coverage`` recomputes the variant from
(C, dtype) and fails at import if a (mode, dtype, variant) triple of the table has no case.
Head: ``head_*16_kernel<3 / 4>`` (16-bit, C = 96 / 128), ``head_*_kernel<4>`` (C <= 128) and
``<8>`` (C <= 256).

Inputs: about one row in eight of every tensor is adversarial (a large common offset
30 + 0.5 randn, a dyadic constant row 7.25 with variance 0, one 100.0 outlier in zeros,
1e-3 randn, alternating +-6e4), the rest randn.  Narrow rows take a smaller offset
(min(30, 3 sqrt C); constant 1.25 below C = 16): over 2e5 rows of 4 or 8 elements the spread of
some rows collapses, any f32 x - mean then loses offset / spread * 2^-24, and a plain f32
PyTorch evaluation of the add-mode long case at C = 4 already missed the dx bound (1.19) with
the wide-row offsets.  The adversarial rows of the tensors of one case
never coincide (a +-6e4 row of a and of b would overflow f16 in a + 1.25 b), and the f16
*gradient* tensors (dy, dres*) alternate +-100, not +-6e4: rstd reaches 316 on a constant row and
~100 on a narrow randn row, and the f16 dx would overflow.  Short cases run 1, 3, 256 / TPR + 1
and 257 rows (the nearest counts the gather modes allow, plus their 2 x 6 x 10 / 2 x 3 x 5
grids); long cases run 3 * 4096 * (256 / TPR) + 37 rows forward and 3 * nparts_cap * (256 / TPR)
+ 37 rows backward (3 samples, rows_per_sample = ceil(rows / 3), scales {0, 1.25, 1}), so every
lane group walks at least three rows of the prefetched loops with a ragged last pass.

Tolerance rule (u_T = 2^-9 bf16, 2^-12 f16, 0 f32; tau = 1e-4, the project's fp32 tolerance):

* y, dx, db, head dz, per element: |out - ref| <= 2 u_T |ref| + tau A_row (+ 2^-25 for f16, half
  the spacing of its subnormals: below 2^-14 a stored f16 has no relative accuracy, and dx of a
  +-6e4 row lies there), A_row the row's max of
  the summed absolute addends of the output (y: |xhat gamma| + |beta|; dx: |LN'| + |dres| +
  |dres2| + |dres3|; db: scale times that).  Rows with scale 0 have A_row = 0: db must be 0.
* s (add mode) against the fp64 sum a + scale b: one storage rounding, |out - ref| <= 2 u_T |ref|
  + 2^-22 A_row (A_row = max |a| + |scale b|; the f32 multiply and add round once each).  y and
  the backward are then referred to the kernel's own s.
* rstd: relative 1e-5; a constant row has rstd = eps^-1/2.  mean: |out - ref| <= 1e-5 mean|x|
  over the row (a relative error against the mean itself has no meaning where the mean of a
  randn row happens to vanish; the sum is judged against its absolute addends like the rest).
* head logit (an f32 row sum): |out - ref| <= tau sum_c (|xhat gamma w| + |beta w|).
* column sums (dgamma, dbeta, head dw; also part rows summed in fp64 when dgamma = dbeta = NULL,
  and |initial value| added to the sum under accumulate): |out - ref| <= K 2^-24 sum_rows |term|,
  the terms split into their addends like everything above (dgamma: |dy| rstd (|x| + |mean|), so
  the cancellation in x - mean of an offset row is part of the condition; dbeta: |dy|).
  K = 8 times the worst such ratio of an f32 ``torch.sum(dim=0)`` of the fp64 terms on the long
  cases: 7.99 on the device (its column sum over 2e5 narrow rows is a long sequential chain), so
  K = 64.  (One-row cases, where the f32 sum is one rounding of one term: 0.98.)

Measured on an MI355X (profiles/r07b_ln_matrix_ratios.txt; the whole module: 198 tests in 8.9 s,
the slowest 1.6 s, a long case 0.05 s), worst err / bound over the module, bf16 / f16 / f32:

    y       0.971 / 0.830 / 0.131      s       0.996 / 0.999 / 0.250
    dx      0.971 / 0.999 / 0.923      db      0.971 / 0.836 / 0.923
    mean    0.014 / 0.009 / 0.017      rstd    0.075 / 0.075 / 0.075
    dgamma  0.138 / 0.160 / 0.088      dbeta   0.080 / 0.057 / 0.075
    head: logit 0.004 / 0.004 / 0.010, dz 0.971 / 0.999 / 0.011, dgamma 0.048 / 0.044 / 0.049,
          dbeta 0.109 / 0.109 / 0.085, dw 0.071 / 0.071 / 0.055

The 16-bit 0.97 .. 0.999 are the one storage rounding 2 u_T allows (an element just above a
power of two).  The f32 dx / db 0.923 is one row of the add-mode long case at C = 4 (dy =
+-6e4 alternating, |LN'| = 3e-3 |dy gamma| rstd after cancellation; the next row sits at 0.10).
With the forward prefetch changed to fetch(r) in place of fetch(r + stride) (a scratch build,
not kept) the twelve 16-bit KMAX = 1 long cases fail and every short case still passes.

Found by this module: head_fwd16_kernel at C = 96 took mean = sum * (1 / 96); the inexact
reciprocal, contracted into v - mean, left d = -2^-25 |mean| on a constant row, and the logit
missed its bound by 1.78 (long-head-*-C96-h16x3).  It divides now.
"""
import math

import pytest
import torch

from _parity_refs import (d2s2_rows, ln_add_ref, ln_d2s2_ref, ln_head_ref, ln_merge_ref, ln_plain_ref,
                          merge_rows)

pytestmark = pytest.mark.gpu

DEV = "cuda"
EPS = 1e-5
TAU = 1e-4
K_COL = 64.0  # 8 x 7.99, the worst f32 torch.sum ratio measured on the long cases (module docstring)
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
DTYPES = [BF16, F16, F32]
DTNAME = {F32: "f32", BF16: "bf16", F16: "f16"}
U_T = {F32: 0.0, BF16: 2.0 ** -9, F16: 2.0 ** -12}
# half the spacing 2^-24 of the f16 subnormals: below 2^-14 a stored f16 has no relative accuracy
FLOOR_T = {F32: 0.0, BF16: 0.0, F16: 2.0 ** -25}
PLAIN, ADD, MERGE, D2S2 = 0, 1, 2, 3
MODENAME = {PLAIN: "plain", ADD: "add", MERGE: "merge", D2S2: "d2s"}

REACHABLE = {BF16: [(16, 1), (32, 1), (64, 1), (32, 4), (64, 4)],
             F16: [(16, 1), (32, 1), (64, 1), (32, 4), (64, 4)],
             F32: [(16, 1), (32, 1), (64, 1), (32, 4), (64, 4), (64, 8)]}
W16 = [8, 96, 128, 136, 256, 264, 512, 520, 1024, 1032, 2048]
W32 = [4, 48, 64, 68, 128, 132, 256, 260, 512, 516, 1024, 1028, 2048]
# merge: C = 4 Cin with Cin % VW == 0 -- the nearest legal widths on both sides of each boundary
M16 = [32, 96, 128, 160, 256, 288, 512, 544, 1024, 1056, 2048]
M32 = [16, 48, 64, 80, 128, 144, 256, 272, 512, 528, 1024, 1040, 2048]
HEAD_WIDTHS = [4, 64, 96, 128, 132, 192, 256]


def _vw(dtype):
    return 4 if dtype == F32 else 8


def variant(C, dtype):
    """(TPR, KMAX) launch_fwd / launch_bwd pick for a row of C elements."""
    n = C // _vw(dtype)
    for cap, v in ((16, (16, 1)), (32, (32, 1)), (64, (64, 1)), (128, (32, 4)), (256, (64, 4)), (512, (64, 8))):
        if n <= cap:
            return v
    raise ValueError(C)


def head_variant(C, dtype):
    if dtype != F32 and C in (96, 128):
        return "h16x%d" % (C // 32)
    return "hx4" if C <= 128 else "hx8"


def _widths(mode, dtype):
    if mode == MERGE:
        return M32 if dtype == F32 else M16
    return W32 if dtype == F32 else W16


SHORT = [(mode, dt, C) for mode in (PLAIN, ADD, MERGE, D2S2) for dt in DTYPES for C in _widths(mode, dt)]
# one long case per (dtype, variant), at the variant's smallest width
LONG = [(mode, dt, min(C for C in _widths(mode, dt) if variant(C, dt) == v))
        for mode in (ADD, PLAIN) for dt in DTYPES for v in REACHABLE[dt]]
HEAD = [(dt, C) for dt in DTYPES for C in HEAD_WIDTHS]
HEAD_LONG = [(dt, C) for dt in (BF16, F16) for C in (96, 128)]


def _id(mode, dt, C):
    return "%s-%s-C%d-v%dx%d" % ((MODENAME[mode], DTNAME[dt], C) + variant(C, dt))


def _head_id(dt, C):
    return "head-%s-C%d-%s" % (DTNAME[dt], C, head_variant(C, dt))


def _assert_coverage():
    want = {(m, dt, v) for m in (PLAIN, ADD, MERGE, D2S2) for dt in DTYPES for v in REACHABLE[dt]}
    got = {(m, dt, variant(C, dt)) for m, dt, C in SHORT}
    assert got == want, want ^ got
    assert {(m, dt, variant(C, dt)) for m, dt, C in LONG} == {t for t in want if t[0] in (ADD, PLAIN)}
    for dt in DTYPES:  # both edges of every boundary: the last width of a variant, the first legal one of the next
        for ws, step in ((_widths(PLAIN, dt), 1), (_widths(MERGE, dt), 4)):
            chunks = sorted(c // _vw(dt) for c in ws)
            assert chunks[-1] * _vw(dt) == 2048
            for cap in (16, 32, 64, 128, 256):
                above = [n for n in chunks if n > cap]
                assert cap in chunks and (not above or min(above) == cap + step), (dt, cap)
    want_h = {(dt, v) for dt in DTYPES for v in ("hx4", "hx8")} | {(dt, v) for dt in (BF16, F16)
                                                                 for v in ("h16x3", "h16x4")}
    assert {(dt, head_variant(C, dt)) for dt, C in HEAD} == want_h
    assert len({_id(*c) for c in SHORT}) == len(SHORT) and len({_id(*c) for c in LONG}) == len(LONG)


_assert_coverage()


# ----------------------------------------------------------------------------- plumbing
def _L():
    from semantic_segmentation_of_stylegan2_artifacts_amd import _lib
    return _lib


def _p(t):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _code(dtype):
    return {F32: 0, BF16: 1, F16: 2}[dtype]


SENT = 12288.0  # exact in every storage type


class Buf:
    """An output buffer of n elements in front of a guard of 64 sentinel elements; the payload
    starts as NaN, so an element the kernel never wrote fails the comparison."""

    def __init__(self, n, dtype):
        self.full = torch.full((n + 64,), float("nan"), device=DEV, dtype=dtype)
        self.full[n:] = SENT
        self.n = n
        self.t = self.full[:n]

    def check(self, what):
        assert bool((self.full[self.n:] == SENT).all()), f"{what}: wrote past its end"
        assert bool(torch.isfinite(self.t).all()), f"{what}: unwritten or non-finite elements"
        return self.t


def _mix(rows, C, dtype, seed, slot, rot, big=6e4):
    """[rows, C] randn with about one adversarial row in eight.  slot: the tensor's number within
    its case (distinct slots never share an adversarial row); rot moves the pattern per case."""
    g = torch.Generator(device=DEV).manual_seed(seed * 16 + slot)
    z = torch.randn(rows, C, generator=g, device=DEV)
    r = torch.arange(rows, device=DEV) + ((slot + rot) % 8) + 8 * (rot % 5)
    adv, kind = (r % 8 == 0), (r // 8) % 5
    col = torch.arange(C, device=DEV)

    def k(i):
        return (adv & (kind == i)).unsqueeze(1)

    out = torch.where(k(0), min(30.0, 3.0 * math.sqrt(C)) + 0.5 * z, z)
    out = torch.where(k(1), torch.full_like(z, 7.25 if C >= 16 else 1.25), out)
    hot = col.unsqueeze(0) == (r % C).unsqueeze(1)
    out = torch.where(k(2), torch.where(hot, 100.0, 0.0).to(z.dtype), out)
    out = torch.where(k(3), 1e-3 * z, out)
    out = torch.where(k(4), (big * (1 - 2 * (col % 2))).to(z.dtype).unsqueeze(0).expand_as(z), out)
    return out.to(dtype).contiguous()


def _gbig(dtype):
    return 100.0 if dtype == F16 else 6e4


def _bbig(dtype):
    return 5e4 if dtype == F16 else 6e4  # a + 1.25 b stays below the f16 maximum 65504


def _affine(C, seed):
    g = torch.Generator(device=DEV).manual_seed(1000 + seed)
    gamma = 1 + 0.1 * torch.randn(C, generator=g, device=DEV)
    beta = 0.1 * torch.randn(C, generator=g, device=DEV)
    gamma[C // 2] = 0.0
    gamma[C - 1] = -1.5
    return gamma.contiguous(), beta.contiguous()


# worst err / bound per (output, dtype), and the f32 torch.sum ratios K_COL comes from
STATS = {}


def _note(name, dtype, ratio):
    key = (name, DTNAME.get(dtype, dtype))
    STATS[key] = max(STATS.get(key, 0.0), float(ratio))


def _ratio(err, bound):
    """max err / bound; a zero bound demands a zero error."""
    bad = (bound == 0) & (err > 0)
    if bool(bad.any()):
        return float("inf")
    q = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.zeros_like(err))
    return float(q.max()) if q.numel() else 0.0


def _elem(name, tag, dtype, out, ref, a_row, abs_c=TAU):
    """|out - ref| <= 2 u_T |ref| + abs_c A_row, per element, A_row per row."""
    out = out.double().reshape(ref.shape)
    bound = 2 * U_T[dtype] * ref.abs() + abs_c * a_row.reshape(-1, 1) + FLOOR_T[dtype]
    q = _ratio((out - ref).abs(), bound)
    print(f"{tag} {name}: err/bound {q:.3f}")
    _note(name, dtype, q)
    assert q <= 1.0, f"{tag} {name}: err / bound = {q:.3f}"


def _stats_chk(tag, dtype, mean, rstd, ref):
    xr = ref["xr"]
    qm = _ratio((mean.double() - ref["mean"]).abs(), 1e-5 * xr.abs().mean(-1))
    qr = _ratio((rstd.double() - ref["rstd"]).abs(), 1e-5 * ref["rstd"])
    const = (xr == xr[:, :1]).all(-1)
    if bool(const.any()):  # variance 0: rstd = eps^-1/2
        qr = max(qr, _ratio((rstd.double()[const] - EPS ** -0.5).abs(), torch.full_like(ref["rstd"][const], 1e-5 * EPS ** -0.5)))
    print(f"{tag} mean: err/bound {qm:.3f}  rstd: {qr:.3f}")
    _note("mean", dtype, qm)
    _note("rstd", dtype, qr)
    assert qm <= 1.0 and qr <= 1.0, f"{tag}: mean {qm:.3f} rstd {qr:.3f}"


def _col(name, tag, dtype, out, ref, abs_sum, terms=None, kind="long"):
    """|out - ref| <= K 2^-24 sum_rows |term| per column (abs_sum: that sum, fp64); terms: the
    fp64 terms themselves, for the f32 torch.sum figure K_COL is derived from."""
    unit = 2.0 ** -24 * abs_sum
    q = _ratio((out.double().reshape(-1) - ref).abs(), K_COL * unit)
    print(f"{tag} {name}: err/bound {q:.3f}")
    _note(name, dtype, q)
    if terms is not None:
        s32 = terms.float().sum(0).double()
        _note("sum32_" + kind, "any", _ratio((s32 - ref).abs(), unit))
    assert q <= 1.0, f"{tag} {name}: err / bound = {q:.3f}"


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nln matrix: worst err / bound per (output, dtype); sum32_*: f32 torch.sum of the fp64 terms / (2^-24 sum|term|)")
    for (name, dt), v in sorted(STATS.items()):
        print(f"  LNMATRIX {name:12s} {dt:5s} {v:.4f}")


# ----------------------------------------------------------------------------- one case
class Case:
    """The tensors of one (mode, dtype, C, rows) case, its forward through the kernel (checked)
    and the pieces every backward option needs."""

    def __init__(self, mode, dtype, C, shape, seed, nsamples=1, scales=None):
        self.mode, self.dtype, self.C = mode, dtype, C
        self.tag = f"{MODENAME[mode]}/{DTNAME[dtype]}/C{C}/{'x'.join(map(str, shape))}"
        rot = seed
        big = _gbig(dtype)
        self.gamma, self.beta = _affine(C, seed)
        self.H = self.W = self.Cin = 0
        if mode == MERGE:
            B, H, W = shape
            self.H, self.W, self.Cin = H, W, C // 4
            self.rows = B * (H // 2) * (W // 2)
            self.x = _mix(B * H * W, C // 4, dtype, seed, 0, rot).view(B, H, W, C // 4)
            self.rowsof = merge_rows
        elif mode == D2S2:
            B, H, W = shape
            self.H, self.W = H, W
            self.rows = B * 4 * H * W
            self.x = _mix(B * H * W, 4 * C, dtype, seed, 0, rot).view(B, H, W, 4 * C)
            self.rowsof = d2s2_rows
        else:
            (self.rows,) = shape
            self.x = _mix(self.rows, C, dtype, seed, 0, rot)
            self.rowsof = lambda t: t.reshape(-1, C)
        rows = self.rows
        self.rps = -(-rows // nsamples)
        self.scale = None if scales is None else torch.tensor(scales, device=DEV, dtype=torch.float32)
        self.b = _mix(rows, C, dtype, seed, 1, rot, _bbig(dtype)) if mode == ADD else None
        self.dy = _mix(rows, C, dtype, seed, 2, rot, big)
        self.dres = [_mix(rows, C, dtype, seed, 3 + i, rot, big) for i in range(3)] if mode in (PLAIN, ADD) else []
        n = _L().lib().msu_ln_part_blocks(rows, C)
        cap = 512 if C >= 384 else 1024
        assert n == max(1, min(-(-rows // 16), cap))
        self.nparts = n

    # ---- forward
    def fwd(self, use_b=True, use_scale=True, use_s=True):
        m, dt, C, rows = self.mode, self.dtype, self.C, self.rows
        y, mean, rstd = Buf(rows * C, dt), Buf(rows, F32), Buf(rows, F32)
        s = Buf(rows * C, dt) if (m == ADD and use_s) else None
        b = self.b if (m == ADD and use_b) else None
        sc = self.scale if (m == ADD and use_scale) else None
        _L().call("msu_layernorm_fwd", _code(dt), m, _p(self.x), _p(b), _p(sc), self.rps, _p(s.t if s else None),
                  _p(self.gamma), _p(self.beta), _p(y.t), _p(mean.t), _p(rstd.t), rows, C, self.H, self.W, self.Cin,
                  EPS, _stream())
        torch.cuda.synchronize()
        return (y.check("y"), mean.check("mean"), rstd.check("rstd"), s.check("s").view(rows, C) if s else None, b, sc)

    def check_fwd(self, use_b=True, use_scale=True, use_s=True, s_from=None):
        """Runs the forward and checks it; returns (s or x, mean, rstd) for the backward.
        s_from: the kernel's s of an earlier launch with the same operands (for s_out = NULL)."""
        m, dt, C = self.mode, self.dtype, self.C
        y, mean, rstd, s, b, sc = self.fwd(use_b, use_scale, use_s)
        tag = self.tag + f"/fwd(b={int(b is not None)},sc={int(sc is not None)},s={int(s is not None)})"
        if m == ADD:
            s_k = s if s is not None else s_from
            ref = ln_add_ref(self.x, b, sc, self.rps, self.gamma, self.beta, None, EPS, s=s_k)
            if s is not None:
                a_abs = self.x.double().abs()
                if b is not None:
                    bb = b.double().abs()
                    a_abs = a_abs + (bb if sc is None else ref["scale_rows"].abs() * bb)
                _elem("s", tag, dt, s, ref["s"], a_abs.amax(-1), abs_c=2.0 ** -22)
        elif m == PLAIN:
            ref = ln_plain_ref(self.x, self.gamma, self.beta, None, EPS)
        elif m == MERGE:
            ref = ln_merge_ref(self.x, self.gamma, self.beta, None, EPS)
        else:
            ref = ln_d2s2_ref(self.x, self.gamma, self.beta, None, EPS)
        g64, b64 = self.gamma.double(), self.beta.double()
        xhat = (ref["xr"] - ref["mean"].unsqueeze(-1)) * ref["rstd"].unsqueeze(-1)
        _elem("y", tag, dt, y, ref["y"], ((xhat * g64).abs() + b64.abs()).amax(-1))
        _stats_chk(tag, dt, mean, rstd, ref)
        return (s if m == ADD else self.x), mean, rstd

    # ---- backward
    def check_bwd(self, xs, mean, rstd, nres=0, use_db=True, use_scale=True, out="direct", tail=None, api3=False,
                  kind="short"):
        """xs: the normalised input the backward reads (add: the kernel's s).  out: 'direct'
        (dgamma / dbeta written), 'acc' (accumulate = 1 onto non-zero values), 'part' (dgamma =
        dbeta = NULL: only the partial rows).  tail: msu_tail_reduce_mode for this launch."""
        m, dt, C, rows, n = self.mode, self.dtype, self.C, self.rows, self.nparts
        lib = _L()
        has_res = m in (PLAIN, ADD)
        dres = self.dres[:nres] if has_res else []
        sc = self.scale if (m == ADD and use_scale) else None
        dx = Buf(self.x.numel() if m != ADD else rows * C, dt)
        db = Buf(rows * C, dt) if (m == ADD and use_db) else None
        part = torch.full((n * 3 * C,), float("nan"), device=DEV, dtype=torch.float32)  # ops._ln_parts
        init = None
        if out == "part":
            dg = dbt = None
        else:
            both = torch.full((2 * C + 128,), SENT, device=DEV, dtype=torch.float32)
            # contiguous [dgamma | dbeta] (one reduction launch) or, under accumulate, apart
            dg, dbt = (both[:C], both[C:2 * C]) if out == "direct" else (both[:C], both[C + 64:2 * C + 64])
            if out == "acc":
                gi = torch.Generator(device=DEV).manual_seed(77)
                dg.copy_(3.0 * torch.randn(C, generator=gi, device=DEV))
                dbt.copy_(3.0 * torch.randn(C, generator=gi, device=DEV))
                init = torch.cat([dg, dbt]).double()
            guard = both.clone()
        prev = lib.lib().msu_tail_reduce_mode(tail) if tail is not None else None
        try:
            r = [_p(t) for t in dres] + [None] * (3 - len(dres))
            head = (_code(dt), m, _p(self.dy), _p(xs))
            rest = (_p(self.gamma), _p(mean), _p(rstd), _p(dx.t), _p(db.t if db else None), _p(sc), self.rps,
                    _p(part), n, _p(dg), _p(dbt), rows, C, self.H, self.W, self.Cin, int(out == "acc"), _stream())
            if api3 or nres > 1:
                lib.call("msu_layernorm_bwd3", *head, r[0], r[1], r[2], *rest)
            else:
                lib.call("msu_layernorm_bwd", *head, r[0], *rest)
            torch.cuda.synchronize()
        finally:
            if prev is not None:
                lib.lib().msu_tail_reduce_mode(prev)
        tag = self.tag + f"/bwd(nres={len(dres)},db={int(db is not None)},sc={int(sc is not None)},{out},tail={tail})"
        # reference: LN'(dy) at the input the kernel normalised, plus the residual gradients
        if m == ADD:
            ref = ln_plain_ref(xs, self.gamma, self.beta, self.dy, EPS, dres=dres)
        elif m == PLAIN:
            ref = ln_plain_ref(self.x, self.gamma, self.beta, self.dy, EPS, dres=dres)
        elif m == MERGE:
            ref = ln_merge_ref(self.x, self.gamma, self.beta, self.dy, EPS)
        else:
            ref = ln_d2s2_ref(self.x, self.gamma, self.beta, self.dy, EPS)
        dx_ref = self.rowsof(ref["dx"])
        res_abs = sum((t.double().abs() for t in dres), torch.zeros_like(dx_ref))
        res_sum = sum((t.double() for t in dres), torch.zeros_like(dx_ref))
        a_row = ((dx_ref - res_sum).abs() + res_abs).amax(-1)      # |LN'| + |dres| + |dres2| + |dres3|
        _elem("dx", tag, dt, self.rowsof(dx.check("dx").view(self.x.shape if m != ADD else (rows, C))), dx_ref, a_row)
        if db is not None:
            idx = torch.arange(rows, device=DEV) // self.rps
            scr = torch.ones(rows, device=DEV, dtype=torch.float64) if sc is None else sc.double()[idx]
            _elem("db", tag, dt, db.check("db"), dx_ref * scr.unsqueeze(-1), a_row * scr.abs())
        # column sums
        dy64 = self.dy.double()
        mu, rs = ref["mean"].unsqueeze(-1), ref["rstd"].unsqueeze(-1)
        tg = dy64 * (ref["xr"] - mu) * rs
        ag = (dy64.abs() * rs * (ref["xr"].abs() + ref["xr"].abs().mean(-1, keepdim=True))).sum(0)
        ab = dy64.abs().sum(0)
        if out == "part":
            p = part[:n * 2 * C].double().view(n, 2, C)
            assert bool(torch.isfinite(p).all()), f"{tag}: unwritten partial rows"
            got_g, got_b = p[:, 0].sum(0), p[:, 1].sum(0)
            refg, refb = ref["dgamma"], ref["dbeta"]
        else:
            seen = both.clone()
            seen[dg.storage_offset():dg.storage_offset() + C] = guard[dg.storage_offset():dg.storage_offset() + C]
            seen[dbt.storage_offset():dbt.storage_offset() + C] = guard[dbt.storage_offset():dbt.storage_offset() + C]
            assert torch.equal(seen, guard), f"{tag}: dgamma / dbeta wrote outside their C elements"
            got_g, got_b = dg, dbt
            refg, refb = ref["dgamma"], ref["dbeta"]
            if init is not None:
                refg, refb = refg + init[:C], refb + init[C:]
                ag, ab = ag + init[:C].abs(), ab + init[C:].abs()
        _col("dgamma", tag, dt, got_g, refg, ag, None if init is not None else tg, kind)
        _col("dbeta", tag, dt, got_b, refb, ab, None if init is not None else dy64, kind)


# backward options, cycled over the row counts of a case so that every (mode, dtype, width) runs
# each of them once: (nres, db, bscale, out, tail mode, through msu_layernorm_bwd3)
BWD_ADD = [(0, True, True, "direct", None, False), (1, True, True, "acc", None, False),
           (2, False, True, "part", None, True), (3, True, True, "direct", 0, True),
           (1, True, False, "direct", 1, True), (3, False, False, "acc", None, True),
           (0, False, True, "part", None, True), (2, True, True, "acc", 0, True)]
BWD_PLAIN = [(0, False, False, "direct", None, False), (1, False, False, "acc", None, False),
             (2, False, False, "part", None, True), (3, False, False, "direct", 0, True),
             (1, False, False, "part", None, True), (3, False, False, "acc", 1, True),
             (0, False, False, "acc", 0, True), (2, False, False, "direct", None, True)]
BWD_GATHER = [(0, False, False, "direct", None, False), (0, False, False, "acc", None, False),
              (0, False, False, "part", None, False), (0, False, False, "direct", 0, True),
              (0, False, False, "acc", 1, True), (0, False, False, "part", 0, False),
              (0, False, False, "direct", None, True), (0, False, False, "acc", 0, False)]
# forward variants of add mode next to the full one: (b, bscale, s_out)
FWD_ADD = [(True, False, True), (False, False, True), (True, True, False), (False, True, False)]


def _short_shapes(mode, dtype, C):
    tpr = variant(C, dtype)[0]
    edge = 256 // tpr + 1
    if mode == MERGE:    # rows = B (H/2) (W/2): 1, 3, edge, 257 and the 2 x 6 x 10 grid (30 rows)
        return [(1, 2, 2), (1, 2, 6), (1, 2, 2 * edge), (1, 2, 514), (2, 6, 10)]
    if mode == D2S2:     # rows = 4 B H W: the multiples of 4 next to 1, 3, edge, 257 and the 2 x 3 x 5 grid
        e4 = -(-edge // 4)
        return [(1, 1, 1), (1, 1, 3), (1, 1, e4), (1, 5, 13), (2, 3, 5)]
    return [(1,), (3,), (edge,), (257,)]


@pytest.mark.parametrize("mode,dtype,C", SHORT, ids=[_id(*c) for c in SHORT])
def test_short_rows(mode, dtype, C):
    opts = {ADD: BWD_ADD, PLAIN: BWD_PLAIN}.get(mode, BWD_GATHER)
    wi = _widths(mode, dtype).index(C)
    for i, shape in enumerate(_short_shapes(mode, dtype, C)):
        case = Case(mode, dtype, C, shape, seed=7 * wi + i + 1, nsamples=3, scales=[0.0, 1.25, 1.0])
        xs, mean, rstd = case.check_fwd()
        if mode == ADD:
            ub, usc, us = FWD_ADD[(i + wi) % 4]
            case.check_fwd(ub, usc, us, s_from=xs if ub else case.x)  # s_out = NULL: the s of the same operands
        for j in range(2):
            nres, db, sc, out, tail, api3 = opts[(2 * i + j + wi) % 8]
            case.check_bwd(xs, mean, rstd, nres, db, sc, out, tail, api3, kind="one_row" if case.rows == 1 else "short")


def _long_rows(C, dtype):
    g = 256 // variant(C, dtype)[0]
    cap = 512 if C >= 384 else 1024
    return 3 * 4096 * g + 37, 3 * cap * g + 37


@pytest.mark.parametrize("mode,dtype,C", LONG, ids=["long-" + _id(*c) for c in LONG])
def test_long_rows(mode, dtype, C):
    """Every lane group walks >= 3 rows with a ragged last pass, forward (grid cap 4096) and
    backward (msu_ln_part_blocks cap): add mode with bscale {0, 1.25, 1} over 3 samples, plain
    mode with dres (+ dres2 + dres3 at the forward's row count)."""
    rf, rb = _long_rows(C, dtype)
    for rows, full in ((rf, True), (rb, False)):
        case = Case(mode, dtype, C, (rows,), seed=3 + int(full), nsamples=3, scales=[0.0, 1.25, 1.0])
        g = 256 // variant(C, dtype)[0]
        assert rows >= 3 * case.nparts * g and rows % (case.nparts * g), (rows, case.nparts)
        assert not full or (rows >= 3 * 4096 * g and rows % (4096 * g)), rows
        xs, mean, rstd = case.check_fwd()
        if mode == ADD:
            case.check_bwd(xs, mean, rstd, nres=3 if full else 1, use_db=True, use_scale=True,
                           out="direct" if full else "acc", api3=full, kind="long")
        else:
            case.check_bwd(xs, mean, rstd, nres=3 if full else 1, out="direct" if full else "part", api3=full,
                           kind="long")
        del case, xs, mean, rstd
    torch.cuda.empty_cache()


# ----------------------------------------------------------------------------- head
def _head_case(dtype, C, rows, seed, kind):
    lib = _L()
    tag = f"head/{DTNAME[dtype]}/C{C}/{rows}"
    z = _mix(rows, C, dtype, seed, 0, seed)
    gamma, beta = _affine(C, seed)
    g = torch.Generator(device=DEV).manual_seed(2000 + seed)
    w = (0.3 * torch.randn(C, generator=g, device=DEV)).contiguous()
    dl = _mix(rows, 1, F32, seed, 2, seed, big=100.0).reshape(-1).contiguous()
    logit, mean, rstd = Buf(rows, F32), Buf(rows, F32), Buf(rows, F32)
    lib.call("msu_head_fwd", _code(dtype), _p(z), _p(gamma), _p(beta), _p(w), _p(logit.t), _p(mean.t), _p(rstd.t),
             rows, C, EPS, _stream())
    torch.cuda.synchronize()
    ref = ln_head_ref(z, gamma, beta, w, dl, EPS)
    g64, b64, w64 = gamma.double(), beta.double(), w.double()
    mu, rs = ref["mean"].unsqueeze(-1), ref["rstd"].unsqueeze(-1)
    xhat = (ref["xr"] - mu) * rs
    q = _ratio((logit.check("logit").double() - ref["logit"]).abs(),
               TAU * ((xhat * g64 * w64).abs() + (b64 * w64).abs()).sum(-1))
    print(f"{tag} logit: err/bound {q:.3f}")
    _note("logit", dtype, q)
    assert q <= 1.0, f"{tag} logit: err / bound = {q:.3f}"
    _stats_chk(tag, dtype, mean.check("mean"), rstd.check("rstd"), ref)
    n = lib.lib().msu_ln_part_blocks(rows, C)
    for acc in (0, 1):
        dz = Buf(rows * C, dtype)
        part = torch.full((n * 3 * C,), float("nan"), device=DEV, dtype=torch.float32)
        both = torch.full((3 * C + 64,), SENT, device=DEV, dtype=torch.float32)
        init = torch.zeros(3 * C, device=DEV, dtype=torch.float64)
        if acc:
            gi = torch.Generator(device=DEV).manual_seed(78)
            both[:3 * C] = 3.0 * torch.randn(3 * C, generator=gi, device=DEV)
            init = both[:3 * C].double().clone()
        lib.call("msu_head_bwd2", _code(dtype), _p(dl), _p(z), _p(gamma), _p(beta), _p(w), _p(mean.t), _p(rstd.t),
                 _p(dz.t), _p(part), n, _p(both[:C]), _p(both[C:2 * C]), _p(both[2 * C:3 * C]), rows, C, acc, _stream())
        torch.cuda.synchronize()
        t = tag + f"/bwd(acc={acc})"
        assert bool((both[3 * C:] == SENT).all()), f"{t}: parameter gradients wrote past their end"
        _elem("head_dz", t, dtype, dz.check("dz"), ref["dz"], ref["dz"].abs().amax(-1))
        dl64 = dl.double().unsqueeze(-1)
        # dgamma_c = w_c sum dl xhat_c, dbeta_c = w_c sum dl, dw_c = sum dl (xhat_c gamma_c + beta_c)
        a_x = dl64.abs() * rs * (ref["xr"].abs() + ref["xr"].abs().mean(-1, keepdim=True))
        terms = {"head_dgamma": (dl64 * xhat * w64, a_x * w64.abs()),
                 "head_dbeta": (dl64 * w64.expand_as(xhat), dl64.abs() * w64.abs().expand_as(xhat)),
                 "head_dw": (dl64 * (xhat * g64 + b64), a_x * g64.abs() + dl64.abs() * b64.abs())}
        for i, (name, key) in enumerate((("head_dgamma", "dgamma"), ("head_dbeta", "dbeta"), ("head_dw", "dw"))):
            tt, ta = terms[name]
            ini = init[i * C:(i + 1) * C]
            _col(name, t, dtype, both[i * C:(i + 1) * C], ref[key] + ini, ta.sum(0) + ini.abs(),
                 None if acc else tt, kind)


@pytest.mark.parametrize("dtype,C", HEAD, ids=[_head_id(*c) for c in HEAD])
def test_head_short_rows(dtype, C):
    for i, rows in enumerate((1, 3, 33, 65, 257)):  # 256 / TPR + 1 for TPR = 8 (generic) and 4 (16-bit)
        _head_case(dtype, C, rows, seed=11 * HEAD_WIDTHS.index(C) + i + 1, kind="one_row" if rows == 1 else "short")


@pytest.mark.parametrize("dtype,C", HEAD_LONG, ids=["long-" + _head_id(*c) for c in HEAD_LONG])
def test_head_long_rows(dtype, C):
    """The prefetched 16-bit head backward: 1024 blocks x 64 row groups walk >= 3 rows each."""
    rows = 3 * 1024 * 64 + 37
    assert _L().lib().msu_ln_part_blocks(rows, C) == 1024
    _head_case(dtype, C, rows, seed=5, kind="long")
    torch.cuda.empty_cache()


def test_refused_merge_width_raises():
    """Cin = 6 in f32 passes C % 4 but a 16-byte chunk would straddle two gathered quadrants:
    the guard in csrc/layernorm.hip refuses it before any launch and the op raises."""
    from semantic_segmentation_of_stylegan2_artifacts_amd import ops
    x = torch.randn(1, 4, 4, 6, device=DEV)
    with pytest.raises(_L().HipLibraryError):
        ops.merge_layer_norm(x, torch.ones(24, device=DEV), torch.zeros(24, device=DEV))
    with pytest.raises(_L().HipLibraryError):
        ops.merge_layer_norm(torch.randn(1, 5, 4, 16, device=DEV), torch.ones(64, device=DEV),
                             torch.zeros(64, device=DEV))
