"""Every refine-conv kernel of csrc/conv3x3.h against exact and fp64 references, judged per element.

The C ABI is driven directly (``_lib.call`` with ``ops._conv_weight`` and ``ops._p / _dt / _s``).
The references are tests/_parity_refs.py: ``conv3x3_ref64`` (nine shifted float64 matmuls, no
library convolution), the same on absolute values (the condition term), GELU / GELU' from
``torch.erf`` and ``conv3x3_wgrad_ref64``; they run on the device and are fed exactly the stored
operands.

Kernel matrix (``kernel_for`` restates conv_nt's dispatch, ``_assert_coverage`` fails at import if
a row has no case; every case also asserts ``msu_conv3x3_route`` and reads back the
``msu_conv_mode`` bits it set, restored in a ``finally``):

    v3       bf16 f16  (96, 96), (128, 128)        fwd0 fwd2 dual0 dual2 dg1 dg3, tile queue and static
    generic  bf16 f16  (96, 96)                    fwd1 fwd3 (GELU on load; the v3 kernel has none)
                       (80, 96), (72, 96)          fwd0..3 dual0 dual2  (X rows narrower than the padded weights)
                       (96, 80)                    dg1 dg3  (GEMM in 80 / out 96)
                       (16, 16) (32, 32) (64, 64) (40, 16) (8, 64), (128, 128) under mode bit 1
             f32       (16, 16) (96, 96) (128, 128) (40, 16)
                                                   fwd0..3 dual0 dual2 dg1 dg3
             (the first three rows were the persistent register-staged v2 kernel's until it was
             retired; their figures on the generic kernel are listed apart below)
    wgrad v2       bf16 f16  96, 128               in_mode 0..3, overwrite and accumulate, nchunk = the
                                                   op's _CONV_WGRAD_BLOCKS and a small one (2, or 64 at
                                                   the large shape: several tiles per workgroup)
    wgrad generic  all three (32, 32) (40, 16) (64, 64), (128, 128) under mode bit 1, f32 (96, 96)
                                                   in_mode 0..3 (overwrite at _CONV_WGRAD_BLOCKS,
                                                   accumulate at nchunk 3)

(fwdM: msu_conv3x3_fwd2 with in_mode M, dualM: the same with Y2, dgM: msu_conv3x3_dgrad with
out_mode M.)  Widths an entry point does not serve are asserted to return -2: the dgrad of
(40, 16) and (8, 64) (its GEMM output width Cin is no multiple of 16) and the forward of
(96, 80) (no kernel with five 16-wide output tiles).

Shapes: (1, 8, 8), (1, 16, 32), (1, 20, 36), (2, 40, 56) and -- on the persistent routes (v3,
wgrad v2) -- (1, 260, 264): 297 tiles of 8 x 32, more than the 256 workgroups.  The generic
kernels (one workgroup per tile) run (1, 36, 68) instead: ragged in both directions for the f32
kernel's 4-row and the 16-bit kernel's 16-row tiles.  (96, 96) and (128, 128) keep the large
shape for their v3 forms; their GELU-on-load forms (generic) leave it out.  All are divisible
by 4: the d2s forms view the same stored tensor as [B, H/4, W/4, 16 C].

Every output (z, GELU(z), dx, dW, db) and the weight-gradient workspace sit between two NaN
bands of 4096 elements; after each launch the bands must still be NaN and the output free of NaN.

Two kinds of case, both in every test:

(a) exact.  Activations, dY and bias integers in [-2, 2], weights in {-1, 0, 1}: exact in bf16,
    f16 and f32, every partial sum an integer far below 2^24.  z (in_mode 0, 2) must EQUAL
    ``ref64.to(dtype)`` bit for bit (the kernels round to nearest even); dW and db must EQUAL the
    float64 reference, and under accumulate an integer initial gradient plus it.  GELU(z) and dx
    of these cases are judged by rule (b).
(b) rounding.  randn operands (w = randn / sqrt(9 Cin)), each rounded once to the storage type,
    the reference fed the same values.  16-bit GELU on load rounds gelu(x) to 16 bits before the
    MFMA, so those forms draw x from VSET: the multiples of 1/8 in [-4, 4] whose float64 GELU lies
    at least 1e-5 (test_gelu's f32 tolerance, ~30 x erf_fast's error at |x| <= 4) from the nearest
    rounding boundary of the storage type, plus 0 -- 53 values for bf16 (20 negative), 44 for f16
    (11 negative), asserted at import.  The reference operand is then round16(gelu64(x)), the
    kernel's own.  f32 takes randn.

Tolerance rule (u_T = 2^-9 bf16, 2^-12 f16, 0 f32; tau = 1e-4; f16 adds the 2^-25 floor):

* z:   |out - ref| <= 2 u_T |ref| + tau A,  A = sum |act| |w| + |b| of that element.
* Y2:  |out - gelu64(z)| <= 2 u_T |ref| + tau (1 + A).  Both kernels apply GELU to the STORED
       (rounded) z (conv3x3_kernel: gelu_f(to_f32(from_f32(v))); v3: gelu8 of the packed
       store), so z here is the kernel's own z, as the LayerNorm module refers y to its own s.
* dx:  |out - conv64 gelu'64(S)| <= 2 u_T |ref| + tau (1 + |gelu'64(S)|) sum |dy| |w|;
       |gelu'(S)| >= 0.1 on at least 80 % of the elements is asserted on the reference
       (S = randn + 0.5: 90 %; a standard normal gives 82 %, which a 1024-element case can miss).
* dW, db (rounding): |out - ref| <= K 2^-24 sum_pixels |term| (+ |initial value| under
       accumulate).  K = 8 x the worst such ratio of an f32 evaluation of the reference (the same
       nine matmuls, float64 terms cast to f32, on the device) over the module's cases: 7.97 for
       dW (at 2 x 40 x 56; 6.3 at 64 pixels, 3.2 at 68640) and 0.91 for db, so K = 63.8.

Sensitivity (references only, no kernel): a reference with one 8-channel chunk of one tap zeroed
violates the z bound and the dx bound on at least 1 % of the elements, one case per route
(measured: z 89 .. 97 %, dx 85 .. 89 %).

Measured on an MI355X (profiles/r14a_conv_matrix_ratios.txt; the whole module: 221 tests in
8.3 s, the slowest 1.16 s -- the first launch of the process -- and 0.43 s for a weight-gradient
case of the large shape), worst err / bound over the module, bf16 / f16 / f32:

    z    0.951 / 0.764 / 0.006      Y2   0.918 / 0.652 / 0.0003     dx   0.871 / 0.500 / 0.002
    dW   0.044 / 0.046 / 0.100      db   0.006 / 0.010 / 0.029      (exact cases: all equal)

Since the v2 kernel was retired (profiles/r15a_tests.txt; 221 tests in 7.9 s, the slowest 1.17 s)
the module's worst figures above are unchanged to the digit.  The rows that moved from v2 to the
generic kernel -- 16-bit (96, 96) fwd1 fwd3, (80, 96), (72, 96), the dgrad of (96, 80) -- give,
bf16 / f16:

    z    0.907 / 0.534              Y2   0.877 / 0.450              dx   0.791 / 0.357

inside the unchanged rule and below the other generic 16-bit rows (z 0.951 / 0.764, Y2 0.918 /
0.652, dx 0.871 / 0.500).

The 16-bit 0.5 .. 0.95 are the one storage rounding 2 u_T allows; without it (f32) the kernels sit
two to three orders of magnitude inside tau A.  In units of 2^-24 sum |term| the kernels' dW is
at most 2.9 (16-bit) and 6.4 (f32): no more than the f32 matmul of the reference.

Measured on the parent of the change that retired the v2 kernel (three kernels then; the rows
above that were v2's ran it): two scratch builds (not kept) with a wrong halo value at one image
corner in conv3x3_kernel, the v2 and the v3 kernel: (1) one 8-channel chunk of one tap taken from
the neighbouring pixel, (2) one element of pixel (0, 0) zeroed.  Under both, all 185 cases of this module that run a changed
kernel fail (the 36 others run none: the wgrad v2 cases, Cin = 8, the sensitivity cases).  The
tests that existed before (test_gpu_conv_c128.py, test_gpu_ops.py -k refine_conv, 97 cases) notice
(1) in 74 cases -- its error, 0.17 .. 0.29, is above their 0.07 -- and (2) in 46, five of them bf16.

Found by this module: nothing; every kernel of the matrix meets the rule above.  The widths the
entry points do not serve return -2 and leave the output untouched, which the cases assert.
"""
import math

import pytest
import torch

from _parity_refs import (conv3x3_abs64, conv3x3_dgrad_weight, conv3x3_ref64, conv3x3_wgrad_abs64,
                          conv3x3_wgrad_ref64, d2s4_rearrange, gelu64, gelu_grad64)

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 4096  # elements of each NaN band (a multiple of 8: the outputs stay 16-B aligned)
TAU = 1e-4
K_SUM = 63.8  # 8 x 7.97, the worst f32-matmul ratio of the reference over the module's cases (module docstring)
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
DTNAME = {F32: "f32", BF16: "bf16", F16: "f16"}
U_T = {F32: 0.0, BF16: 2.0 ** -9, F16: 2.0 ** -12}
FLOOR_T = {F32: 0.0, BF16: 0.0, F16: 2.0 ** -25}
SHAPES = [(1, 8, 8), (1, 16, 32), (1, 20, 36), (2, 40, 56), (1, 260, 264)]
GENERIC_SHAPES = SHAPES[:4] + [(1, 36, 68)]
FWD_FORMS = ("fwd0", "fwd1", "fwd2", "fwd3", "dual0", "dual2")
DG_FORMS = ("dg1", "dg3")


# ----------------------------------------------------------------------------- GELU value set
def _round_margin(g, dtype):
    """Distance of the float64 values g to the nearest rounding boundary of dtype."""
    r = g.to(dtype)
    bits = r.view(torch.int16)
    up, dn = (bits + 1).view(dtype).double(), (bits - 1).view(dtype).double()
    r = r.double()
    return torch.minimum((g - (r + up) / 2).abs(), (g - (r + dn) / 2).abs())


def _value_set(dtype):
    x = torch.arange(-32, 33, dtype=torch.float64) / 8
    v = x[(_round_margin(gelu64(x), dtype) >= 1e-5) | (x == 0)]
    nz = v[v != 0]
    assert bool((_round_margin(gelu64(nz), dtype) >= 1e-5).all())
    assert len(v) >= 40 and int((v < 0).sum()) >= 10, (dtype, len(v))
    assert bool((v.to(dtype).double() == v).all())
    return v


VSET = {BF16: _value_set(BF16), F16: _value_set(F16)}
assert (len(VSET[BF16]), int((VSET[BF16] < 0).sum())) == (53, 20)
assert (len(VSET[F16]), int((VSET[F16] < 0).sum())) == (44, 11)


# ----------------------------------------------------------------------------- kernel matrix
def kernel_for(dtype, cin, cout, gelu, wide):
    """conv_nt's pick for GEMM widths cin -> cout (None: no kernel, the entry point returns -2)."""
    if dtype != F32:
        if not gelu and cin == cout and (cin == 96 or (cin == 128 and not wide)):
            return "v3"
    return "generic" if cout // 16 in (1, 2, 4, 6, 8) else None


def conv_forms(dtype, Cin, Cout, wide):
    """[(form, kernel or None)] of a conv Cin -> Cout: what each entry point does with it."""
    out = []
    for f in FWD_FORMS:
        ok = Cout % 16 == 0 and Cin % 8 == 0 and max(Cin, Cout) <= 128
        out.append((f, kernel_for(dtype, Cin, Cout, f in ("fwd1", "fwd3"), wide) if ok else None))
    for f in DG_FORMS:  # GEMM input Cout, GEMM output Cin
        ok = Cout % 16 == 0 and Cin % 16 == 0 and max(Cin, Cout) <= 128
        out.append((f, kernel_for(dtype, Cout, Cin, False, wide) if ok else None))
    return out


def wgrad_kernel(dtype, Cin, Cout, wide):
    if dtype != F32 and Cin == Cout and (Cin == 96 or (Cin == 128 and not wide)):
        return "wgrad_v2"
    return "wgrad_generic"


def expected_route(dtype, Cin, Cout):
    return 3 if dtype != F32 and Cin == Cout and Cin in (96, 128) else 0


# (dtype, Cin, Cout, wide = msu_conv_mode bit 1, shape)
CONV_CASES = []
WGRAD_CASES = []
for _dt in (BF16, F16):
    for _w in ((96, 96), (128, 128)):
        CONV_CASES += [(_dt, _w[0], _w[1], False, s) for s in SHAPES]
    for _w in ((80, 96), (72, 96), (96, 80), (16, 16), (32, 32), (64, 64), (40, 16), (8, 64)):
        CONV_CASES += [(_dt, _w[0], _w[1], False, s) for s in GENERIC_SHAPES]
    CONV_CASES += [(_dt, 128, 128, True, s) for s in GENERIC_SHAPES]
    for _c in (96, 128):
        WGRAD_CASES += [(_dt, _c, _c, False, s) for s in SHAPES]
for _w in ((16, 16), (96, 96), (128, 128), (40, 16)):
    CONV_CASES += [(F32, _w[0], _w[1], False, s) for s in GENERIC_SHAPES]
for _dt in (BF16, F16, F32):
    for _w in ((32, 32), (40, 16), (64, 64)):
        WGRAD_CASES += [(_dt, _w[0], _w[1], False, s) for s in GENERIC_SHAPES]
    WGRAD_CASES += [(_dt, 128, 128, True, s) for s in GENERIC_SHAPES]
WGRAD_CASES += [(F32, 96, 96, False, s) for s in GENERIC_SHAPES]


def _skipped(kernel, shape):
    """The generic kernel has one workgroup per tile and no loop over tiles: at (96, 96) and
    (128, 128) its GELU-on-load forms sit beside the v3 forms and leave the large shape out."""
    return kernel == "generic" and shape == SHAPES[4]


def _scheds(forms):
    return (("queue", 1), ("static", 0)) if any(k == "v3" for _, k in forms) else (("-", 1),)


def _cid(case):
    dt, Cin, Cout, wide, (B, H, W) = case
    return "%s-%dto%d%s-%dx%dx%d" % (DTNAME[dt], Cin, Cout, "-wide" if wide else "", B, H, W)


def _assert_coverage():
    got, large = set(), set()
    for dt, Cin, Cout, wide, shape in CONV_CASES:
        forms = conv_forms(dt, Cin, Cout, wide)
        for f, k in forms:
            for s, _ in _scheds(forms):
                if (k == "v3" or s != "static") and not _skipped(k, shape):
                    got.add((k or "rejected", dt, (Cin, Cout), wide, f, s if k == "v3" else "-"))
                    if shape == SHAPES[4]:
                        large.add(k)
    want = set()
    for dt in (BF16, F16):
        for C in (96, 128):
            for f in ("fwd0", "fwd2", "dual0", "dual2", "dg1", "dg3"):
                want |= {("v3", dt, (C, C), False, f, s) for s in ("queue", "static")}
        want |= {("generic", dt, (96, 96), False, f, "-") for f in ("fwd1", "fwd3")}
        want |= {("generic", dt, w, False, f, "-") for w in ((80, 96), (72, 96)) for f in FWD_FORMS}
        want |= {("generic", dt, (96, 80), False, f, "-") for f in DG_FORMS}
        want |= {("rejected", dt, (96, 80), False, f, "-") for f in FWD_FORMS}
    for dt, widths in ((BF16, ((16, 16), (32, 32), (64, 64), (40, 16), (8, 64), (128, 128))),
                       (F16, ((16, 16), (32, 32), (64, 64), (40, 16), (8, 64), (128, 128))),
                       (F32, ((16, 16), (96, 96), (128, 128), (40, 16)))):
        for w in widths:
            wide = dt != F32 and w == (128, 128)
            want |= {("generic", dt, w, wide, f, "-") for f in FWD_FORMS}
            want |= {("generic" if w[0] % 16 == 0 else "rejected", dt, w, wide, f, "-") for f in DG_FORMS}
    assert want <= got, sorted(map(str, want - got))
    # the large shape on the persistent kernel only (no rejected form either: the width with
    # one, (96, 80), runs the generic shapes)
    assert large == {"v3"}
    gotw = {(wgrad_kernel(dt, Cin, Cout, wide), dt, (Cin, Cout), wide) for dt, Cin, Cout, wide, _ in WGRAD_CASES}
    wantw = {("wgrad_v2", dt, (C, C), False) for dt in (BF16, F16) for C in (96, 128)}
    wantw |= {("wgrad_generic", dt, w, False) for dt in (BF16, F16, F32) for w in ((32, 32), (40, 16), (64, 64))}
    wantw |= {("wgrad_generic", dt, (128, 128), True) for dt in (BF16, F16, F32)} | {("wgrad_generic", F32, (96, 96), False)}
    assert gotw == wantw, sorted(map(str, gotw ^ wantw))
    for cases in (CONV_CASES, WGRAD_CASES):
        assert len({_cid(c) for c in cases}) == len(cases)
        assert all(H % 4 == 0 and W % 4 == 0 for _, _, _, _, (_, H, W) in cases)  # every shape serves d2s
    # the large shape only where a persistent kernel takes part; the generic rows run (1, 36, 68)
    for dt, Cin, Cout, wide, shape in CONV_CASES:
        kinds = {k for _, k in conv_forms(dt, Cin, Cout, wide)}
        assert (shape == SHAPES[4]) <= ("v3" in kinds)
    for dt, Cin, Cout, wide, shape in WGRAD_CASES:
        assert (shape == SHAPES[4]) <= (wgrad_kernel(dt, Cin, Cout, wide) == "wgrad_v2")


_assert_coverage()


# ----------------------------------------------------------------------------- plumbing
def _ops():
    from semantic_segmentation_of_stylegan2_artifacts_amd import ops
    return ops


def _L():
    from semantic_segmentation_of_stylegan2_artifacts_amd import _lib
    return _lib


def _set_mode(lib, mode):
    """Sets msu_conv_mode and reads it back: the bits a case relies on are the bits in force."""
    lib.msu_conv_mode(mode)
    assert lib.msu_conv_mode(mode) == mode


class Band:
    """n elements between two NaN bands of GUARD elements; the payload starts as NaN too (or
    as ``init``, for an accumulated gradient)."""

    def __init__(self, n, dtype, init=None):
        self.n = n
        self.buf = torch.full((n + 2 * GUARD,), float("nan"), device=DEV, dtype=dtype)
        self.t = self.buf[GUARD:GUARD + n]
        if init is not None:
            self.t.copy_(init.reshape(-1))

    def bands(self, what):
        assert bool(torch.isnan(self.buf[:GUARD]).all()), f"{what}: the band before it was written"
        assert bool(torch.isnan(self.buf[GUARD + self.n:]).all()), f"{what}: the band after it was written"

    def check(self, what):
        self.bands(what)
        assert not bool(torch.isnan(self.t).any()), f"{what}: elements left unwritten (or NaN)"
        return self.t


STATS = {}


def _note(name, dtype, ratio):
    key = (name, DTNAME.get(dtype, dtype))
    STATS[key] = max(STATS.get(key, 0.0), float(ratio))


def _ratio(err, bound):
    """max err / bound; a zero bound demands a zero error."""
    if bool(((bound == 0) & (err > 0)).any()):
        return float("inf")
    q = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.zeros_like(err))
    return float(q.max()) if q.numel() else 0.0


def _elem(name, tag, dtype, out, ref, abs_bound):
    """|out - ref| <= 2 u_T |ref| + abs_bound (+ the f16 floor), per element."""
    out = out.double().reshape(ref.shape)
    q = _ratio((out - ref).abs(), 2 * U_T[dtype] * ref.abs() + abs_bound + FLOOR_T[dtype])
    print(f"{tag} {name}: err/bound {q:.3f}")
    _note(name, dtype, q)
    assert q <= 1.0, f"{tag} {name}: err / bound = {q:.3f}"


def _sum(name, tag, dtype, out, ref, abs_sum):
    """|out - ref| <= K 2^-24 sum |term| per element of a pixel sum."""
    q = _ratio((out.double().reshape(ref.shape) - ref).abs(), K_SUM * 2.0 ** -24 * abs_sum)
    print(f"{tag} {name}: err/bound {q:.3f}")
    _note(name, dtype, q)
    assert q <= 1.0, f"{tag} {name}: err / bound = {q:.3f}"


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nconv matrix: worst err / bound per (output, dtype); sum32_*: the reference's nine matmuls in f32 / (2^-24 sum|term|)")
    for (name, dt), v in sorted(STATS.items()):
        print(f"  CONVMATRIX {name:12s} {dt:5s} {v:.4f}")


# ----------------------------------------------------------------------------- operands
class Operands:
    """Stored operands of one (dtype, Cin, Cout, shape, kind) and the conv's input image in
    float64 as each form's kernel sees it."""

    def __init__(self, dtype, Cin, Cout, shape, exact, dev=DEV):
        B, H, W = shape
        self.dtype, self.Cin, self.Cout, self.shape, self.exact = dtype, Cin, Cout, shape, exact
        g = torch.Generator(device=dev).manual_seed(((Cin * 131 + Cout) * 521 + H * 269 + W) * 4 + 2 * exact)

        def randn(*s):
            return torch.randn(*s, generator=g, device=dev)

        def ints(lo, hi, *s):
            return torch.randint(lo, hi + 1, s, generator=g, device=dev).float()

        if exact:
            self.x, self.xg = ints(-2, 2, B, H, W, Cin).to(dtype), None
            self.w, self.b = ints(-1, 1, Cout, Cin, 3, 3), ints(-2, 2, Cout)
            self.dz = ints(-2, 2, B, H, W, Cout).to(dtype)
        else:
            self.x = randn(B, H, W, Cin).to(dtype)
            if dtype == F32:
                self.xg = randn(B, H, W, Cin)
            else:  # GELU on load: x from the value set
                v = VSET[dtype].to(dev)
                self.xg = v[torch.randint(0, len(v), (B, H, W, Cin), generator=g, device=dev)].to(dtype)
            self.w = (randn(Cout, Cin, 3, 3) / math.sqrt(9 * Cin)).to(dtype).float()  # rounded once
            self.b = 0.1 * randn(Cout)
            self.dz = randn(B, H, W, Cout).to(dtype)
        # the pre-activation of the dgrad epilogue.  |gelu'| >= 0.1 holds on 82 % of a standard
        # normal, which 1024 elements miss by chance; on 90 % of randn + 0.5 (31 % still negative)
        self.s = (randn(B, H, W, Cin) + 0.5).to(dtype)

    def logical(self, t, d2s):
        """A stored [B, H, W, C] tensor as the image the kernel addresses (d2s: the same memory
        read as [B, H/4, W/4, 16 C] and mapped through the depth-to-space rearrange)."""
        B, H, W = self.shape
        C = t.shape[-1]
        return d2s4_rearrange(t.reshape(B, H // 4, W // 4, 16 * C), C) if d2s else t

    def image(self, gelu, d2s):
        a = (self.xg if gelu else self.x).double()
        if gelu:
            a = gelu64(a)
            if self.dtype != F32:
                a = a.to(self.dtype).double()  # the kernel's own 16-bit operand
        return self.logical(a, d2s)


def _code(dtype):
    return {F32: 0, BF16: 1, F16: 2}[dtype]


# ----------------------------------------------------------------------------- forward / dgrad
def _conv_kind(lib, dt, Cin, Cout, wide, shape, exact):
    ops = _ops()
    B, H, W = shape
    forms = conv_forms(dt, Cin, Cout, wide)
    o = Operands(dt, Cin, Cout, shape, exact)
    tag0 = f"{_cid((dt, Cin, Cout, wide, shape))}/{'exact' if exact else 'round'}"
    st = ops._s(o.x)
    wt = ops._conv_weight(o.w, dt, 0) if any(k for f, k in forms if f in FWD_FORMS) else None
    wf = ops._conv_weight(o.w, dt, 1) if any(k for f, k in forms if f in DG_FORMS) else None
    nin, nout = B * H * W * Cin, B * H * W * Cout
    zrefs, dref = {}, []

    def zref(gelu, d2s):
        if (gelu, d2s) not in zrefs:
            a = o.image(gelu, d2s)
            zrefs[(gelu, d2s)] = (conv3x3_ref64(a, o.w, o.b), conv3x3_abs64(a, o.w, o.b))
        return zrefs[(gelu, d2s)]

    for sname, bit in _scheds(forms):
        _set_mode(lib, bit | (2 if wide else 0))
        for form, kern in forms:
            tag = f"{tag0}/{form}/{kern}/{sname}"
            mode = int(form[-1])
            if kern is None:  # a width this entry point does not serve: -2, nothing launched
                wz = torch.zeros(9 * 128 * 128, device=DEV, dtype=dt)
                if form in FWD_FORMS:
                    y = Band(nout, dt)
                    rc = lib.msu_conv3x3_fwd2(ops._dt(o.x), mode, ops._p(o.x), ops._p(wz), ops._p(o.b), ops._p(y.t),
                                              None, B, H, W, Cin, Cout, st)
                else:
                    y = Band(nin, dt)
                    rc = lib.msu_conv3x3_dgrad(ops._dt(o.x), mode, ops._p(o.dz), ops._p(wz), ops._p(o.s), ops._p(y.t),
                                               B, H, W, Cin, Cout, st)
                torch.cuda.synchronize()
                assert rc == -2, f"{tag}: returned {rc}"
                assert bool(torch.isnan(y.buf).all()), f"{tag}: rejected, yet the output was written"
                continue
            if (sname == "static" and kern != "v3") or (exact and form in ("fwd1", "fwd3")) or _skipped(kern, shape):
                continue
            if form in FWD_FORMS:
                gelu, d2s, dual = bool(mode & 1), bool(mode & 2), form.startswith("dual")
                z, y2 = Band(nout, dt), (Band(nout, dt) if dual else None)
                _L().call("msu_conv3x3_fwd2", ops._dt(o.x), mode, ops._p(o.xg if gelu else o.x), ops._p(wt), ops._p(o.b),
                          ops._p(z.t), ops._p(y2.t) if dual else None, B, H, W, Cin, Cout, st)
                torch.cuda.synchronize()
                zk = z.check(tag + " z").view(B, H, W, Cout)
                ref, A = zref(gelu, d2s)
                if exact:
                    assert torch.equal(zk, ref.to(dt)), f"{tag} z: not equal to the exact result"
                    _note("z", dt, 0.0)
                else:
                    _elem("z", tag, dt, zk, ref, TAU * A)
                if dual:  # GELU of the kernel's own stored z
                    y2k = y2.check(tag + " Y2")
                    _elem("Y2", tag, dt, y2k, gelu64(zk), TAU * (1 + A))
            else:
                d2s = bool(mode & 2)
                if not dref:
                    wd = conv3x3_dgrad_weight(o.w)
                    dref += [conv3x3_ref64(o.dz, wd), conv3x3_abs64(o.dz, wd)]
                gp = gelu_grad64(o.logical(o.s, d2s))
                assert float((gp.abs() >= 0.1).double().mean()) >= 0.8
                dx = Band(nin, dt)
                _L().call("msu_conv3x3_dgrad", ops._dt(o.x), mode, ops._p(o.dz), ops._p(wf), ops._p(o.s), ops._p(dx.t),
                          B, H, W, Cin, Cout, st)
                torch.cuda.synchronize()
                dxk = o.logical(dx.check(tag + " dx").view(B, H, W, Cin), d2s)
                _elem("dx", tag, dt, dxk, dref[0] * gp, TAU * (1 + gp.abs()) * dref[1])


@pytest.mark.parametrize("case", CONV_CASES, ids=_cid)
def test_conv_matrix(case):
    dt, Cin, Cout, wide, shape = case
    lib = _L().lib()
    assert lib.msu_conv3x3_route(_code(dt), Cin, Cout) == expected_route(dt, Cin, Cout)
    # bit 0 of the route is the v3 kernel; at 128 it also needs msu_conv_mode bit 1 clear
    v3 = any(k == "v3" for _, k in conv_forms(dt, Cin, Cout, wide))
    assert v3 == bool(expected_route(dt, Cin, Cout) & 1 and not (wide and Cin == 128))
    prev = lib.msu_conv_mode(1)
    try:
        for exact in (True, False):
            _conv_kind(lib, dt, Cin, Cout, wide, shape, exact)
    finally:
        lib.msu_conv_mode(prev)


# ----------------------------------------------------------------------------- weight gradient
def _small_nchunk(shape):
    B, H, W = shape
    tiles = B * -(-W // 32) * -(-H // 4)
    return 2 if tiles <= 64 else 64


def _wgrad_kind(lib, dt, Cin, Cout, wide, shape, exact):
    ops = _ops()
    B, H, W = shape
    kern = wgrad_kernel(dt, Cin, Cout, wide)
    o = Operands(dt, Cin, Cout, shape, exact)
    big = ops._CONV_WGRAD_BLOCKS
    if kern == "wgrad_v2":
        launches = [(big, 0), (big, 1), (_small_nchunk(shape), 0), (_small_nchunk(shape), 1)]
    else:
        launches = [(big, 0), (3, 1)]
    g = torch.Generator(device=DEV).manual_seed(Cin + 7 * H + exact)
    for mode in ((0, 2) if exact else (0, 1, 2, 3)):
        a = o.image(bool(mode & 1), bool(mode & 2))
        dw64, db64 = conv3x3_wgrad_ref64(a, o.dz)
        aw, ab = conv3x3_wgrad_abs64(a, o.dz)
        if not exact:  # the figure K_SUM is derived from
            dw32, db32 = conv3x3_wgrad_ref64(a, o.dz, torch.float32)
            q32 = _ratio((dw32.double() - dw64).abs(), 2.0 ** -24 * aw)
            _note("sum32_dW", "any", q32)
            _note("sum32_dW %5d px" % (B * H * W), "any", q32)
            _note("sum32_db", "any", _ratio((db32.double() - db64).abs(), 2.0 ** -24 * ab))
        src = o.xg if mode & 1 else o.x
        for nchunk, acc in launches:
            tag = f"{_cid((dt, Cin, Cout, wide, shape))}/{'exact' if exact else 'round'}/{kern}/in{mode}/n{nchunk}/acc{acc}"
            if acc and exact:
                w0 = torch.randint(-8, 9, dw64.shape, generator=g, device=DEV).float()
                b0 = torch.randint(-8, 9, db64.shape, generator=g, device=DEV).float()
            elif acc:
                w0 = torch.randn(dw64.shape, generator=g, device=DEV)
                b0 = torch.randn(db64.shape, generator=g, device=DEV)
            else:
                w0 = b0 = None
            nws = lib.msu_conv3x3_wgrad_workspace(nchunk, Cin, Cout, 0, 0)
            ws, dw, db = Band(nws, F32), Band(dw64.numel(), F32, w0), Band(Cout, F32, b0)
            _L().call("msu_conv3x3_wgrad2", ops._dt(src), mode, ops._p(src), ops._p(o.dz), ops._p(dw.t), ops._p(db.t),
                      ops._p(ws.t), nchunk, B, H, W, Cin, Cout, acc, ops._s(src))
            torch.cuda.synchronize()
            ws.bands(tag + " workspace")
            dwk, dbk = dw.check(tag + " dW").view(dw64.shape), db.check(tag + " db")
            rw, rb = (dw64, db64) if not acc else (dw64 + w0.double(), db64 + b0.double())
            if exact:
                assert torch.equal(dwk.double(), rw), f"{tag} dW: not equal to the exact sum"
                assert torch.equal(dbk.double(), rb), f"{tag} db: not equal to the exact sum"
                _note("dW", dt, 0.0)
                _note("db", dt, 0.0)
            else:
                _sum("dW", tag, dt, dwk, rw, aw if not acc else aw + w0.double().abs())
                _sum("db", tag, dt, dbk, rb, ab if not acc else ab + b0.double().abs())


@pytest.mark.parametrize("case", WGRAD_CASES, ids=_cid)
def test_wgrad_matrix(case):
    dt, Cin, Cout, wide, shape = case
    lib = _L().lib()
    route = lib.msu_conv3x3_route(_code(dt), Cin, Cout)
    assert route == expected_route(dt, Cin, Cout)
    # bit 1 of the route is the persistent kernel; at 128 it also needs msu_conv_mode bit 1 clear
    assert (wgrad_kernel(dt, Cin, Cout, wide) == "wgrad_v2") == bool(route & 2 and not (wide and Cin == 128))
    prev = lib.msu_conv_mode(1)
    try:
        _set_mode(lib, 1 | (2 if wide else 0))
        for exact in (True, False):
            _wgrad_kind(lib, dt, Cin, Cout, wide, shape, exact)
    finally:
        lib.msu_conv_mode(prev)


# ----------------------------------------------------------------------------- sensitivity
# (route, dtype, Cin, Cout, GELU on load): one rounding case per route, references only
SENSITIVITY = [("v3_96", BF16, 96, 96, False), ("v3_128", F16, 128, 128, False), ("generic96_gelu", BF16, 96, 96, True),
               ("generic96_narrow", F16, 80, 96, False), ("generic16", BF16, 64, 64, True), ("generic32", F32, 96, 96, False)]


def sensitivity_fractions(dtype, Cin, Cout, gelu, dev):
    """Fractions of z and dx elements on which a reference with one 8-channel chunk of one tap
    zeroed breaks the module's bounds."""
    o = Operands(dtype, Cin, Cout, (1, 20, 36), False, dev)
    tap, ch = (Cin + Cout) % 9, (Cin // 8) // 2
    a = o.image(gelu, False)
    ref, A = conv3x3_ref64(a, o.w, o.b), conv3x3_abs64(a, o.w, o.b)
    w_bad = o.w.clone()
    w_bad[:, 8 * ch:8 * ch + 8, tap // 3, tap % 3] = 0
    bad = conv3x3_ref64(a, w_bad, o.b)
    fz = ((bad - ref).abs() > 2 * U_T[dtype] * ref.abs() + TAU * A + FLOOR_T[dtype]).double().mean()
    wd = conv3x3_dgrad_weight(o.w)
    gp = gelu_grad64(o.s)
    ref, Ad = conv3x3_ref64(o.dz, wd) * gp, conv3x3_abs64(o.dz, wd)
    wd_bad = wd.clone()
    chd = (Cout // 8) // 2
    wd_bad[:, 8 * chd:8 * chd + 8, tap // 3, tap % 3] = 0
    bad = conv3x3_ref64(o.dz, wd_bad) * gp
    fx = ((bad - ref).abs() > 2 * U_T[dtype] * ref.abs() + TAU * (1 + gp.abs()) * Ad + FLOOR_T[dtype]).double().mean()
    return float(fz), float(fx)


@pytest.mark.parametrize("route,dtype,Cin,Cout,gelu", SENSITIVITY, ids=[s[0] for s in SENSITIVITY])
def test_bounds_catch_a_dropped_chunk(route, dtype, Cin, Cout, gelu):
    fz, fx = sensitivity_fractions(dtype, Cin, Cout, gelu, DEV)
    print(f"{route}: z bound broken on {100 * fz:.1f} %, dx bound on {100 * fx:.1f} % of the elements")
    assert fz >= 0.01 and fx >= 0.01
