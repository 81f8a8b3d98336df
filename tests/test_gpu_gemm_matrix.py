"""Every forward GEMM kernel form -- the token GEMM (csrc/gemm_tok.h), the tiled NT GEMM
(csrc/gemm_nt.hip, gemm_pp.h) and the one-pass Linear backward (csrc/gemm_linbwd.hip) -- against
exact and fp64 references, judged per element.

The C ABI is driven directly (``_lib.call`` / the raw entry points with ``ops._p / _dt / _s``).  The
references are tests/_parity_refs.py: ``gemm_ref64`` (one float64 matmul), ``gemm_abs64`` (the
same on absolute values: the condition term) and ``gelu64`` / ``gelu_grad64``; they run on the
device and are fed exactly the stored operands.

Kernel matrix (``_assert_coverage`` fails at import if a row has no case; every case asserts,
through ``msu_tok_gemm_plan_epi`` / ``msu_nt_gemm_plan2``, the kernel form it is meant to hit):

    token GEMM    bf16 f16  one case per reachable (kc, nc, nst, nw), enumerated at import by
                            sweeping the plan call over N, K <= 3072 at the smallest N x K of the
                            form: 37 forms under the plain epilogue, 23 with split A, 18 under the
                            GELU epilogues (asserted; the 48-deep stage serves the plain epilogue
                            only).  Plain, plain + bias, split A (K1 = K / 2 and K1 = 8), GELU dual
                            (separate Y2 and Y2 aliasing Y: bit-identical), GELU'.  M in {1, 33,
                            1000}; the first form of every (kc, nst, nw) also at M = 32 (2 S + 5) + 7
                            (S waves over the row groups, from the plan: six waves walk three
                            tiles, the last of them ragged).
    NT GEMM       bf16 f16  nk = K / 64 in {1, 2, 3, 5}
        128 x 128 two-stage    (mode bits 1-2 = 3)  [N, K] and KN, three epilogues, split A
        256 x 128 three-stage  (bits 1-2 = 2)       [N, K] and KN, three epilogues, split A
                               shapes (1, 32), (100, 160) and one of 2.25 x the resident
                               workgroups' tiles at N = 160 with a ragged last M tile: every odd
                               workgroup walks ragged-N tiles only, three of them in a row
        128 x 192              (bits 1-2 = 1)       three epilogues; (1, 192), (100, 384), the large one
        256 x 192 two-stage    (cost model)         three epilogues; the large shape: N = 192 and
                               2 CUs + 3 tiles of 256 rows, the last ragged
        ping-pong kernel       (bit 0) plain and GELU dual at nk in {3, 5}: exactly 3/4 of a round of
                               tiles (N = 192) and two rounds (N = 384)
      (the 192-wide forms need N % 192 == 0 and the cost model picks 256 x 192 only at large M,
      so those forms have no (1, 32) / ragged-N shape: nt_cfg sends such shapes elsewhere.)
    msu_linear_bwd  bf16 f16  (K, N) = (96, 288), (96, 96), (96, 384), (384, 96), (384, 96) with H,
                            (384, 96) with X = null and H; M in {1, 31, 65, 1000} and
                            ts (2 CUs + 3) + 5 rows (ts = 64 / 32 token steps: three steps for the
                            first workgroups); overwrite, accumulate, db = null.
    refusals      N % 32, K % 64 (NT), split A with K1 % 64 (NT), K1 % 8 and the 48-deep stage
                  (token), GELU' with a bias, a GELU epilogue at K % 48 (token), H at (96, 96):
                  the stated code, the banded output untouched.
    predicate     for every N, K <= 3072 (multiples of 32 / 16) and every epilogue (and split A)
                  "supported" and "the launch at M = 32 returns 0" agree.

Harness: every operand and output (A, A2, W, bias, H, Y, Y2, dX, dW, db, workspace) sits between
two NaN bands of 4096 elements; after each launch the bands are still NaN and the outputs hold
no NaN.  Every case launches twice into separate banded outputs, which must be bit-identical.
``msu_nt_gemm_mode`` bits are restored in a ``finally``.

Two kinds of case, both in every test:

(a) exact.  A, dY and bias integers in [-2, 2], weights in {-1, 0, 1}: every partial sum is an
    integer below 2^24, so Y / H / dX (plain) must EQUAL ``ref64.to(dtype)`` bit for bit (the
    kernels round to nearest even); dW / db must EQUAL float64, under accumulate an integer
    initial value plus it.  GELU and GELU' outputs of these cases fall under (b).
(b) rounding.  randn operands, w = randn / sqrt(K), bias randn, each rounded once to the storage
    type.  u_T = 2^-9 bf16, 2^-12 f16 (f16 adds a 2^-25 floor); A = sum |a| |w| + |b|:
    * Y / H:  |out - ref| <= 2 u_T |ref| + kappa 2^-24 A.
    * Y2:     |out - gelu64(H)| <= 2 u_T |ref| + 1e-5 (1 + |H|), H the kernel's own stored H
              (1e-5: test_gelu's f32 bar).
    * GELU':  |out - ref| <= 2 u_T |ref| + kappa 2^-24 (1 + |gelu'64(H)|) sum |dy| |w|, H = randn
              + 0.5, |gelu'| >= 0.1 on >= 80 % of the reference asserted (but for one-row cases of
              fewer than 256 elements and M = 1 of msu_linear_bwd: so few draws miss 80 % by chance).
    * dW/db:  |out - ref| <= kappa_s 2^-24 sum |term| (+ |initial| under accumulate).
    The X = null form of msu_linear_bwd (X = round16(gelu_fast(H))) draws H from the conv module's
    VSET, so the reference operand round16(gelu64(H)) is the kernel's own (no 80 % assertion there:
    VSET is uniform on [-4, 4]).
    kappa and kappa_s are 8 x the worst ratio err / (2^-24 A) that an f32 evaluation of the
    reference itself (the same matmul, fp64 operands cast to f32, on the device) reaches over the
    module's cases; ``KAPPA 2^-24 <= 1e-4`` (the project's tau) is asserted.  Figures: see below.

Sensitivity (references only, one per family): a reference with one 8-wide k chunk of W zeroed
violates the Y bound on >= 50 % of the elements.

Measured on an MI355X (profiles/r18a_gemm_matrix_ratios.txt, per family, form and dtype, taken
when the NT kernel still had an A3W2 ring and a tile queue, both removed since; the whole
module: 183 tests in 6.4 s, the slowest 0.48 s -- the first launch of the process -- then
0.20 s for the predicate sweep's 3344 launches and 0.07 s for a large NT case).

kappa: the reference's f32 matmul reaches 7.61 x 2^-24 A at tok/plain-kc96-nc64-nst2-nw8, f16,
131239 x 64 x 96 (7.27 for dX of msu_linear_bwd at 16453 x 384 x 96, 7.07 / 7.02 on the NT shapes
65536 x 384 x 320 / 131621 x 192 x 320), so kappa = 60.9 and kappa 2^-24 = 3.6e-6, 28 x below tau.
kappa_s: dW 4.32 (linbwd 96 x 288, f16, M = 65), db 0.31, so kappa_s = 34.5.

Worst err / bound over the module, bf16 / f16 (exact cases: all equal):

    token GEMM   Y 0.995 / 0.987   split A 0.994 / 0.984   H 0.994 / 0.984   Y2 0.964 / 0.919   GELU' 0.991 / 0.968
    NT GEMM      Y 0.995 / 0.986   H 0.994 / 0.986   Y2 0.964 / 0.919   GELU' 0.993 / 0.976   (ping-pong: Y, H 0.994 / 0.981)
    linear_bwd   dX 0.994 / 0.981   dX GELU' 0.991 / 0.961   dW 0.064 / 0.050   db 0.029 / 0.029

The 0.96 .. 0.995 are the one storage rounding: 2 u_T is exactly the worst relative error of a
round to nearest (2^-8 bf16, 2^-11 f16), which some of 10^7 elements nearly meet; the kappa term
is what is left for the accumulation (with tau in its place the same cases read 0.96 / 0.77: the
rule has no slack to hide a wrong element in).  dW / db sit at 2.2 x 2^-24 sum |term| at most: below the
f32 matmul of the reference.  Sensitivity at the final kappa: tok 92.8 %, nt 99.7 %, linbwd dX
97.3 % of the elements break the bound (at tau: 87.1, 99.0, 96.5 %).

Two scratch builds (not kept):
(1) ``tokgemm_kernel`` drops bias_lo (the bias k-block holds round16(b) alone).  All 110 token-GEMM
    cases of this module fail; the agreement sweep, which runs the kernel but judges return codes
    only, passes.  Of the tests that existed before (test_gpu_tok_gemm.py, test_gpu_linbwd.py: 146
    ran, 4 skipped) none noticed.
(2) ``gemm_nt_kernel`` counts a ragged wave's stores as issued (``epi_full = true``), the miscount
    that once let waves read stale LDS.  Run once: no failure -- all 56 NT cases of this module and
    all 604 of test_gpu_nt_gemm.py passed.  It is a race: the over-counted wait lets a ragged wave
    pass the barrier with its share of a K step's DMA in flight, and that DMA was issued a whole
    step earlier; on an otherwise idle device it has landed by then.  The cases that would show it
    (256 x 128 three-stage at nk = 3, 5 on the large shapes: odd workgroups walk three ragged-N
    tiles in a row, every launch repeated and compared bit for bit) are in place.

Found by this module: nothing in the kernels; every form of the matrix meets the rule above.  From
the source (and fixed with this module): ``tok_plan`` planned the GELU epilogues and split A at the
48-deep stage, which ``gemm_tok_k48.hip`` instantiates for the plain epilogue only, so
``msu_tok_gemm_supported_epi`` returned 1 where ``msu_tok_gemm`` returned -3 (K = 48, 144, 240, ...).
``test_tok_predicate_agrees_with_launch`` now holds predicate and launch together over every
N, K <= 3072.
"""
import ctypes
import math

import pytest
import torch

from _parity_refs import gelu64, gelu_grad64, gemm_abs64, gemm_ref64
from test_gpu_conv_matrix import VSET

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 4096  # elements of each NaN band (a multiple of 8: the payload stays 16-B aligned)
KAPPA = 60.9    # 8 x 7.61, the worst f32-matmul ratio of the reference over the module's Y / H / dX cases (docstring)
KAPPA_S = 34.5  # 8 x 4.32, the same over its dW / db cases
assert KAPPA * 2.0 ** -24 <= 1e-4 and KAPPA_S * 2.0 ** -24 <= 1e-4  # never looser than the project's tau
BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
DTYPES = (BF16, F16)
DTNAME = {BF16: "bf16", F16: "f16", F32: "f32"}
U_T = {BF16: 2.0 ** -9, F16: 2.0 ** -12}
FLOOR_T = {BF16: 0.0, F16: 2.0 ** -25}
PLAIN, DUAL, GRAD = 0, 1, 2
EPS24 = 2.0 ** -24


# ----------------------------------------------------------------------------- plumbing
def _ops():
    from semantic_segmentation_of_stylegan2_artifacts_amd import ops
    return ops


def _L():
    from semantic_segmentation_of_stylegan2_artifacts_amd import _lib
    return _lib


def tok_plan(M, N, K, epi=PLAIN, concat=0):
    """(kc, nc, nst, nw, nchunk, grid) msu_tok_gemm launches, or None (host only)."""
    out = (ctypes.c_long * 6)()
    if _L().lib().msu_tok_gemm_plan_epi(M, N, K, epi, concat, out) != 0:
        assert out[1] == 0
        return None
    return (out[0], out[1], out[2] // 100, out[2] % 100, out[3], out[4])


def nt_plan(M, N, K, epi=PLAIN, wkn=0):
    """dict(rows, bn, ring, pp, tiles, grid, queue, cus) of msu_nt_gemm / _kn under the mode in force."""
    out = (ctypes.c_long * 8)()
    assert _L().lib().msu_nt_gemm_plan2(M, N, K, epi, wkn, out) == 0, (M, N, K)
    return dict(zip(("rows", "bn", "ring", "pp", "tiles", "grid", "queue", "cus"), out))


def _set_mode(lib, mode):
    """Sets msu_nt_gemm_mode and reads it back: the bits a case relies on are the bits in force."""
    lib.msu_nt_gemm_mode(mode)
    assert lib.msu_nt_gemm_mode(mode) == mode


class Band:
    """n elements between two NaN bands of GUARD elements; the payload starts as NaN too (or as
    ``init``: an operand, or an accumulated gradient)."""

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

    def untouched(self, what):
        assert bool(torch.isnan(self.buf).all()), f"{what}: refused, yet the output was written"


def banded(t):
    """The operand t between two NaN bands (a kernel that reads past it computes NaN)."""
    return Band(t.numel(), t.dtype, t).t.view(t.shape)


def _bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def _same(tag, a, b):
    assert torch.equal(_bits(a), _bits(b)), f"{tag}: two launches differ"


STATS = {}
FORM = [""]  # the kernel form the running case hits: figures are kept per output and per (output, form)


def _note(name, dtype, ratio, tag=""):
    for key in ((name, DTNAME.get(dtype, dtype)), (f"{name} @ {FORM[0]}", DTNAME.get(dtype, dtype))):
        if key not in STATS or float(ratio) > STATS[key][0]:
            STATS[key] = (float(ratio), tag)


def _ratio(err, bound):
    """max err / bound; a zero bound demands a zero error."""
    if bool(((bound == 0) & (err > 0)).any()):
        return float("inf")
    q = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.zeros_like(err))
    return float(q.max()) if q.numel() else 0.0


def _elem(name, tag, dtype, out, ref, abs_bound):
    """|out - ref| <= 2 u_T |ref| + abs_bound (+ the f16 floor), per element."""
    err = (out.double().reshape(ref.shape) - ref).abs()
    q = _ratio(err, 2 * U_T[dtype] * ref.abs() + abs_bound + FLOOR_T[dtype])
    print(f"{tag} {name}: err/bound {q:.3f}")
    _note(name, dtype, q, tag)
    assert q <= 1.0, f"{tag} {name}: err / bound = {q:.3f}"


def _sum(name, tag, dtype, out, ref, abs_sum, init=None):
    """|out - ref| <= kappa_s 2^-24 sum |term| (+ |initial|) per element of a token sum."""
    bound = KAPPA_S * EPS24 * (abs_sum if init is None else abs_sum + init.double().abs().reshape(abs_sum.shape))
    q = _ratio((out.double().reshape(ref.shape) - ref).abs(), bound)
    print(f"{tag} {name}: err/bound {q:.3f}")
    _note(name, dtype, q, tag)
    assert q <= 1.0, f"{tag} {name}: err / bound = {q:.3f}"


def _f32_figure(name, tag, a, w, b, ref, A):
    """The figure kappa / kappa_s derive from: the reference's own matmul in f32 / (2^-24 A)."""
    y32 = gemm_ref64(a, w, b, F32).double()
    _note(name, "any", _ratio((y32 - ref).abs(), EPS24 * A), tag)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\ngemm matrix: worst err / bound per (output, dtype) and the case that set it; f32_*: the "
          "reference's matmul in f32 / (2^-24 A)")
    for (name, dt), (v, tag) in sorted(STATS.items()):
        print(f"  GEMMMATRIX {name:44s} {dt:5s} {v:8.4f}  {tag}")


class Gen:
    def __init__(self, seed):
        self.g = torch.Generator(device=DEV).manual_seed(seed)

    def randn(self, *s):
        return torch.randn(*s, generator=self.g, device=DEV)

    def ints(self, lo, hi, *s):
        return torch.randint(lo, hi + 1, s, generator=self.g, device=DEV).float()


class Operands:
    """Stored (banded) operands of one (dtype, M, N, K, kind): a [M, K], w [N, K], bias [N] f32,
    h [M, N] (the GELU' pre-activation), and float64 references computed once on demand."""

    def __init__(self, dtype, M, N, K, exact, seed=0):
        g = Gen(((M * 131 + N) * 521 + K) * 4 + 2 * exact + seed)
        self.dtype, self.M, self.N, self.K, self.exact = dtype, M, N, K, exact
        if exact:
            a, w, b = g.ints(-2, 2, M, K), g.ints(-1, 1, N, K), g.ints(-2, 2, N)
        else:
            a, w, b = g.randn(M, K), g.randn(N, K) / math.sqrt(K), g.randn(N)
        self.a, self.w, self.b = banded(a.to(dtype)), banded(w.to(dtype)), banded(b)
        self.h = banded((g.randn(M, N) + 0.5).to(dtype))
        self._ref = {}

    def ref(self, bias):
        """(a . w^T (+ b), sum |a| |w| (+ |b|)) in float64."""
        if bias not in self._ref:
            b = self.b if bias else None
            self._ref[bias] = (gemm_ref64(self.a, self.w, b), gemm_abs64(self.a, self.w, b))
            if not self.exact:
                _f32_figure("f32_Y", self.tag, self.a, self.w, b, *self._ref[bias])
        return self._ref[bias]

    def gp(self):
        if "gp" not in self._ref:
            gp = gelu_grad64(self.h)
            assert float((gp.abs() >= 0.1).double().mean()) >= 0.8 or gp.numel() < 256
            self._ref["gp"] = gp
        return self._ref["gp"]

    tag = ""


def _judge_y(o, tag, name, yk, bias):
    ref, A = o.ref(bias)
    yk = yk.view(o.M, o.N)
    if o.exact:
        assert torch.equal(yk, ref.to(o.dtype)), f"{tag} {name}: not equal to the exact result"
        _note(name, o.dtype, 0.0)
    else:
        _elem(name, tag, o.dtype, yk, ref, KAPPA * EPS24 * A)


def _judge_y2(o, tag, hk, y2k):
    hk = hk.view(o.M, o.N).double()
    _elem("Y2", tag, o.dtype, y2k.view(o.M, o.N), gelu64(hk), 1e-5 * (1 + hk.abs()))


def _judge_grad(o, tag, name, yk):
    ref, A = o.ref(False)
    gp = o.gp()
    _elem(name, tag, o.dtype, yk.view(o.M, o.N), ref * gp, KAPPA * EPS24 * (1 + gp.abs()) * A)


# ----------------------------------------------------------------------------- token GEMM
def _tok_forms(epi, concat):
    """{(kc, nc, nst, nw): (N, K)}: every form tok_plan reaches over N, K <= 3072, at its smallest N x K."""
    forms = {}
    for K in range(16, 3073, 16):
        for N in range(32, 3073, 32):
            p = tok_plan(1000, N, K, epi, concat)
            if p is not None and (p[:4] not in forms or N * K < forms[p[:4]][0] * forms[p[:4]][1]):
                forms[p[:4]] = (N, K)
    return forms


TOK_PLAIN_FORMS = _tok_forms(PLAIN, 0)
TOK_CAT_FORMS = _tok_forms(PLAIN, 1)
TOK_GELU_FORMS = _tok_forms(DUAL, 0)
assert (len(TOK_PLAIN_FORMS), len(TOK_CAT_FORMS), len(TOK_GELU_FORMS)) == (37, 23, 18)
assert _tok_forms(GRAD, 0) == TOK_GELU_FORMS
# split A: the plain forms but the 48-deep ones; the GELU forms: those with nc <= 192 of them
assert TOK_CAT_FORMS == {f: s for f, s in TOK_PLAIN_FORMS.items() if f[0] != 48}
assert set(TOK_GELU_FORMS) == {f for f in TOK_CAT_FORMS if f[1] <= 192}
assert [TOK_PLAIN_FORMS[f] for f in ((128, 64, 3, 4), (128, 128, 2, 4), (128, 288, 2, 4))] == [(64, 128), (128, 256), (288, 128)]


def _first_per_ring(forms):
    seen, out = set(), set()
    for f in sorted(forms):
        if (f[0], f[2], f[3]) not in seen:
            seen.add((f[0], f[2], f[3]))
            out.add(f)
    return out


TOK_LONG = {PLAIN: _first_per_ring(TOK_PLAIN_FORMS), DUAL: _first_per_ring(TOK_GELU_FORMS)}
TOK_CASES = [("plain", f, dt) for f in sorted(TOK_PLAIN_FORMS) for dt in DTYPES]
TOK_CASES += [("gelu", f, dt) for f in sorted(TOK_GELU_FORMS) for dt in DTYPES]


def _tok_id(case):
    group, (kc, nc, nst, nw), dt = case
    return "%s-kc%d-nc%d-nst%d-nw%d-%s" % (group, kc, nc, nst, nw, DTNAME[dt])


def _tok_long_m(N, K, epi):
    """M = 32 (2 S + 5) + 7, S = the waves over the row groups of that M's own plan."""
    p = tok_plan(1 << 30, N, K, epi)
    S = p[5] // p[4] * p[3]
    M = 32 * (2 * S + 5) + 7
    p = tok_plan(M, N, K, epi)
    assert p[5] // p[4] * p[3] == S and -(-M // 32) == 2 * S + 6  # waves 0..5: three tiles, wave 5's last one 7 rows
    return M


def _tok_call(dt, a, a2, K1, w, b, y, y2, h, M, N, K, epi):
    ops = _ops()
    return _L().lib().msu_tok_gemm(ops._dt(a), ops._p(a), ops._p(a2), K1, ops._p(w), ops._p(b), ops._p(y), ops._p(y2),
                                   ops._p(h), M, N, K, epi, ops._s(a))


def _tok_run(o, tag, epi, bias=True, K1=0, alias=False):
    """Two launches into separate banded outputs; returns the first's (Y, Y2)."""
    M, N, K, dt = o.M, o.N, o.K, o.dtype
    a, a2 = o.a, None
    if K1:
        a, a2 = banded(o.a[:, :K1].contiguous()), banded(o.a[:, K1:].contiguous())
    outs = []
    for i in range(2):
        y = Band(M * N, dt)
        y2 = y if alias else (Band(M * N, dt) if epi == DUAL else None)
        rc = _tok_call(dt, a, a2, K1, o.w, o.b if bias else None, y.t, y2.t if y2 else None,
                       o.h if epi == GRAD else None, M, N, K, epi)
        assert rc == 0, f"{tag}: returned {rc}"
        torch.cuda.synchronize()
        outs.append((y.check(tag + " Y"), y2.check(tag + " Y2") if y2 else None))
    _same(tag + " Y", outs[0][0], outs[1][0])
    if epi == DUAL:
        _same(tag + " Y2", outs[0][1], outs[1][1])
    return outs[0]


@pytest.mark.parametrize("case", TOK_CASES, ids=_tok_id)
def test_tok_gemm_matrix(case):
    group, form, dt = case
    N, K = (TOK_PLAIN_FORMS if group == "plain" else TOK_GELU_FORMS)[form]
    epi0 = PLAIN if group == "plain" else DUAL
    FORM[0] = "kc%d-nc%d-nst%d-nw%d" % form
    Ms = [1, 33, 1000] + ([_tok_long_m(N, K, epi0)] if form in TOK_LONG[epi0] else [])
    for M in Ms:
        for epi, concat in (((PLAIN, 0), (PLAIN, 1)) if group == "plain" else ((DUAL, 0), (GRAD, 0))):
            p = tok_plan(M, N, K, epi, concat)
            assert (p[:4] if p else None) == (form if (form[0] != 48 or not concat) else None), (M, N, K, epi, concat, p)
        for exact in (True, False):
            o = Operands(dt, M, N, K, exact)
            o.tag = tag0 = f"tok/{_tok_id(case)}/{M}x{N}x{K}/{'exact' if exact else 'round'}"
            if group == "plain":
                for bias in (False, True):
                    y, _ = _tok_run(o, f"{tag0}/plain{'+b' if bias else ''}", PLAIN, bias)
                    _judge_y(o, f"{tag0}/plain{'+b' if bias else ''}", "tok_Y", y, bias)
                for K1 in ((K // 2, 8) if M == 33 else (K // 2,)):
                    tag = f"{tag0}/cat{K1}"
                    if form[0] == 48:  # no split-A form of the 48-deep stage: -2, nothing launched
                        y = Band(M * N, dt)
                        rc = _tok_call(dt, o.a, o.a, K1, o.w, o.b, y.t, None, None, M, N, K, PLAIN)
                        torch.cuda.synchronize()
                        assert rc == -2, f"{tag}: returned {rc}"
                        y.untouched(tag)
                        continue
                    y, _ = _tok_run(o, tag, PLAIN, True, K1)
                    _judge_y(o, tag, "tok_Y_cat", y, True)
            else:
                h, y2 = _tok_run(o, tag0 + "/dual", DUAL)
                _judge_y(o, tag0 + "/dual", "tok_H", h, True)
                _judge_y2(o, tag0 + "/dual", h, y2)
                g, _ = _tok_run(o, tag0 + "/gelu_only", DUAL, alias=True)
                _same(tag0 + "/gelu_only vs Y2", g, y2)
                d, _ = _tok_run(o, tag0 + "/grad", GRAD, bias=False)
                _judge_grad(o, tag0 + "/grad", "tok_dgelu", d)


def test_tok_predicate_agrees_with_launch():
    """For every N, K <= 3072 and every epilogue (and split A): "supported" (msu_tok_gemm_supported_epi;
    for split A the plan call) and "msu_tok_gemm at M = 32 returns 0" agree.  Before tok_plan knew
    that the 48-deep stage serves the plain epilogue only, the predicate said 1 and the launch
    returned -3 wherever K % 48 == 0 with K a multiple of neither 96 nor 128 (K = 48, 144, 240, ...)."""
    lib, ops = _L().lib(), _ops()
    M, NMAX = 32, 3072
    a, w = torch.ones(M * NMAX, device=DEV, dtype=BF16), torch.ones(NMAX * NMAX, device=DEV, dtype=BF16)
    b, h = torch.zeros(NMAX, device=DEV), torch.zeros(M * NMAX, device=DEV, dtype=BF16)
    y, y2 = Band(M * NMAX, BF16), Band(M * NMAX, BF16)
    st = ops._s(a)
    bad, launched = [], 0
    for K in range(16, NMAX + 1, 16):
        for N in range(32, NMAX + 1, 32):
            for epi, cat in ((PLAIN, 0), (DUAL, 0), (GRAD, 0), (PLAIN, 1)):
                sup = tok_plan(M, N, K, epi, 1) is not None if cat else lib.msu_tok_gemm_supported_epi(M, N, K, epi) == 1
                assert cat or sup == (tok_plan(M, N, K, epi) is not None)
                rc = lib.msu_tok_gemm(1, ops._p(a), ops._p(a) if cat else None, 8 if cat else 0, ops._p(w),
                                      None if epi == GRAD else ops._p(b), ops._p(y.t), ops._p(y2.t) if epi == DUAL else None,
                                      ops._p(h) if epi == GRAD else None, M, N, K, epi, st)
                launched += rc == 0
                k48 = K % 48 == 0 and K % 96 != 0 and K % 128 != 0  # the 48-deep stage: split A refused at the entry
                if sup != (rc == 0) or (not sup and rc != (-2 if cat and k48 else -3)):
                    bad.append((N, K, epi, cat, sup, rc))
    torch.cuda.synchronize()
    y.bands("Y")
    y2.bands("Y2")
    assert not bad, (len(bad), bad[:8])
    assert launched == 1280 + 3 * 688  # the supported (N, K) of the plain / GELU dual, GELU', split-A plans


# ----------------------------------------------------------------------------- NT GEMM
NKS = (1, 2, 3, 5)
# form -> (mode bits, rows, columns, ring, KN and split-A variants)
NT_FORMS = {"128x128": (6, 128, 128, 2, True), "256x128": (4, 256, 128, 3, True), "128x192": (2, 128, 192, 2, False),
            "256x192": (0, 256, 192, 2, False)}
# shape group -> [(shape name, forms run on it)]
NT_SHAPES = {"n128": [("one", ("128x128", "256x128")), ("ragged", ("128x128", "256x128")), ("large", ("128x128", "256x128"))],
             "n192": [("one", ("128x192",)), ("ragged", ("128x192",)), ("large", ("128x192", "256x192"))]}
NT_CASES = [(grp, sh, dt, nk) for grp in NT_SHAPES for sh, _ in NT_SHAPES[grp] for dt in DTYPES for nk in NKS]
PP_CASES = [(sh, dt, nk) for sh in ("three_quarters", "two_rounds") for dt in DTYPES for nk in (3, 5)]


def _nt_variants(form, nk):
    """[(layout, epilogue, bias, K1)] of a form at nk K steps."""
    out = [("nk", PLAIN, False, 0), ("nk", PLAIN, True, 0), ("nk", DUAL, True, 0), ("nk", GRAD, False, 0)]
    if NT_FORMS[form][4]:
        out += [("kn", PLAIN, False, 0), ("kn", PLAIN, True, 0), ("kn", DUAL, True, 0), ("kn", GRAD, False, 0)]
        if nk >= 2:
            out += [("nk", PLAIN, True, K1) for K1 in sorted({64, 64 * nk - 64})]
    return out


def _nt_shape(lib, grp, sh, K):
    """(M, N) of a shape name, from the CU count and the plan call."""
    cus = nt_plan(1, 32, 64)["cus"]
    if grp == "n128":
        if sh != "large":
            return {"one": (1, 32), "ragged": (100, 160)}[sh]
        # 2.25 x the resident workgroups' tiles (2 per CU at 128 rows, 1 at 256) over two column
        # tiles, the second with 32 live columns; + a ragged last M tile.  The same M serves both.
        tiles_m = -(-9 * 2 * cus // (4 * 2)) + 1
        return 128 * (tiles_m - 1) + 37, 160
    if sh != "large":
        return {"one": (1, 192), "ragged": (100, 384)}[sh]
    # 2 CUs + 3 tiles of 256 rows (the first three workgroups walk three), the last ragged, where
    # the cost model picks the 256 x 192 tile
    _set_mode(lib, 0)
    M = 256 * (2 * cus + 2) + 37
    p = nt_plan(M, 192, K)
    assert (p["rows"], p["bn"], p["tiles"], p["grid"]) == (256, 192, 2 * cus + 3, cus), p
    return M, 192


def _nt_call(o, layout, epi, bias, K1, y, y2, wk):
    ops = _ops()
    lib = _L().lib()
    st = ops._s(o.a)
    dtc, b, h = ops._dt(o.a), ops._p(o.b if bias else None), ops._p(o.h if epi == GRAD else None)
    if K1:
        return lib.msu_nt_gemm_cat(dtc, ops._p(o.a1[K1]), ops._p(o.a2[K1]), K1, ops._p(o.w), b, ops._p(y), o.M, o.N, o.K, st)
    fn, w = (lib.msu_nt_gemm_kn, wk) if layout == "kn" else (lib.msu_nt_gemm, o.w)
    return fn(dtc, ops._p(o.a), ops._p(w), b, ops._p(y), ops._p(y2), h, o.M, o.N, o.K, epi, st)


def _nt_launch(o, tag, layout, epi, bias, K1, wk):
    y = Band(o.M * o.N, o.dtype)
    y2 = Band(o.M * o.N, o.dtype) if epi == DUAL else None
    rc = _nt_call(o, layout, epi, bias, K1, y.t, y2.t if y2 else None, wk)
    assert rc == 0, f"{tag}: returned {rc}"
    torch.cuda.synchronize()
    return y.check(tag + " Y"), (y2.check(tag + " Y2") if y2 else None)


def _nt_judge(o, tag, epi, bias, y, y2):
    if epi == GRAD:
        _judge_grad(o, tag, "nt_dgelu", y)
    else:
        _judge_y(o, tag, "nt_H" if epi == DUAL else "nt_Y", y, bias)
        if epi == DUAL:
            _judge_y2(o, tag, y, y2)


def _nt_operands(dt, M, N, K, exact, split):
    o = Operands(dt, M, N, K, exact, seed=1)
    o.a1 = {K1: banded(o.a[:, :K1].contiguous()) for K1 in split}
    o.a2 = {K1: banded(o.a[:, K1:].contiguous()) for K1 in split}
    return o, banded(o.w.t().contiguous())


@pytest.mark.parametrize("case", NT_CASES, ids=lambda c: "%s-%s-%s-nk%d" % (c[0], c[1], DTNAME[c[2]], c[3]))
def test_nt_gemm_matrix(case):
    grp, sh, dt, nk = case
    lib = _L().lib()
    forms = dict(NT_SHAPES[grp])[sh]
    K = 64 * nk
    prev = lib.msu_nt_gemm_mode(0)
    try:
        M, N = _nt_shape(lib, grp, sh, K)
        for exact in (True, False):
            o, wk = _nt_operands(dt, M, N, K, exact, sorted({64, K - 64}) if nk >= 2 and grp == "n128" else ())
            o.tag = tag0 = f"nt/{grp}-{sh}/{M}x{N}x{K}/{DTNAME[dt]}/{'exact' if exact else 'round'}"
            for form in forms:
                mode, rows, bn, ring, _ = NT_FORMS[form]
                for layout, epi, bias, K1 in _nt_variants(form, nk):
                    tag = f"{tag0}/{form}/{layout}/epi{epi}{'+b' if bias else ''}{'/cat%d' % K1 if K1 else ''}"
                    _set_mode(lib, mode)
                    FORM[0] = f"{form}/{layout}"
                    p = nt_plan(M, N, K, epi, layout == "kn")
                    assert (p["rows"], p["bn"], p["ring"], p["pp"], p["queue"]) == (rows, bn, ring, 0, 0), (tag, p)
                    assert p["tiles"] == -(-M // rows) * -(-N // bn) and p["grid"] == min(p["tiles"], p["cus"] * (2 if rows == 128 else 1))
                    if sh == "large":
                        assert p["tiles"] > 2 * p["grid"]  # some workgroup walks three tiles
                    y, y2 = _nt_launch(o, tag, layout, epi, bias, K1, wk)
                    yb, y2b = _nt_launch(o, tag, layout, epi, bias, K1, wk)
                    _same(tag + " Y", y, yb)
                    if epi == DUAL:
                        _same(tag + " Y2", y2, y2b)
                    _nt_judge(o, tag, epi, bias, y, y2)
    finally:
        lib.msu_nt_gemm_mode(prev)


@pytest.mark.parametrize("case", PP_CASES, ids=lambda c: "%s-%s-nk%d" % (c[0], DTNAME[c[1]], c[2]))
def test_nt_pingpong_matrix(case):
    sh, dt, nk = case
    lib = _L().lib()
    K = 64 * nk
    prev = lib.msu_nt_gemm_mode(1)
    FORM[0] = "pingpong"
    try:
        _set_mode(lib, 1)
        cus = nt_plan(256, 192, K)["cus"]
        # exactly 3/4 of a round of 256 x 192 tiles (N = 192); two whole rounds (N = 384)
        M, N = (256 * (3 * cus // 4), 192) if sh == "three_quarters" else (256 * cus, 384)
        for exact in (True, False):
            o, wk = _nt_operands(dt, M, N, K, exact, ())
            o.tag = tag0 = f"pp/{sh}/{M}x{N}x{K}/{DTNAME[dt]}/{'exact' if exact else 'round'}"
            for epi, bias in ((PLAIN, False), (PLAIN, True), (DUAL, True)):
                tag = f"{tag0}/epi{epi}{'+b' if bias else ''}"
                p = nt_plan(M, N, K, epi)
                assert (p["rows"], p["bn"], p["pp"], p["grid"]) == (256, 192, 1, min(p["tiles"], cus)), (tag, p)
                assert p["tiles"] == (3 * cus // 4 if sh == "three_quarters" else 2 * cus)
                y, y2 = _nt_launch(o, tag, "nk", epi, bias, 0, wk)
                yb, y2b = _nt_launch(o, tag, "nk", epi, bias, 0, wk)
                _same(tag + " Y", y, yb)
                if epi == DUAL:
                    _same(tag + " Y2", y2, y2b)
                _nt_judge(o, tag, epi, bias, y, y2)
            # the GELU' epilogue stays on gemm_nt_kernel under bit 0
            assert nt_plan(M, N, K, GRAD)["pp"] == 0
    finally:
        lib.msu_nt_gemm_mode(prev)


# ----------------------------------------------------------------------------- msu_linear_bwd
# (K, N, H given, X null)
LB_FORMS = [(96, 288, False, False), (96, 96, False, False), (96, 384, False, False), (384, 96, False, False),
            (384, 96, True, False), (384, 96, True, True)]
LB_CASES = [(f, dt) for f in LB_FORMS for dt in DTYPES]


def _lb_id(case):
    (K, N, hh, xnull), dt = case
    return "%dx%d%s%s-%s" % (K, N, "-H" if hh else "", "-Xnull" if xnull else "", DTNAME[dt])


def _lb_long_m(lib, K, N):
    """Three steps for the first workgroups: grid = min(steps, CUs), 64-row steps at (96, 288) / (96, 96)."""
    cus = lib.msu_linear_bwd_workspace(1 << 30, K, N) // (N * K + N)
    ts = 64 if (K, N) in ((96, 288), (96, 96)) else 32
    M = ts * (2 * cus + 2) + 5
    assert lib.msu_linear_bwd_workspace(M, K, N) // (N * K + N) == cus
    assert lib.msu_linear_bwd_workspace(ts * (cus - 1), K, N) // (N * K + N) == cus - 1  # ts is the step
    return M


@pytest.mark.parametrize("case", LB_CASES, ids=_lb_id)
def test_linear_bwd_matrix(case):
    (K, N, hh, xnull), dt = case
    lib, ops = _L().lib(), _ops()
    FORM[0] = _lb_id(case).rsplit("-", 1)[0]
    for M in (1, 31, 65, 1000, _lb_long_m(lib, K, N)):
        assert lib.msu_linear_bwd_supported(M, K, N) == 1
        for exact in (True, False):
            tag0 = f"linbwd/{_lb_id(case)}/{M}/{'exact' if exact else 'round'}"
            g = Gen((M * 131 + N) * 521 + K + 2 * exact + 4 * xnull)
            if exact:
                dy, x, w = g.ints(-2, 2, M, N), g.ints(-2, 2, M, K), g.ints(-1, 1, N, K)
            else:
                dy, x, w = g.randn(M, N), g.randn(M, K), g.randn(N, K) / math.sqrt(N)
            dy, w = banded(dy.to(dt)), w.to(dt)
            wt = banded(w.t().contiguous())  # W^T [K][N]
            h = None
            if xnull:  # X = round16(gelu(H)), H from the value set: the kernel's own operand
                v = VSET[dt].to(DEV)
                h = banded(v[torch.randint(0, len(v), (M, K), generator=g.g, device=DEV)].to(dt))
                x64 = gelu64(h).to(dt).double()
                xk = None
            else:
                xk = banded(x.to(dt))
                x64 = xk.double()
                if hh:
                    h = banded((g.randn(M, K) + 0.5).to(dt))
            # dX [M, K] = dY . W: the "weight" of that GEMM is W^T [K, N]
            dx64, dxA = gemm_ref64(dy, wt), gemm_abs64(dy, wt)
            if not exact:
                _f32_figure("f32_dX", tag0, dy, wt, None, dx64, dxA)
            gp = None
            if h is not None:
                gp = gelu_grad64(h)
                if not xnull:
                    assert float((gp.abs() >= 0.1).double().mean()) >= 0.8 or M < 8
            # dW [N, K] = dY^T X, db [N] = column sums of dY
            dyt, xt = dy.double().t().contiguous(), x64.t().contiguous()
            dw64, dwA = gemm_ref64(dyt, xt), gemm_abs64(dyt, xt)
            db64, dbA = dy.double().sum(0), dy.double().abs().sum(0)
            if not exact:
                _f32_figure("f32_dW", tag0, dyt, xt, None, dw64, dwA)
                _note("f32_db", "any", _ratio((dy.float().sum(0).double() - db64).abs(), EPS24 * dbA), tag0)
            nws = lib.msu_linear_bwd_workspace(M, K, N)
            for form in ("overwrite", "accumulate", "nodb"):
                tag = f"{tag0}/{form}"
                acc = form == "accumulate"
                if acc:
                    w0, b0 = (g.ints(-8, 8, N, K), g.ints(-8, 8, N)) if exact else (g.randn(N, K), g.randn(N))
                else:
                    w0 = b0 = None
                outs = []
                for i in range(2):
                    ws, dx, dw = Band(nws, F32), Band(M * K, dt), Band(N * K, F32, w0)
                    db = Band(N, F32, b0) if form != "nodb" else None
                    _L().call("msu_linear_bwd", ops._dt(dy), ops._p(dy), ops._p(xk), ops._p(wt), ops._p(h), ops._p(dx.t),
                              ops._p(dw.t), ops._p(db.t) if db else None, ops._p(ws.t), M, K, N, int(acc), ops._s(dy))
                    torch.cuda.synchronize()
                    ws.bands(tag + " workspace")
                    outs.append((dx.check(tag + " dX"), dw.check(tag + " dW"), db.check(tag + " db") if db else None))
                (dxk, dwk, dbk), second = outs
                for u, r, what in zip(outs[0], second, ("dX", "dW", "db")):
                    if u is not None:
                        _same(f"{tag} {what}", u, r)
                dxk, dwk = dxk.view(M, K), dwk.view(N, K)
                if gp is not None:
                    _elem("lb_dX_gelu", tag, dt, dxk, dx64 * gp, KAPPA * EPS24 * (1 + gp.abs()) * dxA)
                elif exact:
                    assert torch.equal(dxk, dx64.to(dt)), f"{tag} dX: not equal to the exact result"
                else:
                    _elem("lb_dX", tag, dt, dxk, dx64, KAPPA * EPS24 * dxA)
                rw, rb = (dw64, db64) if not acc else (dw64 + w0.double(), db64 + b0.double())
                if exact and not xnull:
                    assert torch.equal(dwk.double(), rw), f"{tag} dW: not equal to the exact sum"
                else:
                    _sum("lb_dW", tag, dt, dwk, rw, dwA, w0)
                if dbk is not None and exact:
                    assert torch.equal(dbk.double(), rb), f"{tag} db: not equal to the exact sum"
                elif dbk is not None:
                    _sum("lb_db", tag, dt, dbk, rb, dbA, b0)


# ----------------------------------------------------------------------------- refusals
def test_refused_forms_return_their_code_and_write_nothing():
    lib, ops = _L().lib(), _ops()
    M = 64
    z = torch.zeros(M * 512, device=DEV, dtype=BF16)
    zf = torch.zeros(512 * 512, device=DEV)
    st = ops._s(z)
    p = ops._p
    y, y2 = Band(M * 512, BF16), Band(M * 512, BF16)
    dw, db, ws = Band(512 * 512, F32), Band(512, F32), Band(1 << 20, F32)
    nt, kn, cat, tok = lib.msu_nt_gemm, lib.msu_nt_gemm_kn, lib.msu_nt_gemm_cat, lib.msu_tok_gemm
    refused = [
        ("nt N % 32", -2, lambda: nt(1, p(z), p(z), None, p(y.t), None, None, M, 100, 128, PLAIN, st)),
        ("nt K % 64", -2, lambda: nt(1, p(z), p(z), None, p(y.t), None, None, M, 128, 96, PLAIN, st)),
        ("kn K % 64", -2, lambda: kn(1, p(z), p(z), None, p(y.t), None, None, M, 128, 96, PLAIN, st)),
        ("nt cat K1 % 64", -3, lambda: cat(1, p(z), p(z), 32, p(z), p(zf), p(y.t), M, 128, 128, st)),
        ("nt cat without A2", -3, lambda: cat(1, p(z), None, 64, p(z), p(zf), p(y.t), M, 128, 128, st)),
        ("nt GELU' with a bias", -3, lambda: nt(1, p(z), p(z), p(zf), p(y.t), None, p(z), M, 128, 128, GRAD, st)),
        ("nt GELU dual without a bias", -3, lambda: nt(1, p(z), p(z), None, p(y.t), p(y2.t), None, M, 128, 128, DUAL, st)),
        ("nt f32", -3, lambda: nt(0, p(z), p(z), None, p(y.t), None, None, M, 128, 128, PLAIN, st)),
        ("tok N % 32", -2, lambda: tok(1, p(z), None, 0, p(z), None, p(y.t), None, None, M, 100, 96, PLAIN, st)),
        ("tok K % 16", -2, lambda: tok(1, p(z), None, 0, p(z), None, p(y.t), None, None, M, 96, 104, PLAIN, st)),
        ("tok GELU' with a bias", -3, lambda: tok(1, p(z), None, 0, p(z), p(zf), p(y.t), None, p(z), M, 96, 96, GRAD, st)),
        ("tok split A K1 % 8", -2, lambda: tok(1, p(z), p(z), 44, p(z), p(zf), p(y.t), None, None, M, 96, 96, PLAIN, st)),
        ("tok split A without a bias", -3, lambda: tok(1, p(z), p(z), 48, p(z), None, p(y.t), None, None, M, 96, 96, PLAIN, st)),
        ("tok split A at K = 144", -2, lambda: tok(1, p(z), p(z), 72, p(z), p(zf), p(y.t), None, None, M, 96, 144, PLAIN, st)),
        ("tok GELU dual at K = 48", -3, lambda: tok(1, p(z), None, 0, p(z), p(zf), p(y.t), p(y2.t), None, M, 96, 48, DUAL, st)),
        ("tok GELU' at K = 240", -3, lambda: tok(1, p(z), None, 0, p(z), None, p(y.t), None, p(z), M, 96, 240, GRAD, st)),
        ("linbwd H at (96, 96)", -3, lambda: lib.msu_linear_bwd(1, p(z), p(z), p(z), p(z), p(y.t), p(dw.t), p(db.t), p(ws.t), M, 96, 96, 0, st)),
        ("linbwd (128, 128)", -2, lambda: lib.msu_linear_bwd(1, p(z), p(z), p(z), None, p(y.t), p(dw.t), p(db.t), p(ws.t), M, 128, 128, 0, st)),
        ("linbwd neither X nor H", -2, lambda: lib.msu_linear_bwd(1, p(z), None, p(z), None, p(y.t), p(dw.t), p(db.t), p(ws.t), M, 384, 96, 0, st)),
    ]
    assert lib.msu_tok_gemm_supported_epi(M, 96, 48, PLAIN) == 1 and lib.msu_tok_gemm_supported_epi(M, 96, 48, DUAL) == 0
    assert lib.msu_tok_gemm_supported_epi(M, 96, 144, GRAD) == 0 and tok_plan(M, 96, 144, PLAIN, 1) is None
    for what, code, launch in refused:
        rc = launch()
        torch.cuda.synchronize()
        assert rc == code, f"{what}: returned {rc}, not {code}"
        for band in (y, y2, dw, db, ws):
            band.untouched(what)


# ----------------------------------------------------------------------------- sensitivity
# (family, dtype, M, N, K): one rounding case per family, references only
SENSITIVITY = [("tok", BF16, 512, 64, 3072), ("nt", F16, 512, 160, 320), ("linbwd_dx", BF16, 512, 96, 384)]


def sensitivity_fraction(dtype, M, N, K, dev=DEV, kappa=None):
    """Fraction of Y elements on which a reference with one 8-wide k chunk of W zeroed breaks the Y bound."""
    g = torch.Generator(device=dev).manual_seed(M + N + K)
    a = torch.randn(M, K, generator=g, device=dev).to(dtype)
    w = (torch.randn(N, K, generator=g, device=dev) / math.sqrt(K)).to(dtype)
    b = torch.randn(N, generator=g, device=dev)
    ref, A = gemm_ref64(a, w, b), gemm_abs64(a, w, b)
    w_bad = w.clone()
    c = (K // 8) // 2
    w_bad[:, 8 * c:8 * c + 8] = 0
    bad = gemm_ref64(a, w_bad, b)
    bound = 2 * U_T[dtype] * ref.abs() + (KAPPA if kappa is None else kappa) * EPS24 * A + FLOOR_T[dtype]
    return float(((bad - ref).abs() > bound).double().mean())


@pytest.mark.parametrize("family,dtype,M,N,K", SENSITIVITY, ids=[s[0] for s in SENSITIVITY])
def test_bounds_catch_a_dropped_chunk(family, dtype, M, N, K):
    FORM[0] = "reference"
    f = sensitivity_fraction(dtype, M, N, K)
    print(f"{family}: Y bound broken on {100 * f:.1f} % of the elements")
    _note("sensitivity_" + family, dtype, f)
    assert f >= 0.5


# ----------------------------------------------------------------------------- coverage
def _assert_coverage():
    """Every row of the module docstring's matrix has a case."""
    # token GEMM: every reachable form, under every epilogue that reaches it, both dtypes
    got = {(grp, f, dt) for grp, f, dt in TOK_CASES}
    want = {("plain", f, dt) for f in TOK_PLAIN_FORMS for dt in DTYPES} | {("gelu", f, dt) for f in TOK_GELU_FORMS for dt in DTYPES}
    assert got == want and len(TOK_CASES) == len(got)
    for epi, forms in ((PLAIN, TOK_PLAIN_FORMS), (DUAL, TOK_GELU_FORMS)):
        assert {(f[0], f[2], f[3]) for f in TOK_LONG[epi]} == {(f[0], f[2], f[3]) for f in forms}
    # NT GEMM: (form, layout, epilogue, split A, shape, nk, dtype)
    got = set()
    for grp, sh, dt, nk in NT_CASES:
        for form in dict(NT_SHAPES[grp])[sh]:
            for layout, epi, bias, K1 in _nt_variants(form, nk):
                got.add((form, layout, epi, bool(K1), sh, nk, dt))
    want = set()
    for dt in DTYPES:
        for nk in NKS:
            for form in ("128x128", "256x128"):
                for sh in ("one", "ragged", "large"):
                    want |= {(form, lay, epi, False, sh, nk, dt) for lay in ("nk", "kn") for epi in (PLAIN, DUAL, GRAD)}
                    if nk >= 2:
                        want.add((form, "nk", PLAIN, True, sh, nk, dt))
            for sh in ("one", "ragged", "large"):
                want |= {("128x192", "nk", epi, False, sh, nk, dt) for epi in (PLAIN, DUAL, GRAD)}
            want |= {("256x192", "nk", epi, False, "large", nk, dt) for epi in (PLAIN, DUAL, GRAD)}
    assert want <= got, sorted(map(str, want - got))
    assert {(sh, dt, nk) for sh, dt, nk in PP_CASES} == {(sh, dt, nk) for sh in ("three_quarters", "two_rounds")
                                                          for dt in DTYPES for nk in (3, 5)}
    assert {c for c in LB_CASES} == {((K, N, hh, xn), dt) for K, N, hh, xn in
                                     ((96, 288, False, False), (96, 96, False, False), (96, 384, False, False),
                                      (384, 96, False, False), (384, 96, True, False), (384, 96, True, True))
                                     for dt in DTYPES}
    assert {s[0] for s in SENSITIVITY} == {"tok", "nt", "linbwd_dx"}


_assert_coverage()
