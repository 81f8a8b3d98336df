"""GPU: the Linear weight-gradient kernels (csrc/gemm_wgrad.hip: ``wgrad_wave_kernel`` at wave
tile 96 / 128 and every (waves along N, waves along K) split, the generic ``wgrad_kernel<T, 3|4>``,
and the split reduction ``colsum_multi``) through direct ``msu_linear_wgrad_ld`` launches,
against a CPU float64 ``dy.T @ x`` / ``dy.sum(0)``.

Harness: dY, X, dW, db and the workspace each live inside a larger NaN buffer (bands of GUARD
elements, a multiple of 8: 16-B alignment holds); the workspace is exactly
``msu_wgrad_workspace(M, N, K)`` floats, NaN before the launch.  After it the bands of the outputs
and of the workspace are still NaN and the outputs hold none: a row read past M brings a NaN
into a product, a slab element left unwritten stays NaN, a workspace overrun clears a band.

(a) exact: operands are integers in [-2, 2], exact in bf16 / f16 / f32; with M <= 65549 every
    partial sum is an integer below 2^24, so any f32 summation order is exact and dW / db must
    EQUAL the float64 reference.  Each case asserts, through ``msu_linear_wgrad_plan``, the kernel
    it is meant to hit.
(b) launch forms on exact integers: accumulate, db == null, a column slice of a wider gradient
    (ldw = 2K, either half), two launches, a second stream, M == 0.
(c) rounding: randn operands rounded once to the 16-bit format against float64 of the same
    rounded operands, max|got - ref| <= 1e-4 max|ref| (the bound of test_gpu_linbwd.py and
    test_linear_cat_direct_grad_accumulates for these f32 sums).
"""
import ctypes
import functools
import os

import pytest
import torch

from semantic_segmentation_of_stylegan2_artifacts_amd import _lib

gpu = pytest.mark.gpu

DEV = "cuda"
GUARD = 4096  # elements of each NaN band (a multiple of 8: the tensors stay 16-B aligned)
NAN = float("nan")
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
DT = {F32: 0, BF16: 1, F16: 2}
NAME = {F32: "f32", BF16: "bf16", F16: "f16"}

# (N, K) -> the (wave tile / 16, waves along N, waves along K) its 16-bit launches take
# ((0, 1, 1): the generic kernel; f32 always takes the generic kernel)
TILE96 = {(96, 96): (6, 1, 1), (192, 96): (6, 2, 1), (96, 192): (6, 1, 2), (288, 96): (6, 3, 1),
          (96, 288): (6, 1, 3), (384, 96): (6, 4, 1), (96, 384): (6, 1, 4), (192, 192): (6, 2, 2),
          (576, 192): (6, 2, 2),    # 3 x 1 workgroup tiles
          (384, 384): (6, 2, 2)}    # 2 x 2 workgroup tiles
TILE128 = {(128, 128): (0, 1, 1),   # ring too shallow for (8, 1, 1): generic kernel, 128 tile
           (256, 128): (8, 2, 1), (128, 256): (8, 1, 2), (384, 128): (8, 3, 1), (128, 384): (8, 1, 3),
           (512, 128): (8, 4, 1), (128, 512): (8, 1, 4), (256, 256): (8, 2, 2), (512, 512): (8, 2, 2)}
RAGGED = {(32, 48): (0, 1, 1), (40, 200): (0, 1, 1), (136, 104): (0, 1, 1)}
# empty trailing splits need the split count capped by the workgroup target, not by M: at
# M <= 65549 the one-tile shapes of the 64- and 128-row stages never are, these are
CAPPED = {(480, 96): (6, 1, 1),     # 5 x 1 tiles, 128-row stages
          (192, 480): (6, 2, 1),    # 1 x 5 tiles, 64-row stages
          (256, 640): (8, 2, 1),    # the same at tile 128
          (104, 296): (0, 1, 1)}    # generic kernel (64-row stages), 2 x 4 ragged tiles
EXPECT = {**TILE96, **TILE128, **RAGGED, **CAPPED}
MS = [1, 31, 129, 1000, 2305, 4099]
EXTRA_M = {(384, 384): [20001], (512, 512): [20001],
           (288, 96): [65549], (384, 96): [65549], (96, 384): [65549], (384, 128): [65549]}
F32_SHAPES = list(RAGGED) + [(96, 96), (128, 128)]


def _exact_cases():
    out = []
    for (N, K) in list(TILE96) + list(TILE128) + list(RAGGED):
        for M in MS + EXTRA_M.get((N, K), []):
            for dt in (BF16, F16) + ((F32,) if (N, K) in F32_SHAPES else ()):
                out.append((M, N, K, dt))
    for (N, K) in CAPPED:
        for M in (31, 65549):
            for dt in (BF16, F16) + ((F32,) if EXPECT[(N, K)][0] == 0 else ()):
                out.append((M, N, K, dt))
    return out


EXACT_CASES = _exact_cases()
# one shape per distinct kernel: the fifteen reachable wave instantiations and both generic tiles
FORM_SHAPES = list(TILE96)[:8] + list(TILE128)[:8] + [(136, 104)]


def _id(c):
    M, N, K, dt = c
    return f"{N}x{K}-M{M}-{NAME[dt]}"


def plan(dtype, M, N, K):
    out = (ctypes.c_int * 6)()
    assert _lib.lib().msu_linear_wgrad_plan(DT[dtype], M, N, K, out) == 0
    return tuple(out)


def _empty_splits(p, M):
    S, mchunk = p[4], p[5]
    return sum(1 for s in range(S) if s * mchunk >= M)


# ------------------------------------------------------------------ what the case list reaches
@pytest.mark.skipif(not os.path.exists(_lib.LIB_PATH), reason="library not built")
def test_exact_cases_reach_every_kernel_and_split_edge():
    """No device needed.  The exact cases hit every reachable wave instantiation in both 16-bit
    formats and both generic tiles in all three types; per rows-per-stage value 32 / 64 / 128 at
    least one case has an empty trailing split and one a split shorter than a stage; the M the
    cases add for this have the empty splits they were chosen for."""
    hit = {}
    for M, N, K, dt in EXACT_CASES:
        p = plan(dt, M, N, K)
        tile = 16 * p[0] if p[0] else (128 if N % 128 == 0 and K % 128 == 0 else 96)
        hit.setdefault((dt, tile) + p[:3], []).append((M, p))
    splits = [(1, 1), (2, 1), (4, 1), (1, 2), (2, 2), (1, 4), (3, 1), (1, 3)]
    want = {(dt, 16 * ntw, ntw, wn, wk) for dt in (BF16, F16) for ntw in (6, 8) for wn, wk in splits}
    want -= {(BF16, 128, 8, 1, 1), (F16, 128, 8, 1, 1)}   # unreachable: tests/test_wgrad_plan.py
    want |= {(dt, tile, 0, 1, 1) for dt in (F32, BF16, F16) for tile in (96, 128)}
    assert set(hit) == want
    for dt in (BF16, F16):
        for rows in (32, 64, 128):
            ps = [(M, p) for k, v in hit.items() if k[0] == dt for M, p in v if p[3] == rows]
            assert any(_empty_splits(p, M) for M, p in ps), f"no empty split at {rows}-row stages"
            assert any(M < rows for M, p in ps), f"no short split at {rows}-row stages"
    # every kernel, not only every stage height, sees a split of fewer rows than a stage
    for k, v in hit.items():
        assert any(M < p[3] for M, p in v), k
    for dt in (BF16, F16):
        for N, K in ((384, 384), (512, 512)):
            assert _empty_splits(plan(dt, 20001, N, K), 20001) == 1
        for N, K in ((288, 96), (384, 96), (96, 384), (384, 128)):
            assert _empty_splits(plan(dt, 65549, N, K), 65549) == 28
        for N, K in CAPPED:
            assert _empty_splits(plan(dt, 65549, N, K), 65549) >= 2
    assert _empty_splits(plan(F32, 65549, 104, 296), 65549) >= 2


# ------------------------------------------------------------------ harness
def _banded(n, dtype):
    buf = torch.full((n + 2 * GUARD,), NAN, device=DEV, dtype=dtype)
    return buf, buf[GUARD:GUARD + n]


def _bands_intact(buf, n, what):
    assert torch.isnan(buf[:GUARD]).all(), f"{what}: the band before it was written"
    assert torch.isnan(buf[GUARD + n:]).all(), f"{what}: the band after it was written"


def _operands(dy, x, dtype):
    """dY [M][N] and X [M][K] (CPU tensors) on the device, each between NaN bands."""
    out = []
    for t in (dy, x):
        _, v = _banded(t.numel(), dtype)
        v.copy_(t.reshape(-1).to(dtype))
        out.append(v)
    return out


def _launch(dtype, dyd, xd, M, N, K, accumulate=0, ldw=None, col=0, dw_init=None, db_init=None, use_db=True):
    """One msu_linear_wgrad_ld launch on the current stream.  dW is the column slice
    [:, col : col + K] of an [N][ldw] f32 matrix that starts as dw_init (NaN when None), db an
    [N] vector that starts as db_init (NaN when None; not passed when use_db is false).
    Returns the whole matrix and db on the CPU after the band checks."""
    from semantic_segmentation_of_stylegan2_artifacts_amd import ops
    lib = _lib.lib()
    ldw = ldw or K
    assert col + K <= ldw
    wbuf, w = _banded(N * ldw, F32)
    bbuf, b = _banded(N, F32)
    if dw_init is not None:
        w.copy_(dw_init.reshape(-1))
    if db_init is not None:
        b.copy_(db_init)
    nws = lib.msu_wgrad_workspace(M, N, K)
    sbuf, ws = _banded(nws, F32)
    rc = lib.msu_linear_wgrad_ld(DT[dtype], dyd.data_ptr(), xd.data_ptr(), w.data_ptr() + 4 * col, ldw,
                                 b.data_ptr() if use_db else None, ws.data_ptr(), M, N, K, accumulate,
                                 ops._s(w))
    assert rc == 0, rc
    torch.cuda.synchronize()
    _bands_intact(wbuf, N * ldw, "dW")
    _bands_intact(bbuf, N, "db")
    _bands_intact(sbuf, nws, "workspace")
    wm = w.view(N, ldw).cpu()
    bv = b.cpu()
    assert not torch.isnan(wm[:, col:col + K]).any(), "dW: elements left unwritten (or NaN read)"
    if use_db:
        assert not torch.isnan(bv).any(), "db: elements left unwritten (or NaN read)"
    return wm, bv


class Exact:
    """Integer operands of one (M, N, K) and their float64 products, computed once."""

    def __init__(self, M, N, K):
        g = torch.Generator().manual_seed(1000003 * M + 1009 * N + K)
        self.dy = torch.randint(-2, 3, (M, N), generator=g, dtype=torch.int8)
        self.x = torch.randint(-2, 3, (M, K), generator=g, dtype=torch.int8)
        dy64 = self.dy.double()
        self.dw = dy64.t() @ self.x.double()
        self.db = dy64.sum(0)
        assert self.dw.abs().max().item() <= 4 * M < 2 ** 24


@functools.lru_cache(maxsize=None)
def _exact(M, N, K):
    return Exact(M, N, K)


def _check_kernel(dtype, M, N, K):
    want = EXPECT[(N, K)] if dtype != F32 else (0, 1, 1)
    assert plan(dtype, M, N, K)[:3] == want, "the plan moved this case onto another kernel"


# ------------------------------------------------------------------ (a) exact
@gpu
@pytest.mark.parametrize("case", EXACT_CASES, ids=_id)
def test_exact_integers(case):
    M, N, K, dtype = case
    _check_kernel(dtype, M, N, K)
    e = _exact(M, N, K)
    dyd, xd = _operands(e.dy, e.x, dtype)
    dw, db = _launch(dtype, dyd, xd, M, N, K)
    assert torch.equal(dw.double(), e.dw), f"dW: {(dw.double() - e.dw).abs().max().item()} off"
    assert torch.equal(db.double(), e.db), f"db: {(db.double() - e.db).abs().max().item()} off"


# ------------------------------------------------------------------ (b) launch forms
def _ints(shape, bound, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-bound, bound + 1, shape, generator=g).float()


@gpu
@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "f16"])
@pytest.mark.parametrize("M", [2305, 4099])
@pytest.mark.parametrize("N,K", FORM_SHAPES, ids=[f"{n}x{k}" for n, k in FORM_SHAPES])
def test_launch_forms(N, K, M, dtype):
    _check_kernel(dtype, M, N, K)
    e = _exact(M, N, K)
    dyd, xd = _operands(e.dy, e.x, dtype)
    dw, db = _launch(dtype, dyd, xd, M, N, K)
    assert torch.equal(dw.double(), e.dw) and torch.equal(db.double(), e.db)

    # accumulate onto preset integers (|dW0 + ref| <= 1000 + 4 M: still exact)
    dw0, db0 = _ints((N, K), 1000, 11 * N + K), _ints((N,), 1000, 13 * N + K)
    aw, ab = _launch(dtype, dyd, xd, M, N, K, accumulate=1, dw_init=dw0, db_init=db0)
    assert torch.equal(aw.double(), dw0.double() + e.dw), "accumulate: dW"
    assert torch.equal(ab.double(), db0.double() + e.db), "accumulate: db"

    # db == null: the same dW, and a db-sized sentinel vector stays as it was
    sent_b = _ints((N,), 1000, 17 * N + K) + 0.5
    nw, nb = _launch(dtype, dyd, xd, M, N, K, db_init=sent_b, use_db=False)
    assert torch.equal(nw, dw), "db == null: dW differs"
    assert torch.equal(nb, sent_b), "db == null: the bias buffer was written"
    nw, nb = _launch(dtype, dyd, xd, M, N, K, accumulate=1, dw_init=dw0, db_init=sent_b, use_db=False)
    assert torch.equal(nw, aw) and torch.equal(nb, sent_b), "db == null, accumulate"

    # a column half of an [N][2K] matrix: the other half keeps its sentinel bits
    sent = _ints((N, 2 * K), 1000, 19 * N + K) + 0.25
    for col in (0, K):
        other = slice(K, 2 * K) if col == 0 else slice(0, K)
        lw, lb = _launch(dtype, dyd, xd, M, N, K, ldw=2 * K, col=col, dw_init=sent)
        assert torch.equal(lw[:, col:col + K], dw) and torch.equal(lb, db), f"ldw = 2K, column {col}"
        assert torch.equal(lw[:, other].view(torch.int32), sent[:, other].view(torch.int32)), \
            f"ldw = 2K, column {col}: the other half was written"
        init = sent.clone()
        init[:, col:col + K] = dw0
        lw, lb = _launch(dtype, dyd, xd, M, N, K, accumulate=1, ldw=2 * K, col=col, dw_init=init, db_init=db0)
        assert torch.equal(lw[:, col:col + K], aw) and torch.equal(lb, ab), f"ldw = 2K accumulate, column {col}"
        assert torch.equal(lw[:, other].view(torch.int32), sent[:, other].view(torch.int32)), \
            f"ldw = 2K accumulate, column {col}: the other half was written"

    # two launches, and a launch on a second stream
    w2, b2 = _launch(dtype, dyd, xd, M, N, K)
    assert torch.equal(w2.view(torch.int32), dw.view(torch.int32)) and torch.equal(b2, db), "two launches differ"
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        w3, b3 = _launch(dtype, dyd, xd, M, N, K)
    torch.cuda.current_stream().wait_stream(side)
    assert torch.equal(w3.view(torch.int32), dw.view(torch.int32)) and torch.equal(b3, db), "second stream differs"


@gpu
@pytest.mark.parametrize("dtype", [F32, BF16, F16], ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("N,K", [(96, 96), (384, 128), (136, 104)], ids=["96x96", "384x128", "136x104"])
def test_no_rows(N, K, dtype):
    """M == 0: overwrite zeroes exactly the [N][K] slice of an ldw = 2K matrix, and db;
    accumulate changes nothing."""
    _, dyd = _banded(0, dtype)
    _, xd = _banded(0, dtype)
    sent = _ints((N, 2 * K), 1000, 23 * N + K) + 0.25
    sent_b = _ints((N,), 1000, 29 * N + K) + 0.5
    for col in (0, K):
        other = slice(K, 2 * K) if col == 0 else slice(0, K)
        w, b = _launch(dtype, dyd, xd, 0, N, K, ldw=2 * K, col=col, dw_init=sent, db_init=sent_b)
        assert torch.equal(w[:, col:col + K], torch.zeros(N, K)) and torch.equal(b, torch.zeros(N))
        assert torch.equal(w[:, other], sent[:, other]), "the other half was written"
        w, b = _launch(dtype, dyd, xd, 0, N, K, ldw=2 * K, col=col, dw_init=sent, use_db=False, db_init=sent_b)
        assert torch.equal(w[:, col:col + K], torch.zeros(N, K)) and torch.equal(b, sent_b)
        w, b = _launch(dtype, dyd, xd, 0, N, K, accumulate=1, ldw=2 * K, col=col, dw_init=sent, db_init=sent_b)
        assert torch.equal(w, sent) and torch.equal(b, sent_b), "accumulate of no rows changed the gradient"


# ------------------------------------------------------------------ (c) rounding
ROUND_SHAPES = FORM_SHAPES + [(32, 48), (40, 200)]
ROUND_CASES = [(4099, N, K) for N, K in ROUND_SHAPES] + \
              [(65549, N, K) for N, K in ((288, 96), (384, 96), (96, 384), (384, 128))]


class Rounded:
    def __init__(self, M, N, K, dtype):
        g = torch.Generator().manual_seed(7 * M + 31 * N + K)
        self.dy = torch.randn(M, N, generator=g).to(dtype)
        self.x = torch.randn(M, K, generator=g).to(dtype)
        dy64 = self.dy.double()
        self.dw = dy64.t() @ self.x.double()
        self.db = dy64.sum(0)


@gpu
@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "f16"])
@pytest.mark.parametrize("M,N,K", ROUND_CASES, ids=[f"{n}x{k}-M{m}" for m, n, k in ROUND_CASES])
def test_rounded_randn_against_float64(M, N, K, dtype):
    """Measured on an MI355X, worst max|got - ref| / max|ref| over all 46 cases: dW 2.26e-7
    (32x48, f16), db 1.71e-7 (384x96, M = 65549, f16), against the bound 1e-4: the f32 sums sit
    at a few ulp.  A wrong operand format (bf16 bits through the f16 MFMA, a wrong ones operand
    for db) or one dropped row per split misses the bound by orders of magnitude."""
    _check_kernel(dtype, M, N, K)
    r = Rounded(M, N, K, dtype)
    dyd, xd = _operands(r.dy, r.x, dtype)
    dw, db = _launch(dtype, dyd, xd, M, N, K)
    rw = (dw.double() - r.dw).abs().max().item() / r.dw.abs().max().item()
    rb = (db.double() - r.db).abs().max().item() / r.db.abs().max().item()
    print(f"wgrad rounding {N}x{K} M={M} {NAME[dtype]}: dW {rw:.3e} db {rb:.3e} (bound 1e-4)")
    assert rw <= 1e-4, f"dW: {rw:.3e} of max|ref|"
    assert rb <= 1e-4, f"db: {rb:.3e} of max|ref|"
