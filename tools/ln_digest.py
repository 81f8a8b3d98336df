"""SHA-256 digests of what csrc/layernorm.hip's row kernels write on seeded inputs, through the C
ABI: forward y, s, mean, rstd; backward dx, db, dgamma, dbeta (with dres, dres2, dres3 in plain
and add mode, db and a per-sample scale in add mode); and the raw partial rows of a backward with
dgamma = dbeta = NULL.  Every mode x {bf16, f16, f32} x the smallest width of each reachable
<TPR, KMAX> variant (the tables of tests/test_gpu_ln_matrix.py, imported), at 256 / TPR + 1 rows
and at the matrix's long forward row count (every lane group walks at least three rows, forward
and backward, with a ragged last pass).  A change that keeps the arithmetic of every output keeps
every line; compare two builds of the library with
    MSU_LIB_OVERRIDE=/other/libmsunet_hip.so python tools/ln_digest.py > a.txt
    python tools/ln_digest.py > b.txt && diff a.txt b.txt
(the '#' line names the library, by its path from the repository's root, and is the only one allowed
to differ)."""
import hashlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_gpu_ln_matrix as M  # noqa: E402
from semantic_segmentation_of_stylegan2_artifacts_amd import _lib  # noqa: E402

DEV = "cuda"
EPS = 1e-5
SCALES = [0.5, 1.25, 1.0]


def digest(t):
    return hashlib.sha256(t.contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()[:24]


def _p(t):
    return None if t is None else t.data_ptr()


def _shape(mode, rows):
    """A source shape with at least `rows` logical rows (exactly `rows` outside depth-to-space)."""
    if mode == M.MERGE:
        return (1, 2, 2 * rows)
    if mode == M.D2S2:
        return (1, 1, -(-rows // 4))
    return (rows,)


def run(mode, dt, C, rows):
    g = torch.Generator(device=DEV).manual_seed(1000003 * mode + 7919 * C + rows)

    def rnd(*shape, dtype=dt):
        return torch.randn(*shape, generator=g, device=DEV).to(dtype)

    H = W = Cin = 0
    if mode == M.MERGE:
        _, H, W = _shape(mode, rows)
        Cin = C // 4
        x = rnd(1, H, W, Cin)
        rows = (H // 2) * (W // 2)
    elif mode == M.D2S2:
        _, H, W = _shape(mode, rows)
        x = rnd(1, H, W, 4 * C)
        rows = 4 * H * W
    else:
        x = rnd(rows, C)
    add, res = mode == M.ADD, mode in (M.PLAIN, M.ADD)
    gamma, beta = 1 + 0.1 * rnd(C, dtype=torch.float32), 0.1 * rnd(C, dtype=torch.float32)
    b = rnd(rows, C) if add else None
    scale = torch.tensor(SCALES, device=DEV) if add else None
    rps = -(-rows // 3)
    dy = rnd(rows, C)
    dres = [rnd(rows, C) for _ in range(3)] if res else [None] * 3
    st = torch.cuda.current_stream().cuda_stream
    code = M._code(dt)

    def out(n, dtype=dt):
        return torch.full((n,), float("nan"), device=DEV, dtype=dtype)

    y, mean, rstd = out(rows * C), out(rows, torch.float32), out(rows, torch.float32)
    s = out(rows * C) if add else None
    _lib.call("msu_layernorm_fwd", code, mode, _p(x), _p(b), _p(scale), rps, _p(s), _p(gamma), _p(beta), _p(y),
              _p(mean), _p(rstd), rows, C, H, W, Cin, EPS, st)
    line = f"fwd y {digest(y)} s {digest(s) if add else '-'} mean {digest(mean)} rstd {digest(rstd)}"
    xs = s if add else x
    n = _lib.lib().msu_ln_part_blocks(rows, C)
    for partials_only in (False, True):
        dx, db = out(x.numel()), out(rows * C) if add else None
        part = out(n * 3 * C, torch.float32)  # ops._ln_parts
        dgb = None if partials_only else out(2 * C, torch.float32)
        _lib.call("msu_layernorm_bwd3", code, mode, _p(dy), _p(xs), _p(dres[0]), _p(dres[1]), _p(dres[2]), _p(gamma),
                  _p(mean), _p(rstd), _p(dx), _p(db), _p(scale), rps, _p(part), n,
                  _p(None if partials_only else dgb[:C]), _p(None if partials_only else dgb[C:]), rows, C, H, W, Cin, 0,
                  st)
        torch.cuda.synchronize()
        if partials_only:
            line += f" | part[{n}] {digest(part[:n * 2 * C])} dx {digest(dx)}"
        else:
            line += (f" | bwd dx {digest(dx)} db {digest(db) if add else '-'} dgamma {digest(dgb[:C])}"
                     f" dbeta {digest(dgb[C:])}")
    return line


print(f"# library: {os.path.relpath(_lib.LIB_PATH, ROOT)}")
for mode in (M.PLAIN, M.ADD, M.MERGE, M.D2S2):
    for dt in M.DTYPES:
        for v in M.REACHABLE[dt]:
            C = min(c for c in M._widths(mode, dt) if M.variant(c, dt) == v)
            for rows in (256 // v[0] + 1, M._long_rows(C, dt)[0]):
                print(f"{M.MODENAME[mode]} {M.DTNAME[dt]} C={C} <{v[0]},{v[1]}> rows~{rows}: {run(mode, dt, C, rows)}")
                torch.cuda.empty_cache()
