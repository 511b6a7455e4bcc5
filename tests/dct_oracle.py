"""CPU restatement of the reference's DCT interpolator (gridding/wassgridsurface/DCTInterpolator.py) in numpy, test infrastructure only.

dtype=np.float32 follows the reference's own op sequence (torch autograd + torch.optim.Rprop in fp32); dtype=np.float64 is the
same algorithm in fp64 (what the GPU's gradient is checked against).  The Rprop state is fp32 in both unless rprop_fp64 is set.
The start value x0 is injected (the reference draws it from torch.rand).  Separate bases for rows (size H) and columns (size W)
extend the reference to rectangular grids; for W == H both are the reference's one basis.
"""
from __future__ import annotations

import functools

import numpy as np

DEFAULTS = {"Nfreqs": 150, "MAX_ITERS": 500, "TOLERANCE_CHANGE": 1e-4, "REGULARIZER_ALPHA": 8e-7, "LEARNING_RATE": 5.0}


def dct_basis(n: int, rows: int | None = None) -> np.ndarray:
    """C = scipy.fftpack.dct(eye(n), type=3, norm='ortho') in closed form, fp64: C[r, k], row r = frequency r.  rows: only the
    first rows of C (the same values; an 8200-cell axis with 16 frequencies needs no 8200 x 8200 matrix)."""
    r = np.arange(n if rows is None else rows, dtype=np.int64)[:, None]
    k = np.arange(n, dtype=np.int64)[None, :]
    m = (r * (2 * k + 1)) % (4 * n)                      # the angle reduced exactly (period 4n in units of pi / 2n)
    C = np.sqrt(2.0 / n) * np.cos(np.pi * m / (2.0 * n))
    C[0, :] = 1.0 / np.sqrt(n)
    return C


def _sign(v):
    return np.sign(v).astype(v.dtype)


def evaluate(I, x, alpha, dtype=np.float64):
    """(gradient, data loss, |x|_1) at x of the loss sum M (Irec - I)^2 / sum M + alpha |x|_1 (I: NaN = no data)."""
    H, W = I.shape
    nf = x.shape[0]
    M = (~np.isnan(I)).astype(dtype)
    I0 = np.where(np.isnan(I), 0, I).astype(dtype)
    Ay = dct_basis(H, nf).astype(np.float32).astype(dtype)
    Ax = dct_basis(W, nf).astype(np.float32).astype(dtype)
    x = x.astype(dtype)
    Irec = Ay.T @ x @ Ax
    d = Irec - I0
    S = M.sum()
    data = float(np.sum(d * d * M) / S)
    g = (Ay @ ((2 * d * M) / S) @ Ax.T) + dtype(alpha) * _sign(x)
    return g, data, float(np.abs(x).sum())


def _grad_fp32(Dc_y, Dc_x, I0, M, S, x, alpha):
    """The reference's autograd in fp32: Irec = (Dc^T @ P) @ Dc with the zero-padded P, backward through both products."""
    H, W = I0.shape
    nf = x.shape[0]
    P = np.zeros((H, W), np.float32)
    P[:nf, :nf] = x
    A1 = Dc_y.T @ P
    Irec = A1 @ Dc_x
    d = Irec - I0
    inv = np.float32(1.0) / S
    gI = (np.float32(2.0) * d) * inv * M
    gA1 = gI @ Dc_x.T
    gP = Dc_y @ gA1
    return gP[:nf, :nf] + np.float32(alpha) * _sign(x), Irec


def interpolate(I, x0, opts=None, dtype=np.float32, max_iters=None):
    """DCTInterpolator.__call__ with an injected x0: returns (Irec float32, x float32, steps run, converged, last fdelta)."""
    o = dict(DEFAULTS)
    o.update({k: v for k, v in (opts or {}).items() if v is not None})
    if max_iters is not None:
        o["MAX_ITERS"] = max_iters
    H, W = I.shape
    nf = int(o["Nfreqs"])
    M = (~np.isnan(I)).astype(np.float32)
    I0 = np.where(np.isnan(I), 0, I).astype(np.float32)
    x = np.array(x0, np.float32).reshape(nf, nf)
    prev = np.zeros_like(x)
    step = np.full_like(x, np.float32(o["LEARNING_RATE"]))
    lo, hi = np.float32(1e-6), np.float32(50.0)
    if dtype == np.float32:
        Dc_y = dct_basis(H).astype(np.float32)
        Dc_x = dct_basis(W).astype(np.float32)
        S = np.float32(M.sum())

        def grad(xv):
            return _grad_fp32(Dc_y, Dc_x, I0, M, S, xv, o["REGULARIZER_ALPHA"])[0]
    else:
        def grad(xv):
            return evaluate(I, xv, o["REGULARIZER_ALPHA"], np.float64)[0].astype(np.float32)
    steps, converged, fdelta = 0, False, 0.0
    for ii in range(int(o["MAX_ITERS"]) + 1):
        g = grad(x)
        s = np.sign(g * prev)
        eta = np.where(s > 0, np.float32(1.2), np.where(s < 0, np.float32(0.5), np.float32(1.0))).astype(np.float32)
        step = np.minimum(np.maximum(step * eta, lo), hi)
        g = np.where(s < 0, np.float32(0), g).astype(np.float32)
        xn = (x - _sign(g) * step).astype(np.float32)
        prev = g
        steps = ii + 1
        if ii % 50 == 0:
            fdelta = float(np.max(np.abs(xn - x)))
            x = xn
            if fdelta < o["TOLERANCE_CHANGE"]:
                converged = True
                break
        else:
            x = xn
    if dtype == np.float32:
        Irec = _grad_fp32(Dc_y, Dc_x, I0, M, S, x, o["REGULARIZER_ALPHA"])[1]
    else:
        Ay = dct_basis(H).astype(np.float32).astype(np.float64)[:nf]
        Ax = dct_basis(W).astype(np.float32).astype(np.float64)[:nf]
        Irec = (Ay.T @ x.astype(np.float64) @ Ax).astype(np.float32)
    return Irec.astype(np.float32), x, steps, converged, fdelta


def rprop_steps(I, x0, opts, n_steps):
    """n_steps Rprop steps from x0 with the fp64 gradient and fp32 state (no tolerance check): (x, last step sizes)."""
    o = dict(DEFAULTS)
    o.update(opts or {})
    nf = x0.shape[0]
    x = np.array(x0, np.float32)
    prev = np.zeros_like(x)
    step = np.full_like(x, np.float32(o["LEARNING_RATE"]))
    for _ in range(n_steps):
        g = evaluate(I, x, o["REGULARIZER_ALPHA"], np.float64)[0].astype(np.float32)
        s = np.sign(g * prev)
        eta = np.where(s > 0, np.float32(1.2), np.where(s < 0, np.float32(0.5), np.float32(1.0))).astype(np.float32)
        step = np.minimum(np.maximum(step * eta, np.float32(1e-6)), np.float32(50.0))
        g = np.where(s < 0, np.float32(0), g).astype(np.float32)
        x = (x - _sign(g) * step).astype(np.float32)
        prev = g
    assert x.shape == (nf, nf)
    return x, step


# ---- the shapes the GPU tests sweep (tests/test_grid_dct_shapes_gpu.py) and what they reach (tests/test_grid_dct.py)
# (H, W, Nf).  Chosen by the launch plan, not by the numbers: every k_dct_resid<NFT> instance, two and three passes over the
# f-tiles, one and eight column chunks, ragged last chunks, chunks that leave waves without a tile, sizes below 16 and size 1.
SHAPE_CASES = [
    (16, 16, 16), (1, 40, 1), (40, 1, 1),
    (17, 33, 17), (50, 37, 33), (70, 115, 60),
    (90, 131, 80), (100, 97, 96), (112, 105, 100),
    (113, 120, 113), (130, 144, 129), (150, 150, 150),
    (176, 176, 176), (330, 322, 321),
    (8200, 16, 16), (16, 4096, 16), (24, 2300, 20),
]


def plan(H: int, W: int, nf: int) -> dict:
    """The launch plan of grid_dct.hip for one problem, restated: dct_plan() (Wp, Hp, nfp, the nchunk / tpc arithmetic) and the
    pass split of dct_forward() (FT_GROUP = 10 f-tiles per k_dct_resid launch, `n = min(FT_GROUP, nfp / 16 - fg)`), with
    RESID_WAVES = 4.  Only used to choose where tests look and to assert what the case table reaches, never for expected values.
    nchunk, tpc: column chunks and 16-column tiles per chunk; last: tiles of the last chunk; nft: the NFT of each launch."""
    rup16 = lambda v: (v + 15) & ~15
    Wp, Hp, nfp = rup16(W), rup16(H), rup16(nf)
    nct, nrb = Wp // 16, Hp // 16
    nchunk = max(1, min((512 + nrb - 1) // nrb, nct, 8))
    tpc = (nct + nchunk - 1) // nchunk
    nchunk = (nct + tpc - 1) // tpc
    ft = nfp // 16
    return {"Wp": Wp, "Hp": Hp, "nfp": nfp, "nchunk": nchunk, "tpc": tpc, "last": nct - (nchunk - 1) * tpc,
            "nft": [min(10, ft - fg) for fg in range(0, ft, 10)]}


@functools.lru_cache(maxsize=16)
def _basis32(n: int, rows: int) -> np.ndarray:
    return dct_basis(n, rows).astype(np.float32)


def probe_expected(H, W, nf, cell, z, coef=None, c=0.5, count=1):
    """(gradient float32 nf x nf, data loss) in closed form for a grid whose only data cell that matters is cell = (y, x) of value
    z, alpha = 0, and an x that is zero, or zero except x[coef] = c.  Every contraction of the kernels then has one non-zero term,
    so their f32 fma chains round once per product and the result is the same sequence of f32 products on the f32 bases:
      Irec[y, x] = fl(fl(c Ax[g, x]) Ay[f, y]),  R = cs fl(Irec - z),  G[f', g'] = fl(Ay[f', y] fl(R Ax[g', x])).
    count: the number of data cells of the grid (cs = 2 / count as the kernel forms it, the loss is this cell's share)."""
    y, x = cell
    Ay, Ax = _basis32(H, nf), _basis32(W, nf)
    ir = np.float32(0)
    if coef is not None:
        f, g = coef
        ir = np.float32(np.float32(c) * Ax[g, x]) * Ay[f, y]
    d = np.float32(ir - np.float32(z))
    cs = np.float32(2) * (np.float32(1) / np.float32(count))
    u = (d * cs) * Ax[:, x]
    G = Ay[:, y][:, None] * u[None, :]
    assert G.dtype == np.float32
    return G, float(d) ** 2 / count


def holey_surface(H: int, W: int, seed: int, keep: float = 0.6) -> np.ndarray:
    """A band-limited surface (a few long-crested waves, as the GPU tests' band_limited) with random and disc-shaped holes but no
    footprint: every 16-row block and every 16-column tile keeps data, so every workgroup and wave of k_dct_resid has some.
    Grids one cell wide or high get the plain random mask only."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    yy /= H; xx /= W
    z = np.zeros((H, W))
    for _ in range(8):
        k = rng.uniform(3, 20) * 2 * np.pi
        th = rng.uniform(0, np.pi)
        z += rng.uniform(0.05, 0.3) * np.cos(k * (np.cos(th) * xx + np.sin(th) * yy) + rng.uniform(0, 2 * np.pi))
    m = rng.random((H, W)) < keep
    if H > 1 and W > 1:
        for _ in range(5):
            cy, cx, r = rng.uniform(0.2, 0.8), rng.uniform(0.2, 0.8), rng.uniform(0.02, 0.06)
            m &= (yy - cy) ** 2 + (xx - cx) ** 2 >= r * r
    for r0 in range(0, H, 16):
        assert m[r0:r0 + 16].any(), "a 16-row block without data"
    for c0 in range(0, W, 16):
        assert m[:, c0:c0 + 16].any(), "a 16-column tile without data"
    return np.where(m, z, np.nan).astype(np.float32)


def eval_point(nf: int, seed: int) -> np.ndarray:
    """Coefficients to evaluate the loss at: uniform in [-0.5, 1) with 5 % exact zeros (sign(0) = 0)."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-0.5, 1.0, (nf, nf)).astype(np.float32)
    x[rng.random((nf, nf)) < 0.05] = 0.0
    return x


def tile_errors(g, gr) -> tuple[np.ndarray, int]:
    """norm(g - gr) over each 16 x 16 tile of the gradient (ragged edge tiles included), and the number of tiles."""
    nf = gr.shape[0]
    nt = (nf + 15) // 16
    d = np.zeros((nt * 16, nt * 16))
    d[:nf, :nf] = np.asarray(g, np.float64) - gr
    return np.sqrt((d.reshape(nt, 16, nt, 16) ** 2).sum(axis=(1, 3))), nt * nt


def splitmix_x0(seed: int, nf: int) -> np.ndarray:
    """The seeded start value of grid_dct.hip (dct_random_x0) restated: splitmix64 of seed + golden * (i + 1), top 24 bits."""
    with np.errstate(over="ignore"):
        z = np.uint64(seed % (1 << 64)) + np.uint64(0x9E3779B97F4A7C15) * np.arange(1, nf * nf + 1, dtype=np.uint64)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z ^= z >> np.uint64(31)
    return ((z >> np.uint64(40)).astype(np.float32) * np.float32(1.0 / 16777216.0)).reshape(nf, nf)
