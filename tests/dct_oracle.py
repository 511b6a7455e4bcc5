"""CPU restatement of the reference's DCT interpolator (gridding/wassgridsurface/DCTInterpolator.py) in numpy, test infrastructure only.

dtype=np.float32 follows the reference's own op sequence (torch autograd + torch.optim.Rprop in fp32); dtype=np.float64 is the
same algorithm in fp64 (what the GPU's gradient is checked against).  The Rprop state is fp32 in both unless rprop_fp64 is set.
The start value x0 is injected (the reference draws it from torch.rand).  Separate bases for rows (size H) and columns (size W)
extend the reference to rectangular grids; for W == H both are the reference's one basis.
"""
from __future__ import annotations

import numpy as np

DEFAULTS = {"Nfreqs": 150, "MAX_ITERS": 500, "TOLERANCE_CHANGE": 1e-4, "REGULARIZER_ALPHA": 8e-7, "LEARNING_RATE": 5.0}


def dct_basis(n: int) -> np.ndarray:
    """C = scipy.fftpack.dct(eye(n), type=3, norm='ortho') in closed form, fp64: C[r, k], row r = frequency r."""
    r = np.arange(n, dtype=np.int64)[:, None]
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
    Ay = dct_basis(H).astype(np.float32).astype(dtype)[:nf]
    Ax = dct_basis(W).astype(np.float32).astype(dtype)[:nf]
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
