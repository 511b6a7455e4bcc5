"""numpy restatement of the grid set-up (wass_amd/csrc/grid_setup.hip, wass_amd.gridding.setup_grid): the checker, never imported by
the product.

  quantile(a, q)            np.quantile(a, q) for method "linear", restated from numpy 2.2.6 (lib/_function_base_impl.py): the virtual
                            index (n - 1) * q of _QuantileMethods["linear"], _get_indexes, _get_gamma and _lerp with its t >= 0.5
                            branch, on the fully sorted array.  One NaN gives all NaN.
  key / unkey               the order-preserving map double <-> uint64 of the device (-0.0 below +0.0).
  select(a, q, skip=None)   the device's selection step by step on the host: six digit passes (11, 11, 11, 11, 11, 9 bits) for a[lo],
                            the tie rule, the pass for the smallest key above a[lo] ("next"), then quantile's interpolation.  skip
                            names one pass (0 .. 5 or "next") that is left out: a skipped digit pass takes the lowest digit present
                            and keeps the rank, a skipped "next" takes a[hi] = a[lo], a skipped "tie" leaves the tie rule out and
                            always takes the next larger key for a[hi].  The GPU tests use it to show that a probe set can fail:
                            with the step it aims at skipped, the answer changes.
  aligned_z(pts, R, T, b)   z = -(((R20 x + R21 y) + R22 z) + T2) * b, every product and sum rounded on its own.
  sea_plane_RT, zrange, grid_axes, wavenumbers   setup()'s algebra (wassgridsurface.py:82-174), written from its expressions.
"""
import numpy as np

SHIFTS = (53, 42, 31, 20, 9, 0)
NBITS = (11, 11, 11, 11, 11, 9)
_SIGN = np.uint64(1) << np.uint64(63)


def indexes(n, q):
    """(lo, hi, gamma) per q: the resolved neighbouring positions in the sorted array and numpy's interpolation weight."""
    q = np.atleast_1d(np.asarray(q, np.float64))
    virt = (n - 1) * q
    prev = np.floor(virt)
    nxt = prev + 1
    above = virt >= n - 1
    prev[above] = -1
    nxt[above] = -1
    below = virt < 0
    prev[below] = 0
    nxt[below] = 0
    prev = prev.astype(np.intp)
    nxt = nxt.astype(np.intp)
    gamma = virt - prev
    return np.where(prev < 0, prev + n, prev), np.where(nxt < 0, nxt + n, nxt), gamma


def lerp(a, b, t):
    a, b, t = (np.asarray(v, np.float64) for v in (a, b, t))
    with np.errstate(invalid="ignore"):
        diff = b - a
        r = a + diff * t
        return np.where(t >= 0.5, b - diff * (1 - t), r)


def quantile(a, q):
    a = np.sort(np.asarray(a, np.float64).ravel())
    qs = np.atleast_1d(np.asarray(q, np.float64))
    if a.size == 0 or np.isnan(a[-1]):
        return np.full(qs.shape, np.nan)
    lo, hi, gamma = indexes(a.size, qs)
    return lerp(a[lo], a[hi], gamma)


def key(a):
    u = np.ascontiguousarray(a, np.float64).view(np.uint64)
    return np.where(u & _SIGN != 0, ~u, u | _SIGN)


def unkey(k):
    k = np.asarray(k, np.uint64)
    return np.where(k & _SIGN != 0, k ^ _SIGN, ~k).astype(np.uint64).view(np.float64)


def select(a, q, skip=None):
    a = np.asarray(a, np.float64).ravel()
    qs = np.atleast_1d(np.asarray(q, np.float64))
    if a.size == 0 or np.isnan(a).any():
        return np.full(qs.shape, np.nan)
    keys = key(a)
    los, his, gammas = indexes(a.size, qs)
    out = np.empty(qs.size)
    for i, (lo, hi, gamma) in enumerate(zip(los, his, gammas)):
        cand, k, prefix = keys, int(lo), 0
        for p, (shift, nbits) in enumerate(zip(SHIFTS, NBITS)):
            digit = ((cand >> np.uint64(shift)) & np.uint64((1 << nbits) - 1)).astype(np.int64)
            hist = np.bincount(digit, minlength=1 << nbits)
            if p == skip:
                b = int(np.flatnonzero(hist)[0])
            else:
                cum = np.cumsum(hist)
                b = int(np.searchsorted(cum, k, side="right"))
                k -= int(cum[b] - hist[b])
            prefix = (prefix << nbits) | b
            cand = cand[digit == b]
            k = min(k, cand.size - 1)                       # only a skipped pass can leave the rank outside
        lo_key = np.uint64(prefix)
        eq = int((keys == lo_key).sum())
        above = keys[keys > lo_key]
        if hi == lo or skip == "next" or (k + 1 < eq and skip != "tie") or above.size == 0:
            hi_key = lo_key
        else:
            hi_key = above.min()
        out[i] = lerp(unkey(lo_key), unkey(hi_key), gamma)
    return out


def aligned_z(pts, R, T, baseline):
    """pts: (N, 3).  The heights the device hands to the selection."""
    pts = np.asarray(pts, np.float64)
    R = np.asarray(R, np.float64).reshape(3, 3)
    T = np.asarray(T, np.float64).reshape(3)
    with np.errstate(invalid="ignore", over="ignore"):
        return -(((R[2, 0] * pts[:, 0] + R[2, 1] * pts[:, 1]) + R[2, 2] * pts[:, 2]) + T[2]) * np.float64(baseline)


def sea_plane_RT(plane):
    a, b, c, d = (float(v) for v in plane)
    q = (1 - c) / (a * a + b * b)
    return (np.array([[1 - a * a * q, -a * b * q, -a], [-a * b * q, 1 - b * b * q, -b], [a, b, c]]), np.array([[0.0], [0.0], [d]]))


def zrange(z02, z98):
    """:122-129: 1.5 times the quantiles, made symmetric with the larger magnitude kept -> (zmin, zmax)."""
    zmax, zmin = z98 * 1.5, z02 * 1.5
    return (-zmax, zmax) if abs(zmax) > abs(zmin) else (zmin, -zmin)


def grid_axes(xmin, xmax, ymin, ymax, Nx, Ny):
    return np.meshgrid(np.linspace(xmin, xmax, Nx), np.linspace(ymin, ymax, Ny))


def wavenumbers(Nx, Ny, x_spacing, y_spacing):
    kx = np.array([float(i) / Nx * (2.0 * np.pi / x_spacing) for i in range(-(Nx // 2), Nx // 2)])
    ky = np.array([float(i) / Ny * (2 * np.pi / y_spacing) for i in range(-(Ny // 2), Ny // 2)])
    KX, KY = np.meshgrid(kx, ky)
    return KX, KY, 1.0 / (Nx * Ny)
