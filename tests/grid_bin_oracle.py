"""numpy fp64 restatement of the front end of the gridding stage (grid.hip: alignment on the sea plane, binning, the per-cell
statistic), written from the behaviour of gridding/wassgridsurface/wassgridsurface.py:316-346: the checker of grid.hip, never
imported by the product.  The inverse-distance fill and the closing of the mask are oracle/grid_oracle.py's idw_from_cells.

  align(pts, R, T, baseline)     :318  (Rpl @ mesh + Tpl, z negated) * CAM_BASELINE, element-wise and left to right: BLAS fixes
                                       neither the order of the sum nor the use of FMA, and a point one ulp from a cell boundary
                                       changes its cell with either.
  bin(ax, ay, gs)                :322-326  floor((a - xmin) / (xmax - xmin) * (W - 1) + 0.5) in that order of roundings.
  bin_prescaled(a, lo, hi, n)    the other order, floor((a - lo) * ((n - 1) / (hi - lo)) + 0.5): what grid.hip computed before it
                                 was made to bin like the reference.  Kept so that the tests can show where the two part.
  boundary_lattice(lo, hi, n)    the n + 2 nominal half-cell boundaries (k + 0.5) (hi - lo) / (n - 1) + lo, k = -1 .. n, each with
                                 its two nearest doubles on either side: where the two expressions part.
  cells_median / cells_mean_fixed / cells_mean   the per-cell statistic, vectorised (two million points on a 1024 x 1024 grid take about a second).
"""
from collections import namedtuple

import numpy as np

GridSpec = namedtuple("GridSpec", "xmin xmax ymin ymax width height")


def align(pts, R, T, baseline):
    """pts: (N, 3) camera-frame points.  Returns ax, ay, az (float64, N each)."""
    pts = np.asarray(pts, np.float64)
    R = np.asarray(R, np.float64).reshape(3, 3)
    T = np.asarray(T, np.float64).reshape(3)
    b = np.float64(baseline)
    x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
    with np.errstate(invalid="ignore"):                             # 0 * inf: a non-finite coordinate makes the point NaN, as on the device
        ax = (R[0, 0] * x + R[0, 1] * y + R[0, 2] * z + T[0]) * b
        ay = (R[1, 0] * x + R[1, 1] * y + R[1, 2] * z + T[1]) * b
        az = -(R[2, 0] * x + R[2, 1] * y + R[2, 2] * z + T[2]) * b
    return ax, ay, az


def bin_axis(a, lo, hi, n):
    """The reference's order: subtract, divide by the extent, multiply by n - 1, add 0.5, floor (float64, NaN stays NaN)."""
    a = np.asarray(a, np.float64)
    with np.errstate(invalid="ignore"):
        return np.floor((a - np.float64(lo)) / (np.float64(hi) - np.float64(lo)) * np.float64(n - 1) + 0.5)


def bin_prescaled(a, lo, hi, n):
    a = np.asarray(a, np.float64)
    s = np.float64(n - 1) / (np.float64(hi) - np.float64(lo))
    with np.errstate(invalid="ignore"):
        return np.floor((a - np.float64(lo)) * s + 0.5)


def bin(ax, ay, gs):
    """Returns (cell index int64 = fy * width + fx, -1 outside the grid; the in-grid flag).  Non-finite coordinates are outside."""
    fx = bin_axis(ax, gs.xmin, gs.xmax, gs.width)
    fy = bin_axis(ay, gs.ymin, gs.ymax, gs.height)
    with np.errstate(invalid="ignore"):
        ok = (fx >= 0) & (fx < gs.width) & (fy >= 0) & (fy < gs.height)
    cell = np.full(fx.shape, -1, np.int64)
    cell[ok] = fy[ok].astype(np.int64) * gs.width + fx[ok].astype(np.int64)
    return cell, ok


def boundary_lattice(lo, hi, n):
    k = np.arange(-1, n + 1, dtype=np.float64)
    b = (k + 0.5) * (np.float64(hi) - np.float64(lo)) / np.float64(n - 1) + np.float64(lo)
    dn1 = np.nextafter(b, -np.inf); dn2 = np.nextafter(dn1, -np.inf)
    up1 = np.nextafter(b, np.inf); up2 = np.nextafter(up1, np.inf)
    return np.stack([dn2, dn1, b, up1, up2], axis=1).ravel()


def _segments(cell, ok, ng):
    c = np.asarray(cell)[ok]
    cnt = np.bincount(c, minlength=ng).astype(np.int64)
    start = np.cumsum(cnt) - cnt
    return c, cnt, start


def cells_median(cell, ok, az, width, height):
    """(height, width) float64: the median of each cell's az (the mean of the two middle values as 0.5 * (a + b) where the count
    is even), NaN where a cell is empty."""
    ng = width * height
    c, cnt, start = _segments(cell, ok, ng)
    z = np.asarray(az, np.float64)[ok]
    zs = z[np.lexsort((z, c))]                                   # by cell, then by height
    out = np.full(ng, np.nan)
    occ = np.flatnonzero(cnt)
    hi = start[occ] + cnt[occ] // 2
    lo = np.where(cnt[occ] % 2 == 1, hi, hi - 1)
    out[occ] = np.where(lo == hi, zs[hi], 0.5 * (zs[lo] + zs[hi]))
    return out.reshape(height, width)


def cells_mean_fixed(cell, ok, az, width, height):
    """The documented contract of the mean statistic, in integers: every height is rounded to 2^-24 (ties to even), the integers
    are summed exactly, and the cell is sum / 2^24 / count in float64.  NaN where a cell is empty."""
    ng = width * height
    c, cnt, _ = _segments(cell, ok, ng)
    q = np.rint(np.asarray(az, np.float64)[ok] * 2.0 ** 24).astype(np.int64)
    s = np.zeros(ng, np.int64)
    np.add.at(s, c, q)
    with np.errstate(invalid="ignore", divide="ignore"):
        out = np.where(cnt > 0, s.astype(np.float64) / 2.0 ** 24 / cnt.astype(np.float64), np.nan)
    return out.reshape(height, width)


def cells_mean(cell, ok, az, width, height):
    """The plain float64 mean (np.add.at in point order)."""
    ng = width * height
    c, cnt, _ = _segments(cell, ok, ng)
    s = np.zeros(ng, np.float64)
    np.add.at(s, c, np.asarray(az, np.float64)[ok])
    with np.errstate(invalid="ignore", divide="ignore"):
        out = np.where(cnt > 0, s / cnt, np.nan)
    return out.reshape(height, width)


def counts(cell, ok, width, height):
    return np.bincount(np.asarray(cell)[ok], minlength=width * height).reshape(height, width)
