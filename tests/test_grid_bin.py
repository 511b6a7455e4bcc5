"""tests/grid_bin_oracle.py checked against itself, against oracle/grid_oracle.py and against numpy, and the place where the two
ways of writing the bin expression part (no GPU needed)."""
import numpy as np
import pytest

import grid_bin_oracle as B
from oracle import grid_oracle as G


def _cloud(seed, n, gs, ties=True):
    rng = np.random.default_rng(seed)
    ax = rng.uniform(gs.xmin - 1.0, gs.xmax + 1.0, n)
    ay = rng.uniform(gs.ymin - 1.0, gs.ymax + 1.0, n)
    az = rng.integers(-40, 41, n) / 16.0 if ties else rng.normal(0, 1, n)
    return ax, ay, az


def test_cells_median_equals_numpy_median_per_cell():
    gs = B.GridSpec(-3.0, 4.0, 1.0, 6.0, 13, 9)                     # 117 cells, 6000 points: counts of 30 to 70, odd and even, many ties
    ax, ay, az = _cloud(1, 6000, gs)
    cell, ok = B.bin(ax, ay, gs)
    assert 0 < ok.sum() < ok.size
    px, py = cell[ok] % gs.width, cell[ok] // gs.width
    want = G.cell_values(px, py, az[ok], gs.width, gs.height, "median")
    got = B.cells_median(cell, ok, az, gs.width, gs.height)
    assert np.array_equal(got, want, equal_nan=True)
    cnt = B.counts(cell, ok, gs.width, gs.height)
    assert (cnt % 2 == 0).any() and (cnt % 2 == 1).any() and np.array_equal(cnt == 0, np.isnan(got))
    # a sparse cloud: empty cells, single points, pairs
    ax, ay, az = _cloud(2, 150, gs, ties=False)
    cell, ok = B.bin(ax, ay, gs)
    px, py = cell[ok] % gs.width, cell[ok] // gs.width
    got = B.cells_median(cell, ok, az, gs.width, gs.height)
    assert np.isnan(got).any() and np.array_equal(got, G.cell_values(px, py, az[ok], gs.width, gs.height, "median"), equal_nan=True)


def test_cells_mean_fixed_is_the_plain_mean_on_dyadic_heights_and_close_to_it_elsewhere():
    gs = B.GridSpec(-3.0, 4.0, 1.0, 6.0, 13, 9)
    ax, ay, az = _cloud(3, 6000, gs)
    cell, ok = B.bin(ax, ay, gs)
    px, py = cell[ok] % gs.width, cell[ok] // gs.width
    fixed = B.cells_mean_fixed(cell, ok, az, gs.width, gs.height)
    plain = B.cells_mean(cell, ok, az, gs.width, gs.height)
    assert np.array_equal(plain, G.cell_values(px, py, az[ok], gs.width, gs.height, "mean"), equal_nan=True)
    assert np.array_equal(fixed, plain, equal_nan=True)             # multiples of 1/16: every sum is exact either way
    ax, ay, az = _cloud(4, 6000, gs, ties=False)
    cell, ok = B.bin(ax, ay, gs)
    fixed = B.cells_mean_fixed(cell, ok, az, gs.width, gs.height)
    plain = B.cells_mean(cell, ok, az, gs.width, gs.height)
    e = ~np.isnan(plain)
    assert np.array_equal(np.isnan(fixed), ~e)
    assert 0 < np.abs(fixed[e] - plain[e]).max() <= 2.0 ** -25 + 1e-13          # half a quantum per point, hence per mean


def test_align_and_bin_equal_grid_oracle():
    plane = np.array([0.02, 0.81, 0.586, -11.0]); plane[:3] /= np.linalg.norm(plane[:3])
    R, T = G.compute_sea_plane_RT(plane)
    rng = np.random.default_rng(5)
    n = 5000
    X = rng.uniform(-6, 6, n); Y = rng.uniform(-3, 3, n)
    Z = (-plane[3] - plane[0] * X - plane[1] * Y) / plane[2] + 0.05 * np.sin(X * 2.0)
    gs = B.GridSpec(-12.0, 12.0, -30.0, -5.0, 96, 80)
    ax, ay, az = B.align(np.stack([X, Y, Z], axis=1), R, T, 2.5)
    cell, ok = B.bin(ax, ay, gs)
    # grid_oracle's own expression on the same aligned points
    px = np.floor((ax - gs.xmin) / (gs.xmax - gs.xmin) * (gs.width - 1) + 0.5)
    py = np.floor((ay - gs.ymin) / (gs.ymax - gs.ymin) * (gs.height - 1) + 0.5)
    good = (px >= 0) & (px < gs.width) & (py >= 0) & (py < gs.height)
    assert np.array_equal(ok, good) and 0 < ok.sum() < n
    assert np.array_equal(cell[ok], (py[good] * gs.width + px[good]).astype(np.int64)) and (cell[~ok] == -1).all()
    # and the whole of grid_idw (its alignment is a BLAS product: the same cells on a cloud that keeps clear of the boundaries)
    ref, rmask = G.grid_idw(np.stack([X, Y, Z]), plane, 2.5, *gs, cell="median")
    got, mask = G.idw_from_cells(B.cells_median(cell, ok, az, gs.width, gs.height))
    assert np.array_equal(mask, rmask) and 0.05 < mask.mean() < 1.0
    np.testing.assert_allclose(got[mask == 1], ref[mask == 1], rtol=0, atol=1e-12)
    # non-finite coordinates are outside
    c2, ok2 = B.bin(np.array([np.nan, np.inf, -np.inf, 0.0]), np.array([-10.0, -10.0, -10.0, np.nan]), gs)
    assert not ok2.any() and (c2 == -1).all()


# xmin, xmax, W, the probes of the boundary lattice, the probes that the two expressions put into different cells
DIVERGENCE = [(-12.0, 12.0, 96, 490, 55), (-70.0, 70.0, 1024, 5130, 463), (-50.0, 50.0, 1000, 5010, 445), (-12.3, 17.9, 333, 1675, 136),
              (0.0, 95.0, 96, 490, 12), (-64.0, 64.0, 1025, 5135, 0)]


@pytest.mark.parametrize("lo,hi,n,probes,differ", DIVERGENCE)
def test_the_two_bin_expressions_part_on_the_boundary_lattice_only(lo, hi, n, probes, differ):
    """floor((a - lo) / (hi - lo) * (n - 1) + 0.5), the reference's, against floor((a - lo) * ((n - 1) / (hi - lo)) + 0.5): one
    rounding less and another place for it.  Within two ulps of a nominal cell boundary they disagree about the cell for about a
    tenth of the probes; on two million uniform points they never do, which is why a random cloud cannot tell them apart and the
    GPU test places its points on this lattice."""
    p = B.boundary_lattice(lo, hi, n)
    assert p.size == probes == 5 * (n + 2)
    a, b = B.bin_axis(p, lo, hi, n), B.bin_prescaled(p, lo, hi, n)
    assert int((a != b).sum()) == differ
    assert (np.abs(a - b) <= 1).all()
    # both orders take every lattice point to one of the two cells its boundary separates
    k = np.repeat(np.arange(-1, n + 1), 5)
    assert ((a == k) | (a == k + 1)).all() and ((b == k) | (b == k + 1)).all()
    r = np.random.default_rng(n).uniform(lo - 0.1 * (hi - lo), hi + 0.1 * (hi - lo), 2_000_000)
    assert np.array_equal(B.bin_axis(r, lo, hi, n), B.bin_prescaled(r, lo, hi, n))


def test_exact_edges_of_the_unit_scale_setup():
    """xmin = 0, xmax = W - 1: the scale is exactly 1, fx = floor(a + 0.5).  -0.5 is in (cell 0), the double below is out;
    W - 0.5 is out, the double below is in (cell W - 1)."""
    w = 96
    a = np.array([-0.5, np.nextafter(-0.5, -np.inf), w - 0.5, np.nextafter(w - 0.5, -np.inf)])
    f = B.bin_axis(a, 0.0, w - 1.0, w)
    assert f.tolist() == [0.0, -1.0, float(w), float(w - 1)]
    gs = B.GridSpec(0.0, w - 1.0, 0.0, 9.0, w, 10)
    cell, ok = B.bin(a, np.full(4, 3.0), gs)
    assert ok.tolist() == [True, False, False, True] and cell.tolist() == [3 * w, -1, -1, 3 * w + w - 1]
