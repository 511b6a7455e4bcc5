"""The front end of the gridding stage (grid.hip: alignment, binning, the per-cell mean and median, the inverse-distance fill and
the closing of the mask) against tests/grid_bin_oracle.py and oracle/grid_oracle.py's idw_from_cells.

Most clouds are gridded with a wass_grid_setup of R = I, T = 0, baseline = 1: the aligned point is then the input point, the
heights are dyadic, and cell membership and every cell value are decided exactly -- the assertions are array_equal."""
import ctypes as C
import time

import numpy as np
import pytest

import grid_bin_oracle as B
from oracle import grid_oracle as G
from wass_amd.stereo import dct_opts, grid_setup

pytestmark = pytest.mark.gpu

I3, T0 = np.eye(3), np.zeros(3)
STATS = ("median", "mean")
MESH_W = 1024


def _setup(gs, R=I3, T=T0, baseline=1.0):
    return grid_setup(R, T, baseline, gs.xmin, gs.xmax, gs.ymin, gs.ymax, gs.width, gs.height)


def _unit(w, h):
    """The setup whose scale is exactly 1: the point (c, r) is the centre of cell (r, c) and every coordinate is exact."""
    return B.GridSpec(0.0, w - 1.0, 0.0, h - 1.0, w, h)


def _upload(ctx, pts, valid):
    """pts (N, 3), valid (N,) as an organised cloud MESH_W wide; the padding is invalid."""
    n = len(pts)
    rows = max(1, -(-n // MESH_W))
    p = np.zeros((rows * MESH_W, 3)); v = np.zeros(rows * MESH_W, np.uint8)
    p[:n] = pts; v[:n] = valid
    return ctx.mesh_upload(v.reshape(rows, MESH_W), p.reshape(rows, MESH_W, 3))


def _cells(ctx, mesh, gsc, cell):
    import torch
    dev = torch.device("cuda", ctx.device_id)
    d = torch.full((gsc.height, gsc.width), 7.0, dtype=torch.float32, device=dev)
    torch.cuda.synchronize(dev)
    mesh.grid_cells_dev(gsc, d, cell)
    ctx.synchronize()
    return d.cpu().numpy()


def _cells_via_dct(ctx, mesh, gsc, cell, any_in_grid):
    """cells_out of wass_mesh_grid_dct (one Rprop step on two frequencies: the solve is not what is looked at).  A cloud without a
    point in the grid gives WASS_ERR_TOO_FEW_POINTS and still hands the (all-NaN) cell map over."""
    o = dct_opts({"Nfreqs": 2, "MAX_ITERS": 0})
    grid = np.empty((gsc.height, gsc.width), np.float32); cells = np.full((gsc.height, gsc.width), 7.0, np.float32)
    rc = ctx._lib.wass_mesh_grid_dct(ctx._h, mesh._h, C.byref(gsc), {"mean": 0, "median": 1}[cell], C.byref(o), None, None,
                                     grid.ctypes.data, cells.ctypes.data, None, None)
    assert rc == (0 if any_in_grid else -6), rc
    return cells


def _want(cell, ok, az, gs, stat):
    f = B.cells_median if stat == "median" else B.cells_mean_fixed
    return f(cell, ok, az, gs.width, gs.height).astype(np.float32)


def _assert_same_map(got, want, what):
    assert got.dtype == np.float32 and got.shape == want.shape
    if not np.array_equal(got, want, equal_nan=True):
        occ = int((np.isnan(got) != np.isnan(want)).sum())
        val = int((~np.isnan(got) & ~np.isnan(want) & (got != want)).sum())
        pytest.fail(f"{what}: occupancy differs in {occ} cells, the value in {val} more")


def _dyadic(rng, n):
    return rng.integers(-65536, 65537, n) / 1024.0                  # multiples of 2^-10 in +-64: sums and medians are exact


# ---- a. the boundary lattice
def _lattice_cloud(gs, seed):
    """One point per probe of the x lattice (each boundary's five probes in rows 0..4) and of the y lattice (columns W-1 .. W-5),
    every point with a height of its own."""
    lx = B.boundary_lattice(gs.xmin, gs.xmax, gs.width)
    ly = B.boundary_lattice(gs.ymin, gs.ymax, gs.height)
    row = gs.ymin + (np.arange(lx.size) % 5) * (gs.ymax - gs.ymin) / (gs.height - 1)
    col = gs.xmin + (gs.width - 1 - np.arange(ly.size) % 5) * (gs.xmax - gs.xmin) / (gs.width - 1)
    x = np.r_[lx, col]; y = np.r_[row, ly]
    z = np.random.default_rng(seed).permutation(x.size) / 1024.0 - 2.0
    return np.stack([x, y, z], axis=1), lx.size, ly.size


LATTICES = [B.GridSpec(-12.0, 12.0, -30.0, -5.0, 96, 80), B.GridSpec(-70.0, 70.0, -70.0, 70.0, 1024, 1024),
            B.GridSpec(-12.3, 17.9, -50.0, 50.0, 333, 1000)]


@pytest.mark.parametrize("gs", LATTICES, ids=lambda g: f"{g.width}x{g.height}")
def test_boundary_lattice_bins_like_the_reference(gpu_ctx, gs):
    """Points within two ulps of every nominal cell boundary, in x and in y: the cell map equals the oracle's bit for bit, which
    it does only if the device evaluates floor((a - xmin) / (xmax - xmin) * (W - 1) + 0.5) with the reference's roundings.  With
    the scale (W - 1) / (xmax - xmin) precomputed, 55 of the 490 x probes of the 96-wide setup and 463 of the 5130 of the 1024-wide
    one land in the neighbouring cell (tests/test_grid_bin.py); the message says whether a differing map is that one."""
    pts, nx, ny = _lattice_cloud(gs, 7)
    ax, ay, az = B.align(pts, I3, T0, 1.0)
    assert np.array_equal(ax, pts[:, 0]) and np.array_equal(ay, pts[:, 1]) and np.array_equal(az, -pts[:, 2])
    cell, ok = B.bin(ax, ay, gs)
    # the other expression, for the message only
    fx, fy = B.bin_prescaled(ax, gs.xmin, gs.xmax, gs.width), B.bin_prescaled(ay, gs.ymin, gs.ymax, gs.height)
    ok2 = (fx >= 0) & (fx < gs.width) & (fy >= 0) & (fy < gs.height)
    cell2 = np.where(ok2, fy * gs.width + fx, -1).astype(np.int64)
    moved = int((cell2 != cell).sum())
    mesh = _upload(gpu_ctx, pts, np.ones(len(pts), np.uint8))
    for stat in STATS:
        got = _cells(gpu_ctx, mesh, _setup(gs), stat)
        want = _want(cell, ok, az, gs, stat)
        if not np.array_equal(got, want, equal_nan=True):
            other = np.array_equal(got, _want(cell2, ok2, az, gs, stat), equal_nan=True)
            pytest.fail(f"{stat} cells of the {gs.width} x {gs.height} lattice ({nx} + {ny} probes):"
                        f" {int((~((got == want) | (np.isnan(got) & np.isnan(want)))).sum())} cells differ from the oracle; the map {'IS' if other else 'is NOT'} the one of the precomputed-scale expression,"
                        f" which misplaces {moved} probes")


def test_exact_edges_far_points_and_non_finite_coordinates(gpu_ctx):
    """xmin = 0, xmax = W - 1 (scale exactly 1).  fx = -0.5 is in (cell 0) and the double below is out; W - 0.5 is out and the
    double below is in; the same in y.  Points far outside on all four sides and valid points whose x or y is NaN or +-inf are
    dropped, and nothing else changes.  A non-finite z is not specified today (llrint of it is undefined) and is left out."""
    w, h = 129, 33                                                  # W - 1 and H - 1 powers of two: the division and the product are exact
    gs = _unit(w, h)
    dn = lambda v: np.nextafter(v, -np.inf)                          # noqa: E731
    edge = [(-0.5, 3.0, 1.0), (dn(-0.5), 4.0, 2.0), (w - 0.5, 5.0, 3.0), (dn(w - 0.5), 6.0, 4.0),
            (7.0, -0.5, 5.0), (8.0, dn(-0.5), 6.0), (9.0, h - 0.5, 7.0), (10.0, dn(h - 0.5), 8.0),
            (-0.5, -0.5, 9.0), (dn(w - 0.5), dn(h - 0.5), 10.0)]
    rng = np.random.default_rng(3)
    body = np.stack([rng.uniform(-0.5, w - 0.5, 3000), rng.uniform(-0.5, h - 0.5, 3000), _dyadic(rng, 3000)], axis=1)
    base = np.r_[np.array(edge), body]
    ax, ay, az = B.align(base, I3, T0, 1.0)
    cell, ok = B.bin(ax, ay, gs)
    assert ok[:10].tolist() == [True, False, False, True, True, False, False, True, True, True]
    assert cell[[0, 3, 4, 7, 8, 9]].tolist() == [3 * w, 6 * w + w - 1, 7, (h - 1) * w + 10, 0, h * w - 1]
    far = [(s * m, 5.0, 1.0) for s in (-1, 1) for m in (1e3, 1e6, 1e300)] + [(5.0, s * m, 1.0) for s in (-1, 1) for m in (1e3, 1e6, 1e300)]
    bad = [(v, 5.0, 1.0) for v in (np.nan, np.inf, -np.inf)] + [(5.0, v, 1.0) for v in (np.nan, np.inf, -np.inf)] + [(np.nan, np.nan, 1.0), (np.inf, -np.inf, 1.0)]
    full = np.r_[base, np.array(far), np.array(bad)]
    full = full[rng.permutation(len(full))]
    fa = B.align(full, I3, T0, 1.0)
    fcell, fok = B.bin(fa[0], fa[1], gs)
    assert fok.sum() == ok.sum()
    m_base = _upload(gpu_ctx, base, np.ones(len(base), np.uint8))
    m_full = _upload(gpu_ctx, full, np.ones(len(full), np.uint8))
    for stat in STATS:
        want = _want(cell, ok, az, gs, stat)
        assert np.array_equal(_want(fcell, fok, fa[2], gs, stat), want, equal_nan=True)
        _assert_same_map(_cells(gpu_ctx, m_base, _setup(gs), stat), want, f"{stat}, edges")
        _assert_same_map(_cells(gpu_ctx, m_full, _setup(gs), stat), want, f"{stat}, edges + far + non-finite")
        _assert_same_map(_cells_via_dct(gpu_ctx, m_full, _setup(gs), stat, True), want, f"{stat}, edges + far + non-finite, cells_out")


# ---- b. the shape table of the cell map
SHAPES = [(2, 2), (2, 500), (500, 2), (31, 33), (32, 32), (25, 41), (257, 33), (300, 7), (513, 300), (1024, 1024), (1025, 1023)]


@pytest.mark.parametrize("w,h", SHAPES, ids=lambda v: str(v))
def test_cell_map_shape_table(gpu_ctx, w, h):
    """Every size class of k_grid_scan (ng < 1024 with idle threads, 1023 / 1024 / 1025, a million cells and one more or less per
    thread), grids wider than one 256-wide workgroup row, and clouds of 0, 1, 255, 256, 257, ng / 3 and 8 ng valid points (2 ng at a
    million cells) among invalid ones: both statistics, through wass_mesh_grid_cells_dev and through the cells_out of
    wass_mesh_grid_dct, equal the oracle bit for bit, the NaN pattern included."""
    ng = w * h
    gs = B.GridSpec(-12.3, 17.9, -30.0, -5.0, w, h)
    gsc = _setup(gs)
    rng = np.random.default_rng(1000 * w + h)
    t0 = time.time()
    for n in (0, 1, 255, 256, 257, ng // 3 + 1, (2 if ng > 1_000_000 else 8) * ng):
        total = n + n // 3 + 5                                      # the rest is invalid: in the grid, with heights that would show
        pts = np.stack([rng.uniform(gs.xmin - 1.0, gs.xmax + 1.0, total), rng.uniform(gs.ymin - 1.0, gs.ymax + 1.0, total),
                        _dyadic(rng, total)], axis=1)
        valid = np.zeros(total, np.uint8)
        valid[rng.permutation(total)[:n]] = 1
        pts[valid == 0, 2] = 1000.0
        v = valid.astype(bool)
        ax, ay, az = B.align(pts[v], I3, T0, 1.0)
        cell, ok = B.bin(ax, ay, gs)
        mesh = _upload(gpu_ctx, pts, valid)
        for stat in STATS:
            want = _want(cell, ok, az, gs, stat)
            assert n > 0 or np.isnan(want).all()
            _assert_same_map(_cells(gpu_ctx, mesh, gsc, stat), want, f"{w} x {h}, n = {n}, {stat}, cells_dev")
            _assert_same_map(_cells_via_dct(gpu_ctx, mesh, gsc, stat, bool(ok.any())), want, f"{w} x {h}, n = {n}, {stat}, cells_out")
        mesh.close()
    print(f"{w} x {h}: {time.time() - t0:.1f} s")


# ---- c. stated counts
def _runs(rng, k, kind):
    if kind == 0:
        return np.sort(_dyadic(rng, k))                            # already sorted
    if kind == 1:
        return np.sort(_dyadic(rng, k))[::-1].copy()               # reversed
    if kind == 2:
        return rng.integers(-2, 3, k) / 4.0                        # ties
    return np.where(rng.random(k) < 0.5, 0.0, -0.0) if k % 2 else np.r_[np.full(k // 2, -0.0), np.full(k - k // 2, 0.0)]


def _stated(cells_and_values):
    """One point at the centre of cell (r, c) per value, in the order given."""
    pts = [np.stack([np.full(len(v), float(c)), np.full(len(v), float(r)), -np.asarray(v, np.float64)], axis=1) for (r, c), v in cells_and_values]
    return np.concatenate(pts) if pts else np.zeros((0, 3))


def _check_stated(ctx, gs, pts):
    ax, ay, az = B.align(pts, I3, T0, 1.0)
    cell, ok = B.bin(ax, ay, gs)
    assert ok.all()
    mesh = _upload(ctx, pts, np.ones(len(pts), np.uint8))
    for stat in STATS:
        _assert_same_map(_cells(ctx, mesh, _setup(gs), stat), _want(cell, ok, az, gs, stat), f"{stat}, stated counts")
    return B.counts(cell, ok, gs.width, gs.height)


def test_stated_counts_per_cell(gpu_ctx):
    """Cell k of a row holds exactly k points, k = 0 .. 40, four rows with four kinds of values (an ascending run, a descending
    run, ties, +0.0 / -0.0); two single cells hold 5000 (ascending) and 5001 (descending) points; one cell holds every point of a
    cloud.  Both statistics are exact.  The points arrive in the stated order (k_grid_bucket_fill may still reorder a segment)."""
    gs = _unit(64, 8)
    rng = np.random.default_rng(12)
    cv = [((1 + kind, k), _runs(rng, k, kind)) for kind in range(4) for k in range(41)]
    cnt = _check_stated(gpu_ctx, gs, _stated(cv))
    assert all(cnt[1 + kind, :41].tolist() == list(range(41)) for kind in range(4)) and cnt.sum() == 4 * 820
    cnt = _check_stated(gpu_ctx, gs, _stated([((0, 0), _runs(rng, 5000, 0)), ((7, 63), _runs(rng, 5001, 1))]))
    assert cnt[0, 0] == 5000 and cnt[7, 63] == 5001 and cnt.sum() == 10001
    for k, kind in ((7001, 1), (6000, 2), (3000, 3)):
        cnt = _check_stated(gpu_ctx, gs, _stated([((3, 17), _runs(rng, k, kind))]))
        assert cnt[3, 17] == k == cnt.sum()


# ---- d. general R, production geometry
def _plane_cloud(rng, n):
    plane = np.array([0.02, 0.81, 0.586, -11.0]); plane[:3] /= np.linalg.norm(plane[:3])
    X = rng.uniform(-6, 6, n); Y = rng.uniform(-3, 3, n)
    Z = (-plane[3] - plane[0] * X - plane[1] * Y) / plane[2] + 0.05 * np.sin(X * 2.0) + 0.03 * np.cos(Y * 3.0)
    return plane, np.stack([X, Y, Z], axis=1), (rng.random(n) < 0.8).astype(np.uint8)


@pytest.mark.parametrize("w,h,n", [(1024, 1024, 2_500_000), (300, 257, 400_000)], ids=["1024x1024", "300x257"])
def test_general_alignment_at_production_size(gpu_ctx, w, h, n):
    """The plane and the baseline of the other gridding tests.  No aligned point lies within 2^-30 of a cell of a boundary (a
    condition on the input, checked first), so occupancy is decided and must be equal.  The device aligns with the same
    operations in the same order (no FMA contraction), so the heights are the same doubles: median cells equal the oracle's
    bit for bit, mean cells equal the fixed-point contract bit for bit and lie within 2^-25 + 2^-24 |z| of the plain fp64 mean
    (half a 2^-24 quantum per point, hence per mean, plus the float32 rounding of the output).  Permuted points: the same map."""
    rng = np.random.default_rng(w)
    plane, pts, valid = _plane_cloud(rng, n)
    R, T = G.compute_sea_plane_RT(plane)
    gs = B.GridSpec(-14.0, 13.0, -50.0, -26.0, w, h)                # most of the cloud, and some of it outside on every side
    v = valid.astype(bool)
    ax, ay, az = B.align(pts[v], R, T, 2.5)
    ux = (ax - gs.xmin) / (gs.xmax - gs.xmin) * (w - 1) + 0.5
    uy = (ay - gs.ymin) / (gs.ymax - gs.ymin) * (h - 1) + 0.5
    margin = min(np.abs(ux - np.rint(ux)).min(), np.abs(uy - np.rint(uy)).min())
    assert margin > 2.0 ** -30, margin
    cell, ok = B.bin(ax, ay, gs)
    assert 0.7 * v.sum() < ok.sum() < v.sum()
    gsc = _setup(gs, R, T, 2.5)
    perm = rng.permutation(n)
    mesh, mesh2 = _upload(gpu_ctx, pts, valid), _upload(gpu_ctx, pts[perm], valid[perm])
    med = _cells(gpu_ctx, mesh, gsc, "median")
    _assert_same_map(med, _want(cell, ok, az, gs, "median"), "median")
    mean = _cells(gpu_ctx, mesh, gsc, "mean")
    plain = B.cells_mean(cell, ok, az, w, h)
    assert np.array_equal(np.isnan(mean), np.isnan(plain))
    e = ~np.isnan(plain)
    assert e.sum() > 1000 and (np.abs(mean[e].astype(np.float64) - plain[e]) <= 2.0 ** -25 + 2.0 ** -24 * np.abs(plain[e])).all()
    _assert_same_map(mean, _want(cell, ok, az, gs, "mean"), "mean against the fixed-point contract")
    assert np.array_equal(_cells(gpu_ctx, mesh2, gsc, "median"), med, equal_nan=True)
    assert np.array_equal(_cells(gpu_ctx, mesh2, gsc, "mean"), mean, equal_nan=True)


# ---- e. the inverse-distance fill and the closing on stated occupancy
def _patterns(w, h, rng):
    def at(cells):
        m = np.zeros((h, w), bool)
        for r, c in cells:
            m[r, c] = True
        return m
    yy, xx = np.mgrid[0:h, 0:w]
    out = {}
    for name, rc in (("corner00", (0, 0)), ("corner0W", (0, w - 1)), ("cornerH0", (h - 1, 0)), ("cornerHW", (h - 1, w - 1)),
                     ("edge_top", (0, w // 2)), ("edge_bottom", (h - 1, w // 2)), ("edge_left", (h // 2, 0)), ("edge_right", (h // 2, w - 1)),
                     ("centre", (h // 2, w // 2))):
        out[name] = at([rc])
    for x in range(254, 259):
        if x < w:
            out[f"x{x}"] = at([(h // 2, x)])
    out["empty"] = np.zeros((h, w), bool)
    out["full"] = np.ones((h, w), bool)
    out["checkerboard"] = (xx + yy) % 2 == 0
    for gap in (4, 5):
        a = w // 2 - 7                                              # the band crosses x = 255 | 256 where the grid is that wide
        a = 253 if w > 262 else a
        out[f"cols_gap{gap}"] = (xx < a) | (xx >= a + gap)
        b = h // 2 - 2
        out[f"rows_gap{gap}"] = (yy < b) | (yy >= b + gap)
    out["random5"] = rng.random((h, w)) < 0.05
    return out


@pytest.mark.parametrize("w,h", [(96, 80), (257, 33), (300, 41), (513, 64)], ids=lambda v: str(v))
def test_idw_fill_and_closing_on_stated_occupancy(gpu_ctx, w, h):
    """One point per wanted cell.  The mask equals idw_from_cells'; outside it the grid is NaN; an occupied cell keeps its value
    exactly; a filled cell is an fp64 convex combination of at most 24 cell values whose weights come from pow(), which may
    differ from numpy's by an ulp of fp64 -- 10^7 times below the float32 rounding of the output, hence the bound
    |gpu - float32(ref)| <= 2^-23 max |z| over the window.  A band of 4 empty columns or rows is closed, a band of 5 is not."""
    gs = _unit(w, h)
    rng = np.random.default_rng(w + h)
    worst = 0.0
    for name, occ in _patterns(w, h, rng).items():
        r, c = np.nonzero(occ)
        z = _dyadic(rng, r.size)
        pts = np.stack([c.astype(np.float64), r.astype(np.float64), -z], axis=1)
        zz = np.full((h, w), np.nan); zz[r, c] = z
        ref, rmask = G.idw_from_cells(zz)
        if name.startswith(("cols_gap", "rows_gap")):                # the closing does what the case is there for
            band = ~occ
            assert rmask[band].all() == name.endswith("4") and rmask[occ].all()
        if name == "empty":
            assert not rmask.any()
        if len(pts) == 0:
            mesh = _upload(gpu_ctx, np.zeros((1, 3)), np.zeros(1, np.uint8))
        else:
            mesh = _upload(gpu_ctx, pts, np.ones(len(pts), np.uint8))
        absz = np.pad(np.where(occ, np.abs(np.nan_to_num(zz)), 0.0), 2)
        winmax = np.max([absz[i:i + h, j:j + w] for i in range(5) for j in range(5)], axis=0)
        for stat in STATS:
            grid, mask = mesh.grid_idw(cell=stat, gs=_setup(gs))
            assert grid.dtype == np.float32 and mask.dtype == np.uint8
            assert np.array_equal(mask, rmask), f"{name}, {stat}: the mask differs in {(mask != rmask).sum()} cells"
            assert np.isnan(grid[mask == 0]).all() and np.isfinite(grid[mask == 1]).all()
            keep = occ & (mask == 1)
            assert np.array_equal(grid[keep], zz[keep].astype(np.float32)), f"{name}, {stat}: occupied cells"
            fill = ~occ & (mask == 1)
            if fill.any():
                err = np.abs(grid[fill].astype(np.float64) - ref[fill].astype(np.float32).astype(np.float64))
                bound = 2.0 ** -23 * winmax[fill]
                ratio = float((err / bound).max())
                worst = max(worst, ratio)
                assert ratio <= 1.0, f"{name}, {stat}: filled cells, largest |gpu - ref| / bound = {ratio:.3f}"
        mesh.close()
    print(f"{w} x {h}: largest |gpu - ref| / bound over the filled cells of all patterns = {worst:.3f}")
