"""DCT surface interpolation on the GPU (grid_dct.hip, wass_grid_dct*) against the numpy oracle (tests/dct_oracle.py) and the
reference's recorded output (tests/golden/dct_interp.npz, made by tests/golden/make_golden_dct.py)."""
import ctypes as C
import os

import numpy as np
import pytest

import dct_oracle as D
import wass_amd
from wass_amd import _lib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "dct_interp.npz")


def band_limited(n_h, n_w, seed, keep=0.6):
    """A sea-like surface of a few long-crested waves on a footprint-shaped mask with holes (NaN = no data)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:n_h, 0:n_w].astype(np.float64)
    yy /= n_h; xx /= n_w
    z = np.zeros((n_h, n_w))
    for _ in range(8):
        k = rng.uniform(3, 20) * 2 * np.pi
        th = rng.uniform(0, np.pi)
        z += rng.uniform(0.05, 0.3) * np.cos(k * (np.cos(th) * xx + np.sin(th) * yy) + rng.uniform(0, 2 * np.pi))
    foot = (np.abs(xx - 0.5) < 0.15 + 0.3 * yy) & (yy > 0.05) & (yy < 0.95)
    holes = np.zeros_like(foot)
    for _ in range(5):
        cy, cx, r = rng.uniform(0.2, 0.8), rng.uniform(0.3, 0.7), rng.uniform(0.02, 0.06)
        holes |= (yy - cy) ** 2 + (xx - cx) ** 2 < r * r
    return np.where(foot & ~holes & (rng.random((n_h, n_w)) < keep), z, np.nan).astype(np.float32)


def data_loss(irec, zz):
    m = ~np.isnan(zz)
    return float(np.mean((irec[m].astype(np.float64) - zz[m]) ** 2))


def assert_matches(got, want, zz, got_loss, steps, want_steps):
    """The tolerance model of the issue, measured on the CPU: fp32 vs fp64 restatements of the reference differ by 0.27 % of the
    data's std (rms inside the footprint) and 0.3 % in data loss, the Rprop sign rule amplifying rounding; outside the footprint
    only the L1 term constrains the extrapolation, so there the grid need only be finite."""
    m = ~np.isnan(zz)
    std = float(np.nanstd(zz))
    rms = float(np.sqrt(np.mean((got[m].astype(np.float64) - want[m]) ** 2)))
    assert rms <= 0.01 * std, (rms, std)
    assert abs(got_loss - data_loss(want, zz)) <= 0.02 * data_loss(want, zz)
    assert abs(steps - want_steps) in (0, 50)
    assert np.isfinite(got).all()


# ---- one evaluation of loss and gradient against the fp64 oracle
# Bound: every contraction is an f32 MFMA chain, error <= 1.5e-7 * sum |a b| per element (cdna_hip_programming.md, FP32-input
# MFMA, K <= 1024).  The gradient is three chained contractions (K = Nf, W, H) of an orthonormal basis, so the normwise error is
# about 3 * 1.5e-7 * (a growth factor of the |.|-sums over the norms, a few units for these bases) <= 1e-5; 2e-5 leaves a factor 2.
# The data loss is an fp64 sum of squares of f32 residuals whose own error is 1.5e-7 relative to |Irec|: <= 1e-5.
@pytest.mark.parametrize("n", [64, 512, 1024])
def test_eval_matches_fp64_oracle(gpu_ctx, n):
    nf = min(150, n)
    zz = band_limited(n, n, seed=n)
    rng = np.random.default_rng(n + 1)
    x = rng.uniform(-0.5, 1.0, (nf, nf)).astype(np.float32)
    x[rng.random((nf, nf)) < 0.05] = 0.0                            # sign(0) = 0
    g, dl, rl = gpu_ctx.grid_dct_eval(zz, x, alpha=8e-7)
    gr, dlr, rlr = D.evaluate(zz, x, 8e-7, np.float64)
    assert np.linalg.norm(g - gr) <= 2e-5 * np.linalg.norm(gr)
    assert abs(dl - dlr) <= 1e-5 * dlr
    assert abs(rl - rlr) <= 1e-6 * rlr


# ---- Rprop semantics: a few steps from a given x0 against fp64 gradient + fp32 Rprop state
@pytest.mark.parametrize("max_iters", [0, 1, 4])
def test_rprop_steps_match_oracle(gpu_ctx, max_iters):
    n, nf = 128, 32
    zz = band_limited(n, n, seed=5)
    x0 = np.random.default_rng(6).random((nf, nf)).astype(np.float32)
    opts = {"Nfreqs": nf, "MAX_ITERS": max_iters, "TOLERANCE_CHANGE": 0.0}
    _, coeffs, info = gpu_ctx.grid_dct(zz, opts, x0=x0)
    assert info["steps"] == max_iters + 1 and not info["converged"]
    want, step = D.rprop_steps(zz, x0, opts, max_iters + 1)
    assert np.mean(coeffs == want) >= 0.999
    assert (np.abs(coeffs - want) <= step * (1 + 1e-6)).all()


# ---- pinned to the reference's own output
@pytest.mark.parametrize("case", ["one", "default", "early"])
def test_golden_reference_cases(gpu_ctx, case):
    g = np.load(GOLDEN)
    zz = g[str(g[f"{case}_zz"])]
    o = g[f"{case}_opts"]
    opts = {"Nfreqs": int(o[0]), "MAX_ITERS": int(o[1]), "TOLERANCE_CHANGE": float(o[2]), "REGULARIZER_ALPHA": float(o[3]),
            "LEARNING_RATE": float(o[4])}
    grid, _, info = gpu_ctx.grid_dct(zz, opts, x0=g[f"{case}_x0"])
    assert grid.dtype == np.float32 and grid.shape == zz.shape
    assert_matches(grid, g[f"{case}_irec"], zz, info["data_loss"], info["steps"], int(g[f"{case}_steps"]))
    assert abs(info["data_loss"] - data_loss(grid, zz)) <= 1e-6 * data_loss(grid, zz) + 1e-12


# ---- the default size and options
def test_default_size_against_fp32_oracle(gpu_ctx):
    n, nf = 512, 150
    zz = band_limited(n, n, seed=21)
    x0 = np.random.default_rng(22).random((nf, nf)).astype(np.float32)
    opts = {"Nfreqs": nf, "TOLERANCE_CHANGE": 0.0}                  # all 501 steps
    grid, _, info = gpu_ctx.grid_dct(zz, opts, x0=x0)
    want, _, steps, _, _ = D.interpolate(zz, x0, opts, dtype=np.float32)
    assert info["steps"] == 501 == steps
    assert_matches(grid, want, zz, info["data_loss"], info["steps"], steps)
    assert np.sqrt(data_loss(grid, zz)) <= 2 * np.sqrt(data_loss(want, zz))


# ---- determinism, the mesh path and point order
def _cloud(rng, w, h):
    plane = np.array([0.02, 0.81, 0.586, -11.0]); plane[:3] /= np.linalg.norm(plane[:3])
    X = rng.uniform(-6, 6, (h, w)); Y = rng.uniform(-3, 3, (h, w))
    Z = (-plane[3] - plane[0] * X - plane[1] * Y) / plane[2] + 0.05 * np.sin(X * 2.0) + 0.03 * np.cos(Y * 3.0)
    valid = (rng.random((h, w)) < 0.7).astype(np.uint8)
    return plane, valid, np.stack([X, Y, Z], axis=-1)


def test_deterministic_and_mesh_path_equals_cell_map_path(gpu_ctx):
    from oracle import grid_oracle as G
    rng = np.random.default_rng(31)
    w, h = 200, 160
    plane, valid, p3d = _cloud(rng, w, h)
    args = dict(baseline=2.5, xmin=-12.0, xmax=12.0, ymin=-30.0, ymax=-5.0, width=96, height=80)
    opts = {"Nfreqs": 40, "MAX_ITERS": 120}
    mesh = gpu_ctx.mesh_upload(valid, p3d)
    g1, cells, c1, i1 = mesh.grid_dct(plane, **args, dct_options=opts, seed=3)
    g2, cells2, c2, _ = mesh.grid_dct(plane, **args, dct_options=opts, seed=3)
    np.testing.assert_array_equal(g1, g2); np.testing.assert_array_equal(c1, c2); np.testing.assert_array_equal(cells, cells2)
    # the mesh path == the cell-map path on its own cells_out, bit for bit
    g3, c3, _ = gpu_ctx.grid_dct(cells, opts, seed=3)
    np.testing.assert_array_equal(g1, g3); np.testing.assert_array_equal(c1, c3)
    # cells_out is the binned map of the IDW path's oracle (same 2e-6 as tests/test_grid_gpu.py: 2^-24 fixed point, f32 output)
    pts = p3d[valid.astype(bool)].T.copy()
    R, T = G.compute_sea_plane_RT(plane)
    m = (R @ pts + T); m[2] *= -1.0; m *= args["baseline"]
    px = np.floor((m[0] - args["xmin"]) / (args["xmax"] - args["xmin"]) * (args["width"] - 1) + 0.5)
    py = np.floor((m[1] - args["ymin"]) / (args["ymax"] - args["ymin"]) * (args["height"] - 1) + 0.5)
    ok = (px >= 0) & (px < args["width"]) & (py >= 0) & (py < args["height"])
    ref = G.cell_values(px[ok].astype(np.int64), py[ok].astype(np.int64), m[2, ok], args["width"], args["height"])
    np.testing.assert_array_equal(np.isnan(cells), np.isnan(ref))
    e = ~np.isnan(ref)
    assert e.sum() > 500
    np.testing.assert_allclose(cells[e], ref[e], rtol=0, atol=2e-6)
    assert i1["steps"] >= 1 and np.isfinite(g1).all()
    # a different point order: the same grid, bit for bit
    perm = rng.permutation(w * h)
    mesh2 = gpu_ctx.mesh_upload(valid.ravel()[perm].reshape(h, w), p3d.reshape(-1, 3)[perm].reshape(h, w, 3))
    g4, _, _, _ = mesh2.grid_dct(plane, **args, dct_options=opts, seed=3)
    np.testing.assert_array_equal(g1, g4)
    # median cells, too
    g5, cells5, _, _ = mesh.grid_dct(plane, **args, cell="median", dct_options=opts, seed=3)
    assert np.array_equal(np.isnan(cells5), np.isnan(cells)) and np.isfinite(g5).all()


# ---- rectangular grids and edge cases
def test_rectangular_grid_matches_oracle(gpu_ctx):
    h, w, nf = 72, 120, 24
    zz = band_limited(h, w, seed=41)
    x0 = np.random.default_rng(42).random((nf, nf)).astype(np.float32)
    opts = {"Nfreqs": nf, "MAX_ITERS": 200}
    grid, _, info = gpu_ctx.grid_dct(zz, opts, x0=x0)
    want, _, steps, _, _ = D.interpolate(zz, x0, opts, dtype=np.float32)
    assert grid.shape == (h, w)
    assert_matches(grid, want, zz, info["data_loss"], info["steps"], steps)


def test_user_mask_and_error_codes(gpu_ctx):
    n, nf = 64, 16
    zz = band_limited(n, n, seed=51)
    um = (np.random.default_rng(52).random((n, n)) < 0.8).astype(np.uint8)
    opts = {"Nfreqs": nf, "MAX_ITERS": 30}
    g0, _, _ = gpu_ctx.grid_dct(zz, opts)
    g1, _, _ = gpu_ctx.grid_dct(zz, opts, user_mask=um)
    assert np.array_equal(np.isnan(g1), um == 0)
    np.testing.assert_array_equal(g1[um == 1], g0[um == 1])
    for bad in (0, -3, n + 1):
        with pytest.raises(wass_amd.WassError) as e:
            gpu_ctx.grid_dct(zz, {"Nfreqs": bad})
        assert e.value.code == -1
    with pytest.raises(wass_amd.WassError) as e:
        gpu_ctx.grid_dct(np.full((40, 30), np.nan, np.float32), {"Nfreqs": 8})
    assert e.value.code == -6
    # the raw call: an all-NaN grid and the documented code, and the context still works afterwards
    o = wass_amd.stereo.dct_opts({"Nfreqs": 8})
    out = np.zeros((40, 30), np.float32)
    empty = np.full((40, 30), np.nan, np.float32)
    rc = gpu_ctx._lib.wass_grid_dct(gpu_ctx._h, empty.ctypes.data, 30, 40, C.byref(o), None, None, out.ctypes.data, None, None)
    assert rc == -6 and np.isnan(out).all()
    g2, _, _ = gpu_ctx.grid_dct(zz, opts)
    np.testing.assert_array_equal(g0, g2)


def test_dct_interpolator_drop_in(gpu_ctx):
    from wass_amd.gridding import DCTInterpolator
    n = 64
    zz = band_limited(n, n, seed=61)
    keep = zz.copy()
    opts = {"Nfreqs": 20, "MAX_ITERS": 60, "TOLERANCE_CHANGE": None}
    irec, ones = DCTInterpolator(n, n, opts, ctx=gpu_ctx)(zz, verbose=False)
    assert irec.dtype == np.float32 and ones.dtype == np.float32 and irec.shape == ones.shape == (n, n) and (ones == 1).all()
    np.testing.assert_array_equal(np.isnan(zz), np.isnan(keep))            # the caller's map is left alone
    want, _, _ = gpu_ctx.grid_dct(zz, {"Nfreqs": 20, "MAX_ITERS": 60})
    np.testing.assert_array_equal(irec, want)
    assert isinstance(_lib.DctInfo(), C.Structure)
