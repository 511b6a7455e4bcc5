"""Grid set-up without a GPU: the numpy restatement of np.quantile and of the device's selection (tests/grid_setup_oracle.py) held
to numpy itself, the alignment's order of sums against the reference's R @ mesh + T, the four-point homography, setup()'s algebra on
a synthetic rig, the config.mat round trip into grid_sequence's key access, the readers and the command line's exit codes."""
import os
import subprocess
import sys

import numpy as np
import pytest

import grid_setup_oracle as G
from test_cli import _write_png, _write_xml
from wass_amd import gridding, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NS = (1, 2, 3, 49, 50, 51, 1000, 4097)
QS = (0.0, 0.02, 0.5, 0.98, 1.0)


def _arrays(n, seed):
    rng = np.random.default_rng(seed)
    base = rng.normal(0.0, 0.7, n)
    ulp = np.full(n, 1.25)
    for i in range(1, n):
        ulp[i] = np.nextafter(ulp[i - 1], 2.0)
    zeros = np.where(rng.random(n) < 0.5, -0.0, 0.0)
    inf = base.copy(); inf[:: max(1, n // 7)] = np.inf; inf[n // 2] = -np.inf
    return {"normal": base, "ties": rng.integers(-3, 4, n).astype(np.float64), "equal": np.full(n, -2.5), "ulp": rng.permutation(ulp),
            "zeros": zeros, "zeros+": np.concatenate([zeros, [1.0, -1.0]]), "inf": inf}


@pytest.mark.parametrize("n", NS)
def test_quantile_restatement_equals_numpy(n):
    for name, a in _arrays(n, seed=n).items():
        for q in QS + (list(QS),):
            with np.errstate(invalid="ignore"):
                want = np.atleast_1d(np.quantile(a, q))
            got, sel = G.quantile(a, q), G.select(a, q)
            if name.startswith("zeros"):                    # numpy does not define which zero it returns: compare by value
                assert (got == want).all() and (sel == want).all(), (name, q)
            elif name == "inf":
                np.testing.assert_array_equal(got, want, err_msg=f"{name} {q}")     # NaN counts as equal here
                np.testing.assert_array_equal(sel, want, err_msg=f"{name} {q}")
            else:
                assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (name, q, got, want)
                assert np.array_equal(sel.view(np.uint64), want.view(np.uint64)), (name, q, sel, want)


def test_one_nan_gives_all_nan():
    a = np.random.default_rng(1).normal(size=51)
    a[17] = np.nan
    assert np.isnan(np.quantile(a, list(QS))).all()
    assert np.isnan(G.quantile(a, list(QS))).all() and np.isnan(G.select(a, list(QS))).all()
    assert np.isnan(G.quantile(-a, 0.5)).all()              # a NaN with its sign bit set too


def test_keys_keep_the_order():
    a = np.array([-np.inf, -1e300, -1.0, -5e-324, -0.0, 0.0, 5e-324, 2.2e-308, 1.0, np.nextafter(1.0, 2.0), 1e300, np.inf])
    k = G.key(a)
    assert (np.diff(k.astype(object)) > 0).all()
    assert np.array_equal(G.unkey(k).view(np.uint64), a.view(np.uint64))


# The largest differences seen between the oracle's stated order of sums and the reference's BLAS product on these 100 000 points
# ("Grid set-up"): 327 680 ulps of z, at a height of 8e-5 -- z is what is left when terms of the size of T2 * baseline
# cancel, so an ulp of a small z is far below the rounding of the terms -- which is 2.5 ulps of T2 * baseline, 8.9e-15 in all.  Each
# bound is twice the value seen plus one ulp.  This is the distance to the reference's expression on the CPU, not a tolerance of
# the GPU, which must equal the oracle exactly.
ALIGN_ULPS_OF_Z_SEEN = 327680.0
ALIGN_ULPS_OF_T2_SEEN = 2.5


def test_alignment_order_of_sums_against_the_reference_expression():
    rng = np.random.default_rng(2024)
    n = 100_000
    plane = np.array([0.03, 0.80, 0.59, -11.0]); plane[:3] /= np.linalg.norm(plane[:3])
    R, T = G.sea_plane_RT(plane)
    X = rng.uniform(-40, 40, n); Y = rng.uniform(-6, 3, n)
    Z = (-plane[3] - plane[0] * X - plane[1] * Y) / plane[2] + rng.normal(0, 0.4, n)
    mesh = np.stack([X, Y, Z])                               # 3 x N, as load_camera_mesh returns it
    ref = R @ mesh + T                                       # align_on_sea_plane_RT (wass_utils.py:54-61)
    ref[2, :] *= -1.0
    ref = ref[2] * 2.5
    got = G.aligned_z(mesh.T, R, T, 2.5)
    ulps = np.abs(got - ref) / np.spacing(np.abs(ref))
    ulps_t2 = np.abs(got - ref) / np.spacing(abs(plane[3]) * 2.5)
    print("largest difference: %.1f ulps of z (at z = %.3g), %.2f ulps of T2 * baseline" % (ulps.max(), ref[ulps.argmax()], ulps_t2.max()))
    assert ulps.max() <= 2 * ALIGN_ULPS_OF_Z_SEEN + 1
    assert ulps_t2.max() <= 2 * ALIGN_ULPS_OF_T2_SEEN + 1


def _apply(H, p):
    q = np.c_[p, np.ones(len(p))] @ np.asarray(H).T
    return q[:, :2] / q[:, 2:]


def test_homography_maps_the_points_and_recovers_a_known_one():
    src = np.array([[12.5, 30.0], [300.25, 41.0], [280.0, 200.5], [5.0, 190.0]])
    dst = np.array([[-25.0, -60.0], [25.0, -60.0], [25.0, -10.0], [-25.0, -10.0]])
    H = gridding.homography_4pt(src, dst)
    assert H[2, 2] == 1.0
    assert np.abs(_apply(H, src) - dst).max() <= 1e-9 * 50.0
    Hi = gridding.homography_4pt(dst, src)
    assert np.abs(_apply(Hi, dst) - src).max() <= 1e-9 * 300.0
    # a known homography whose four correspondences are exact in float32 (w = 1, 2, 2, 1)
    K = np.array([[1.5, 0.25, 8.0], [0.5, 2.0, -4.0], [1.0 / 256, 0.0, 1.0]])
    s = np.array([[0.0, 0.0], [256.0, 0.0], [256.0, 512.0], [0.0, 512.0]])
    d = _apply(K, s)
    assert np.array_equal(d.astype(np.float32).astype(np.float64), d)
    assert np.abs(gridding.homography_4pt(s, d) - K).max() <= 1e-9 * np.abs(K).max()


def test_homography_refuses_collinear_points():
    ok = np.array([[0.0, 0.0], [10.0, 0.0], [10.0, 10.0], [0.0, 10.0]])
    for bad in (np.array([[0.0, 0.0], [5.0, 5.0], [10.0, 10.0], [0.0, 10.0]]), np.array([[0.0, 1.0], [1.0, 1.0], [2.0, 1.0], [3.0, 1.0]]),
                np.array([[2.0, 2.0]] * 4)):
        with pytest.raises(ValueError):
            gridding.homography_4pt(bad, ok)
        with pytest.raises(ValueError):
            gridding.homography_4pt(ok, bad)
    with pytest.raises(ValueError):
        gridding.homography_4pt(ok[:3], ok[:3])


# ---- a synthetic rig and its work directory (shared with tests/test_grid_setup_gpu.py)
IW, IH = 320, 240
PLANE = np.array([0.02, 0.81, 0.586, -11.0]); PLANE[:3] /= np.linalg.norm(PLANE[:3])
BASELINE = 2.5


def rig_files():
    rig = synth.rig_geometry(IW, IH)
    K = rig["K_left"]
    P0 = K @ np.hstack([np.eye(3), np.zeros((3, 1))])
    P1 = K @ np.hstack([rig["R"], -np.asarray(rig["T"], float).reshape(3, 1)])
    return {"K0": K, "K1": rig["K_right"], "R": rig["R"], "T": np.asarray(rig["T"], float), "P0cam": P0, "P1cam": P1}


def write_workdir(wd, picture=None, mesh_bytes=None):
    """The files setup() reads from a frame's directory."""
    os.makedirs(wd, exist_ok=True)
    f = rig_files()
    _write_xml(os.path.join(wd, "intrinsics_00000000.xml"), "intr", f["K0"])
    _write_xml(os.path.join(wd, "intrinsics_00000001.xml"), "intr", f["K1"])
    np.savetxt(os.path.join(wd, "Cam0_poseR.txt"), f["R"]); np.savetxt(os.path.join(wd, "Cam0_poseT.txt"), f["T"])
    np.savetxt(os.path.join(wd, "P0cam.txt"), f["P0cam"]); np.savetxt(os.path.join(wd, "P1cam.txt"), f["P1cam"])
    if picture is not None:
        os.makedirs(os.path.join(wd, "undistorted"), exist_ok=True)
        _write_png(os.path.join(wd, "undistorted", "00000000.png"), picture)
    if mesh_bytes is not None:
        with open(os.path.join(wd, "mesh_cam.xyzC"), "wb") as fh:
            fh.write(mesh_bytes)
    return f


def _algebra(Nx=64, Ny=48, z02=-0.31, z98=0.27, size_x=24.0, size_y=None, **kw):
    f = rig_files()
    size_y = size_x * (Ny - 1) / (Nx - 1) if size_y is None else size_y
    return f, gridding.setup_algebra(f["K0"], f["K1"], f["R"], f["T"], f["P0cam"], f["P1cam"], PLANE, BASELINE, np.array([0.0, -17.5]),
                                     size_x, size_y, Nx, Ny, IW, IH, z02, z98, **kw)


def test_setup_algebra_on_a_synthetic_rig():
    f, r = _algebra(fps=12.5, timestring="20260101_000000")
    assert set(r) == set(gridding.CONFIG_MAT_KEYS)
    toNorm = np.array([[2.0 / IW, 0, -1, 0], [0, 2.0 / IH, -1, 0], [0, 0, 1, 0], [0, 0, 0, 1.0]])
    corners = np.array([[r["xmin"], r["ymin"]], [r["xmax"], r["ymin"]], [r["xmax"], r["ymax"]], [r["xmin"], r["ymax"]]])
    assert (r["xmin"], r["xmax"]) == (-12.0, 12.0) and r["ymax"] - r["ymin"] == pytest.approx(24.0 * 47 / 63, rel=1e-15)
    # the corners at height 0 through P0plane are where a pinhole camera sees the points of the sea plane they stand for
    g = np.c_[corners, np.zeros(4), np.ones(4)].T
    pix = np.linalg.inv(toNorm) @ r["P0plane"] @ g
    pix = (pix[:2] / pix[2]).T
    Rpl, Tpl = G.sea_plane_RT(PLANE)
    cam = (Rpl.T @ (np.c_[corners / BASELINE, np.zeros(4)].T * np.array([[1.0], [1.0], [-1.0]]) - Tpl)).T     # grid -> camera frame
    assert np.abs(cam @ PLANE[:3] + PLANE[3]).max() < 1e-12                     # they lie on the plane
    want = (f["K0"] @ cam.T).T
    want = want[:, :2] / want[:, 2:]
    assert np.abs(pix - want).max() <= 1e-9 * IW
    # Cam0toGrid: the camera centre stands |d| above the plane, in metres
    c = r["Cam0toGrid"] @ np.array([0, 0, 0, 1.0])
    assert c[3] == 1.0 and abs(c[2] - abs(PLANE[3]) * BASELINE) <= 1e-12 * abs(PLANE[3]) * BASELINE
    c1 = r["Cam1toGrid"] @ np.array([0, 0, 0, 1.0])                             # camera 1 sits one baseline along camera 0's x
    assert abs(np.linalg.norm(c1[:3] - c[:3]) - BASELINE) <= 1e-9
    # the homographies take the projected corners back (both sides as float32, which is what the reference hands to findHomography)
    corners = corners.astype(np.float32).astype(np.float64)
    assert np.abs(_apply(r["Hcam0toGrid"], pix.astype(np.float32)) - corners).max() <= 1e-9 * 24.0
    assert np.abs(_apply(r["Hcam0toTexture"], pix.astype(np.float32)) - np.array([[0, 0], [64, 0], [64, 48], [0, 48]])).max() <= 1e-9 * 64
    pix1 = np.linalg.inv(toNorm) @ r["P1plane"] @ g
    assert np.abs(_apply(r["Hcam1toGrid"], (pix1[:2] / pix1[2]).T.astype(np.float32)) - corners).max() <= 1e-9 * 24.0
    # zmin / zmax: symmetric, the larger magnitude kept
    assert (r["zmin"], r["zmax"]) == (-0.31 * 1.5, 0.31 * 1.5) == G.zrange(-0.31, 0.27)
    r2 = _algebra(z02=-0.1, z98=0.4)[1]
    assert (r2["zmin"], r2["zmax"]) == (-0.4 * 1.5, 0.4 * 1.5) == G.zrange(-0.1, 0.4)
    # the grid, the wavenumbers and the rest
    XX, YY = G.grid_axes(r["xmin"], r["xmax"], r["ymin"], r["ymax"], 64, 48)
    assert np.array_equal(r["XX"], XX) and np.array_equal(r["YY"], YY) and r["XX"].shape == (48, 64)
    KX, KY, sc = G.wavenumbers(64, 48, XX[0, 1] - XX[0, 0], YY[1, 0] - YY[0, 0])
    assert np.array_equal(r["KX_ab"], KX) and np.array_equal(r["KY_ab"], KY) and r["spec_scale"] == sc == 1.0 / (64 * 48)
    assert r["x_spacing"] == XX[0, 1] - XX[0, 0] and r["N"] == 64 and r["CAM_BASELINE"] == r["scale"] == BASELINE
    assert r["P0cam"].shape == (3, 4) and r["Tpl"].shape == (3, 1) and r["RTplane"].shape == (4, 4) and r["fps"] == 12.5
    assert np.allclose(r["RTplane"] @ np.vstack([np.hstack([Rpl, Tpl]), [0, 0, 0, 1]]), np.eye(4), atol=1e-12)
    with pytest.raises(ValueError):
        _algebra(size_x=24.0, size_y=24.0)                                       # spacings 0.38 and 0.51


def test_config_mat_round_trip_into_grid_sequence(tmp_path):
    import scipy.io
    _, r = _algebra(fps=5.0)
    path = str(tmp_path / "config.mat")
    scipy.io.savemat(path, {k: r[k] for k in gridding.CONFIG_MAT_KEYS})
    back = scipy.io.loadmat(path)
    for k in gridding.CONFIG_MAT_KEYS:
        if k != "timestring":
            assert np.array_equal(np.squeeze(back[k]), np.squeeze(np.asarray(r[k], np.float64))), k
    # grid_sequence reads every key it needs from either form and stops at the empty frame list, before the first GPU call
    for setup in (r, path, dict(r, cam0_rectified=None, coverage=0.5)):
        with pytest.raises(ValueError, match="no frames"):
            gridding.grid_sequence([], setup)


def test_gridconfig_files(tmp_path):
    path = gridding.generate_gridconfig(tmp_path)
    assert open(path).read() == "[Area]\narea_center_x=0.0\narea_center_y=-35.0\narea_size=50\nN=1024\n"
    c = gridding.read_gridconfig(path)
    assert c["area_center"].tolist() == [0.0, -35.0] and (c["area_size_x"], c["area_size_y"], c["Nx"], c["Ny"]) == (50.0, 50.0, 1024, 1024)
    other = tmp_path / "rect.txt"
    other.write_text("[Area]\narea_center_x=1.5\narea_center_y=-20\narea_size_x=24\narea_size_y=17.9\nNx=64\nNy=48\narea_size=99\nN=7\n")
    c = gridding.read_gridconfig(other)
    assert c["area_center"].tolist() == [1.5, -20.0] and (c["area_size_x"], c["area_size_y"], c["Nx"], c["Ny"]) == (24.0, 17.9, 64, 48)
    with pytest.raises(FileNotFoundError):
        gridding.read_gridconfig(tmp_path / "absent.txt")


def test_read_opencv_matrix(tmp_path):
    K = np.array([[288.0, 0.0, 160.0], [0.0, 288.125, 120.0], [0.0, 0.0, 1.0]]) * (1 + 2.0 ** -40)
    _write_xml(str(tmp_path / "a.xml"), "intr", K)
    got = gridding.read_opencv_matrix(tmp_path / "a.xml", "intr")
    assert got.dtype == np.float64 and np.array_equal(got, K)
    (tmp_path / "b.xml").write_text('<?xml version="1.0"?>\n<opencv_storage>\n<dist type_id="opencv-matrix">\n  <rows>5</rows>\n  <cols>1</cols>\n'
                                    '  <dt>f</dt>\n  <data>\n    -1.25e-01 2.5e-02\n    0.\n    1.e-03\n    -7.</data></dist>\n'
                                    '<intr type_id="opencv-matrix"><rows>1</rows><cols>2</cols><dt>d</dt><data>1. 2.</data></intr>\n'
                                    '</opencv_storage>\n')
    d = gridding.read_opencv_matrix(tmp_path / "b.xml", "dist")
    assert d.dtype == np.float32 and d.shape == (5, 1) and np.array_equal(d.ravel(), np.array([-0.125, 0.025, 0.0, 1e-3, -7.0], np.float32))
    assert gridding.read_opencv_matrix(tmp_path / "b.xml", "intr").tolist() == [[1.0, 2.0]]
    with pytest.raises(ValueError):
        gridding.read_opencv_matrix(tmp_path / "b.xml", "absent")


def test_mean_plane(tmp_path):
    planes = np.array([[0.1, 0.8, 0.6, -11.0], [np.nan] * 4, [0.3, 0.7, 0.5, -10.0]])
    assert np.array_equal(gridding.mean_plane(planes), np.nanmean(planes, axis=0))
    np.savetxt(tmp_path / "planes.txt", planes)
    assert np.array_equal(gridding.mean_plane(tmp_path / "planes.txt"), np.nanmean(planes, axis=0))


def test_command_line_exit_codes(tmp_path):
    wd, out = tmp_path / "wd", tmp_path / "out"
    write_workdir(str(wd / "000000_wd"))
    np.savetxt(wd / "planes.txt", PLANE.reshape(1, 4))
    out.mkdir()
    run = lambda *a: subprocess.run([sys.executable, "-m", "wass_amd.gridding", *a], cwd=ROOT, capture_output=True, text=True)  # noqa: E731
    p = run(str(wd), str(out), "--action", "generateconfig")
    assert p.returncode == 0 and (out / "gridconfig.txt").exists(), p.stderr
    p = run(str(wd), str(out), "--action", "setup")                             # sys.exit(-1), as the reference
    assert p.returncode == 255 and "--gridconfig" in p.stdout
    # the other codes in this process: the same function, without another interpreter start
    cfg = str(out / "gridconfig.txt")
    assert gridding.main([str(wd), str(tmp_path / "absent"), "--action", "setup", "--gridconfig", cfg]) == -1
    assert gridding.main([str(wd), str(out), "--action", "setup", "--gridconfig", str(out / "absent.txt")]) == -1
    assert gridding.main([str(tmp_path), str(out), "--action", "setup", "--gridconfig", cfg]) == -1        # no frames
    assert gridding.main([str(wd), str(out), "--action", "grid"]) != 0
    assert gridding.main([str(wd), str(out)]) == -2
