"""The LinearND interpolator on the GPU (wass_amd/csrc/grid_linear.hip) against its numpy restatement (tests/linearnd_oracle.py;
tests/test_linearnd.py holds that one to scipy).  Unless a scene says otherwise: the flags equal the oracle's, the values are
bit-equal where both say 0, NaN where both say 1, and the nodes where either side says 2 or 3 are counted -- on the random scenes
they are held to the 1 % that test_linearnd.py asserts of the oracle alone."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import grid_seq_oracle as S
import linearnd_oracle as L
import wass_amd
from test_linearnd import CAP, N, oracle_scene
from wass_amd import gridding, stereo

pytestmark = pytest.mark.gpu


def _gs(ext, W, H, R=np.eye(3), T=np.zeros(3), baseline=1.0):
    return stereo.grid_setup(R, T, baseline, *ext, W, H)


def gpu(ctx, x, y, z, ext, W, H, **options):
    return gridding.linear_nd(np.stack([np.asarray(v, np.float64) for v in (x, y, z)]), _gs(ext, W, H), ctx=ctx, return_flags=True, **options)


def hold(got, ref, cap=None):
    """the comparison of this file's docstring; returns the number of uncertified nodes"""
    out, flags, info = got
    rout, rflags = ref[0], ref[1]
    assert out.shape == rout.shape and out.dtype == np.float64 and flags.dtype == np.uint8
    assert info["counts"] == np.bincount(flags.ravel(), minlength=4).tolist()
    assert info["n_taken"] == ref[3]["n_taken"]
    uncertain = int(((flags >= 2) | (rflags >= 2)).sum())
    assert np.array_equal(flags, rflags), (np.bincount(flags.ravel(), minlength=4), np.bincount(rflags.ravel(), minlength=4))
    both0, both1 = (flags == 0) & (rflags == 0), (flags == 1) & (rflags == 1)
    assert np.array_equal(out[both0], rout[both0])
    assert np.isnan(out[both1]).all() and np.isnan(out[flags == 3]).all()
    if cap is not None:
        assert uncertain <= cap * flags.size
    return uncertain


@functools.lru_cache(maxsize=None)
def cloud(n, seed=2):
    return L.scene("uniform", seed=seed, n=n)


@functools.lru_cache(maxsize=None)
def oracle_cloud(n, W, H):
    return L.interpolate(*cloud(n), *L.UNIT, W, H)


# ---- random scenes; the acceleration grid from one cell (the kernel's own brute force) to far finer than the cloud
@pytest.mark.parametrize("accel", [None, (1, 1), (7, 13), (200, 200)])
@pytest.mark.parametrize("kind", L.SCENES)
def test_random_scenes(gpu_ctx, kind, accel):
    x, y, z, *ref = oracle_scene(kind)
    got = gpu(gpu_ctx, x, y, z, L.UNIT, N, N, accel=accel)
    hold(got, ref, cap=CAP)
    if accel is not None:
        assert got[2]["accel"] == accel
    assert got[2]["status"] == 0 and 3 <= got[2]["hull_vertices"] <= got[2]["hull_candidates"] <= 5120


# ---- lattices on both sides of the 8 x 8 patch and of the last partial workgroup
@pytest.mark.parametrize("W,H", [(1, 1), (1, 7), (7, 1), (2, 2), (8, 8), (9, 7), (33, 65), (64, 64)])
def test_lattices(gpu_ctx, W, H):
    hold(gpu(gpu_ctx, *cloud(300), L.UNIT, W, H), oracle_cloud(300, W, H))


@pytest.mark.parametrize("n", [0, 1, 2, 3, 4, 7, 300, 5000])
def test_cloud_sizes(gpu_ctx, n):
    ref = oracle_cloud(n, 9, 7)
    got = gpu(gpu_ctx, *cloud(n), L.UNIT, 9, 7)
    hold(got, ref)
    assert got[2]["status"] == (-6 if n < 3 else 0) and ref[3]["too_few"] == (n < 3)
    if n < 3:
        assert got[2]["counts"] == [0, 63, 0, 0]


def test_order_independence_and_repeatability(gpu_ctx):
    x, y, z, *ref = oracle_scene("clump")
    first = gpu(gpu_ctx, x, y, z, L.UNIT, N, N)
    again = gpu(gpu_ctx, x, y, z, L.UNIT, N, N)
    assert np.array_equal(first[0], again[0], equal_nan=True) and np.array_equal(first[1], again[1])
    perm = np.random.default_rng(11).permutation(x.size)
    moved = gpu(gpu_ctx, x[perm], y[perm], z[perm], L.UNIT, N, N)
    assert np.array_equal(moved[1], first[1])
    # the same triangles; the canonical order of the vertices follows the indices, so the last bit may move
    m = first[1] == 0
    assert (np.abs(moved[0][m] - first[0][m]) <= L.value_bound(x, y, z, ref[2][m])).all()
    # and bit for bit what the definition gives for the permuted cloud
    inv = np.argsort(perm)
    for r, c in zip(*np.nonzero(m)):
        tri = inv[ref[2][r, c]]
        f, v = L.certify(x[perm], y[perm], z[perm], tri, *(np.linspace(0, 1, N)[c], np.linspace(0, 1, N)[r]))
        assert f == 0 and v == moved[0][r, c]
    assert moved[2]["n_taken"] == first[2]["n_taken"] == ref[3]["n_taken"] and moved[2]["counts"] == first[2]["counts"]


# ---- exact cases
def test_three_points_vertices_midpoints_centroid(gpu_ctx):
    x, y, z = np.array([0.0, 6.0, 0.0]), np.array([0.0, 0.0, 6.0]), np.array([1.0, 7.0, -5.0])
    ext = (0.0, 6.0, 0.0, 6.0)
    ref = L.interpolate(x, y, z, *ext, 7, 7)
    out, flags, info = got = gpu(gpu_ctx, x, y, z, ext, 7, 7)
    hold(got, ref)
    for (c, r), v in {(0, 0): 1.0, (6, 0): 7.0, (0, 6): -5.0, (3, 0): 4.0, (0, 3): -2.0, (2, 2): 1.0}.items():
        assert flags[r, c] == 0 and out[r, c] == v                                   # on the axes and inside: certified, small integers: exact
    assert flags[3, 3] == 2 and out[3, 3] == 1.0                                     # on the slanted hull edge: within the bound of it
    assert (flags[np.add.outer(np.arange(7), np.arange(7)) > 6] == 1).all()


def test_node_on_a_cloud_point(gpu_ctx):
    x, y, z = (v.copy() for v in cloud(300))
    q = np.linspace(0.0, 1.0, 9)
    for k, (c, r) in enumerate(((4, 3), (2, 5), (6, 1))):
        x[k], y[k] = q[c], np.linspace(0.0, 1.0, 7)[r]
    ref = L.interpolate(x, y, z, *L.UNIT, 9, 7)
    out, flags, info = got = gpu(gpu_ctx, x, y, z, L.UNIT, 9, 7)
    hold(got, ref)
    for k, (c, r) in enumerate(((4, 3), (2, 5), (6, 1))):
        assert flags[r, c] == 0 and abs(out[r, c] - z[k]) <= 4 * L.EPS * abs(z[k])  # one weight is 1, two are 0: a product and a quotient


def test_duplicates_area_border_and_bad_coordinates(gpu_ctx):
    # duplicates of half the cloud with another z, behind the originals: the lower index stands
    x, y, z = L.scene("uniform", seed=3, n=300)
    x, y, z = np.r_[x, x[:150]], np.r_[y, y[:150]], np.r_[z, z[:150] + 1.0]
    hold(gpu(gpu_ctx, x, y, z, L.UNIT, 9, 7, accel=(3, 3)), L.interpolate(x, y, z, *L.UNIT, 9, 7))
    # ... and in front of them
    hold(gpu(gpu_ctx, x[::-1], y[::-1], z[::-1], L.UNIT, 9, 7), L.interpolate(x[::-1], y[::-1], z[::-1], *L.UNIT, 9, 7))
    # points on the border of the area, one ulp outside it, NaN and infinite coordinates
    x, y, z = L.scene("uniform", seed=5, n=200)
    x[:40], y[40:80] = np.repeat([0.0, 1.0], 20), np.repeat([0.0, 1.0], 20)
    x[80:84] = [np.nextafter(0.0, -1.0), np.nextafter(1.0, 2.0), 0.5, 0.5]
    y[82:84] = [np.nextafter(0.0, -1.0), np.nextafter(1.0, 2.0)]
    x[84:87], y[87:90] = [np.nan, np.inf, -np.inf], [np.nan, np.inf, -np.inf]
    z[90] = np.nan                                                                    # a height is not a coordinate: the point stands
    ref = L.interpolate(x, y, z, *L.UNIT, 9, 7)
    assert ref[3]["n_taken"] == 190
    hold(gpu(gpu_ctx, x, y, z, L.UNIT, 9, 7), ref)


def test_collinear_cloud(gpu_ctx):
    t = np.arange(1, 8) / 8.0                                                         # dyadic: exactly collinear in fp64
    out, flags, info = gpu(gpu_ctx, t, 0.5 * t + 0.125, t, L.UNIT, 5, 4)
    assert info["status"] == -6 and np.isnan(out).all() and (flags == 1).all() and info["counts"] == [0, 20, 0, 0] and info["n_taken"] == 7


def test_square_lattice(gpu_ctx):
    x, y, z = L.square_lattice(6)
    ext = (-0.75, 5.75, -0.75, 5.75)
    out, flags, info = got = gpu(gpu_ctx, x, y, z, ext, 14, 14)
    hold(got, L.interpolate(x, y, z, *ext, 14, 14))
    XX, YY = np.meshgrid(*L.nodes(*ext, 14, 14))
    outside = (XX < 0) | (XX > 5) | (YY < 0) | (YY > 5)
    assert np.array_equal(flags == 1, outside) and (flags[~outside] == 2).all()
    assert np.abs(out[~outside] - (2.0 * XX - 3.0 * YY + 1.0)[~outside]).max() <= 16 * L.EPS * 25 * 2


# ---- entries
def test_mesh_entry_host_entry_and_argument_errors(gpu_ctx):
    import torch
    rng = np.random.default_rng(21)
    plane = np.array([0.02, 0.81, 0.586, -11.0]); plane[:3] /= np.linalg.norm(plane[:3])
    R, T, _, _ = wass_amd.RT_from_plane(plane)
    n, W, H, b = 3000, 33, 17, 2.5
    p = np.stack([rng.uniform(-6, 6, n), rng.uniform(-3, 3, n), np.zeros(n)])
    p[2] = (-plane[3] - plane[0] * p[0] - plane[1] * p[1]) / plane[2] + 0.05 * np.sin(2.0 * p[0])
    R, T = np.asarray(R, np.float64).reshape(3, 3), np.asarray(T, np.float64).ravel()
    al = [(R[k, 0] * p[0] + R[k, 1] * p[1] + R[k, 2] * p[2] + T[k]) * b for k in range(3)]      # grid_align_bin's expressions
    al[2] = -al[2]
    ext = (float(np.quantile(al[0], 0.1)), float(np.quantile(al[0], 0.9)), float(np.quantile(al[1], 0.05)), float(np.quantile(al[1], 0.8)))
    gs = _gs(ext, W, H, R, T, b)
    want = gridding.linear_nd(np.stack(al), gs, ctx=gpu_ctx, return_flags=True)
    assert want[2]["counts"][0] > 300 and 1000 < want[2]["n_taken"] < n
    dev = torch.device("cuda", gpu_ctx.device_id)
    d_out = torch.empty((H, W), dtype=torch.float64, device=dev)
    d_flags = torch.empty((H, W), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    mesh = gridding.upload_camera_mesh(gpu_ctx, p)
    info = mesh.grid_linear_dev(gs, d_out, d_flags)
    mesh.close()
    assert info == want[2]
    assert np.array_equal(d_out.cpu().numpy(), want[0], equal_nan=True) and np.array_equal(d_flags.cpu().numpy(), want[1])
    # host arrays
    lib, out, flags, counts = gpu_ctx._lib, np.empty((H, W)), np.empty((H, W), np.uint8), (C.c_uint64 * 4)()
    a = [np.ascontiguousarray(v) for v in al]
    call = lambda g, xs=a[0], o=out: lib.wass_grid_linear(gpu_ctx._h, xs.ctypes.data if xs is not None else None, a[1].ctypes.data, a[2].ctypes.data,
                                                          n, C.byref(g), o.ctypes.data if o is not None else None, flags.ctypes.data, counts)
    assert call(gs) == 0
    assert np.array_equal(out, want[0], equal_nan=True) and np.array_equal(flags, want[1]) and list(counts) == want[2]["counts"]
    # argument errors
    for bad in (_gs(ext, 0, H), _gs(ext, W, 0), _gs((ext[1], ext[0], ext[2], ext[3]), W, H), _gs((ext[0], ext[0], ext[2], ext[3]), W, H),
                _gs((ext[0], ext[1], ext[3], ext[3]), W, H)):
        assert call(bad) == -1
    assert call(gs, xs=None) == -1 and call(gs, o=None) == -1
    assert call(_gs((ext[0], ext[0], ext[2], ext[3]), 1, H)) in (0, -6)              # one column: xmax == xmin is no error


def _frames_on_disk(tmp_path, oracle, plane):
    rng = np.random.default_rng(900)
    w, h, dirs = 60, 40, []
    for i in range(3):
        X = rng.uniform(-6, 6, (h, w)); Y = rng.uniform(-3, 3, (h, w))
        Z = (-plane[3] - plane[0] * X - plane[1] * Y) / plane[2] + 0.05 * np.sin(X * 2.0 + 0.3 * i)
        valid = (rng.random((h, w)) < 0.7).astype(np.uint8) * (i != 1)               # the middle frame is empty
        d = tmp_path / ("%06d_wd" % (2 * i + 4))
        d.mkdir()
        (d / "mesh_cam.xyzC").write_bytes(oracle.encode_xyzc(valid, np.ascontiguousarray(np.stack([X, Y, Z], axis=-1)), plane))
        dirs.append(str(d))
    return dirs


def test_grid_sequence_linear_nd(gpu_ctx, oracle, tmp_path):
    import torch
    from wass_amd.gridding import grid_sequence, load_camera_mesh, upload_camera_mesh
    plane = np.array([0.02, 0.81, 0.586, -11.0]); plane[:3] /= np.linalg.norm(plane[:3])
    dirs = _frames_on_disk(tmp_path, oracle, plane)
    R, T, _, _ = wass_amd.RT_from_plane(plane)
    W, H = 48, 40                                                                     # the cloud covers about a quarter of this extent
    setup = {"Rpl": R, "Tpl": T.reshape(3, 1), "CAM_BASELINE": np.array([[2.5]]), "xmin": np.array([[-12.0]]), "xmax": np.array([[12.0]]),
             "ymin": np.array([[-30.0]]), "ymax": np.array([[-5.0]]), "XX": np.zeros((H, W)), "fps": np.array([[12.5]])}
    um = np.ones((H, W), np.uint8); um[:, :3] = 0
    res = grid_sequence(dirs, setup, user_mask=um * 255, ctx=gpu_ctx, algorithm="LinearND")
    gs = stereo.grid_setup(R, T, 2.5, -12.0, 12.0, -30.0, -5.0, W, H)
    dev = torch.device("cuda", gpu_ctx.device_id)
    d_out, d_flags = torch.empty((H, W), dtype=torch.float64, device=dev), torch.empty((H, W), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    zi, infos = [], []
    for d in dirs:
        mesh = upload_camera_mesh(gpu_ctx, load_camera_mesh(os.path.join(d, "mesh_cam.xyzC")))
        info = mesh.grid_linear_dev(gs, d_out, d_flags)
        mesh.close()
        f = d_out.cpu().numpy().astype(np.float32)                                    # the one rounding
        f[um == 0] = np.nan
        zi.append(f); infos.append({"counts": info["counts"], "n_taken": info["n_taken"]})
    assert infos[0]["counts"][0] > 100 and infos[1] == {"counts": [0, W * H, 0, 0], "n_taken": 0}
    zi = np.stack(zi)
    want = S.sequence_stats(zi)
    assert res.linear_info == infos and res.dct_info == [] and res.empty_frames == [1]
    assert np.array_equal(res.Z, want["z_mm"], equal_nan=True) and np.isnan(res.Z[1]).all() and np.isnan(res.Z[:, :, :3]).all()
    # the empty frame's minimum and maximum are NaN and go into zmin and zmax, as np.min over the frames does in the reference
    assert np.array_equal([res.zmin, res.zmax], [want["zmin"], want["zmax"]], equal_nan=True)
    assert np.array_equal(res.frame_min, want["frame_min"], equal_nan=True) and np.array_equal(res.frame_max, want["frame_max"], equal_nan=True)
    assert np.array_equal(res.mean_perpoint_mm, want["mean_perpoint_mm"], equal_nan=True)
    assert res.workdir.tolist() == [4, 6, 8]
    # --force-zero-mean, on the two frames that hold data (an empty frame makes the per-point mean NaN everywhere); several
    # frames go through the pass in slices of one, whatever `batch` says
    for batch in (8, 1):
        zm = grid_sequence(dirs[::2], setup, user_mask=um * 255, ctx=gpu_ctx, algorithm="LinearND", force_zero_mean=True, batch=batch)
        wz = S.sequence_stats(zi[::2], force_zero_mean=True)
        assert np.array_equal(zm.Z, S.zero_mean(wz["z_mm"], wz["mean_perpoint_mm"]), equal_nan=True) and np.isfinite(zm.Z).sum() > 200
        assert np.array_equal(zm.mean_perpoint_mm, wz["mean_perpoint_mm"], equal_nan=True)
        assert zm.zmin == wz["zmin"] and zm.zmax == -wz["zmin"] and zm.zmean == 0.0
        assert zm.linear_info == infos[::2] and zm.empty_frames == []
    for kw in (dict(mf=3), dict(refine=object())):
        with pytest.raises(ValueError, match="LinearND"):
            grid_sequence(dirs, setup, ctx=gpu_ctx, algorithm="LinearND", **kw)
    with pytest.raises(ValueError):
        grid_sequence(dirs, setup, ctx=gpu_ctx, algorithm="IDW")
    # DCT, named or not, is what it was
    opts = {"Nfreqs": 8, "MAX_ITERS": 60}
    a = grid_sequence(dirs[::2], setup, mf=3, alg_options=opts, ctx=gpu_ctx)
    b = grid_sequence(dirs[::2], setup, mf=3, alg_options=opts, ctx=gpu_ctx, algorithm="DCT")
    assert np.array_equal(a.Z, b.Z, equal_nan=True) and a.dct_info == b.dct_info and a.linear_info is None and b.linear_info is None
    assert a.zmean == b.zmean and a.empty_frames == b.empty_frames == []


# ---- caps
def test_walk_step_cap(gpu_ctx):
    """Most walks of this scene take more than two steps: with the cap lowered to two those nodes carry flag 3 and NaN, the others are
    what they were, and the call returns.  The oracle's walk takes the same steps (every choice in it is determined)."""
    x, y, z, *full = oracle_scene("hole")
    ref = L.interpolate(x, y, z, *L.UNIT, N, N, max_steps=2)
    n3 = int((ref[1] == 3).sum())
    assert 100 < n3 < (full[1] == 0).sum()
    got = gpu(gpu_ctx, x, y, z, L.UNIT, N, N, max_walk_steps=2)
    hold(got, ref)
    assert got[2]["counts"][3] == n3
    kept = ref[1] == 0
    assert np.array_equal(got[0][kept], full[0][kept])
