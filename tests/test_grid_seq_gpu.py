"""The sequence layer of the gridding stage on the GPU: the batched DCT solve against single solves (bit for bit: a frame keeps the
order of every sum whatever batch it is solved in), the --mf median filter and the sequence accumulator against their numpy
restatements (tests/grid_seq_oracle.py), and grid_sequence end to end against the same frames taken one by one."""
import ctypes as C
import os

import numpy as np
import pytest

import grid_seq_oracle as S
import wass_amd
from test_grid_dct_gpu import band_limited

pytestmark = pytest.mark.gpu

INFO_KEYS = ("steps", "converged", "data_loss", "reg_loss", "fdelta")


def _maps(h, w, n, seed0):
    return np.stack([band_limited(h, w, seed=seed0 + i, keep=0.5 + 0.04 * i) for i in range(n)])


def _assert_frame_equals_single(bg, bc, bi, k, sg, sc, si):
    assert np.array_equal(bg[k], sg, equal_nan=True), f"grid of frame {k}"
    assert np.array_equal(bc[k], sc), f"coefficients of frame {k}"
    for key in INFO_KEYS:
        assert bi[k][key] == si[key], (k, key, bi[k][key], si[key])


# ---- 1. batch equals singles
SIZES = [(64, 64, 16, 120), (96, 128, 24, 120), (136, 200, 40, 120), (512, 512, 150, 100)]     # h, w, Nfreqs, MAX_ITERS


@pytest.mark.parametrize("h,w,nf,iters", SIZES)
def test_batch_equals_singles(gpu_ctx, h, w, nf, iters):
    import torch
    zz = _maps(h, w, 8, seed0=100 + h)
    rng = np.random.default_rng(h + w)
    x0 = rng.random((8, nf, nf)).astype(np.float32)
    um = (rng.random((h, w)) < 0.85).astype(np.uint8)
    opts = {"Nfreqs": nf, "MAX_ITERS": iters}
    variants = {"seeded": dict(x0=None, user_mask=None), "x0+mask": dict(x0=x0, user_mask=um)}
    for name, v in variants.items():
        singles = [gpu_ctx.grid_dct(zz[i], opts, x0=None if v["x0"] is None else v["x0"][i], user_mask=v["user_mask"], seed=7)
                   for i in range(8)]
        assert len({s[2]["data_loss"] for s in singles}) == 8                   # distinct problems
        for nb in (1, 3, 8):
            bg, bc, bi, st = gpu_ctx.grid_dct_batch(zz[:nb], opts, x0=None if v["x0"] is None else v["x0"][:nb],
                                                    user_mask=v["user_mask"], seed=7)
            assert bg.shape == (nb, h, w) and bc.shape == (nb, nf, nf) and (st == 0).all()
            for k in range(nb):
                _assert_frame_equals_single(bg, bc, bi, k, *singles[k])
        # the device entry, on the largest batch
        dev = torch.device("cuda", gpu_ctx.device_id)
        d_zz = torch.from_numpy(zz).to(dev)
        d_out = torch.empty_like(d_zz)
        d_co = torch.empty((8, nf, nf), dtype=torch.float32, device=dev)
        d_x0 = None if v["x0"] is None else torch.from_numpy(v["x0"]).to(dev)
        d_um = None if v["user_mask"] is None else torch.from_numpy(v["user_mask"]).to(dev)
        torch.cuda.synchronize(dev)
        bi, st = gpu_ctx.grid_dct_batch_dev(d_zz, d_out, opts, d_x0=d_x0, d_user_mask=d_um, d_coeffs=d_co, seed=7)
        bg, bc = d_out.cpu().numpy(), d_co.cpu().numpy()
        assert (st == 0).all()
        for k in range(8):
            _assert_frame_equals_single(bg, bc, bi, k, *singles[k])


# ---- 2. frames stop on their own
def test_frames_stop_on_their_own(gpu_ctx):
    n, nf = 64, 16
    rng = np.random.default_rng(3)
    zz = np.stack([np.full((n, n), 0.3, np.float32), band_limited(n, n, 1), band_limited(n, n, 2),
                   rng.normal(0, 1, (n, n)).astype(np.float32), band_limited(n, n, 4)])
    x0 = np.broadcast_to(np.random.default_rng(9).random((nf, nf)).astype(np.float32), (5, nf, nf)).copy()
    opts = {"Nfreqs": nf, "MAX_ITERS": 500, "TOLERANCE_CHANGE": 1e-2}
    singles = [gpu_ctx.grid_dct(zz[i], opts, x0=x0[i]) for i in range(5)]
    steps = [s[2]["steps"] for s in singles]
    assert len(set(steps)) >= 2, steps                              # otherwise this test shows nothing
    assert any(s[2]["converged"] for s in singles)
    for order in (np.arange(5), np.arange(5)[::-1]):
        bg, bc, bi, st = gpu_ctx.grid_dct_batch(zz[order], opts, x0=x0[order])
        assert (st == 0).all()
        assert [i["steps"] for i in bi] == [steps[j] for j in order]
        for k, j in enumerate(order):
            _assert_frame_equals_single(bg, bc, bi, k, *singles[j])


# ---- 3. frames without data
def test_empty_frame_in_the_middle_and_all_empty(gpu_ctx):
    h, w, nf = 80, 112, 20
    zz = _maps(h, w, 3, seed0=300)
    zz[1] = np.nan
    opts = {"Nfreqs": nf, "MAX_ITERS": 60}
    bg, bc, bi, st = gpu_ctx.grid_dct_batch(zz, opts, seed=2)
    assert st.tolist() == [0, -6, 0]
    assert np.isnan(bg[1]).all() and np.isnan(bc[1]).all()
    assert bi[1] == {"steps": 0, "converged": False, "data_loss": 0.0, "reg_loss": 0.0, "fdelta": 0.0}
    for k in (0, 2):
        _assert_frame_equals_single(bg, bc, bi, k, *gpu_ctx.grid_dct(zz[k], opts, seed=2))
    bg, _, bi, st = gpu_ctx.grid_dct_batch(np.full((2, h, w), np.nan, np.float32), opts)
    assert st.tolist() == [-6, -6] and np.isnan(bg).all() and all(i["steps"] == 0 for i in bi)
    # argument errors as in the single call
    o = wass_amd.stereo.dct_opts(opts)
    buf = np.zeros((1, h, w), np.float32)
    status = (C.c_int * 1)()
    rc = gpu_ctx._lib.wass_grid_dct_batch(gpu_ctx._h, buf.ctypes.data, 0, w, h, C.byref(o), None, None, buf.ctypes.data, None, None, status)
    assert rc == -1
    with pytest.raises(wass_amd.WassError) as e:
        gpu_ctx.grid_dct_batch(zz, {"Nfreqs": h + 1})
    assert e.value.code == -1


# ---- 4. scratch reuse
def test_scratch_reuse_across_shapes(gpu_ctx):
    big = _maps(200, 136, 8, seed0=400)
    small = _maps(48, 64, 2, seed0=450)
    ob, os_ = {"Nfreqs": 40, "MAX_ITERS": 70}, {"Nfreqs": 12, "MAX_ITERS": 70}
    a = gpu_ctx.grid_dct_batch(big, ob)
    b = gpu_ctx.grid_dct_batch(small, os_)
    c = gpu_ctx.grid_dct_batch(big, ob)
    assert np.array_equal(a[0], c[0]) and np.array_equal(a[1], c[1]) and a[2] == c[2]
    for k in range(2):
        _assert_frame_equals_single(b[0], b[1], b[2], k, *gpu_ctx.grid_dct(small[k], os_))


# ---- 5. the --mf median filter
@pytest.mark.parametrize("k", [3, 5])
@pytest.mark.parametrize("shape", [(1, 9), (37, 53), (512, 512)])
def test_median_equals_oracle(gpu_ctx, k, shape):
    rng = np.random.default_rng(k + shape[1])
    z = rng.normal(0, 0.4, (3,) + shape).astype(np.float32)
    z[:, rng.random(shape) < 0.02] = 0.25                           # ties
    mask = (rng.random(shape) < 0.8).astype(np.uint8)
    got = gpu_ctx.grid_median(z, k)
    assert got.dtype == np.float32 and np.array_equal(got, S.median_blur(z, k))
    zm = z.copy(); zm[:, mask == 0] = np.nan                        # what the solve hands over under a user mask
    got = gpu_ctx.grid_median(zm, k, mask)
    assert np.array_equal(got, S.median_blur(zm, k, mask), equal_nan=True)
    assert np.array_equal(np.isnan(got), np.broadcast_to(mask == 0, got.shape))
    assert np.array_equal(gpu_ctx.grid_median(z[0], k), S.median_blur(z[0], k))          # one map


def test_median_sizes_the_reference_cannot_run_are_refused(gpu_ctx):
    z = np.zeros((2, 16, 16), np.float32)
    for bad in (7, 4, 1, -3):
        with pytest.raises(wass_amd.WassError) as e:
            gpu_ctx.grid_median(z, bad)
        assert e.value.code == -1 and "medianBlur" in str(e.value)
    m = np.ones((16, 16), np.uint8); m[3] = 0
    assert np.array_equal(gpu_ctx.grid_median(z + 1, 0, m), S.median_blur(z + 1, 0, m), equal_nan=True)


# ---- 6. the accumulator
def _push_all(ctx, frames, splits, force_zero_mean):
    import torch
    from wass_amd.stereo import GridSequence
    dev = torch.device("cuda", ctx.device_id)
    n, h, w = frames.shape
    d_z = torch.from_numpy(frames).to(dev)
    d_mm = torch.empty_like(d_z)
    torch.cuda.synchronize(dev)
    seq = GridSequence(ctx, w, h)
    i = 0
    for s in splits:
        seq.push_dev(d_z[i:i + s], d_mm[i:i + s])
        i += s
    assert i == n
    st = seq.finish(force_zero_mean)
    mm = d_mm.cpu().numpy()
    seq.zero_mean_dev(d_mm)
    ctx.synchronize()
    zero = d_mm.cpu().numpy()
    seq.close()
    return st, mm, zero


def _check_against_oracle(st, mm, zero, frames, force_zero_mean):
    """Exact: min / max, the per-point mean, the millimetre slices, the zero-mean cube.  The per-frame mean is an fp64 sum of n
    float32 values taken in another order than numpy's: each of the two sums is off by at most (n - 1) u sum|z| to first order
    (u = 2^-53, one rounding per addition, each bounded by u times a partial sum <= sum|z|), the division adds u |mean| each, so
    |delta| <= 2 (n - 1 + 1) u sum|z| / n = n 2^-52 mean|z|.  zmean is the mean of N such values summed in fp64 in either order:
    the same argument with N terms on top of the largest per-frame bound."""
    want = S.sequence_stats(frames, force_zero_mean)
    eq = lambda a, b: np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)     # noqa: E731
    assert eq(st["frame_min"], want["frame_min"]) and eq(st["frame_max"], want["frame_max"])
    assert eq(st["zmin"], want["zmin"]) and eq(st["zmax"], want["zmax"])
    assert eq(st["mean_perpoint_mm"], want["mean_perpoint_mm"])
    assert st["mean_perpoint_mm"].dtype == np.float64
    assert mm.dtype == np.float32 and eq(mm, want["z_mm"])
    assert eq(zero, S.zero_mean(want["z_mm"], want["mean_perpoint_mm"]))
    assert st["n_frames"] == len(frames)
    bounds = []
    for f, (g, r) in enumerate(zip(st["frame_mean"], want["frame_mean"])):
        ok = ~np.isnan(frames[f])
        n = int(ok.sum())
        if n == 0:
            assert np.isnan(g) and np.isnan(r)
            bounds.append(0.0)
            continue
        bound = n * 2.0 ** -52 * float(np.mean(np.abs(frames[f][ok].astype(np.float64))))
        print(f"frame {f}: mean {g!r} oracle {r!r} |delta| {abs(g - r):.3e} bound {bound:.3e}")
        assert abs(g - r) <= bound
        bounds.append(bound)
    if force_zero_mean:
        assert st["zmean"] == 0.0
    elif np.isnan(want["zmean"]):
        assert np.isnan(st["zmean"])
    else:
        nfr = len(frames)
        zb = max(bounds) + nfr * 2.0 ** -52 * float(np.mean(np.abs(want["frame_mean"])))
        print(f"zmean {st['zmean']!r} oracle {want['zmean']!r} bound {zb:.3e}")
        assert abs(st["zmean"] - want["zmean"]) <= zb


@pytest.mark.parametrize("force_zero_mean", [False, True])
def test_accumulator_equals_oracle_and_does_not_depend_on_the_split(gpu_ctx, force_zero_mean):
    h, w = 150, 210
    rng = np.random.default_rng(77)
    frames = np.stack([0.3 * band_limited(h, w, seed=500 + i, keep=1.0) + np.float32(rng.normal(0, 0.02)) for i in range(11)])
    mask = np.ones((h, w), bool); mask[:, 17] = False; mask[:5] = False
    frames[:, ~mask] = np.nan
    frames[:, mask] = np.nan_to_num(frames[:, mask], nan=0.125)      # data everywhere inside the mask, as after the interpolator
    a = _push_all(gpu_ctx, frames, (4, 4, 3), force_zero_mean)
    b = _push_all(gpu_ctx, frames, (1,) * 11, force_zero_mean)
    for k in ("zmin", "zmax", "zmean", "mean_perpoint_mm", "frame_mean", "frame_min", "frame_max"):
        assert np.array_equal(np.asarray(a[0][k]), np.asarray(b[0][k]), equal_nan=True), k
    assert np.array_equal(a[1], b[1], equal_nan=True) and np.array_equal(a[2], b[2], equal_nan=True)
    _check_against_oracle(*a, frames, force_zero_mean)


@pytest.mark.parametrize("w,h", [(257, 300), (1024, 1024)])
def test_accumulator_equals_oracle_above_65536_cells(gpu_ctx, w, h):
    """k_seq_stats runs at most 256 workgroups of 256 threads: only a map of more than 65 536 cells sends its grid-stride loop
    round a second time (77 100 cells: a second turn for some threads only; 1024 x 1024: sixteen turns for all)."""
    rng = np.random.default_rng(w)
    frames = np.stack([0.3 * band_limited(h, w, seed=600 + i, keep=1.0) + np.float32(rng.normal(0, 0.02)) for i in range(3)])
    mask = np.ones((h, w), bool); mask[:, 17] = False; mask[h - 3] = False
    frames[:, ~mask] = np.nan
    frames[:, mask] = np.nan_to_num(frames[:, mask], nan=0.125)
    for fzm in (False, True):
        a = _push_all(gpu_ctx, frames, (2, 1), fzm)
        b = _push_all(gpu_ctx, frames, (1, 1, 1), fzm)
        for k in ("zmin", "zmax", "zmean", "mean_perpoint_mm", "frame_mean", "frame_min", "frame_max"):
            assert np.array_equal(np.asarray(a[0][k]), np.asarray(b[0][k]), equal_nan=True), k
        assert np.array_equal(a[1], b[1], equal_nan=True) and np.array_equal(a[2], b[2], equal_nan=True)
        _check_against_oracle(*a, frames, fzm)


def test_accumulator_nan_cases(gpu_ctx):
    a = np.array([[1.0, 2.0, np.nan], [3.0, -4.0, np.nan]], np.float32)
    b = np.array([[0.5, 0.5, np.nan], [0.5, 0.5, np.nan]], np.float32)
    _check_against_oracle(*_push_all(gpu_ctx, np.stack([a, b]), (2,), False), np.stack([a, b]), False)
    frames = np.stack([a, np.full_like(a, np.nan), b])
    st, mm, zero = _push_all(gpu_ctx, frames, (1, 2), False)
    assert np.isnan(st["zmin"]) and np.isnan(st["zmax"]) and np.isnan(st["zmean"]) and np.isnan(st["mean_perpoint_mm"]).all()
    _check_against_oracle(st, mm, zero, frames, False)
    # zero_mean before finish is refused
    import torch
    from wass_amd.stereo import GridSequence
    seq = GridSequence(gpu_ctx, 3, 2)
    d = torch.from_numpy(a).to(torch.device("cuda", gpu_ctx.device_id)); torch.cuda.synchronize()
    seq.push_dev(d)
    with pytest.raises(wass_amd.WassError):
        seq.zero_mean_dev(d)
    seq.close()


# ---- 7. grid_sequence end to end
def _sequence_on_disk(tmp_path, oracle, n_frames, plane):
    rng = np.random.default_rng(900)
    w, h = 120, 90
    dirs = []
    for i in range(n_frames):
        X = rng.uniform(-6, 6, (h, w)); Y = rng.uniform(-3, 3, (h, w))
        Z = (-plane[3] - plane[0] * X - plane[1] * Y) / plane[2] + 0.05 * np.sin(X * 2.0 + 0.3 * i) + 0.03 * np.cos(Y * 3.0 - 0.2 * i)
        valid = (rng.random((h, w)) < 0.7).astype(np.uint8)
        d = tmp_path / ("%06d_wd" % (3 * i + 5))
        d.mkdir()
        (d / "mesh_cam.xyzC").write_bytes(oracle.encode_xyzc(valid, np.ascontiguousarray(np.stack([X, Y, Z], axis=-1)), plane))
        dirs.append(str(d))
    return dirs


def test_grid_sequence_end_to_end(gpu_ctx, oracle, tmp_path):
    from wass_amd.gridding import grid_sequence, load_camera_mesh, upload_camera_mesh
    plane = np.array([0.02, 0.81, 0.586, -11.0]); plane[:3] /= np.linalg.norm(plane[:3])
    dirs = _sequence_on_disk(tmp_path, oracle, 10, plane)
    R, T, _, _ = wass_amd.RT_from_plane(plane)
    W, H = 96, 80
    args = dict(baseline=2.5, xmin=-12.0, xmax=12.0, ymin=-30.0, ymax=-5.0, width=W, height=H)
    setup = {"Rpl": R, "Tpl": T.reshape(3, 1), "CAM_BASELINE": np.array([[2.5]]), "xmin": np.array([[-12.0]]), "xmax": np.array([[12.0]]),
             "ymin": np.array([[-30.0]]), "ymax": np.array([[-5.0]]), "XX": np.zeros((H, W)), "fps": np.array([[12.5]])}
    opts = {"Nfreqs": 40, "MAX_ITERS": 120}
    um = np.ones((H, W), np.uint8); um[:, :6] = 0; um[70:, 90:] = 0
    res = grid_sequence(dirs, setup, mf=3, user_mask=um * 255, alg_options=opts, force_zero_mean=True, batch=4, ctx=gpu_ctx)
    # the same frames one by one through the existing single path, then numpy
    zi, infos = [], []
    for d in dirs:
        mesh = upload_camera_mesh(gpu_ctx, load_camera_mesh(os.path.join(d, "mesh_cam.xyzC")))
        g, cells, _, info = mesh.grid_dct(plane, **args, cell="median", dct_options=opts, user_mask=um)
        assert np.isfinite(cells).sum() > 500
        zi.append(S.median_blur(g, 3, um)); infos.append(info)
    zi = np.stack(zi)
    want = S.sequence_stats(zi, force_zero_mean=True)
    assert res.Z.dtype == np.float32 and res.Z.shape == (10, H, W)
    assert np.array_equal(res.Z, S.zero_mean(want["z_mm"], want["mean_perpoint_mm"]), equal_nan=True)
    assert np.array_equal(np.isnan(res.Z), np.broadcast_to(um == 0, res.Z.shape))
    assert np.array_equal(res.mean_perpoint_mm, want["mean_perpoint_mm"], equal_nan=True)
    assert res.zmin == want["zmin"] and res.zmax == -want["zmin"] and res.zmean == 0.0
    assert np.array_equal(res.frame_min, want["frame_min"]) and np.array_equal(res.frame_max, want["frame_max"])
    assert res.dct_info == infos and res.empty_frames == []
    assert res.workdir.tolist() == [3 * i + 5 for i in range(10)]
    assert np.array_equal(res.time, np.arange(10) / 12.5)
    # without the zero-mean pass and the filter, into a caller's array, with another batch size: the plain cube
    out = np.zeros((10, H, W), np.float32)
    res2 = grid_sequence(dirs, setup, alg_options=opts, batch=3, ctx=gpu_ctx, out=out)
    assert res2.Z is out
    singles = np.stack([upload_camera_mesh(gpu_ctx, load_camera_mesh(os.path.join(d, "mesh_cam.xyzC"))).grid_dct(
        plane, **args, cell="median", dct_options=opts)[0] for d in dirs])
    assert np.array_equal(out, singles * np.float32(1000))
    w2 = S.sequence_stats(singles)
    assert res2.zmin == w2["zmin"] and res2.zmax == w2["zmax"]
    # the bound derived in _check_against_oracle: the largest per-frame bound plus the N-term sum of the frame means
    zb = max(np.isfinite(f).sum() * 2.0 ** -52 * float(np.mean(np.abs(f[np.isfinite(f)].astype(np.float64)))) for f in singles) \
        + 10 * 2.0 ** -52 * float(np.mean(np.abs(w2["frame_mean"])))
    assert abs(res2.zmean - w2["zmean"]) <= zb
    with pytest.raises(ValueError):
        grid_sequence(dirs, setup, mf=7, ctx=gpu_ctx)
