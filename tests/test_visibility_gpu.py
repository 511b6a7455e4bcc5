"""wass_amd.postproc's visibility map on the GPU against the numpy oracle of tests/visibility_oracle.py (which test_visibility.py
holds to the reference's own output).  Nothing of the reference is read here.

The march is exact: with the angle rule off the mask is array_equal to the oracle's, on every case.  Angles, element-wise, no
exempt cells: |gpu_f32 - oracle64| <= 0.5 ulp_f32(oracle64) + 4 n with n = visibility_oracle.noise() per cell, NaN where the
oracle is NaN.  With the 88 degree rule on, the mask equals the oracle's except in cells whose oracle angle lies within that
bound of 88 degrees, at most 1 in 10^4 cells of a case (on these cases the oracle has none within 1e-6 degrees).
Discriminating power: on every sea shape a transposed ray, truncation instead of rounding half to even and the maximum of the
wrong frame miss the GPU mask by at least MISS cells (printed).  k * step instead of the accumulated sum differs from it by
rounding only and changes no cell of a sea (the oracle says so, and it is printed); the march, one __device__ function behind
both entry points, is therefore also run on visibility_oracle.tie_scene of every shape, where the two differ in exactly one
cell per marked row.
Every test prints its figures before it asserts."""
import numpy as np
import pytest

import visibility_oracle as VO
import wass_amd
from wass_amd import postproc as P

pytestmark = pytest.mark.gpu

MISS = 50          # cells by which each mistake must miss the mask of a sea case

# name: H, W, du, seed, amp, camera side, height, back
SEAS = {
    "96x257 west": (96, 257, 0.25, 11, 1.0, "west", 4.0, 25.0),
    "200x300 east": (200, 300, 0.2, 12, 1.2, "east", 5.0, 30.0),
    "257x64 south": (257, 64, 0.25, 13, 1.0, "south", 4.0, 20.0),
    "130x1025 north": (130, 1025, 0.2, 14, 1.5, "north", 6.0, 40.0),
    "128x128 over": (128, 128, 0.5, 15, 2.0, "over", 9.0, 0.0),
    "1024x1024 west": (1024, 1024, 0.2, 16, 1.5, "west", 8.0, 60.0),
}


def _sea(name):
    H, W, du, seed, amp, side, height, back = SEAS[name]
    XX, YY = VO.make_grid(H, W, du)
    return VO.make_sea(H, W, du, seed, amp), XX, YY, VO.camera(XX, YY, side, height, back)


def _check_angles(got, a64, n, what):
    assert got.dtype == np.float32 and got.shape == a64.shape
    nan = np.isnan(a64)
    assert np.array_equal(np.isnan(got), nan), "NaN pattern"
    ok = ~nan
    if ok.any():
        ratio = np.abs(got.astype(np.float64) - a64)[ok] / VO.angle_bound(a64, n)[ok]
        print(f"{what}: largest angle error / bound = {ratio.max():.4f}, equal to the rounded oracle in "
              f"{100.0 * np.mean(got[ok] == a64[ok].astype(np.float32)):.4f} % of the cells")
        assert ratio.max() <= 1.0


def _check_rule(mask88, march_mask, a64, n, limit, what):
    """the mask with the angle rule on: the oracle's, except where the oracle's angle is within the angle bound of the limit"""
    with np.errstate(invalid="ignore"):
        want = march_mask | (a64 >= limit).astype(np.uint8)
        near = np.abs(a64 - limit) <= VO.angle_bound(a64, n)
        closest = np.nanmin(np.abs(a64 - limit)) if np.isfinite(a64).any() else np.inf
    print(f"{what}: {100.0 * want.mean():.2f} % occluded with the rule, {int(near.sum())} cells within the bound of {limit}, the closest at {closest:.2e}")
    assert near.sum() <= want.size // 10000
    assert closest > 1e-6
    assert np.array_equal(mask88[~near], want[~near])


@pytest.mark.parametrize("name", list(SEAS))
def test_sea(gpu_ctx, name):
    Z, XX, YY, cam = _sea(name)
    H, W = Z.shape
    origin = cam[:3, 3]
    want, _, steps, not_up = VO.visibility_frame(Z, XX, YY, origin, angle_limit=None)
    a64, n = VO.noise(XX, YY, VO.heights(Z), origin)
    assert not_up == 0
    mask, ang, pct = P.visibility_map(Z[None], XX, YY, cam, angle_limit=None, ctx=gpu_ctx)
    assert mask.dtype == np.uint8 and mask.shape == (1, H, W)
    differ = int((mask[0] != want).sum())
    print(f"{name}: {100.0 * want.mean():.2f} % occluded by the march in {steps} steps, {differ} cells differ")
    assert np.array_equal(mask[0], want)
    assert pct.dtype == np.float64 and pct[0] == 100.0 * want.sum() / (H * W)
    _check_angles(ang[0], a64, n, name)
    mask88, ang88, pct88 = P.visibility_map(Z[None], XX, YY, cam, ctx=gpu_ctx)
    assert ang88.tobytes() == ang.tobytes()
    _check_rule(mask88[0], want, a64, n, 88.0, name)
    assert pct88[0] == 100.0 * mask88[0].sum() / (H * W)
    # what the exact comparison can see
    other = VO.make_sea(H, W, SEAS[name][2], SEAS[name][3] + 100, 0.25 * SEAS[name][4])
    wrong_max = VO.frame_max(VO.heights(other).astype(np.float64) / VO.spacing(XX, YY)[0])
    for what, kw in (("transposed ray", dict(mode="transposed")), ("truncation", dict(mode="trunc")), ("maxz of another frame", dict(maxz=wrong_max)),
                     ("k * step", dict(mode="kstep"))):
        miss = int((VO.visibility_frame(Z, XX, YY, origin, angle_limit=None, **kw)[0] != mask[0]).sum())
        print(f"{name}: {what} misses the mask by {miss} cells")
        assert miss >= (0 if what == "k * step" else MISS)
    # the accumulated sum against k * step, on this shape
    ZZ, rays, rows = VO.tie_scene(H, W)
    got = P.compute_occlusion_mask(ZZ, rays, ctx=gpu_ctx)
    assert np.array_equal(got, VO.march(ZZ, rays)[0])
    miss = int((VO.march(ZZ, rays, mode="kstep")[0] != got).sum())
    print(f"{name}: on the tie scene k * step misses the mask by {miss} cells")
    assert miss == len(rows)


def test_flat_sea_and_wall(gpu_ctx):
    H, W, du, jw = 70, 130, 0.25, 20
    XX, YY = VO.make_grid(H, W, du)
    cam = VO.camera(XX, YY, "west", 5.0, 12.5)
    flat = np.zeros((H, W), np.float32)
    mask, ang, pct = P.visibility_map(flat[None], XX, YY, cam, angle_limit=None, ctx=gpu_ctx)
    assert not mask.any() and pct[0] == 0.0                                          # nothing is occluded on a flat sea
    a64, n = VO.noise(XX, YY, VO.heights(flat), cam[:3, 3])
    _check_angles(ang[0], a64, n, "flat sea")
    # a single wall: h = 1 m, the camera hc = 5 m up and D = 12.5 m in front of it: h D / ((hc - h) dx) = 12.5 cells of shadow
    wall = flat.copy()
    wall[:, jw] = 1000.0
    cam[:3, 3] = (XX[0, jw] - 12.5, YY[31, 0], 5.0)
    mask = P.visibility_map(wall[None], XX, YY, cam, angle_limit=None, ctx=gpu_ctx)[0][0]
    want = np.zeros(W, np.uint8)
    want[jw + 1:jw + 13] = 1
    print("wall: shadow of", int(mask[31].sum()), "cells in the camera's row")
    assert np.array_equal(mask[31], want)
    assert np.array_equal(mask, VO.visibility_frame(wall, XX, YY, cam[:3, 3], angle_limit=None)[0])


def _cube(count, H, W, du, seed):
    return np.stack([VO.make_sea(H, W, du, seed, 0.6 + 0.2 * (t % 5), t=0.4 * t) for t in range(count)])


def test_batches_repeats_and_input_kinds(gpu_ctx, tmp_path):
    import torch
    count, H, W, du = 11, 75, 139, 0.25
    XX, YY = VO.make_grid(H, W, du)
    cam = VO.camera(XX, YY, "east", 4.5, 22.0)
    cube = _cube(count, H, W, du, 21)
    wm, wa, wp = VO.visibility(cube, XX, YY, cam[:3, 3])
    assert len(set(wp)) == count                                                     # frames that differ
    singles = [P.visibility_map(cube[t:t + 1], XX, YY, cam, ctx=gpu_ctx, batch=1) for t in range(count)]
    one_m = np.concatenate([s[0] for s in singles])
    one_a = np.concatenate([s[1] for s in singles])
    assert np.array_equal(one_m, wm)
    assert np.array_equal(np.concatenate([s[2] for s in singles]), wp)
    for t in range(count):
        a64, n = VO.noise(XX, YY, VO.heights(cube[t]), cam[:3, 3])
        _check_angles(one_a[t], a64, n, f"frame {t}")
    for batch in (1, 2, 3, 8, 16):
        m, a, p = P.visibility_map(cube, XX, YY, cam, ctx=gpu_ctx, batch=batch)
        assert m.tobytes() == one_m.tobytes() and a.tobytes() == one_a.tobytes() and np.array_equal(p, wp), batch
    m, a, p = P.visibility_map(cube, XX, YY, cam, ctx=gpu_ctx)                       # repeat
    assert m.tobytes() == one_m.tobytes() and a.tobytes() == one_a.tobytes()
    # a maximum of the wrong frame would be seen: the frames' maxima differ and so do the masks they give
    dx = VO.spacing(XX, YY)[0]
    wrong = VO.visibility_frame(cube[1], XX, YY, cam[:3, 3], angle_limit=None,
                                maxz=VO.frame_max(VO.heights(cube[0]).astype(np.float64) / dx))[0]
    right = P.visibility_map(cube[1:2], XX, YY, cam, angle_limit=None, ctx=gpu_ctx)[0][0]
    print("maxz of frame 0 in frame 1 misses by", int((wrong != right).sum()), "cells")
    assert (wrong != right).sum() >= MISS
    # a strided view, a memmap with outputs given, device tensors
    big = np.full((count, H + 3, W + 7), np.float32(123.0))
    big[:, 2:2 + H, 4:4 + W] = cube
    view = big[:, 2:2 + H, 4:4 + W]
    assert not view.flags.c_contiguous
    m, a, _ = P.visibility_map(view, XX, YY, cam, ctx=gpu_ctx, batch=4)
    assert m.tobytes() == one_m.tobytes() and a.tobytes() == one_a.tobytes()
    mm = np.memmap(tmp_path / "cube.f32", np.float32, "w+", shape=cube.shape)
    mm[:] = cube
    mm.flush()
    om, oa = np.empty(cube.shape, np.uint8), np.empty(cube.shape, np.float32)
    m, a, _ = P.visibility_map(mm, XX, YY, cam, ctx=gpu_ctx, out_occlusion=om, out_angles=oa)
    assert m is om and a is oa and om.tobytes() == one_m.tobytes() and oa.tobytes() == one_a.tobytes()
    d = torch.from_numpy(big).to(f"cuda:{gpu_ctx.device_id}")
    m, a, p = P.visibility_map(d[:, 2:2 + H, 4:4 + W], XX, YY, cam, ctx=gpu_ctx, batch=3)
    assert m.is_cuda and m.cpu().numpy().tobytes() == one_m.tobytes() and a.cpu().numpy().tobytes() == one_a.tobytes()
    assert np.array_equal(p, wp)


def test_undefined_cases(gpu_ctx):
    H, W, du = 64, 200, 0.25
    XX, YY = VO.make_grid(H, W, du)
    cam = VO.camera(XX, YY, "west", 4.0, 20.0)
    cube = _cube(5, H, W, du, 31)
    clean = P.visibility_map(cube, XX, YY, cam, ctx=gpu_ctx)
    holes = cube.copy()
    holes[1] = np.nan                                                                 # an all-NaN frame inside a batch
    holes[3, :, 90:97] = np.nan                                                       # a NaN band
    holes[3, 10:14, 150:] = np.nan
    m, a, p = P.visibility_map(holes, XX, YY, cam, ctx=gpu_ctx, batch=5)
    wm, wa, wp = VO.visibility(holes, XX, YY, cam[:3, 3])
    assert np.array_equal(m, wm) and np.array_equal(p, wp)
    assert not m[1].any() and np.isnan(a[1]).all() and p[1] == 0.0
    assert not m[3][np.isnan(holes[3])].any() and np.isnan(a[3][np.isnan(holes[3])]).all()
    assert np.array_equal(np.isnan(a), np.isnan(wa))
    for t in (0, 2, 4):                                                               # no other frame is touched
        assert m[t].tobytes() == clean[0][t].tobytes() and a[t].tobytes() == clean[1][t].tobytes()
    a64, n = VO.noise(XX, YY, VO.heights(holes[3]), cam[:3, 3])
    _check_angles(a[3], a64, n, "NaN band")
    # exactly over a node: no horizontal component, the march gives 0, the angle is computed
    over = VO.camera(XX, YY, "over_node", 7.0)
    m, a, _ = P.visibility_map(cube[:1], XX, YY, over, ctx=gpu_ctx)
    want, a64, _, _ = VO.visibility_frame(cube[0], XX, YY, over[:3, 3])
    assert np.array_equal(m[0], want) and m[0, H // 3, W // 2] == 0 and np.isfinite(a[0, H // 3, W // 2])
    # a cell at or above the camera: ValueError from the function, a count and mask 0 from the C entry
    high = cube[:1].copy()
    high[0, 5, 7] = 7000.0
    high[0, 9, 9] = 9500.0
    with pytest.raises(ValueError, match="upward"):
        P.visibility_map(high, XX, YY, over, ctx=gpu_ctx)
    import ctypes as C
    mask, ang = np.empty((1, H, W), np.uint8), np.empty((1, H, W), np.float32)
    counts, up = np.zeros(1, np.uint64), C.c_uint64()
    origin = np.ascontiguousarray(over[:3, 3])
    gpu_ctx._check(gpu_ctx._lib.wass_visibility(gpu_ctx._h, high.ctypes.data, H * W, W, 1, H, W, XX.ctypes.data, YY.ctypes.data, origin.ctypes.data,
                                                1e-3, 88.0, 0, mask.ctypes.data, ang.ctypes.data, counts.ctypes.data, C.byref(up)))
    want, _, _, not_up = VO.visibility_frame(high[0], XX, YY, origin)
    assert up.value == not_up == 2 and mask[0, 5, 7] == 0 and mask[0, 9, 9] == 0
    assert np.array_equal(mask[0], want) and counts[0] == want.sum()


def test_compute_occlusion_mask_with_a_ray_field(gpu_ctx):
    import torch
    H, W = 90, 150
    XX, YY = VO.make_grid(H, W, 0.25)
    zf = VO.heights(VO.make_sea(H, W, 0.25, 41, 1.5))
    ZZ = zf.astype(np.float64) / 0.25
    d = VO.rays(XX, YY, zf, VO.camera(XX, YY, "south", 4.0, 15.0)[:3, 3])
    for inv in (False, True):
        want = VO.march(ZZ, d, invert_y_axis=inv)[0]
        got = P.compute_occlusion_mask(ZZ, d, invert_y_axis=inv, ctx=gpu_ctx)
        print(f"invert_y_axis {inv}: {100.0 * want.mean():.2f} % occluded")
        assert got.dtype == np.uint8 and np.array_equal(got, want)
        dev = P.compute_occlusion_mask(torch.from_numpy(ZZ).cuda(gpu_ctx.device_id), torch.from_numpy(d).cuda(gpu_ctx.device_id), inv, ctx=gpu_ctx)
        assert np.array_equal(dev.cpu().numpy(), want)
    assert (VO.march(ZZ, d, invert_y_axis=True)[0] != VO.march(ZZ, d)[0]).sum() >= MISS
    assert np.array_equal(P.compute_occlusion_mask(zf / np.float32(0.25), d, ctx=gpu_ctx), VO.march((zf / np.float32(0.25)).astype(np.float64), d)[0])
    down = d.copy()
    down[3, 4, 2] = 0.0
    with pytest.raises(ValueError, match="upward"):
        P.compute_occlusion_mask(ZZ, down, ctx=gpu_ctx)


def test_grid_sequence_output(gpu_ctx, oracle, tmp_path):
    from test_grid_seq_gpu import _sequence_on_disk
    from wass_amd.gridding import grid_sequence
    plane = np.array([0.02, 0.81, 0.586, -11.0])
    plane[:3] /= np.linalg.norm(plane[:3])
    dirs = _sequence_on_disk(tmp_path, oracle, 6, plane)
    R, T, _, _ = wass_amd.RT_from_plane(plane)
    W, H = 96, 80
    setup = {"Rpl": R, "Tpl": T.reshape(3, 1), "CAM_BASELINE": np.array([[2.5]]), "xmin": np.array([[-12.0]]), "xmax": np.array([[12.0]]),
             "ymin": np.array([[-25.0]]), "ymax": np.array([[-5.0]]), "XX": np.zeros((H, W)), "fps": np.array([[12.5]])}
    um = np.ones((H, W), np.uint8)
    um[:, :6] = 0
    res = grid_sequence(dirs, setup, user_mask=um * 255, alg_options={"Nfreqs": 40, "MAX_ITERS": 120}, batch=4, ctx=gpu_ctx)
    assert res.Z.shape == (6, H, W) and np.isnan(res.Z).any() and np.isfinite(res.Z).any()
    XX, YY = VO.make_grid(H, W, 0.25, -12.0, -25.0)
    cam = np.eye(4)
    # the gridded heights are not zero-mean here (no force_zero_mean): the camera goes 4 m above the highest cell of the cube
    top = float(np.nanmax(res.Z)) * 1e-3
    print(f"grid_sequence output: heights from {np.nanmin(res.Z) * 1e-3:.3f} to {top:.3f} m, {100.0 * np.isnan(res.Z).mean():.1f} % NaN")
    cam[:3, 3] = (0.1, 3.0, top + 4.0)
    m, a, p = P.visibility_map(res.Z, XX, YY, cam, ctx=gpu_ctx)
    wm, wa, wp = VO.visibility(res.Z, XX, YY, cam[:3, 3])
    print("grid_sequence output: occluded per frame", np.round(p, 2))
    assert np.array_equal(m, wm) and np.array_equal(p, wp) and np.array_equal(np.isnan(a), np.isnan(wa))
    for t in range(6):
        a64, n = VO.noise(XX, YY, VO.heights(res.Z[t]), cam[:3, 3])
        _check_angles(a[t], a64, n, f"gridded frame {t}")
