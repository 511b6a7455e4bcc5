"""wass_amd.postproc's polarimetric set-up on the GPU against the numpy oracle of tests/polarimetric_oracle.py (which
test_polarimetric.py holds to the reference's own geometry).  Nothing of the reference is read here.

remap_linear_f32, S, dolp, normals, rays_cam, the march's mask and the four averages are exact: array_equal to the oracle with
the NaN pattern equal.  Angles within visibility_oracle.angle_bound.  The mask with the 85 degree rule equals the oracle's except
in cells whose oracle angle lies within that bound of 85, at most 1 in 10^4 cells of a case.  Discriminating power is printed:
wrong variants of the sampler and of the accumulation must miss the GPU result.
Every test prints its figures before it asserts."""
import functools

import numpy as np
import pytest

import polarimetric_oracle as PO
import radiance_oracle as RO
import visibility_oracle as VO
from wass_amd import postproc as P

pytestmark = pytest.mark.gpu

IH, IW = 240, 320
# name: H, W, du, seed, amp, camera side, height, back (tests/test_visibility_gpu.py's table, by value); where the footprint lies
SEAS = {
    "96x257 west": ((96, 257, 0.25, 11, 1.0, "west", 4.0, 25.0), "inside"),
    "200x300 east": ((200, 300, 0.2, 12, 1.2, "east", 5.0, 30.0), "crossing"),
    "257x64 south": ((257, 64, 0.25, 13, 1.0, "south", 4.0, 20.0), "inside"),
    "128x128 over": ((128, 128, 0.5, 15, 2.0, "over", 9.0, 0.0), "inside"),
}
PER_FRAME = ("S", "occlusion", "angles", "dolp", "normals", "rays_cam")
AVERAGES = ("Savg", "Navg", "Zavg", "valid")


def _same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=np.asarray(a).dtype.kind == "f")


@functools.lru_cache(maxsize=None)
def _scene(name):
    """inputs and the oracle's results of a sea, computed once and not changed by any test"""
    (H, W, du, seed, amp, side, height, back), kind = SEAS[name]
    XX, YY = VO.make_grid(H, W, du)
    cam = VO.camera(XX, YY, side, height, back)
    Z = np.stack([VO.make_sea(H, W, du, seed, amp, t=0.7 * t) for t in range(3)])
    Z[1, H // 3:H // 3 + 3, :] = np.nan                                         # a NaN band in the second frame
    cx, cy = XX.mean(), YY.mean()
    shift = np.eye(4)
    shift[0, 3], shift[1, 3] = -cx, -cy
    Pplane = RO.pplane(IW, IH, XX - cx, YY - cy, kind) @ shift
    K = PO.intrinsics(IW, IH)
    stokes = PO.stokes_pictures(3, IH, IW, seed)
    stokes[0, 1, IH // 2, IW // 2] = np.nan                                      # propagate through the sums of their windows
    stokes[2, 0, IH // 2 + 7, IW // 2 - 9] = np.inf
    args = (stokes, Z, XX, YY, Pplane, cam, K)
    want = PO.setup(*args)
    assert want["not_up"] == 0
    for a in args + tuple(want[k] for k in PER_FRAME + AVERAGES):
        a.setflags(write=False)
    return args, want


def _variants(img, mx, my, got, what):
    for name, kw in (("truncation", dict(rounding="trunc")), ("phase exchanged", dict(swap_phase=True)), ("replicate border", dict(border="replicate"))):
        miss = int((~np.isclose(PO.remap_linear_f32(img, mx, my, **kw), got, rtol=0, atol=0, equal_nan=True)).sum())
        print(f"{what}: {name} misses the GPU result in {miss} of {got.size} cells")
        assert miss > 0


@pytest.mark.parametrize("sh,sw", [(5, 7), (64, 65), (240, 320)])
def test_remap_linear_f32(gpu_ctx, sh, sw):
    import torch
    rng = np.random.default_rng(sw)
    img = (rng.standard_normal((sh, sw)) * 3.0).astype(np.float32)
    for h, w in ((37, 67), (70, 130)):                                           # 1024 phases, the edges and corners, the undefined values
        mx, my = RO.lattice_maps(h, w, sh, sw, 7 + h)
        want = PO.remap_linear_f32(img, mx, my)
        got = P.remap_linear_f32(img, mx, my, ctx=gpu_ctx)
        assert got.dtype == np.float32 and got.shape == (h, w)
        print(f"{sh} x {sw} picture, {h} x {w} maps: {int((~np.isclose(got, want, rtol=0, atol=0, equal_nan=True)).sum())} cells differ, "
              f"{int((want != 0).sum())} cells are not 0")
        assert np.array_equal(got, want, equal_nan=True)
        dev = P.remap_linear_f32(torch.from_numpy(img).cuda(), torch.from_numpy(mx).cuda(), torch.from_numpy(my).cuda(), ctx=gpu_ctx)
        assert dev.is_cuda and np.array_equal(dev.cpu().numpy(), got, equal_nan=True)
        _variants(img, mx, my, got, f"{sh} x {sw}")
    bad = img.copy()
    bad[sh // 2, sw // 2], bad[sh // 3, sw // 4] = np.nan, np.inf
    mx, my = RO.lattice_maps(37, 67, sh, sw, 3)
    want = PO.remap_linear_f32(bad, mx, my)
    got = P.remap_linear_f32(bad, mx, my, ctx=gpu_ctx)
    print(f"{sh} x {sw} with a NaN and an infinite pixel: {int(np.isnan(want).sum())} NaN cells, {int(np.isinf(want).sum())} infinite")
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got, want, equal_nan=True)


def _check_angles(got, a64, n, what):
    assert got.dtype == np.float32 and got.shape == a64.shape
    nan = np.isnan(a64)
    assert np.array_equal(np.isnan(got), nan), "NaN pattern"
    ratio = np.abs(got.astype(np.float64) - a64)[~nan] / VO.angle_bound(a64, n)[~nan]
    print(f"{what}: largest angle error / bound = {ratio.max():.4f}")
    assert ratio.max() <= 1.0


@pytest.mark.parametrize("name", list(SEAS))
def test_polarimetric_setup(gpu_ctx, name):
    import torch
    args, want = _scene(name)
    stokes, Z, XX, YY, Pplane, cam, K = args
    count, H, W = Z.shape
    r = P.polarimetric_setup(*args, outputs=PER_FRAME, ctx=gpu_ctx)
    for k in ("S", "dolp", "normals", "rays_cam"):
        g, w = getattr(r, k), want[k]
        assert g.dtype == w.dtype and g.shape == w.shape, k
        print(f"{name}: {k}: {int((~np.isclose(g, w, rtol=0, atol=0, equal_nan=True)).sum())} of {w.size} values differ, {int(np.isnan(w).sum())} are NaN, "
              f"{int((np.nan_to_num(w) != 0).sum())} are not 0")
        assert np.array_equal(np.isnan(g), np.isnan(w)) and np.array_equal(g, w, equal_nan=True), k
    for k in AVERAGES:
        g, w = getattr(r, k), want[k]
        print(f"{name}: {k}: {int((~np.isclose(g, w, rtol=0, atol=0, equal_nan=True)).sum())} of {w.size} values differ, {int(np.isnan(w).sum())} are NaN")
        assert g.dtype == np.float64 and g.shape == w.shape and np.array_equal(g, w, equal_nan=True), k
    # the march alone is exact; the angles and the 85 degree rule within the visibility map's bound
    off = P.polarimetric_setup(*args, angle_limit=None, outputs=("occlusion",), ctx=gpu_ctx)
    print(f"{name}: {int((off.occlusion != want['march']).sum())} cells of the march's mask differ, {100.0 * want['march'].mean():.2f} % occluded")
    assert np.array_equal(off.occlusion, want["march"])
    near_all = 0
    for t in range(count):
        a64, n = VO.noise(XX, YY, want["zf"][t], cam[:3, 3])
        _check_angles(r.angles[t], a64, n, f"{name} frame {t}")
        with np.errstate(invalid="ignore"):
            near = np.abs(a64 - 85.0) <= VO.angle_bound(a64, n)
        near_all += int(near.sum())
        assert np.array_equal(r.occlusion[t][~near], want["occlusion"][t][~near])
    print(f"{name}: {near_all} cells within the bound of 85 degrees, {100.0 * want['occlusion'].mean():.2f} % occluded with the rule")
    assert near_all <= want["occlusion"].size // 10000
    assert np.array_equal(r.occluded_percent, 100.0 * r.occlusion.reshape(count, -1).sum(1) / float(H * W))
    if near_all == 0:
        assert np.array_equal(r.occluded_percent, want["occluded_percent"])
    # the same bytes whatever the batch, on a repeat, from device tensors, from an iterable; outputs=() still gives the averages
    base = {k: np.asarray(getattr(r, k)).tobytes() for k in PER_FRAME + AVERAGES}
    for what, kw in (("batch 1", dict(batch=1)), ("batch 2", dict(batch=2)), ("batch 3", dict(batch=3)), ("repeat", dict())):
        o = P.polarimetric_setup(*args, outputs=PER_FRAME, ctx=gpu_ctx, **kw)
        assert all(np.asarray(getattr(o, k)).tobytes() == base[k] for k in base), what
    it = P.polarimetric_setup(((f[0], f[1], f[2]) for f in stokes), *args[1:], outputs=PER_FRAME, ctx=gpu_ctx, batch=2)
    assert all(np.asarray(getattr(it, k)).tobytes() == base[k] for k in base), "iterable"
    d = P.polarimetric_setup(torch.tensor(stokes).cuda(), torch.tensor(Z).cuda(), *args[2:], outputs=PER_FRAME, ctx=gpu_ctx, batch=2)
    assert d.S.is_cuda and d.Savg.is_cuda and tuple(d.rays_cam.shape) == (count, 3, H * W)
    assert all(getattr(d, k).cpu().numpy().tobytes() == base[k] for k in base), "device"
    assert np.array_equal(d.occluded_percent, r.occluded_percent)
    none = P.polarimetric_setup(*args, outputs=(), total_frames=10, ctx=gpu_ctx)
    assert all(getattr(none, k) is None for k in PER_FRAME)
    assert all(getattr(none, k).tobytes() == base[k] for k in ("Savg", "Navg", "valid"))
    total = np.zeros((H, W))
    for t in range(count):
        total = total + want["zf"][t].astype(np.float64)
    assert np.array_equal(none.Zavg, total / 10.0, equal_nan=True)
    dn = P.polarimetric_setup(torch.tensor(stokes).cuda(), torch.tensor(Z).cuda(), *args[2:], outputs=(), ctx=gpu_ctx)
    assert all(getattr(dn, k).cpu().numpy().tobytes() == base[k] for k in AVERAGES)
    # what the exact comparison of the averages can see
    for what, kw in (("accumulating in float32", dict(acc_dtype=np.float32)), ("skipping nan_to_num", dict(use_nan_to_num=False))):
        wrong = PO.setup(*args, **kw)["Savg"].astype(np.float64)
        miss = int((~np.isclose(wrong, r.Savg, rtol=0, atol=0, equal_nan=True)).sum())
        print(f"{name}: {what} misses Savg in {miss} of {r.Savg.size} values")
        assert miss > 0


def test_cell_above_the_camera_raises(gpu_ctx):
    args, _ = _scene("128x128 over")
    Z = args[1].copy()
    Z[2, 40, 50] = 20000.0                                                       # 20 m, above the camera at 9 m
    with pytest.raises(ValueError, match="upward"):
        P.polarimetric_setup(args[0], Z, *args[2:], ctx=gpu_ctx)


def test_clip_and_zeromean(gpu_ctx):
    import torch
    rng = np.random.default_rng(5)
    x = (rng.standard_normal((7, 33, 65)) * 10.0 ** rng.uniform(-2, 4, (7, 33, 65))).astype(np.float32)
    x[3, 5, 7] = x[0, 32, 64] = x[6, 0, 0] = np.nan
    want, vmin, vmax = PO.clip_cube(x, -120.5, 300.25)
    got, gmin, gmax = P.clip_cube(x, -120.5, 300.25, ctx=gpu_ctx)
    print(f"clip: {int((~np.isclose(got, want, rtol=0, atol=0, equal_nan=True)).sum())} cells differ, range {gmin} .. {gmax}, oracle {vmin} .. {vmax}")
    assert got.dtype == np.float32 and np.array_equal(got, want, equal_nan=True) and np.array_equal(np.isnan(got), np.isnan(x))
    assert (gmin, gmax) == (vmin, vmax) == (np.float32(-120.5), np.float32(300.25))
    dgot, dmin, dmax = P.clip_cube(torch.from_numpy(x).cuda(), -120.5, 300.25, ctx=gpu_ctx)
    assert dgot.is_cuda and dgot.cpu().numpy().tobytes() == got.tobytes() and (dmin, dmax) == (gmin, gmax)
    wide, vmin, vmax = PO.clip_cube(x, -1e30, 1e30)                              # nothing is clipped: the range is the data's
    _, gmin, gmax = P.clip_cube(x, -1e30, 1e30, ctx=gpu_ctx)
    assert (gmin, gmax) == (vmin, vmax) == (np.nanmin(x), np.nanmax(x))
    _, gmin, gmax = P.clip_cube(np.full((2, 3, 4), np.nan, np.float32), 0.0, 1.0, ctx=gpu_ctx)
    assert np.isnan(gmin) and np.isnan(gmax)
    want = PO.zeromean(x)
    got = P.zeromean(x, ctx=gpu_ctx)
    print(f"zeromean: {int((~np.isclose(got, want, rtol=0, atol=0, equal_nan=True)).sum())} cells differ, {int(np.isnan(want).sum())} are NaN")
    assert got.dtype == np.float32 and np.array_equal(got, want, equal_nan=True) and np.isnan(got[:, 5, 7]).all()
    dx = torch.from_numpy(x).cuda()
    dgot = P.zeromean(dx, ctx=gpu_ctx)
    assert dgot.is_cuda and dgot.cpu().numpy().tobytes() == got.tobytes()
    assert P.zeromean(dx, out=dx, ctx=gpu_ctx) is dx and dx.cpu().numpy().tobytes() == got.tobytes()          # in place
