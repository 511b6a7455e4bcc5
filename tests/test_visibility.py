"""The visibility map without a GPU: the numpy oracle of tests/visibility_oracle.py against the reference's own output
(tests/golden/visibility.npz, made by tests/golden/make_golden_visibility.py), the gradient against np.gradient, the decisions
taken where the reference is undefined, the stated scratch, the ABI and the argument errors of wass_amd.postproc."""
import ctypes as C
import os

import numpy as np
import pytest

import visibility_oracle as VO

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "visibility.npz")


def _golden_cases():
    g = np.load(GOLDEN)
    for n in g["names"]:
        Z = g[f"{n}_Z"]
        H, W = Z.shape
        XX, YY = VO.make_grid(H, W, float(g[f"{n}_du"]))
        yield str(n), Z, XX, YY, g[f"{n}_origin"], np.unpackbits(g[f"{n}_mask"])[:H * W].reshape(H, W), g[f"{n}_angles"]


def test_oracle_against_the_reference():
    """Masks array_equal; angles equal as float32 except where the fp64 values straddle a float32 rounding boundary (the
    reference's dot product runs through BLAS): such cells may differ by one float32 neighbour and must be few."""
    assert os.path.getsize(GOLDEN) < 200000
    seen = 0
    for name, Z, XX, YY, origin, gmask, gang in _golden_cases():
        mask, a, steps, not_up = VO.visibility_frame(Z, XX, YY, origin, angle_limit=None)
        assert not_up == 0 and gang.dtype == np.float32
        assert np.array_equal(mask, gmask), name
        kept = VO.visibility_frame(Z, XX, YY, origin, angle_limit=None, compact=False)[0]
        assert np.array_equal(kept, mask), "dropping ended rays from the arrays must change nothing"
        a32 = a.astype(np.float32)
        differ = a32 != gang
        neighbour = (np.nextafter(a32, np.float32(np.inf)) == gang) | (np.nextafter(a32, np.float32(-np.inf)) == gang)
        print(f"case {name}: {100.0 * mask.mean():.1f} % occluded in {steps} steps, {int(differ.sum())} of {differ.size} angles differ as float32, "
              f"nearest angle to 88 degrees at {np.min(np.abs(a - 88.0)):.2e}")
        assert (neighbour | ~differ).all(), name
        assert differ.sum() <= max(1, differ.size // 10000), name
        assert 0.05 < mask.mean() < 0.6 and steps >= 17
        assert np.min(np.abs(a - 88.0)) > 1e-6
        with88 = VO.visibility_frame(Z, XX, YY, origin)[0]
        assert np.array_equal(with88, gmask | (gang >= 88).astype(np.uint8))
        seen += 1
    assert seen == 3


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_gradient_is_numpy_gradient(dtype):
    from wass_amd import postproc as P
    XX, YY = VO.make_grid(37, 53, 0.3)
    zf = VO.heights(VO.make_sea(37, 53, 0.3, seed=4)).astype(dtype)
    dx, dy = VO.spacing(XX, YY)
    want_y, want_x = np.gradient(zf, dy, dx)
    got_y, got_x = VO.gradient(zf, dy, dx)
    assert got_x.dtype == want_x.dtype == dtype
    assert np.array_equal(got_x, want_x) and np.array_equal(got_y, want_y)
    slope, normals = P.compute_slope_and_normals(XX, YY, zf)
    assert np.array_equal(slope[..., 0], want_x) and np.array_equal(slope[..., 1], want_y)
    ref = np.dstack((want_x, want_y, -np.ones_like(want_x, dtype=np.float64)))
    ref = -ref / np.linalg.norm(ref, axis=-1, keepdims=True)
    assert normals.dtype == np.float64 and np.array_equal(normals, ref)
    # two rows or columns: both edges, no interior
    y2, x2 = VO.gradient(zf[:2, :2], dy, dx)
    w2 = np.gradient(zf[:2, :2], dy, dx)
    assert np.array_equal(y2, w2[0]) and np.array_equal(x2, w2[1])


def test_nan_band_and_all_nan_frame():
    H, W = 60, 90
    XX, YY = VO.make_grid(H, W, 0.25)
    origin = VO.camera(XX, YY, "west", 4.0, 20.0)[:3, 3]
    Z = VO.make_sea(H, W, 0.25, seed=5)
    clean, a_clean, _, _ = VO.visibility_frame(Z, XX, YY, origin)
    assert clean.any()
    Zn = Z.copy()
    Zn[:, 30:34] = np.nan
    mask, a, _, not_up = VO.visibility_frame(Zn, XX, YY, origin)
    assert not_up == 0
    assert not mask[:, 30:34].any() and np.isnan(a[:, 30:34]).all()                 # a NaN cell: mask 0, NaN angle
    assert np.isnan(a[:, 29]).all() and np.isnan(a[:, 34]).all()                     # the stencil touches a NaN
    assert np.isfinite(a[:, :29]).all() and np.isfinite(a[:, 35:]).all()
    assert np.array_equal(a[:, :29], a_clean[:, :29])
    # cells west of the band look towards the camera over clean cells only
    assert np.array_equal(mask[:, :29], clean[:, :29])
    # the band's neighbours are marched although the 88 degree rule cannot catch them
    no_rule = VO.visibility_frame(Zn, XX, YY, origin, angle_limit=None)[0]
    assert np.array_equal(mask[:, 34], no_rule[:, 34]) and no_rule[:, 34:].any()
    # a NaN is never an occluder: no cell is occluded by the band itself
    hole = VO.visibility_frame(np.where(np.isnan(Zn), np.float32(-1e6), Zn), XX, YY, origin, angle_limit=None)[0]
    keep = np.ones((H, W), bool)
    keep[:, 29:35] = False
    assert np.array_equal(no_rule[keep], hole[keep])
    allnan = np.full((H, W), np.nan, np.float32)
    mask, a, steps, not_up = VO.visibility_frame(allnan, XX, YY, origin)
    assert not mask.any() and np.isnan(a).all() and steps == 0 and not_up == 0


def test_camera_over_a_node_and_cell_above_the_camera():
    H, W = 40, 50
    XX, YY = VO.make_grid(H, W, 0.5)
    Z = VO.make_sea(H, W, 0.5, seed=6)
    M = VO.camera(XX, YY, "over_node", 7.0)
    i, j = H // 3, W // 2
    assert M[0, 3] == XX[i, j] and M[1, 3] == YY[i, j]
    mask, a, _, not_up = VO.visibility_frame(Z, XX, YY, M[:3, 3])
    d = VO.rays(XX, YY, VO.heights(Z), M[:3, 3])
    assert d[i, j, 0] == 0 and d[i, j, 1] == 0 and d[i, j, 2] == 1
    assert mask[i, j] == 0 and np.isfinite(a[i, j]) and not_up == 0
    Zh = Z.copy()
    Zh[5, 7] = 7000.0                                                                 # at the camera's height
    Zh[9, 9] = 9000.0                                                                 # above it
    mask, a, _, not_up = VO.visibility_frame(Zh, XX, YY, M[:3, 3])
    assert not_up == 2 and mask[5, 7] == 0 and mask[9, 9] == 0


def test_wall_shadow_in_closed_form():
    """A wall of height h at distance D from a camera hc up shades n = floor(h D / ((hc - h) dx)) cells behind it."""
    H, W, du, jw = 33, 80, 0.25, 20
    XX, YY = VO.make_grid(H, W, du)
    Z = np.zeros((H, W), np.float32)
    Z[:, jw] = 1000.0
    origin = np.array([XX[0, jw] - 12.5, YY[16, 0], 5.0])
    mask = VO.visibility_frame(Z, XX, YY, origin, angle_limit=None)[0]
    n = int(np.floor(1.0 * 12.5 / ((5.0 - 1.0) * du)))
    assert n == 12
    want = np.zeros(W, np.uint8)
    want[jw + 1:jw + 1 + n] = 1
    assert np.array_equal(mask[16], want)
    assert not mask[:, :jw + 1].any() and mask[:, jw + 1:jw + n].all()


def test_mistakes_are_visible_to_the_oracle():
    """The variants the GPU tests use to show their discriminating power differ from the exact march on the golden cases."""
    for name, Z, XX, YY, origin, gmask, _ in _golden_cases():
        for mode in ("transposed", "trunc"):
            assert (VO.visibility_frame(Z, XX, YY, origin, angle_limit=None, mode=mode)[0] != gmask).sum() >= 100, (name, mode)
        low = VO.visibility_frame(Z, XX, YY, origin, angle_limit=None, maxz=0.0)[0]
        assert (low != gmask).sum() >= 100
    ZZ, rays, rows = VO.tie_scene(24, 70)
    exact = VO.march(ZZ, rays)[0]
    kstep = VO.march(ZZ, rays, mode="kstep")[0]
    assert (exact != kstep).sum() == len(rows)


def test_abi_scratch_and_argument_errors():
    from wass_amd import _lib, postproc as P
    lib = _lib.load()
    for name in ("wass_visibility_scratch_bytes", "wass_visibility", "wass_visibility_dev", "wass_occlusion_rays", "wass_occlusion_rays_dev"):
        assert name in _lib.SYMBOLS and hasattr(lib, name)
    al = lambda v: (v + 255) & ~255
    H, W, count = 100, 130, 20
    HW = H * W
    head = al(count * 8) + al(count * 4) + 256
    b, n = P.visibility_scratch_bytes(count, H, W, batch=8, host=True)
    assert n == 8 and b == head + 2 * al(HW * 8) + al(8 * HW * 8) + al(8 * HW * 4) + al(8 * HW) + al(8 * HW * 4)
    b, n = P.visibility_scratch_bytes(count, H, W, batch=8, host=False)
    assert n == 8 and b == head + al(8 * HW * 8)
    assert P.visibility_scratch_bytes(3, H, W, batch=8)[1] == 3                        # no more than there are frames
    # the batch is halved until the scratch fits 16 GiB: 16 B per cell and frame on the device side at 16384 x 16384
    b, n = P.visibility_scratch_bytes(64, 16384, 16384, batch=64, host=False)
    assert n == 4 and b <= 16 << 30 and 8 * 16384 * 16384 * 8 + 256 > 16 << 30
    b, n = P.visibility_scratch_bytes(64, 16384, 16384, batch=64, host=True)
    assert n == 2 and b <= 16 << 30
    with pytest.raises(ValueError):
        P.visibility_scratch_bytes(4, 1, 50)
    bytes_, used = C.c_size_t(), C.c_int()
    assert lib.wass_visibility_scratch_bytes(0, 10, 10, 8, 1, C.byref(bytes_), C.byref(used)) != 0
    assert lib.wass_visibility_scratch_bytes(4, 10, 10, 8, 1, None, None) != 0

    XX, YY = VO.make_grid(6, 8, 0.5)
    cube = np.zeros((2, 6, 8), np.float32)
    cam = VO.camera(XX, YY, "west")
    bad = [dict(data=cube[0]), dict(XX=XX[:, :7]), dict(YY=YY.T), dict(cam_to_grid=np.eye(3)), dict(XX=XX[:, ::-1]), dict(YY=YY[::-1]),
           dict(YY=2.0 * YY), dict(data=cube[:, :1], XX=XX[:1], YY=YY[:1]), dict(data=cube[:, :, :1], XX=XX[:, :1], YY=YY[:, :1]), dict(batch=0)]
    for kw in bad:
        args = dict(data=cube, XX=XX, YY=YY, cam_to_grid=cam)
        args.update(kw)
        with pytest.raises(ValueError):
            P.visibility_map(**args)
    with pytest.raises(ValueError):
        P.compute_occlusion_mask(np.zeros((6, 8)), np.zeros((6, 8, 2)))
    with pytest.raises(ValueError):
        P.compute_slope_and_normals(XX, YY[::-1], np.zeros((6, 8)))
    with pytest.raises(ValueError):
        P.compute_slope_and_normals(XX[:1], YY[:1], np.zeros((1, 8)))
