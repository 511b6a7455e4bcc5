"""The polarimetric set-up without a GPU: the numpy oracle of tests/polarimetric_oracle.py against the reference's own geometry
(tests/golden/polarimetric.npz, recorded by tests/golden/make_golden_polarimetric.py), the bilinear table against the
fixed-point builders, the sampler oracle against a direct fp64 formula, and the host-side pieces of wass_amd.postproc.
Every test prints its figures before it asserts."""
import os

import numpy as np
import pytest

import polarimetric_oracle as PO
import radiance_oracle as RO
import visibility_oracle as VO
from wass_amd import postproc as P

GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "polarimetric.npz"))

# Measured here on the CPU against the golden (numpy 2 with OpenBLAS; the reference's 4-term matrix product against our
# ((P0 X + P1 Y) + P2 z) + P3): the share of float32 map cells that differ, their largest difference in float32 ulps, and the
# largest difference of rays_cam in fp64 ulps.  Each is asserted at twice the measured value, which allows a BLAS that sums
# the product in another order.
# Measured: no map cell differs on either case (0 %, 0 ulps); rays_cam by 60 ulps on case a and 27 on case c, both in components
# close to zero, where an ulp is small against the unit vector's own rounding.
MEASURED_MAP_SHARE = 0.0
MEASURED_MAP_ULPS = 0
MEASURED_RAY_ULPS = 60.0


def _case(name):
    g = {k[len(name) + 1:]: GOLDEN[k] for k in GOLDEN.files if k.startswith(name + "_")}
    Z = g["Z"]
    XX, YY = VO.make_grid(Z.shape[0], Z.shape[1], float(g["du"]))
    Iw, Ih = (int(v) for v in GOLDEN["picture"])
    return g, Z, XX, YY, Iw, Ih


@pytest.mark.parametrize("name", [str(n) for n in GOLDEN["names"]])
def test_oracle_against_the_reference(name):
    g, Z, XX, YY, Iw, Ih = _case(name)
    H, W = Z.shape
    blank = np.zeros((3, Ih, Iw), np.float32)
    f = PO.frame(blank, Z, XX, YY, g["Pplane"], g["cam"], g["K"], angle_limit=85.0)
    assert f["not_up"] == 0
    mask = np.unpackbits(g["mask"])[:H * W].reshape(H, W)
    print(f"case {name}: {int(mask.sum())} of {H * W} cells occluded, {int((mask != f['occlusion']).sum())} differ from the oracle")
    assert np.array_equal(f["occlusion"], mask)
    assert np.array_equal(f["normals"], g["normals"])
    assert np.array_equal(f["normals"], P.compute_slope_and_normals(XX, YY, f["zf"])[1])
    with np.errstate(invalid="ignore"):
        assert np.abs(f["angles"].astype(np.float32).astype(np.float64) - g["angles"]).max() < 1e-4
    for axis in ("mapx", "mapy"):
        u = PO.ulps_f32(f[axis], g[axis])
        share = float(np.mean(u > 0))
        print(f"case {name}: {axis} differs from the reference's in {100.0 * share:.3f} % of the cells, by at most {int(u.max())} float32 ulps")
        assert share <= 2 * MEASURED_MAP_SHARE
        assert u.max() <= 2 * MEASURED_MAP_ULPS
    r = PO.ulps_f64(f["rays_cam"], g["rays_cam"])
    print(f"case {name}: rays_cam differs from the reference's inv(K) @ p2d by at most {r.max():.2f} fp64 ulps")
    assert f["rays_cam"].shape == (3, H * W) and r.max() <= 2 * MEASURED_RAY_ULPS
    assert np.abs(np.sqrt((f["rays_cam"] ** 2).sum(0)) - 1.0).max() < 1e-15


def _same_but_phase_0(tab, fixed, corner):
    """the float table times 2^15 against an int16 table of initInterTab2D, entry for entry: bilinear weights are multiples of
    1 / 1024, so the equality is exact -- but for the one weight that is 1.0, tap (0, 0) of phase 0, whose 32768 saturates to 32767
    in int16 (with the fix-up the missing 1 then goes to tap (1, 1): `corner`)"""
    scaled = tab.astype(np.float64).reshape(1024, 2, 2) * 32768.0
    fixed = np.asarray(fixed).reshape(1024, 2, 2).astype(np.float64)
    assert np.array_equal(scaled, np.rint(scaled))
    assert np.array_equal(scaled[1:], fixed[1:])
    assert np.array_equal(scaled[0], [[32768.0, 0.0], [0.0, 0.0]]) and np.array_equal(fixed[0], [[32767.0, 0.0], [0.0, corner]])


def test_bilinear_table():
    tab = P.bilinear_table()
    assert tab.dtype == np.float32 and tab.shape == (32, 32, 2, 2)
    assert np.array_equal(tab, PO.bilinear_table())
    _same_but_phase_0(tab, RO.inter_tab(2, fixup=False), 0.0)
    _same_but_phase_0(tab, RO.inter_tab(2), 1.0)
    assert np.array_equal(tab.reshape(1024, 4).sum(1), np.ones(1024, np.float32))


def test_bilinear_table_equals_the_c_oracle(oracle):
    _same_but_phase_0(P.bilinear_table(), oracle.inter_tab(2), 1.0)


@pytest.mark.parametrize("sh,sw", [(5, 7), (64, 65), (240, 320)])
def test_sampler_oracle_against_the_direct_formula(sh, sw):
    rng = np.random.default_rng(sh)
    img = rng.standard_normal((sh, sw)).astype(np.float32) * 3.0
    mx, my = RO.lattice_maps(37, 67, sh, sw, 5)
    # the first 1024 cells lie on the k / 32 lattice, every phase once; beyond them only cells that stayed on it are compared
    with np.errstate(invalid="ignore"):
        on = (np.ravel(mx).astype(np.float64) * 32 % 1 == 0) & (np.ravel(my).astype(np.float64) * 32 % 1 == 0) & \
            (np.abs(np.ravel(mx)) < 30000) & (np.abs(np.ravel(my)) < 30000)
    assert on[:1024].all()
    got = PO.remap_linear_f32(img, mx, my).ravel()
    want, tap = PO.bilinear_float(img, np.ravel(mx)[on], np.ravel(my)[on])
    err = np.abs(got[on].astype(np.float64) - want)
    bound = 4.0 * np.spacing(np.maximum(tap, np.finfo(np.float32).tiny).astype(np.float32)).astype(np.float64)
    print(f"{sh} x {sw}: {int(on.sum())} lattice cells, largest error / bound = {np.max(err / bound):.3f}")
    assert (err <= bound).all()


def test_sampler_border_tap_by_tap():
    img = np.arange(1, 36, dtype=np.float32).reshape(5, 7)
    tab = PO.bilinear_table()
    fy, fx = 13, 21
    for sy in range(-3, 7):
        for sx in range(-3, 9):
            mx = np.array([[sx + fx / 32.0]], np.float32)
            my = np.array([[sy + fy / 32.0]], np.float32)
            v = [img[y, x] if 0 <= y < 5 and 0 <= x < 7 else np.float32(0) for y in (sy, sy + 1) for x in (sx, sx + 1)]
            w = tab[fy, fx].ravel()
            want = ((v[0] * w[0] + v[1] * w[1]) + v[2] * w[2]) + v[3] * w[3]
            got = PO.remap_linear_f32(img, mx, my)[0, 0]
            assert got == want and got.dtype == np.float32, (sy, sx)
            if sy in (-1, 4) and 0 <= sx < 6:
                assert got != 0                                                 # one row of the window is inside: not a zero border
    # the undefined map values, and IEEE propagation of a NaN and an infinite pixel
    for bad in (np.nan, np.inf, -np.inf, 2.0 ** 27, -2.0 ** 27):
        assert PO.remap_linear_f32(img, np.array([[bad]], np.float32), np.array([[1.5]], np.float32))[0, 0] == 0
        assert PO.remap_linear_f32(img, np.array([[1.5]], np.float32), np.array([[bad]], np.float32))[0, 0] == 0
    img[2, 3], img[4, 1] = np.nan, np.inf
    assert np.isnan(PO.remap_linear_f32(img, np.array([[2.5]], np.float32), np.array([[1.5]], np.float32))[0, 0])
    assert np.isnan(PO.remap_linear_f32(img, np.array([[3.0]], np.float32), np.array([[2.0]], np.float32))[0, 0])   # weights 1, 0, 0, 0: NaN * 1
    assert PO.remap_linear_f32(img, np.array([[0.5]], np.float32), np.array([[3.5]], np.float32))[0, 0] == np.inf
    assert np.isnan(PO.remap_linear_f32(img, np.array([[0.0]], np.float32), np.array([[4.0]], np.float32))[0, 0])   # inf * 0 at (4, 1)


def test_nan_to_num_and_dolp():
    S = np.array([np.nan, np.inf, -np.inf, 1.5, -0.0, 3e38], np.float32)
    assert np.array_equal(PO.nan_to_num(S), np.nan_to_num(S))
    assert np.array_equal(PO.nan_to_num(S), np.array([0, PO.FLT_MAX, -PO.FLT_MAX, 1.5, 0, 3e38], np.float32))
    S3 = np.array([[2.0, 0.6, 0.8], [np.nan, np.nan, np.nan], [0.0, 0.0, 0.0]], np.float32)
    d = PO.dolp(S3)
    assert d[0] == np.float32(0.5) and np.isnan(d[1]) and np.isnan(d[2])


def test_total_frames_rule():
    H, W, du = 12, 14, 0.5
    XX, YY = VO.make_grid(H, W, du)
    Z = np.stack([VO.make_sea(H, W, du, 3, 0.5, t=0.4 * t) for t in range(3)])
    cam = VO.camera(XX, YY, "west", 5.0, 10.0)
    st = PO.stokes_pictures(3, 24, 32, 1)
    args = (st, Z, XX, YY, RO.pplane(32, 24, XX, YY, "crossing"), cam, PO.intrinsics(32, 24))
    a, b = PO.setup(*args), PO.setup(*args, total_frames=10)
    assert np.array_equal(a["Zavg"] * 3.0 / 10.0, b["Zavg"]) or np.allclose(a["Zavg"] * 0.3, b["Zavg"], rtol=1e-15)
    total = np.zeros((H, W))
    for t in range(3):
        total = total + VO.heights(Z[t]).astype(np.float64)
    assert np.array_equal(b["Zavg"], total / 10.0) and np.array_equal(a["Zavg"], total / 3.0)
    assert np.array_equal(a["Savg"], b["Savg"], equal_nan=True) and np.array_equal(a["Navg"], b["Navg"])
    assert np.abs(np.sqrt((a["Navg"] ** 2).sum(-1)) - 1.0).max() < 1e-15
    assert np.array_equal(a["valid"], 3.0 - a["occlusion"].sum(0))


def test_clip_and_zeromean_oracles():
    rng = np.random.default_rng(2)
    x = (rng.standard_normal((7, 9, 11)) * 100).astype(np.float32)
    x[2, 3, 4] = np.nan
    got, vmin, vmax = PO.clip_cube(x, -50.0, 80.5)
    assert np.array_equal(got, np.clip(x, np.float32(-50.0), np.float32(80.5)), equal_nan=True)
    assert np.isnan(got[2, 3, 4]) and vmin == np.float32(-50.0) and vmax == np.float32(80.5)
    _, vmin, vmax = PO.clip_cube(np.full((2, 2, 2), np.nan, np.float32), 0, 1)
    assert np.isnan(vmin) and np.isnan(vmax)
    zm = PO.zeromean(x)
    for i, j in ((0, 0), (3, 4), (8, 10)):
        s = 0.0
        for t in range(7):
            s += float(x[t, i, j])
        want = np.array([np.float32(float(x[t, i, j]) - s / 7.0) for t in range(7)], np.float32)
        assert np.array_equal(zm[:, i, j], want, equal_nan=True)
    assert np.isnan(zm[:, 3, 4]).all() and not np.isnan(zm[:, 0, 0]).any()


def test_scratch_arithmetic():
    al = lambda v: (v + 255) & ~255
    count, H, W, Ih, Iw, b = 16, 100, 130, 240, 320, 4
    vis, vb = P.visibility_scratch_bytes(b, H, W, b, host=False)
    assert vb == b
    n = b * H * W
    got, used = P.polarimetric_scratch_bytes(count, H, W, Ih, Iw, batch=b, host=True, outputs=P.POL_OUTPUTS)
    want = 2 * al(H * W * 8) + al(H * W * 64) + al(b * 3 * Ih * Iw * 4) + al(n * 4) + al(n) + al(n * 4) + al(n * 12) + al(n * 4) + 2 * al(n * 24) + vis
    assert (got, used) == (want, b)
    got, used = P.polarimetric_scratch_bytes(count, H, W, Ih, Iw, batch=b, host=False, outputs=("S", "occlusion"))
    assert (got, used) == (al(n * 4) + vis, b)
    got, used = P.polarimetric_scratch_bytes(count, H, W, Ih, Iw, batch=b, host=False, outputs=())
    assert (got, used) == (al(n) + al(n * 4) + al(n * 12) + vis, b)
    # the cap of 16 GiB halves the batch until a batch fits: 512 frames of 2456 x 2058 pictures are 31 GB
    def total(b, H=1024, W=1024, Ih=2058, Iw=2456):
        n = b * H * W
        return 2 * al(H * W * 8) + al(H * W * 64) + al(b * 3 * Ih * Iw * 4) + al(n * 4) + al(n) + al(n * 4) + al(n * 12) + \
            P.visibility_scratch_bytes(b, H, W, b, host=False)[0]
    got, used = P.polarimetric_scratch_bytes(512, 1024, 1024, 2058, 2456, batch=512, outputs=())
    assert total(256) > 16 << 30 >= total(128) and (got, used) == (total(128), 128)
    assert P.polarimetric_scratch_bytes(3, H, W, Ih, Iw, batch=8)[1] == 3
    with pytest.raises(ValueError):
        P.polarimetric_scratch_bytes(4, 1, W, Ih, Iw)
    with pytest.raises(ValueError):
        P.polarimetric_scratch_bytes(4, H, W, Ih, 40000)
    with pytest.raises(ValueError):
        P.polarimetric_scratch_bytes(4, H, W, Ih, Iw, outputs=("S", "nonsense"))


def test_argument_errors():
    """all raised before a context is made: no GPU needed"""
    H, W = 6, 8
    XX, YY = VO.make_grid(H, W, 0.5)
    Z = np.zeros((2, H, W), np.float32)
    st = np.zeros((2, 3, 10, 12), np.float32)
    ok = dict(stokes=st, data=Z, XX=XX, YY=YY, Pplane=np.eye(4), cam_to_grid=np.eye(4), K=np.eye(3))
    for bad in (dict(data=Z[0]), dict(stokes=st[:1]), dict(stokes=st[:, :2]), dict(XX=XX[:, :4]), dict(Pplane=np.eye(3)), dict(cam_to_grid=np.eye(3)),
                dict(K=np.eye(4)), dict(batch=0), dict(total_frames=0), dict(outputs=("S", "aolp"))):
        with pytest.raises(ValueError):
            P.polarimetric_setup(**{**ok, **bad})
    with pytest.raises(ValueError):
        P.remap_linear_f32(np.zeros((3, 4, 5), np.float32), np.zeros((2, 2), np.float32), np.zeros((2, 2), np.float32))
    with pytest.raises(ValueError):
        P.remap_linear_f32(np.zeros((3, 4), np.float32), np.zeros((2, 2), np.float32), np.zeros((2, 3), np.float32))
    with pytest.raises(ValueError):
        P.clip_cube(Z, np.nan, 1.0)
    with pytest.raises(ValueError):
        P.clip_cube(Z[0], 0.0, 1.0)
    with pytest.raises(ValueError):
        P.zeromean(Z[0])


def test_zeromean_oracle_reverse_order():
    """the mistake the GPU tests must see: the same mean but for the order of its fp64 sum.  On values of six decades alone the two
    orders differ in the last bits of an fp64 sum, which float32 results do not show; spread_cube's cancelling pairs make them
    differ in the float32 results at the counts the GPU tests use."""
    for count in (16, 17, 40):
        x = PO.spread_cube((count, 5, 257), count)
        plain = PO.spread_cube((count, 5, 257), count, pairs=False)
        assert x.dtype == np.float32 and np.abs(plain).max() < 1e6 and 400 < int((np.abs(x) > 1e16).any(0).sum()) < 900
        assert np.array_equal(np.where(np.abs(x) > 1e16, x, 0).astype(np.float64).sum(0), np.zeros((5, 257)))     # +B and -B cancel
        x[3, 4, 256] = np.nan
        fwd, back = PO.zeromean(x), PO.zeromean(x, reverse=True)
        assert np.array_equal(back, PO.zeromean(x[::-1])[::-1], equal_nan=True)
        s = 0.0
        for t in range(count - 1, -1, -1):
            s += float(x[t, 2, 100])
        assert np.array_equal(back[:, 2, 100], np.array([np.float32(float(v) - s / count) for v in x[:, 2, 100]], np.float32))
        differ = int((fwd != back).sum()) - int(np.isnan(fwd).sum())
        print(f"count {count}: the reverse order changes {differ} of {x.size} cells; without the pairs "
              f"{int((PO.zeromean(plain) != PO.zeromean(plain, reverse=True)).sum())}")
        assert differ > x.size // 10 and np.array_equal(np.isnan(fwd), np.isnan(back))
    one = np.float32([[[3.5]], [[-1.25]]])
    assert np.array_equal(PO.zeromean(one), PO.zeromean(one, reverse=True))


@pytest.mark.parametrize("name", list(PO.SMALL) + ["STRIDED", "CHANGING", "RAGGED"])
def test_edge_scenes_are_decided(name):
    """make_scene, near_85 and the scene tables of the edge tests: no cell at or above the camera, none whose angle lies within the
    visibility map's bound of 85 degrees (the GPU's mask with the rule must then equal the oracle's), something sampled, and for
    pictures of changing size every frame equal to the oracle of that frame alone, the sums running in frame order."""
    key = PO.SMALL[name] if name in PO.SMALL else getattr(PO, name)
    args = PO.make_scene(*key)
    stokes, Z, XX, YY, Pplane, cam, K = args
    count = key[10] if len(key) > 10 else 3
    sizes = [key[9]] * count if isinstance(key[9][0], int) else list(key[9])
    assert Z.shape == (count,) + key[:2] and Z.dtype == np.float32 and [tuple(np.shape(f)) for f in stokes] == [(3,) + s for s in sizes]
    assert isinstance(stokes, np.ndarray) == (len(set(sizes)) == 1)
    want = PO.setup(*args)
    near = PO.near_85(want, XX, YY, cam)
    sampled = int((np.nan_to_num(want["S"]) != 0).sum())
    print(f"{name}: not_up = {want['not_up']}, near_all = {near}, largest angle {np.nanmax(want['angles']):.2f} degrees, "
          f"{100.0 * want['occlusion'].mean():.2f} % occluded, {sampled} of {want['S'].size} samples neither 0 nor NaN, {int(np.isnan(Z).sum())} NaN heights")
    assert want["not_up"] == 0 and near == 0 and sampled > 0
    with np.errstate(invalid="ignore"):
        brute = sum(int((np.abs(a - 85.0) <= VO.angle_bound(a, VO.noise(XX, YY, zf, cam[:3, 3])[1])).sum()) for a, zf in zip(want["angles"], want["zf"]))
    assert brute == near
    Savg, valid = np.zeros(Z.shape[1:] + (3,)), np.zeros(Z.shape[1:])
    for t in range(count):
        f = PO.frame(stokes[t], Z[t], XX, YY, Pplane, cam, K)
        assert f["mapx"].dtype == np.float32
        assert np.array_equal(f["S"], want["S"][t], equal_nan=True) and np.array_equal(f["occlusion"], want["occlusion"][t])
        mx, my = RO.project(Z[t], XX, YY, RO.pcam(Pplane, sizes[t][1], sizes[t][0]))
        assert np.array_equal(f["mapx"], mx, equal_nan=True) and np.array_equal(f["mapy"], my, equal_nan=True)
        Savg = Savg + PO.nan_to_num(f["S"]).astype(np.float64)
        valid = valid + (1.0 - f["occlusion"])
    with np.errstate(all="ignore"):
        assert np.array_equal(want["Savg"], Savg / valid[..., None], equal_nan=True) and np.array_equal(want["valid"], valid)
