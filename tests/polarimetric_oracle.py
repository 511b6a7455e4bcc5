"""numpy restatements of the polarimetric set-up (wass_amd.postproc: remap_linear_f32, polarimetric_setup, clip_cube, zeromean),
with deliberately wrong variants.  Test infrastructure only: nothing here is imported by the package.

The bilinear sampler restates OpenCV 4.5.5's imgwarp.cpp (interpolateLinear, initInterTab2D, remapBilinear for float) from
knowledge: cv2 is not available where this was written, so it is UNPINNED against the real OpenCV (the order of the four-term sum
and whether a build contracts it to FMA are not pinned).  What is checked without OpenCV: the table against the fixed-point
builders of radiance_oracle and oracle/oracle.py, and the sampler against a direct fp64 bilinear formula (tests/test_polarimetric.py).

Seas, grids, cameras, projections and lattice maps come from visibility_oracle and radiance_oracle."""
import numpy as np

import radiance_oracle as RO
import visibility_oracle as VO

F = np.float32
BITS, TAB = 5, 32
FLT_MAX = float(np.finfo(F).max)


# ---- the sampler ------------------------------------------------------------------------------------------------------------------
def bilinear_table() -> np.ndarray:
    """float32 [32, 32, 2, 2] = [fy, fx, ky, kx]: ty[ky] * tx[kx], t = (1 - f / 32, f / 32), every operation in float32"""
    f = np.arange(TAB, dtype=F) * F(1.0 / TAB)
    t = np.stack((F(1) - f, f), -1).astype(F)                                   # [phase, tap]
    return (t[:, None, :, None] * t[None, :, None, :]).astype(F)


def remap_linear_f32(img, mapx, mapy, rounding: str = "even", swap_phase: bool = False, border: str = "constant") -> np.ndarray:
    """cv.remap(img f32, mapx, mapy, INTER_LINEAR, BORDER_CONSTANT 0), restated.  The keyword arguments make the wrong variants:
    rounding 'trunc', the x and y phase exchanged, border 'replicate' (coordinates clamped instead of taps replaced by 0)."""
    img = np.asarray(img, F)
    sh, sw = img.shape
    shape = np.shape(mapx)
    X, okx = RO.quantise(np.ravel(mapx), rounding)
    Y, oky = RO.quantise(np.ravel(mapy), rounding)
    sx, sy = np.clip(X >> BITS, -32768, 32767), np.clip(Y >> BITS, -32768, 32767)
    fx, fy = X & (TAB - 1), Y & (TAB - 1)
    w = bilinear_table()[(fx, fy) if swap_phase else (fy, fx)]                   # [n, ky, kx]
    v = []
    for ky in (0, 1):
        for kx in (0, 1):
            yy, xx = sy + ky, sx + kx
            inside = (yy >= 0) & (yy < sh) & (xx >= 0) & (xx < sw)
            pix = img[np.clip(yy, 0, sh - 1), np.clip(xx, 0, sw - 1)]
            v.append(pix if border == "replicate" else np.where(inside, pix, F(0)))
    with np.errstate(invalid="ignore", over="ignore"):
        out = ((v[0] * w[:, 0, 0] + v[1] * w[:, 0, 1]) + v[2] * w[:, 1, 0]) + v[3] * w[:, 1, 1]
    assert out.dtype == F
    if border != "replicate":
        outside = (sx >= sw) | (sx + 2 <= 0) | (sy >= sh) | (sy + 2 <= 0)
        out = np.where(outside, F(0), out)
    out = np.where(okx & oky, out, F(0))
    return out.reshape(shape)


def bilinear_float(img, x, y):
    """the direct formula in fp64 at the real positions (x, y), pixels outside the picture counting 0:
    (1 - b) ((1 - a) v00 + a v01) + b ((1 - a) v10 + a v11); also the largest |tap| of every window"""
    img = np.asarray(img, np.float64)
    sh, sw = img.shape
    x, y = np.ravel(x).astype(np.float64), np.ravel(y).astype(np.float64)
    ix, iy = np.floor(x).astype(np.int64), np.floor(y).astype(np.int64)
    a, b = x - ix, y - iy

    def tap(yy, xx):
        inside = (yy >= 0) & (yy < sh) & (xx >= 0) & (xx < sw)
        return np.where(inside, img[np.clip(yy, 0, sh - 1), np.clip(xx, 0, sw - 1)], 0.0)

    v00, v01, v10, v11 = tap(iy, ix), tap(iy, ix + 1), tap(iy + 1, ix), tap(iy + 1, ix + 1)
    val = (1 - b) * ((1 - a) * v00 + a * v01) + b * ((1 - a) * v10 + a * v11)
    return val, np.max(np.abs([v00, v01, v10, v11]), axis=0)


# ---- the geometry of a frame --------------------------------------------------------------------------------------------------------
def project_uv(zf, XX, YY, P):
    """(u, v) in fp64: each row ((P0 X + P1 Y) + P2 z) + P3, then the two quotients"""
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        z = np.asarray(zf, F).astype(np.float64)
        r = [((P[k, 0] * XX + P[k, 1] * YY) + P[k, 2] * z) + P[k, 3] for k in range(3)]
        return r[0] / r[2], r[1] / r[2]


def rays_cam(u, v, Kinv):
    """[3, H * W]: q / |q| with q = ((Ki0 u + Ki1 v) + Ki2) per row"""
    u, v = np.ravel(u), np.ravel(v)
    with np.errstate(invalid="ignore", over="ignore"):
        q = np.stack([(Kinv[r, 0] * u + Kinv[r, 1] * v) + Kinv[r, 2] for r in range(3)])
        return q / np.sqrt((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2])


def normals(XX, YY, zf):
    """[H, W, 3] fp64: (-sx, -sy, 1) / sqrt((sx^2 + sy^2) + 1) from the float32 slopes of np.gradient"""
    dx, dy = VO.spacing(XX, YY)
    sy, sx = VO.gradient(np.asarray(zf, F), dy, dx)
    sx, sy = sx.astype(np.float64), sy.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        nn = np.sqrt((sx * sx + sy * sy) + 1.0)
        return np.stack((-(sx / nn), -(sy / nn), 1.0 / nn), -1)


def dolp(S):
    """sqrt(S1^2 + S2^2) / S0 in float32, as numpy computes it on float32 arrays"""
    S = np.asarray(S, F)
    with np.errstate(all="ignore"):
        out = np.sqrt(np.square(S[..., 1]) + np.square(S[..., 2])) / S[..., 0]
    assert out.dtype == F
    return out


def nan_to_num(S):
    """np.nan_to_num of a float32 array, written out: NaN -> 0, +-inf -> +-FLT_MAX"""
    S = np.asarray(S, F)
    out = np.where(np.isnan(S), F(0), S)
    out = np.where(out == np.inf, F(FLT_MAX), out)
    return np.where(out == -np.inf, F(-FLT_MAX), out).astype(F)


def frame(stokes3, Zframe, XX, YY, Pplane, cam_to_grid, K, datascale=1e-3, angle_limit=85.0, **variant):
    """one frame: dict of S [H, W, 3], occlusion, angles (fp64), dolp, normals, rays_cam, zf, mapx, mapy, not_up"""
    stokes3 = [np.asarray(s, F) for s in stokes3]
    Ih, Iw = stokes3[0].shape
    zf = VO.heights(Zframe, datascale)
    u, v = project_uv(zf, XX, YY, RO.pcam(Pplane, Iw, Ih))
    with np.errstate(invalid="ignore", over="ignore"):
        mapx, mapy = u.astype(F), v.astype(F)
    origin = np.asarray(cam_to_grid, np.float64)[:3, -1]
    march, ang, _, not_up = VO.visibility_frame(Zframe, XX, YY, origin, datascale, None)
    mask = march.copy()
    if angle_limit is not None:                         # the rule as visibility_frame applies it
        with np.errstate(all="ignore"):
            mask[(ang >= angle_limit) & ~(VO.rays(XX, YY, zf, origin)[..., 2] <= 0.0)] = 1
    S = np.stack([remap_linear_f32(s, mapx, mapy, **variant) for s in stokes3], -1)
    S[mask == 1] = np.nan
    return dict(S=S, occlusion=mask, march=march, angles=ang, dolp=dolp(S), normals=normals(XX, YY, zf), rays_cam=rays_cam(u, v, np.linalg.inv(np.asarray(K, np.float64))),
                zf=zf, mapx=mapx, mapy=mapy, not_up=not_up)


def setup(stokes, Z, XX, YY, Pplane, cam_to_grid, K, datascale=1e-3, angle_limit=85.0, total_frames=None, acc_dtype=np.float64,
          use_nan_to_num=True):
    """the sequence: per-frame arrays stacked, and Savg, Navg, Zavg, valid.  acc_dtype float32 and use_nan_to_num False are the
    mistakes the tests must be able to see.  `stokes` is a count x 3 x Ih x Iw array or a sequence of count (S0, S1, S2) triples
    whose picture size may change from frame to frame: every frame is projected with the Pcam of its own pictures, and the sums
    run over the frames in order whatever their sizes."""
    count, H, W = np.shape(Z)
    assert len(stokes) == count and all(len(s) == 3 and np.shape(s[0]) == np.shape(s[1]) == np.shape(s[2]) for s in stokes)
    frames = [frame(stokes[t], Z[t], XX, YY, Pplane, cam_to_grid, K, datascale, angle_limit) for t in range(count)]
    Savg, Navg = np.zeros((H, W, 3), acc_dtype), np.zeros((H, W, 3), acc_dtype)
    Zavg, valid = np.zeros((H, W), acc_dtype), np.zeros((H, W), acc_dtype)
    with np.errstate(all="ignore"):
        for f in frames:
            Savg = Savg + (nan_to_num(f["S"]) if use_nan_to_num else f["S"]).astype(acc_dtype)
            valid = valid + (1.0 - f["occlusion"].astype(np.float64)).astype(acc_dtype)
            Navg = Navg + f["normals"].astype(acc_dtype)
            Zavg = Zavg + f["zf"].astype(acc_dtype)
        Savg = Savg / valid[..., None]
        Zavg = Zavg / acc_dtype(count if total_frames is None else total_frames)
        Navg = Navg / np.sqrt((Navg[..., 0] * Navg[..., 0] + Navg[..., 1] * Navg[..., 1]) + Navg[..., 2] * Navg[..., 2])[..., None]
    out = {k: np.stack([f[k] for f in frames]) for k in ("S", "occlusion", "march", "angles", "dolp", "normals", "rays_cam", "zf")}
    out.update(Savg=Savg, Navg=Navg, Zavg=Zavg, valid=valid, not_up=sum(f["not_up"] for f in frames),
               occluded_percent=100.0 * out["occlusion"].reshape(count, -1).sum(1) / float(H * W))
    return out


# ---- clip and zeromean ---------------------------------------------------------------------------------------------------------------
def clip_cube(x, lo, hi):
    x = np.asarray(x, F)
    out = np.minimum(np.maximum(x, F(lo)), F(hi))
    ok = ~np.isnan(out)
    return out, (out[ok].min() if ok.any() else F(np.nan)), (out[ok].max() if ok.any() else F(np.nan))


def zeromean(x, reverse: bool = False):
    """the mean by an fp64 loop over the frames in order, then float32(double(x) - mean).  reverse=True adds the frames from the
    last to the first: the mistake the tests must be able to see."""
    x = np.asarray(x, F)
    with np.errstate(invalid="ignore", over="ignore"):
        total = np.zeros(x.shape[1:], np.float64)
        for t in (range(x.shape[0] - 1, -1, -1) if reverse else range(x.shape[0])):
            total = total + x[t].astype(np.float64)
        mean = total / np.float64(x.shape[0])
        return (x.astype(np.float64) - mean).astype(F)


# ---- scenes -------------------------------------------------------------------------------------------------------------------------
def spread_cube(shape, seed, pairs: bool = True):
    """count x H x W float32: magnitudes over six decades and, in about half of the series of three frames or more, two frames that
    hold +B and -B with B = 2^55 .. 2^69.  Between the two the running fp64 sum is a multiple of ulp(B) >= 8 and drops what it is
    given below that, so which frames are lost depends on the order of the sum: adding the frames backwards gives another mean."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(shape) * 10.0 ** rng.uniform(-2, 4, shape)).astype(F)
    count = shape[0]
    if pairs and count >= 3:
        a = rng.integers(0, count, shape[1:])
        b = (a + rng.integers(1, count, shape[1:])) % count
        big = (2.0 ** rng.integers(55, 70, shape[1:]) * rng.choice([-1.0, 1.0], shape[1:])).astype(F)
        on = rng.random(shape[1:]) < 0.5
        np.put_along_axis(x, a[None], np.where(on, big, np.take_along_axis(x, a[None], 0)[0])[None], 0)
        np.put_along_axis(x, b[None], np.where(on, -big, np.take_along_axis(x, b[None], 0)[0])[None], 0)
    return x


def stokes_pictures(count, h, w, seed):
    """count x 3 x h x w float32: S0 positive around 1, S1 and S2 signed and smaller, all textured so that every tap matters"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    out = np.empty((count, 3, h, w), F)
    for t in range(count):
        out[t, 0] = 1.0 + 0.4 * np.sin(x / 6.1 + t) * np.cos(y / 5.3) + 0.05 * rng.standard_normal((h, w))
        out[t, 1] = 0.3 * np.cos(x / 4.7 - 0.5 * t) + 0.05 * rng.standard_normal((h, w))
        out[t, 2] = 0.25 * np.sin(y / 3.9 + 0.3 * t) + 0.05 * rng.standard_normal((h, w))
    return out


def intrinsics(Iw, Ih):
    f = 1.2 * Iw
    return np.array([[f, 0.0, Iw / 2.0 - 0.5], [0.0, 1.01 * f, Ih / 2.0 + 0.25], [0.0, 0.0, 1.0]])


# ---- the seas of the edge tests (tests/test_polarimetric_edges_gpu.py) ----------------------------------------------------------------
# name: H, W, du, seed, amp, camera side, height, back, footprint, picture (Ih, Iw).  Chosen on the CPU so that the oracle has no cell
# at or above the camera and none whose angle lies within visibility_oracle.angle_bound of 85 degrees: test_edge_scenes_are_decided in
# tests/test_polarimetric.py holds them to that without a GPU.
SMALL = {
    "2x2": (2, 2, 0.5, 21, 0.6, "west", 4.0, 3.0, "inside", (240, 320)),
    "2x65": (2, 65, 0.25, 22, 1.0, "west", 5.0, 4.0, "inside", (240, 320)),
    "5x3": (5, 3, 0.5, 23, 0.8, "south", 4.0, 3.0, "inside", (240, 320)),
    "9x130": (9, 130, 0.25, 24, 1.0, "south", 5.0, 6.0, "crossing", (240, 320)),
    "5x3, 2 x 3 pictures": (5, 3, 0.5, 23, 0.8, "south", 4.0, 3.0, "crossing", (2, 3)),
}
# one ragged column beyond a block of 64 x 4 cells; three frames for the strided views, five for the iterable whose pictures change
# their size after the second frame and for `batch` with a ragged last launch
STRIDED = (64, 65, 0.25, 31, 1.0, "west", 4.0, 12.0, "crossing", (240, 320), 3)
FIVE_SIZES = ((240, 320), (240, 320), (120, 200), (120, 200), (120, 200))
CHANGING = (64, 65, 0.25, 32, 1.0, "west", 4.0, 12.0, "crossing", FIVE_SIZES, 5)
RAGGED = (64, 65, 0.25, 32, 1.0, "west", 4.0, 12.0, "crossing", (120, 200), 5)


def make_scene(H, W, du, seed, amp, side, height, back, kind, sizes, count=3):
    """inputs of a sea of `count` frames whose pictures have the sizes (Ih, Iw) of `sizes`, one for all frames or one per frame:
    (stokes, Z, XX, YY, Pplane, cam, K), stokes an array where the sizes are equal and a list of count arrays of 3 x Ih x Iw if not"""
    sizes = [sizes] * count if isinstance(sizes[0], int) else list(sizes)
    XX, YY = VO.make_grid(H, W, du)
    cam = VO.camera(XX, YY, side, height, back)
    Z = np.stack([VO.make_sea(H, W, du, seed, amp, t=0.7 * t) for t in range(count)])
    if H * W > 100:
        Z[1, H // 2, W // 3:W // 3 + 3] = np.nan
    cx, cy = XX.mean(), YY.mean()
    shift = np.eye(4)
    shift[0, 3], shift[1, 3] = -cx, -cy
    Ih, Iw = sizes[0]
    Pplane = RO.pplane(Iw, Ih, XX - cx, YY - cy, kind) @ shift
    stokes = [stokes_pictures(count, h, w, seed)[t] for t, (h, w) in enumerate(sizes)]
    if Ih * Iw > 100:                                   # propagate through the sums of their windows
        stokes[0][1, Ih // 2, Iw // 2] = np.nan
        stokes[-1][0, sizes[-1][0] // 2 + 7, sizes[-1][1] // 2 - 9] = np.inf
    if len(set(sizes)) == 1:
        stokes = np.stack(stokes)
    return stokes, Z, XX, YY, Pplane, cam, intrinsics(Iw, Ih)


def near_85(want, XX, YY, cam):
    """how many cells of the oracle's frames have an angle within visibility_oracle.angle_bound of 85 degrees"""
    near_all = 0
    for zf in want["zf"]:
        a64, n = VO.noise(XX, YY, zf, cam[:3, 3])
        with np.errstate(invalid="ignore"):
            near_all += int((np.abs(a64 - 85.0) <= VO.angle_bound(a64, n)).sum())
    return near_all


def ulps_f32(a, b):
    """|a - b| in units of the last place of float32 values (same sign assumed where it matters; NaN pairs count 0)"""
    a, b = np.asarray(a, F), np.asarray(b, F)
    both_nan = np.isnan(a) & np.isnan(b)
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, -(ia & 0x7fffffff), ia)
    ib = np.where(ib < 0, -(ib & 0x7fffffff), ib)
    return np.where(both_nan, 0, np.abs(ia - ib))


def ulps_f64(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    both_nan = np.isnan(a) & np.isnan(b)
    with np.errstate(invalid="ignore"):
        return np.where(both_nan, 0.0, np.abs(a - b) / np.spacing(np.maximum(np.abs(a), np.abs(b))))
