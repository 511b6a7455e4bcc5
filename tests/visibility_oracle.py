"""numpy restatement of the reference's visibility map (postproc/wasspost/wasspost.py:495-621, geometry.py:5-100) for the
visibility tests, with the decisions taken where the reference is undefined.  Test infrastructure only:
nothing here is imported by the package.

Per frame: zf = float32(Z * float32(datascale)); the unit ray d from every cell to the camera in fp64, (r0^2 + r1^2) + r2^2 under
the root; slopes as np.gradient gives them for a FLOAT32 array (differences in float32, quotients rounded to float32 -- the
casts are explicit, so that numpy's promotion rules do not matter); normals and the angle in fp64; the march over
Zc = float64(zf) / dx with an accumulated fp64 position, rounding half to even, at most max(H, W) steps.
A ray that has ended takes no further part; whether ended rays are also dropped from the arrays (compact=True, the default,
which keeps 1024 x 1024 cases short) or kept and masked (compact=False) changes no arithmetic: tests compare the two.
"""
import numpy as np

DEG = 180.0 / np.pi


def heights(Z, datascale=1e-3):
    return (np.asarray(Z, np.float32) * np.float32(datascale)).astype(np.float32)


def gradient(zf, dy, dx):
    """(slope_y, slope_x) = np.gradient(zf, dy, dx): the dtype of zf is kept."""
    def line(f, d, axis):
        f = np.moveaxis(f, axis, 0)
        out = np.empty(f.shape, f.dtype)
        d = np.float64(d)
        out[1:-1] = (f[2:] - f[:-2]).astype(np.float64) / (np.float64(2.0) * d)
        out[0] = (f[1] - f[0]).astype(np.float64) / d
        out[-1] = (f[-1] - f[-2]).astype(np.float64) / d
        return np.moveaxis(out, 0, axis)
    return line(zf, dy, 0), line(zf, dx, 1)


def spacing(XX, YY):
    return np.float64(XX[0, 1] - XX[0, 0]), np.float64(YY[1, 0] - YY[0, 0])


def rays(XX, YY, zf, origin, dtype=np.float64):
    """d [H, W, 3]: the unit direction from every cell to the camera."""
    o = np.asarray(origin, np.float64).astype(dtype)
    r = np.stack((XX.astype(dtype) - o[0], YY.astype(dtype) - o[1], zf.astype(dtype) - o[2]), -1)
    with np.errstate(all="ignore"):
        n = np.sqrt((r[..., 0] * r[..., 0] + r[..., 1] * r[..., 1]) + r[..., 2] * r[..., 2])
        return -(r / n[..., None])


def angles(XX, YY, zf, origin, dtype=np.float64):
    """incident angle in degrees [H, W] in `dtype`; the slopes are float32 values by definition, in every dtype"""
    dx, dy = spacing(XX, YY)
    sy, sx = gradient(zf, dy, dx)
    sx, sy = sx.astype(dtype), sy.astype(dtype)
    with np.errstate(all="ignore"):
        nn = np.sqrt((sx * sx + sy * sy) + dtype(1.0))
        n0, n1, n2 = -(sx / nn), -(sy / nn), dtype(1.0) / nn
        d = rays(XX, YY, zf, origin, dtype)
        c = (n0 * d[..., 0] + n1 * d[..., 1]) + n2 * d[..., 2]
        scale = dtype(DEG) if dtype is np.float64 else dtype(180.0) / np.arccos(dtype(-1.0))
        return np.arccos(c) * scale


def ulp_f64(v):
    v = np.abs(np.asarray(v, np.float64))
    return np.where(np.isfinite(v), np.spacing(np.where(np.isfinite(v), v, 0.0)), 0.0)


def noise(XX, YY, zf, origin):
    """(angle64, n): per cell n = |angle64 - angle_longdouble| + 0.5 ulp_f64(angle64).  The first term is the oracle's own fp64 error
    from the float32 slopes onward (the normal, the ray, the product, acos), which near 0 degrees, where acos is ill-conditioned,
    is many ulps; the second is the rounding that every fp64 value of the angle carries and that the first term misses
    wherever the two evaluations happen to round alike.  NaN where the oracle is NaN."""
    a64 = angles(XX, YY, zf, origin, np.float64)
    ald = angles(XX, YY, zf, origin, np.longdouble)
    with np.errstate(all="ignore"):
        n = np.abs(a64.astype(np.longdouble) - ald).astype(np.float64) + 0.5 * ulp_f64(a64)
    return a64, n


def half_ulp_f32(v):
    v = np.abs(np.asarray(v, np.float64))
    _, e = np.frexp(v)
    return np.where(v == 0, 2.0 ** -150, 0.5 * np.exp2(np.maximum(e.astype(np.float64) - 24.0, -149.0)))


def angle_bound(a64, n):
    """|gpu_f32 - angle64| <= 0.5 ulp_f32(angle64) + 4 n"""
    return half_ulp_f32(a64) + 4.0 * n


def frame_max(Zc):
    fin = np.isfinite(Zc)
    return np.float64(Zc[fin].max()) if fin.any() else np.float64(-np.inf)


def march(ZZ, ray_d, invert_y_axis=False, maxz=None, mode="exact", compact=True):
    """(mask uint8 [H, W], steps taken): compute_occlusion_mask(ZZ, ray_d, invert_y_axis) on fp64 arrays.  Rays without ray2 > 0
    and rays of NaN cells do not start.  mode: 'exact', or one of the mistakes the tests must be able to see: 'transposed' (x and
    y of the step swapped), 'kstep' (start + k * step instead of the accumulated sum), 'trunc' (truncation instead of rounding
    half to even).  maxz: the frame's maximum, or a wrong one."""
    ZZ = np.asarray(ZZ, np.float64)
    ray_d = np.asarray(ray_d, np.float64)
    H, W = ZZ.shape
    if maxz is None:
        maxz = frame_max(ZZ)
    with np.errstate(all="ignore"):
        m = np.maximum(np.abs(ray_d[..., 0]), np.abs(ray_d[..., 1]))
        step = (ray_d / m[..., None]).reshape(-1, 3)
    if invert_y_axis:
        step[:, 1] = -step[:, 1]
    if mode == "transposed":
        step = step[:, [1, 0, 2]]
    jj, ii = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    start = np.stack((jj.ravel(), ii.ravel(), ZZ.ravel()), -1)
    alive = (ray_d[..., 2].ravel() > 0.0) & ~np.isnan(ZZ.ravel())
    idx = np.arange(H * W)
    p = start.copy()
    mask = np.zeros(H * W, np.uint8)
    rnd = np.trunc if mode == "trunc" else np.rint
    steps = 0
    for k in range(1, max(H, W) + 1):
        if compact:
            idx, p, step, start = idx[alive], p[alive], step[alive], start[alive]
            alive = np.ones(idx.size, bool)
        if not alive.any():
            break
        steps = k
        with np.errstate(all="ignore"):
            p = start + np.float64(k) * step if mode == "kstep" else p + step
            rj, ri = rnd(p[:, 0]), rnd(p[:, 1])
            ok = alive & (ri >= 0.0) & (ri < H) & (rj >= 0.0) & (rj < W) & (p[:, 2] <= maxz)
            z = ZZ[np.where(ok, ri, 0.0).astype(np.intp), np.where(ok, rj, 0.0).astype(np.intp)]
            occ = ok & (z >= p[:, 2])
        mask[idx[occ]] = 1
        alive = ok & ~occ
    return mask.reshape(H, W), steps


def visibility_frame(Zframe, XX, YY, origin, datascale=1e-3, angle_limit=88.0, maxz=None, mode="exact", compact=True):
    """One frame: (mask uint8, angle float64 degrees, steps, cells at or above the camera)."""
    zf = heights(Zframe, datascale)
    dx, _ = spacing(XX, YY)
    a = angles(XX, YY, zf, origin)
    d = rays(XX, YY, zf, origin)
    with np.errstate(all="ignore"):
        Zc = zf.astype(np.float64) / dx
        not_up = d[..., 2] <= 0.0
    mask, steps = march(Zc, d, maxz=maxz, mode=mode, compact=compact)
    if angle_limit is not None and angle_limit >= 0 and np.isfinite(angle_limit):
        with np.errstate(all="ignore"):
            mask[(a >= angle_limit) & ~not_up] = 1
    return mask, a, steps, int(not_up.sum())


def visibility(Z, XX, YY, origin, datascale=1e-3, angle_limit=88.0):
    """The cube: (masks, angles float64, percent occluded per frame)."""
    Z = np.asarray(Z)
    out = [visibility_frame(Z[t], XX, YY, origin, datascale, angle_limit) for t in range(Z.shape[0])]
    masks = np.stack([o[0] for o in out])
    return masks, np.stack([o[1] for o in out]), 100.0 * masks.reshape(Z.shape[0], -1).sum(1) / float(Z.shape[1] * Z.shape[2])


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def _frac(v):
    return v - np.floor(v)


def make_grid(H, W, du, x0=0.0, y0=0.0):
    XX, YY = np.meshgrid(x0 + du * np.arange(W, dtype=np.float64), y0 + du * np.arange(H, dtype=np.float64))
    return XX, YY


def make_sea(H, W, du, seed=0, amp=1.0, heading=0.3, t=0.0):
    """An H x W float32 frame in MILLIMETRES: twelve cosines with wavelengths of 4 to 32 m around `heading` (radians), phases and
    directions from additive recurrences (closed form, no random-number stream), scaled to a significant height of `amp` metres
    (4 sigma); `t` shifts the phases, for the frames of a cube."""
    XX, YY = make_grid(H, W, du)
    k = np.arange(1, 13, dtype=np.float64)
    lam = 4.0 + 28.0 * _frac(k * 0.5698402910 + 0.17 * seed)
    th = heading + 1.2 * (_frac(k * 0.7548776662 + 0.31 * seed) - 0.5)
    ph = 2.0 * np.pi * _frac((seed + 1.0) * k * 0.6180339887)
    a = np.sqrt(lam)
    a *= (amp / 4.0) / np.sqrt(0.5 * np.sum(a * a))
    z = np.zeros((H, W))
    for n in range(12):
        kk = 2.0 * np.pi / lam[n]
        z += a[n] * np.cos(kk * (np.cos(th[n]) * XX + np.sin(th[n]) * YY) - np.sqrt(9.81 * kk) * t + ph[n])
    return (1000.0 * z).astype(np.float32)


def camera(XX, YY, side="west", height=6.0, back=5.0, along=0.37):
    """A 4 x 4 Cam-to-grid matrix whose last column is a camera `height` metres up and `back` metres outside the given side of the
    grid ('west', 'east': rays dominated by x; 'south', 'north': by y), at the fraction `along` of that side; 'over': above the
    grid, between nodes; 'over_node': exactly above a node."""
    x0, x1, y0, y1 = XX[0, 0], XX[0, -1], YY[0, 0], YY[-1, 0]
    du = XX[0, 1] - XX[0, 0]
    if side == "west":
        o = (x0 - back, y0 + along * (y1 - y0), height)
    elif side == "east":
        o = (x1 + back, y0 + along * (y1 - y0), height)
    elif side == "south":
        o = (x0 + along * (x1 - x0), y0 - back, height)
    elif side == "north":
        o = (x0 + along * (x1 - x0), y1 + back, height)
    elif side == "over":
        o = (x0 + along * (x1 - x0) + 0.3 * du, y0 + (1.0 - along) * (y1 - y0) + 0.4 * du, height)
    elif side == "over_node":
        o = (XX[YY.shape[0] // 3, XX.shape[1] // 2], YY[YY.shape[0] // 3, XX.shape[1] // 2], height)
    else:
        raise ValueError(side)
    M = np.eye(4)
    M[:3, 3] = o
    return M


def tie_scene(H, W, s=0.1):
    """(ZZ, ray_d, rows) for compute_occlusion_mask: a case that tells the accumulated position from k * step, which on a sea
    differ by rounding only and change no mask.  Every ray is (-1, 0, s) over a flat surface, so cell (i, k) arrives above
    column 0 after k steps at the height s + s + ... (k terms); in each of `rows` column 0 carries a wall of exactly that
    height for a k at which k * s is one rounding larger.  The accumulated ray meets the wall (z >= p2 holds with equality), the
    multiplied one passes over it: one cell per row of `rows` differs.  All other rows get steep rays that leave at once."""
    acc = np.zeros(W)
    for k in range(1, W):
        acc[k] = acc[k - 1] + np.float64(s)
    cand = [k for k in range(1, W) if acc[k] < np.float64(k) * np.float64(s)]
    assert cand, "no k with accumulated < multiplied"
    ZZ = np.zeros((H, W))
    ray_d = np.zeros((H, W, 3))
    ray_d[..., 0] = -1.0
    ray_d[..., 2] = 1e3
    rows = list(range(0, H, max(1, H // 32)))[:32]
    for n, i in enumerate(rows):
        ZZ[i, 0] = acc[cand[(7 * n) % len(cand)]]
        ray_d[i, :, 2] = s
    return ZZ, ray_d, rows
