"""numpy restatement of the polarimetric preparation (wass_amd.prepare.polarimetric_prepare), staged: every intermediate picture is
materialised in float32, every product and sum rounded on its own.  Test infrastructure only: nothing here is imported by the package.

OpenCV is not available where this was written: resize, undistort and remap are restated from knowledge of OpenCV 4.5.5 and are
UNPINNED against it.  What ties the map and the sampler to what exists: pushing a u8 picture through undistort_map and the
fixed-point bilinear table equals oracle.undistort (tests/test_prepare_pol.py); the float table is polarimetric_oracle's."""
import numpy as np

import polarimetric_oracle as PO

F = np.float32
NAMES = ("I0", "I45", "I90", "I135")
PI_REF = F(3.1415)                                       # the reference's constant
AOLP_SCALE = F(255.0 / 3.1415)
HDR_DEN = F(2.0) * F(0.3) * F(0.3)


# ---- stage 1: demosaic ---------------------------------------------------------------------------------------------------------------
def demosaic(I):
    """(I0, I45, I90, I135) u8 quarter pictures; an odd last row or column is dropped"""
    I = np.asarray(I, np.uint8)
    m, n = I.shape[0] // 2, I.shape[1] // 2
    I = I[:2 * m, :2 * n]
    return I[1::2, 1::2], I[0::2, 1::2], I[0::2, 0::2], I[1::2, 0::2]


def to_float(q):
    return q.astype(F) * F(F(1.0) / F(255.0))


# ---- stage 2: upscale x2 --------------------------------------------------------------------------------------------------------------
def up_coeffs(size):
    """per destination index: s, s + 1 (clamped for the load only: its weight is 0 there) and a in float32"""
    d = np.arange(2 * size, dtype=F)
    f = (d + F(0.5)) * F(0.5) - F(0.5)
    s = np.floor(f)
    a = (f - s).astype(F)
    s = s.astype(np.int64)
    lo, hi = s < 0, s >= size - 1
    a = np.where(lo | hi, F(0), a).astype(F)
    s = np.where(lo, 0, np.where(hi, size - 1, s))
    return s, np.minimum(s + 1, size - 1), a


def upscale2(q):
    """cv::resize(q, Size(), 2, 2, INTER_LINEAR) for a float32 picture: along x, then along y"""
    q = np.asarray(q, F)
    s, s1, a = up_coeffs(q.shape[1])
    h = q[:, s] * (F(1) - a) + q[:, s1] * a
    s, s1, a = up_coeffs(q.shape[0])
    v = h[s, :] * (F(1) - a)[:, None] + h[s1, :] * a[:, None]
    assert v.dtype == F
    return v


# ---- stage 3: undistort -----------------------------------------------------------------------------------------------------------------
def _inv3(m):
    """cv::invert of a 3 x 3 in closed form, the operations in the library's order"""
    m = [float(v) for v in np.ravel(m)]
    d = m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6])
    d = 1.0 / d
    return [(m[4] * m[8] - m[5] * m[7]) * d, (m[2] * m[7] - m[1] * m[8]) * d, (m[1] * m[5] - m[2] * m[4]) * d,
            (m[5] * m[6] - m[3] * m[8]) * d, (m[0] * m[8] - m[2] * m[6]) * d, (m[2] * m[3] - m[0] * m[5]) * d,
            (m[3] * m[7] - m[4] * m[6]) * d, (m[1] * m[6] - m[0] * m[7]) * d, (m[0] * m[4] - m[1] * m[3]) * d]


def undistort_map(w, h, K, dist):
    """(iu, iv) int64 [h, w]: where cv::undistort reads, in 1/32 pixel.  Stripes of max(1, 4096 / w) rows, the principal point shifted
    by the stripe's origin, the column value an accumulated sum, both divided by _w = ir[8] (which need not be 1 for a calibrated K), the
    polynomial in fp64, round to nearest even."""
    K = np.asarray(K, np.float64).reshape(3, 3)
    k = np.zeros(12)
    k[:len(np.ravel(dist))] = np.ravel(dist)
    xs, ys = np.empty(w), np.empty(h)
    stripe0 = min(max(1, 4096 // max(w, 1)), h)
    for y0 in range(0, h, stripe0):
        Ar = K.copy()
        Ar[1, 2] = K[1, 2] - y0
        ir = _inv3(Ar)
        if y0 == 0:                                     # ir[0], ir[2], ir[8] are the same in every stripe
            _x, ww = ir[2], 1.0 / ir[8]
            for j in range(w):
                xs[j] = _x * ww
                _x += ir[0]
        for i in range(min(stripe0, h - y0)):
            ys[y0 + i] = (i * ir[4] + ir[5]) * (1.0 / (i * ir[7] + ir[8]))
    x, y = np.meshgrid(xs, ys)
    x2, y2 = x * x, y * y
    r2, _2xy = x2 + y2, 2 * x * y
    kr = (1 + ((k[4] * r2 + k[1]) * r2 + k[0]) * r2) / (1 + ((k[7] * r2 + k[6]) * r2 + k[5]) * r2)
    xd = (x * kr + k[2] * _2xy + k[3] * (r2 + 2 * x2) + k[8] * r2 + k[9] * r2 * r2)
    yd = (y * kr + k[2] * (r2 + 2 * y2) + k[3] * _2xy + k[10] * r2 + k[11] * r2 * r2)
    u, v = K[0, 0] * xd + K[0, 2], K[1, 1] * yd + K[1, 2]
    iu = np.rint(np.clip(u * 32, -2147483648.0, 2147483647.0)).astype(np.int64)
    iv = np.rint(np.clip(v * 32, -2147483648.0, 2147483647.0)).astype(np.int64)
    return iu, iv


def _window(iu, iv):
    """the window's origin (the plain cast to int16 of the CV_16SC2 map: it wraps) and the phase"""
    wrap = lambda q: ((q >> 5) + 32768) % 65536 - 32768
    return wrap(iu), wrap(iv), (iv & 31) * 32 + (iu & 31)


def _taps(img, sx, sy):
    sh, sw = img.shape
    out = []
    for ky in (0, 1):
        for kx in (0, 1):
            yy, xx = sy + ky, sx + kx
            inside = (yy >= 0) & (yy < sh) & (xx >= 0) & (xx < sw)
            out.append(np.where(inside, img[np.clip(yy, 0, sh - 1), np.clip(xx, 0, sw - 1)], img.dtype.type(0)))
    return out


def remap_fixed_u8(img, iu, iv, itab):
    """remapBilinear for u8 through the map: int16 weights scaled by 2^15 (itab [1024, 2, 2]), (sum + 2^14) >> 15"""
    sx, sy, a = _window(iu, iv)
    v = [t.astype(np.int64) for t in _taps(np.asarray(img, np.uint8), sx, sy)]
    w = np.asarray(itab, np.int64)[a]
    total = v[0] * w[..., 0, 0] + v[1] * w[..., 0, 1] + v[2] * w[..., 1, 0] + v[3] * w[..., 1, 1]
    return np.clip((total + (1 << 14)) >> 15, 0, 255).astype(np.uint8)


def remap_float(img, iu, iv):
    """remapBilinear for float32 through the same map: the float table, ((v00 w00 + v01 w01) + v10 w10) + v11 w11"""
    sx, sy, a = _window(iu, iv)
    v = _taps(np.asarray(img, F), sx, sy)
    w = PO.bilinear_table().reshape(1024, 2, 2)[a]
    out = ((v[0] * w[..., 0, 0] + v[1] * w[..., 0, 1]) + v[2] * w[..., 1, 0]) + v[3] * w[..., 1, 1]
    assert out.dtype == F
    return out


# ---- stages 4 to 8 ----------------------------------------------------------------------------------------------------------------------
def mix(a0, a45, a90, a135):
    k1, k2 = F(0.75), F(0.25)
    return (((k1 * a0 + k2 * a45) - k2 * a90) + k2 * a135, ((k2 * a0 + k1 * a45) + k2 * a90) - k2 * a135,
            ((-k2 * a0 + k2 * a45) + k1 * a90) + k2 * a135, ((k2 * a0 - k2 * a45) + k2 * a90) + k1 * a135)


def stokes(I0, I45, I90, I135):
    return np.stack(((((I0 + I45) + I90) + I135) * F(0.5), I0 - I90, I45 - I135))


def sat_u8(v):
    """cv::saturate_cast<uchar> of a float: round half to even, clamp, NaN -> 0"""
    with np.errstate(invalid="ignore"):
        r = np.rint(np.asarray(v))
        r = np.where(np.isnan(r), 0, np.clip(r, 0, 255))
    return r.astype(np.uint8)


def nan_range(a):
    ok = ~np.isnan(a)
    return (F(a[ok].min()), F(a[ok].max())) if ok.any() else (F(np.nan), F(np.nan))


def hdr_f32(I):
    """HDR * 255.0f in the float32 chain; the exponential in fp64, rounded once"""
    with np.errstate(all="ignore"):
        w = []
        for c in I:
            d = c - F(0.5)
            arg = (F(-1.0) * (d * d)) / HDR_DEN
            assert arg.dtype == F
            w.append(np.exp(arg.astype(np.float64)).astype(F))
        num = ((w[0] * I[0] + w[1] * I[1]) + w[2] * I[2]) + w[3] * I[3]
        den = ((w[0] + w[1]) + w[2]) + w[3]
        return (num / den) * F(255.0)


def hdr_f64(I):
    """the same from the same float32 channels, everything in fp64"""
    I = [c.astype(np.float64) for c in I]
    with np.errstate(all="ignore"):
        w = [np.exp(-1.0 * ((c - 0.5) * (c - 0.5)) / float(HDR_DEN)) for c in I]
        return sum(wi * c for wi, c in zip(w, I)) / sum(w) * 255.0


def dolp_f32(S):
    with np.errstate(all="ignore"):
        out = np.sqrt(S[1] * S[1] + S[2] * S[2]) / S[0]
    assert out.dtype == F
    return out


def aolp_f32(S):
    """the AOLP index before rint: the arctangent in fp64, folded into [0, 2 pi), rounded to float32"""
    ang = np.arctan2(S[1].astype(np.float64), S[2].astype(np.float64))
    ang = np.where(ang < 0.0, ang + 6.283185307179586, ang).astype(F)
    return ((ang - PI_REF) * F(0.5)) * AOLP_SCALE + F(127.0)


def aolp_f64(S):
    ang = np.arctan2(S[1].astype(np.float64), S[2].astype(np.float64))
    ang = np.where(ang < 0.0, ang + 6.283185307179586, ang)
    return ((ang - float(PI_REF)) * 0.5) * float(AOLP_SCALE) + 127.0


def prepare(mosaic, K, dist, hdr=False):
    """every stage of one frame: dict of quarter, up, und (4 float32 pictures each), I, S [3, 2m, 2n], ranges [8], image, image_f32,
    image_f64, dolp_f32, dolp, aolp_f32, aolp_f64, aolp, channels [4, 2m, 2n]"""
    quarter = [to_float(q) for q in demosaic(mosaic)]
    up = [upscale2(q) for q in quarter]
    H, W = up[0].shape
    iu, iv = undistort_map(W, H, K, dist)
    und = [remap_float(u, iu, iv) for u in up]
    I = mix(*und)
    S = stokes(*I)
    out = dict(quarter=quarter, up=up, und=und, I=I, S=S, iu=iu, iv=iv)
    if hdr:
        out["image_f32"], out["image_f64"] = hdr_f32(I), hdr_f64(I)
    else:
        out["image_f32"] = S[0] * F(127.0)
        out["image_f64"] = out["image_f32"].astype(np.float64)
    out["image"] = sat_u8(out["image_f32"])
    out["dolp_f32"] = dolp_f32(S)
    with np.errstate(all="ignore"):
        out["dolp"] = sat_u8(out["dolp_f32"] * F(255.0))
    out["aolp_f32"], out["aolp_f64"] = aolp_f32(S), aolp_f64(S)
    out["aolp"] = sat_u8(out["aolp_f32"])
    out["channels"] = np.stack([sat_u8(c * F(255.0)) for c in I])
    out["ranges"] = np.array([v for a in (S[0], S[1], S[2], out["dolp_f32"]) for v in nan_range(a)], F)
    return out


# ---- the check of a picture that holds one transcendental function ------------------------------------------------------------------------
def transcendental_bound(o32, o64):
    """per pixel: half a float32 ulp of the fp64 value plus four times the oracle's own largest float32-against-fp64 difference"""
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(o64) & np.isfinite(o32)
        n = float(np.max(np.abs(o32.astype(np.float64) - o64)[ok])) if ok.any() else 0.0
        return 0.5 * np.spacing(np.abs(o64).astype(F)).astype(np.float64) + 4.0 * n, n


def near_boundary(o64, bound):
    """where the fp64 value lies within `bound` of a rounding boundary of the u8 picture, k + 0.5 for k = 0 ... 254 (below 0.5 and above
    254.5 the picture saturates: there is no boundary there); never for NaN"""
    with np.errstate(invalid="ignore"):
        frac = np.abs((o64 - np.floor(o64)) - 0.5)
        return np.isfinite(o64) & (frac <= bound) & (o64 >= 0.5 - bound) & (o64 <= 254.5 + bound)


# ---- scenes -----------------------------------------------------------------------------------------------------------------------------
def camera(w, h):
    """K0 of tests/test_prepare.py::_calibdir for a w x h picture"""
    return np.array([[0.9 * w, 0, w / 2 - 3.5], [0, 0.9 * w, h / 2 + 2.25], [0, 0, 1]])


DIST = {"zero": np.zeros(5), "calibdir": np.array([-0.21, 0.08, 1e-3, -5e-4, 0.01]), "barrel": np.array([-0.45, 0.0, 0.0, 0.0]),
        "eight": np.array([-0.19, 0.07, 8e-4, -4e-4, 0.012, 0.02, -0.015, 0.004]), "pincushion": np.array([0.45, 0.0, 0.0, 0.0])}


def random_mosaic(rows, cols, seed):
    return np.random.default_rng(seed).integers(0, 256, (rows, cols), dtype=np.uint8)


def polariser_mosaic(rows, cols, rho, phi):
    """a linear polariser in front of the camera: I_theta = S0 / 2 (1 + rho cos(2 theta - 2 phi)), S0 smooth; (mosaic u8, S0 fp64)"""
    y, x = np.mgrid[0:rows, 0:cols].astype(np.float64)
    S0 = 0.8 + 0.1 * np.sin(x / 400.0) * np.cos(y / 500.0)
    theta = np.empty((rows, cols))
    theta[1::2, 1::2], theta[0::2, 1::2], theta[0::2, 0::2], theta[1::2, 0::2] = 0.0, np.pi / 4, np.pi / 2, 3 * np.pi / 4
    I = S0 / 2 * (1 + rho * np.cos(2 * theta - 2 * phi))
    return np.rint(I * 255.0).astype(np.uint8), S0
