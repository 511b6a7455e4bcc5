"""numpy restatement of wass_amd.postproc.pyr_up and radiance_upscaled, the weight matrix the restatement is checked against, and
the inputs the CPU tests and the OpenCV pin share.  Test infrastructure only.

One level of pyr_up restates OpenCV 4.5.5's scalar pyrUp_ (modules/imgproc/src/pyramids.cpp) from knowledge: cv2 is not available
where this was written, so it is UNPINNED against the real OpenCV (scripts/pin_with_opencv.py writes tests/golden/pyrup_pin.npz
where cv2 exists; tests/test_pyramid.py reads it when present).  Everything is computed in the input's dtype, one numpy operation
per product and per sum (numpy never fuses them), in this order:

  along x, source row s of length w, r of length 2w:
      0 < j < w-1   r[2j] = (s[j-1] + s[j]*6) + s[j+1]     r[2j+1] = (s[j] + s[j+1])*4
      j = 0         r[0]  = s[0]*6 + s[1]*2                r[1]    = (s[0] + s[1])*4
      j = w-1       r[2w-2] = s[w-2] + s[w-1]*7            r[2w-1] = s[w-1]*8
  (the ends of a row as OpenCV writes them out by hand)
  then along y, on the rows R of the x pass, the three-tap form on reflected indices up(i) = i-1 (1 for i = 0),
  dn(i) = i+1 (h-1 for i = h-1), as OpenCV's row loop does:
      out[2i]   = ((R[up(i)] + R[i]*6) + R[dn(i)]) * (1/64)
      out[2i+1] = ((R[i] + R[dn(i)])*4) * (1/64)
"""
import numpy as np

import radiance_oracle as RO

MAX_LEVELS = 4


def _up_x(s):
    """the x pass over the last axis"""
    T = s.dtype.type
    w = s.shape[-1]
    r = np.empty(s.shape[:-1] + (2 * w,), s.dtype)
    a, b, c = s[..., :-2], s[..., 1:-1], s[..., 2:]
    r[..., 2:2 * w - 2:2] = (a + b * T(6)) + c
    r[..., 1:2 * w - 2:2] = (s[..., :-1] + s[..., 1:]) * T(4)
    r[..., 0] = s[..., 0] * T(6) + s[..., 1] * T(2)
    r[..., 2 * w - 2] = s[..., w - 2] + s[..., w - 1] * T(7)
    r[..., 2 * w - 1] = s[..., w - 1] * T(8)
    return r


def _up_y(R):
    """the y pass over the axis before the last, with the factor 1/64"""
    T = R.dtype.type
    h = R.shape[-2]
    i = np.arange(h)
    up, dn = np.where(i == 0, 1, i - 1), np.where(i == h - 1, h - 1, i + 1)
    out = np.empty(R.shape[:-2] + (2 * h, R.shape[-1]), R.dtype)
    out[..., 0::2, :] = ((R[..., up, :] + R * T(6)) + R[..., dn, :]) * T(0.015625)
    out[..., 1::2, :] = ((R + R[..., dn, :]) * T(4)) * T(0.015625)
    return out


def pyr_up(a, levels: int = 1) -> np.ndarray:
    """cv.pyrUp applied `levels` times to an H x W picture or to every frame of a count x H x W cube, float32 or float64"""
    a = np.asarray(a)
    if a.dtype not in (np.float32, np.float64):
        raise ValueError("float32 or float64")
    if a.ndim not in (2, 3):
        raise ValueError("H x W or count x H x W")
    if a.shape[-1] < 2 or a.shape[-2] < 2:
        raise ValueError("sides of at least 2")
    if not 1 <= int(levels) <= MAX_LEVELS:
        raise ValueError("levels from 1 to 4")
    with np.errstate(invalid="ignore", over="ignore"):
        for _ in range(int(levels)):
            a = _up_y(_up_x(a))
    return a


def weights(n: int) -> np.ndarray:
    """the 2n x n matrix U of one axis: r = U s, with the integer weights of the rules above (the factor 1/8 per axis left out)"""
    U = np.zeros((2 * n, n))
    for i in range(n):
        U[2 * i, i] += 6
        U[2 * i, i - 1 if i > 0 else 1] += 1
        U[2 * i, i + 1 if i < n - 1 else n - 1] += 1
        U[2 * i + 1, i] += 4
        U[2 * i + 1, i + 1 if i < n - 1 else n - 1] += 4
    return U


def radiance_upscaled(images, Z, XX, YY, Pplane, upscalefactor=2, datascale=1e-3):
    """wass_amd.postproc.radiance_upscaled: zf = Z * float32(datascale) in float32, pyr_up of zf (float32) and of the grid (fp64)
    upscalefactor - 1 times, then radiance_oracle's projection and sampler on the finer grid (zf is already in metres: scale 1)"""
    levels = int(upscalefactor) - 1
    if levels == 0:
        return RO.radiance(images, Z, XX, YY, Pplane, datascale)
    with np.errstate(invalid="ignore", over="ignore"):
        zf = np.asarray(Z, np.float32) * np.float32(datascale)
    zu = pyr_up(zf, levels)
    Xu, Yu = pyr_up(np.asarray(XX, np.float64), levels), pyr_up(np.asarray(YY, np.float64), levels)
    out = np.empty(zu.shape, np.float32)
    for t in range(len(zu)):
        P = RO.pcam(Pplane, images[t].shape[1], images[t].shape[0])
        mx, my = RO.project(zu[t], Xu, Yu, P, 1.0)
        out[t] = RO.remap_lanczos4(images[t], mx, my).astype(np.float32) / np.float32(255.0)
    return out


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
SHAPES = [(2, 2), (2, 3), (3, 2), (5, 7), (33, 17)]


def picture(h, w, dtype, seed=0):
    """values of mixed sign and magnitude, so that every rounding of the sums shows"""
    rng = np.random.default_rng(1000 * h + w + seed)
    return (rng.standard_normal((h, w)) * 10.0 ** rng.uniform(-2, 3, (h, w))).astype(dtype)


def pin_inputs():
    """name -> input of the OpenCV pin: the pictures of tests/test_pyramid.py"""
    return {f"{np.dtype(dt).name}_{h}x{w}": picture(h, w, dt) for dt in (np.float32, np.float64) for h, w in SHAPES}
