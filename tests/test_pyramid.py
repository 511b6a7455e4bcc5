"""tests/pyramid_oracle.py (the numpy restatement that the GPU's pyr_up must equal bit for bit, tests/test_pyramid_gpu.py) against
things it was not written from: the weight matrices in fp64, scipy's convolution of the zero-stuffed picture, exact cases, the
spread of a NaN; then the argument checks and the scratch formulas of wass_amd.postproc, which need no GPU.

The bound of the two comparisons.  With eps the spacing of the dtype at 1 (2^-23, 2^-52) and M the same weighted sum taken over
the absolute values of the picture (U_y |src| U_x^T / 64, the magnitude of what is summed: the weights are all positive, the
picture is of mixed sign), a computed cell differs from the exact one by at most 3 eps M to first order: per axis a cell is a
three-term sum (a + 6 b) + c, whose product and two sums each round once, or a two-term sum (b + c) * 4 with one rounding; every
rounding is at most eps / 2 of a partial sum that is at most the cell's share of M; that is 3 roundings, 1.5 eps M, per axis, 3 eps M
for both, and the factor 1 / 64 is exact.  The bound asked is 4 eps M ("4 ulp"), which leaves 1 eps M to the reference: the fp64
matrix product is 2^-29 of that beside a float32 result; beside a float64 result it can itself be off by as much as the oracle
when every rounding of both falls the same way (3 + 3), which independent roundings do not do (their root mean square is about
1 eps M for the two together).  Every test prints its largest figure in units of eps M before it asserts."""
import os

import numpy as np
import pytest
import scipy.signal

import pyramid_oracle as PO
import radiance_oracle as RO
from wass_amd import postproc as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PIN = os.path.join(ROOT, "tests", "golden", "pyrup_pin.npz")
DTYPES = [np.float32, np.float64]
ULPS = 4.0


def _matrix_form(src):
    Uy, Ux = PO.weights(src.shape[0]), PO.weights(src.shape[1])
    s = src.astype(np.float64)
    return Uy @ s @ Ux.T / 64, Uy @ np.abs(s) @ Ux.T / 64


def _in_eps(got, want, mag, dtype):
    return float(np.max(np.abs(got.astype(np.float64) - want) / (np.finfo(dtype).eps * mag)))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("h,w", PO.SHAPES)
def test_matrix_form(h, w, dtype):
    src = PO.picture(h, w, dtype)
    got = PO.pyr_up(src)
    assert got.dtype == dtype and got.shape == (2 * h, 2 * w)
    want, mag = _matrix_form(src)
    worst = _in_eps(got, want, mag, dtype)
    print(f"{h} x {w} {np.dtype(dtype).name}: at most {worst:.3f} eps M from U_y src U_x^T / 64 (bound {ULPS})")
    assert worst <= ULPS


def test_weights_are_the_five_tap_kernel():
    """every row of U sums to 8, every column away from the ends holds 1 4 6 4 1, and the two ends fold the taps that fall outside
    back in (row 0 reads sample 1 twice, the last two rows read the last sample instead of the one past it)"""
    for n in (2, 3, 5, 17):
        U = PO.weights(n)
        assert (U.sum(axis=1) == 8).all()
        for j in range(2, n - 1):
            assert U[2 * j - 2:2 * j + 3, j].tolist() == [1, 4, 6, 4, 1] and U[:, j].sum() == 16
    assert PO.weights(3)[:, 0].tolist() == [6, 4, 1, 0, 0, 0] and PO.weights(3)[:, 2].tolist() == [0, 0, 1, 4, 7, 8]
    assert PO.weights(3)[:, 1].tolist() == [2, 4, 6, 4, 1, 0]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("h,w", [(5, 7), (33, 17)])
def test_interior_against_convolve2d(h, w, dtype):
    src = PO.picture(h, w, dtype, seed=5)
    got = PO.pyr_up(src)
    k = np.array([1, 4, 6, 4, 1], np.float64) / 8
    stuffed = np.zeros((2 * h, 2 * w))
    stuffed[::2, ::2] = src
    want = scipy.signal.convolve2d(stuffed, np.outer(k, k), mode="same")
    mag = scipy.signal.convolve2d(np.abs(stuffed), np.outer(k, k), mode="same")
    inner = np.s_[2:-2, 2:-2]
    worst = _in_eps(got[inner], want[inner], mag[inner], dtype)
    print(f"{h} x {w} {np.dtype(dtype).name}: interior at most {worst:.3f} eps M from convolve2d (bound {ULPS})")
    assert worst <= ULPS
    # and the border is where the two part: zero padding is not the reflection
    assert np.abs(got[0].astype(np.float64) - want[0]).max() > 0


@pytest.mark.parametrize("dtype", DTYPES)
def test_exact_cases(dtype):
    for v in (0, 3, -7, 100):
        assert np.array_equal(PO.pyr_up(np.full((5, 7), v, dtype)), np.full((10, 14), v, dtype))
    ramp = np.tile(np.arange(9, dtype=dtype), (4, 1))
    up = PO.pyr_up(ramp)
    assert up.shape == (8, 18)
    assert np.array_equal(up[:, 2:16], np.tile(np.arange(2, 16, dtype=dtype) * dtype(0.5), (8, 1)))
    rng = np.random.default_rng(3)
    ints = rng.integers(-500, 500, (7, 12)).astype(dtype)          # every sum is a small integer: exact in any order
    assert np.array_equal(PO.pyr_up(ints.T), PO.pyr_up(ints).T)
    assert np.array_equal(PO.pyr_up(np.ascontiguousarray(ints.T), 2), PO.pyr_up(ints, 2).T)
    src = PO.picture(6, 5, dtype, seed=9)
    for levels in (2, 3):
        one = src
        for _ in range(levels):
            one = PO.pyr_up(one)
        assert np.array_equal(PO.pyr_up(src, levels), one)
    cube = np.stack([PO.picture(4, 6, dtype, seed=s) for s in range(3)])
    assert np.array_equal(PO.pyr_up(cube, 2), np.stack([PO.pyr_up(f, 2) for f in cube]))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("r,c", [(0, 0), (5, 8), (0, 4), (3, 0), (5, 3), (2, 4), (1, 1)])
def test_nan_spread(r, c, dtype):
    h, w = 6, 9
    src = PO.picture(h, w, dtype, seed=2)
    src[r, c] = np.nan
    nan = np.isnan(PO.pyr_up(src))
    want = np.zeros((2 * h, 2 * w), bool)
    want[max(2 * r - 2, 0):2 * r + 3, max(2 * c - 2, 0):2 * c + 3] = True
    print(f"NaN at ({r}, {c}): {int(nan.sum())} NaN cells, {int(want.sum())} expected")
    assert np.array_equal(nan, want)


def test_arguments():
    ok = np.zeros((4, 5), np.float32)
    calls = [lambda f: f(np.zeros((1, 5), np.float32)), lambda f: f(np.zeros((5, 1), np.float64)), lambda f: f(np.zeros((3, 4, 1), np.float32)),
             lambda f: f(ok, 0), lambda f: f(ok, 5), lambda f: f(np.zeros((4, 5), np.int32)), lambda f: f(np.zeros((4, 5), np.uint8)),
             lambda f: f(np.zeros((2, 2, 4, 5), np.float32))]
    for f in (PO.pyr_up, P.pyr_up):
        for call in calls:
            with pytest.raises(ValueError):
                call(f)
    for call in (lambda: P.pyr_up(ok, out=np.zeros((8, 10), np.float64)), lambda: P.pyr_up(ok, out=np.zeros((8, 11), np.float32)),
                 lambda: P.pyr_up(ok, out=np.zeros((8, 20), np.float32)[:, ::2]), lambda: P.pyr_up(ok, 2, out=np.zeros((8, 10), np.float32))):
        with pytest.raises(ValueError):
            call()
    buf = np.zeros((16, 10), np.float32)
    with pytest.raises(ValueError):
        P.pyr_up(buf[:4, :5], out=buf[:8])                         # out over the input
    Z = np.zeros((2, 4, 5), np.float32)
    XX, YY = RO.grid(4, 5)
    img = np.zeros((2, 8, 9), np.uint8)
    for call in (lambda: P.radiance_upscaled(img, Z, XX, YY, np.eye(4), upscalefactor=0), lambda: P.radiance_upscaled(img, Z, XX, YY, np.eye(4), upscalefactor=6),
                 lambda: P.radiance_upscaled(img, Z[:, :1], XX[:1], YY[:1], np.eye(4)), lambda: P.radiance_upscaled(img, Z[0], XX, YY, np.eye(4)),
                 lambda: P.radiance_upscaled(img[:1], Z, XX, YY, np.eye(4)), lambda: P.radiance_upscaled(img, Z, XX, YY, np.eye(4), batch=0)):
        with pytest.raises(ValueError):
            call()


def test_radiance_names_the_new_function():
    Z = np.zeros((2, 4, 5), np.float32)
    XX, YY = RO.grid(4, 5)
    with pytest.raises(NotImplementedError, match="radiance_upscaled"):
        P.radiance(np.zeros((2, 8, 9), np.uint8), Z, XX, YY, np.eye(4), upscalefactor=2)


def _al(v):
    return (v + 255) & ~255


def _pyr_bytes(b, H, W, levels, e, host):
    mids = sum(_al(b * 4 ** l * H * W * e) for l in range(1, levels))
    return mids + (_al(b * H * W * e) + _al(b * 4 ** levels * H * W * e) if host else 0)


def _radup_bytes(b, H, W, Ih, Iw, levels, host):
    HW, up = H * W, 4 ** levels * H * W
    grid = 2 * _al(up * 8) + sum(_al(4 ** l * HW * 8) for l in range(1, levels)) + (2 * _al(HW * 8) if host else 0)
    frames = _al(b * HW * 4) + sum(_al(b * 4 ** l * HW * 4) for l in range(1, levels)) + _al(b * up * 4)
    if host:
        frames += _al(b * Ih * Iw) + _al(b * HW * 4) + _al(b * up * 4)
    return grid + frames


def test_scratch_formulas():
    cap = 16 << 30
    for dtype, e in ((np.float32, 4), (np.float64, 8)):
        for count, H, W, levels, batch, host in ((1, 2, 2, 1, 8, True), (3, 5, 7, 1, 8, False), (11, 33, 17, 2, 8, True), (11, 33, 17, 4, 4, False),
                                                 (20, 130, 257, 3, 16, True), (5, 64, 65, 4, 2, True)):
            got, b = P.pyr_up_scratch_bytes(count, H, W, levels, dtype, batch, host)
            assert b == min(batch, count) and got == _pyr_bytes(b, H, W, levels, e, host), (count, H, W, levels, batch, host)
        assert P.pyr_up_scratch_bytes(3, 5, 7, 1, dtype, host=False)[0] == 0
    # a cube that does not fit 8 frames at a time: 1024 x 1024 float64 at 4 levels is 2 GiB a frame for the result alone
    got, b = P.pyr_up_scratch_bytes(100, 1024, 1024, 4, np.float64, 8, True)
    print(f"pyr_up 100 x 1024 x 1024 float64, 4 levels, host: batch {b}, {got} bytes")
    assert b == 4 and got == _pyr_bytes(4, 1024, 1024, 4, 8, True) <= cap < _pyr_bytes(8, 1024, 1024, 4, 8, True)
    got, b = P.pyr_up_scratch_bytes(100, 1024, 1024, 4, np.float64, 8, False)
    assert b == 8 and got == _pyr_bytes(8, 1024, 1024, 4, 8, False) <= cap
    for count, H, W, Ih, Iw, up, batch, host in ((1, 2, 2, 8, 9, 2, 8, True), (9, 9, 13, 40, 56, 3, 4, False), (9, 64, 65, 40, 56, 5, 8, True),
                                                (16, 1024, 1024, 2058, 2456, 2, 8, False)):
        got, b = P.radiance_upscaled_scratch_bytes(count, H, W, Ih, Iw, up, batch, host)
        assert b == min(batch, count) and got == _radup_bytes(b, H, W, Ih, Iw, up - 1, host), (count, H, W, up, batch, host)
    got, b = P.radiance_upscaled_scratch_bytes(64, 2048, 2048, 2058, 2456, 4, 64, True)
    print(f"radiance_upscaled 64 x 2048 x 2048, upscalefactor 4, host: batch {b}, {got} bytes")
    assert b == 4 and got == _radup_bytes(4, 2048, 2048, 2058, 2456, 3, True) <= cap < _radup_bytes(8, 2048, 2048, 2058, 2456, 3, True)
    assert P.radiance_upscaled_scratch_bytes(3, 9, 13, 40, 56, 1) == P.radiance_scratch_bytes(3, 9, 13, 40, 56)
    for call in (lambda: P.pyr_up_scratch_bytes(1, 1, 5), lambda: P.pyr_up_scratch_bytes(1, 5, 5, 0), lambda: P.pyr_up_scratch_bytes(1, 5, 5, 5),
                 lambda: P.pyr_up_scratch_bytes(0, 5, 5), lambda: P.pyr_up_scratch_bytes(1, 5, 5, 1, np.float16),
                 lambda: P.radiance_upscaled_scratch_bytes(1, 1, 5, 8, 9), lambda: P.radiance_upscaled_scratch_bytes(1, 5, 5, 8, 9, 6)):
        with pytest.raises(ValueError):
            call()


@pytest.mark.skipif(not os.path.exists(PIN), reason="tests/golden/pyrup_pin.npz not generated (scripts/pin_with_opencv.py needs cv2)")
def test_opencv_pin():
    """cv.pyrUp itself on the pictures of test_matrix_form: the restatement must reproduce it bit for bit, or the file tells by how
    much OpenCV's build (its vector code may fuse multiply and add) departs"""
    z = np.load(PIN)
    inputs = PO.pin_inputs()
    assert sorted(z["names"].tolist()) == sorted(inputs)
    for name, src in inputs.items():
        assert np.array_equal(z[name + "__src"], src), f"{name}: the stored input is not the test's"
        want, got = z[name + "__dst"], PO.pyr_up(src)
        bad = int((got != want).sum())
        print(f"{name}: {bad} of {want.size} cells differ from OpenCV {z['opencv_version']}")
        assert got.dtype == want.dtype and bad == 0, name
