"""numpy restatements of the two filters of the reference's postproc (wasspost.py:149-371, spectra.py:176-202) for the filter
tests, and the error bounds the GPU results are held to.  Test infrastructure only: nothing here is imported by the package.

sosfiltfilt restates scipy.signal.sosfiltfilt(sos, x, axis=0) with scipy's defaults: the odd padding is built in the INPUT's
dtype (float32: 2 x[0] - x[k] is rounded before anything becomes wider), the steady state zi is in closed form, the
recurrence is transposed direct form II in scipy's order of operations, one sample at a time, vectorised over the series.
`dtype` is the precision of state and arithmetic: np.float64 is what scipy computes, np.longdouble measures the
recurrence's own fp64 noise (noise()).  `padlen` is scipy's argument (None: its default; 0: no extension); VARIANTS are known
mistakes for showing what the tests can tell, never compared with the GPU.
"""
import numpy as np


def padlen(sos):
    sos = np.asarray(sos)
    return 3 * (2 * sos.shape[0] + 1 - int(min((sos[:, 2] == 0).sum(), (sos[:, 5] == 0).sum())))


default_padlen = padlen          # sosfiltfilt's own argument is called padlen, as scipy's is


def sosfilt_zi(sos, dtype=np.float64):
    sos = np.asarray(sos, dtype)
    zi = np.empty((sos.shape[0], 2), dtype)
    scale = dtype(1.0)
    for s in range(sos.shape[0]):
        b, a = sos[s, :3], sos[s, 3:]
        B = b[1:] - a[1:] * b[0]
        z0 = B.sum() / (dtype(1.0) + a[1] + a[2])
        zi[s, 0] = scale * z0
        zi[s, 1] = scale * ((dtype(1.0) + a[1]) * z0 - B[0])
        scale = scale * (b.sum() / a.sum())
    return zi


def _fma(a, b, c):
    """a * b + c rounded once, approximately: the product and the sum in np.longdouble (64-bit significand on x86-64), then one rounding
    to fp64.  An APPROXIMATION of an fma (the exact product has 106 bits, and where long double is fp64 this is no fma at all): enough
    to show that a contracted update does not hide, not a model of the hardware instruction."""
    L = np.longdouble
    return (np.asarray(a, L) * np.asarray(b, L) + np.asarray(c, L)).astype(np.float64)


# One known mistake each, for showing that the probes of tests/filter_probes.py tell it from the oracle (tests/test_filter_edges.py).
# Never compared with the GPU.
VARIANTS = {"reassociated": dict(update="reassociated"),            # z0 = b1 x + (z1 - a1 y)
            "contracted": dict(first="contracted"),                 # y = fma(b0, x, z0), see _fma
            "padding in fp64": dict(pad="fp64"),                    # 2 x[0] - x[k] formed in fp64
            "mean summed pairwise": dict(mean="pairwise")}          # np.mean over a contiguous copy of each series


def _sosfilt(sos, x, zi, update="scipy", first="scipy"):
    """x [n, ...] (overwritten with the output), zi [n_sections, 2, ...]"""
    for n in range(x.shape[0]):
        xc = x[n]
        for s in range(sos.shape[0]):
            y = _fma(sos[s, 0], xc, zi[s, 0]) if first == "contracted" else sos[s, 0] * xc + zi[s, 0]
            if update == "reassociated":
                zi[s, 0] = sos[s, 1] * xc + (zi[s, 1] - sos[s, 4] * y)
            else:
                zi[s, 0] = (sos[s, 1] * xc - sos[s, 4] * y) + zi[s, 1]
            zi[s, 1] = sos[s, 2] * xc - sos[s, 5] * y
            xc = y
        x[n] = xc
    return x


def sosfiltfilt(sos, x, dtype=np.float64, remove_mean=False, padlen=None, update="scipy", first="scipy", pad="input", mean="frames", zi=None):
    """x: [count, ...] float32.  The filtered series in `dtype` (not cast to float32).  padlen: None for scipy's default, else
    0 <= padlen < count as scipy takes it (0: no extension, both passes start from zi times their first sample).  update, first,
    pad, mean: see VARIANTS; the defaults are scipy's arithmetic.  zi: the steady state [n_sections, 2] to start from instead of
    the closed form of sosfilt_zi (scipy's own comes out of a LAPACK solve and differs from it in the last bits)."""
    x = np.asarray(x)
    assert x.dtype == np.float32
    edge = default_padlen(sos) if padlen is None else int(padlen)
    if edge < 0:
        raise ValueError("padlen must not be negative")
    if x.shape[0] <= edge:
        raise ValueError(f"The length of the input vector x must be greater than padlen, which is {edge}.")
    with np.errstate(invalid="ignore", over="ignore"):
        xp = x.astype(np.float64) if pad == "fp64" else x
        ext = np.concatenate((2 * xp[:1] - xp[edge:0:-1], xp, 2 * xp[-1:] - xp[-2:-(edge + 2):-1]), axis=0) if edge else x.copy()
        assert ext.dtype == xp.dtype
        s = np.asarray(sos, np.float64).astype(dtype)
        zi = sosfilt_zi(np.asarray(sos, np.float64), dtype) if zi is None else np.asarray(zi, np.float64).astype(dtype)
        zi = zi.reshape((s.shape[0], 2) + (1,) * (x.ndim - 1))
        y = ext.astype(dtype)
        y = _sosfilt(s, y, zi * y[:1], update, first)
        y = y[::-1].copy()
        y = _sosfilt(s, y, zi * y[:1], update, first)[::-1]
        y = y[edge:y.shape[0] - edge] if edge else y
        if remove_mean:
            if mean == "pairwise":
                m = np.mean(np.ascontiguousarray(np.moveaxis(y, 0, -1)), axis=-1)[None]
            else:
                m = np.mean(y, axis=0, keepdims=True)
            y = y - m
    return np.ascontiguousarray(y)


def noise(sos, x, remove_mean=False, padlen=None):
    """(oracle64, n): n = the largest |oracle64 - oracle_longdouble| over the series that hold no NaN."""
    o64 = sosfiltfilt(sos, x, np.float64, remove_mean, padlen)
    old = sosfiltfilt(sos, x, np.longdouble, remove_mean, padlen)
    with np.errstate(invalid="ignore"):
        d = np.abs(o64.astype(np.longdouble) - old)
    return o64, float(np.nanmax(d)) if np.isfinite(d).any() else 0.0


def half_ulp_f32(v):
    """Half the float32 spacing of the binade that holds |v| (2^-149 at least; 2^-150 for v = 0): what a cast to float32 may move v by."""
    v = np.abs(np.asarray(v, np.float64))
    _, e = np.frexp(v)
    return np.where(v == 0, 2.0 ** -150, 0.5 * np.exp2(np.maximum(e.astype(np.float64) - 24.0, -149.0)))


def temporal_bound(o64, n):
    """|gpu_f32 - oracle64| <= 0.5 ulp_f32(|oracle64|) + 4 n"""
    return half_ulp_f32(o64) + 4.0 * n


def series_cube(count, H, W, seed=1, offset=0.0, drift=0.0):
    """count x H x W float32: per cell a few sinusoids between 0.01 and 0.45 cycles per frame with hashed amplitudes and phases, hashed
    noise, an offset and a linear drift: closed form, no random-number stream."""
    from spectrum_oracle import _hash01
    cell = np.arange(H * W, dtype=np.uint64).reshape(1, H, W)
    t = np.arange(count, dtype=np.float64).reshape(count, 1, 1)
    z = np.full((count, H, W), float(offset)) + drift * t
    for k, f in enumerate((0.0113, 0.043, 0.0832, 0.171, 0.317, 0.449)):
        amp = 300.0 / (k + 1) * (0.5 + _hash01(cell, seed + 11 * k))
        ph = 2 * np.pi * _hash01(cell, seed + 101 + 13 * k)
        z += amp * np.cos(2 * np.pi * f * t + ph)
    idx = cell + np.arange(count, dtype=np.uint64).reshape(count, 1, 1) * np.uint64(H * W)
    z += 20.0 * (_hash01(idx, seed + 977) - 0.5)
    return z.astype(np.float32)


# ---- the spatial filter ------------------------------------------------------------------------------------------------------------
def transfer_function(rows, cols, du, cutoff, order):
    """The reference's fftshifted transfer function [rows, cols]: its W is the number of rows (it is called with W, H = XX.shape)."""
    fr = np.fft.fftshift(np.fft.fftfreq(rows, d=du))
    fc = np.fft.fftshift(np.fft.fftfreq(cols, d=du))
    A, B = np.meshgrid(fc, fr)
    R = np.sqrt(A ** 2 + B ** 2)
    return 1.0 / np.sqrt(1.0 + (R / cutoff) ** (2 * order))


def spatial_apply(surface, Hs):
    """real(ifft2(ifftshift(fftshift(fft2(surface)) * Hs))) in fp64"""
    F = np.fft.fftshift(np.fft.fft2(np.asarray(surface, np.float64)))
    return np.real(np.fft.ifft2(np.fft.ifftshift(F * Hs)))


def spatial_bound(frame):
    """B with ||gpu - oracle||_F <= B for one frame x (rows R, cols C, N = R C); every element's error is then at most B too, and
    the mean's at most B / sqrt(N).  In the 2-norm, because the inverse's 1 / N must be carried: an l1 bound grows with N while
    the output does not.  u = 2^-24.

    One DFT stage of length n is, per output, an f32 fma chain over f32-rounded twiddles: a real input line x gives each of the
    two parts an error of at most (n + 2) u ||x||_1 <= (n + 2) u sqrt(n) ||x||_2, a complex line b (2 n terms per part, |re| + |im|
    <= sqrt(2) |b|) at most (2 n + 2) u sqrt(2) sqrt(n) ||b||_2; the complex error is sqrt(2) times a part's.  Over the n_out outputs
    of the line that is g sqrt(n_out) ||line||_2 with g_real(n) = sqrt(2) (n + 2) u sqrt(n), g_cplx(n) = 2 (2 n + 2) u sqrt(n), and
    over the frame the same with Frobenius norms.  An error already present goes through the exact stage, whose norm is sqrt(n)
    (a part of a DFT matrix has no larger norm).  With a = a bound of the computed array's norm and e = of its error:
      x        e1 = g_real(C) sqrt(C / 2 + 1) ||x||,     a1 = sqrt(C) ||x|| + e1
      y        e2 = sqrt(R) e1 + g_cplx(R) sqrt(R) a1,  a2 = sqrt(R) a1 (1 + g_cplx(R))
      multiply by conj, H w / N (at most 2 / N, fp64 product, one rounding, 2 u with slack)
               e3 = (2 / N) (e2 + 2 u a2),               a3 = (2 / N) a2 (1 + 2 u)
      y again  e4 = sqrt(R) e3 + g_cplx(R) sqrt(R) a3,  a4 = sqrt(R) a3 (1 + g_cplx(R))
      x back, real part only (one part: g_cplx / sqrt(2)), C / 2 + 1 terms, C outputs
               B  = sqrt(C) e4 + g_cplx(C / 2 + 1) / sqrt(2) sqrt(C) a4
    About 0.04 ||x|| at 1024 x 1024 and 0.001 ||x|| at 126 x 132: a worst case (every rounding aligned); the observed error is
    printed beside it."""
    R, C = frame.shape
    u, ch = 2.0 ** -24, C // 2 + 1
    nx = float(np.sqrt(np.sum(np.asarray(frame, np.float64) ** 2)))
    g_real = lambda n: np.sqrt(2.0) * (n + 2) * u * np.sqrt(n)
    g_cplx = lambda n: 2.0 * (2 * n + 2) * u * np.sqrt(n)
    e1 = g_real(C) * np.sqrt(ch) * nx
    a1 = np.sqrt(C) * nx + e1
    e2 = np.sqrt(R) * e1 + g_cplx(R) * np.sqrt(R) * a1
    a2 = np.sqrt(R) * a1 * (1 + g_cplx(R))
    e3 = 2.0 / (R * C) * (e2 + 2 * u * a2)
    a3 = 2.0 / (R * C) * a2 * (1 + 2 * u)
    e4 = np.sqrt(R) * e3 + g_cplx(R) * np.sqrt(R) * a3
    a4 = np.sqrt(R) * a3 * (1 + g_cplx(R))
    return float(np.sqrt(C) * e4 + g_cplx(ch) / np.sqrt(2.0) * np.sqrt(C) * a4)
