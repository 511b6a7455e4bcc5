"""Wave spectra of the gridded cube on the GPU: drop-ins for the two array functions of the reference's
postproc/wasspost/spectra.py, compute_3D_spectrum (:53-171) and compute_spectrum (:9-49), and the statistics wasspost prints
from the latter (wasspost.py:405-419).  `data` is any count x H x W float32 array or memmap, e.g. GridSequenceResult.Z.

Axes, windows and scale factors are computed here in fp64 with the reference's own numpy expressions -- the length of the
wavenumber axes, not the nominal crop, decides the window's size -- and only segments travel to the device (spectrum.hip).
No file is written.  Without a GPU the functions raise, like the rest of the package.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from .stereo import Context


def _hann(n: int, sym: bool = True) -> np.ndarray:
    """scipy.signal.windows.hann(n, sym): general_cosine with [0.5, 0.5] on linspace(-pi, pi); the periodic form is the symmetric
    one of n + 1 without its last sample."""
    if n <= 1:
        return np.ones(max(n, 0))
    m = n if sym else n + 1
    w = 0.5 + 0.5 * np.cos(np.linspace(-np.pi, np.pi, m))
    return w if sym else w[:-1]


@dataclass
class Spectrum3DPlan:
    """What compute_3D_spectrum derives from the cube's shape, du and dt before it touches the data."""
    nt: int                 # frames per segment (even)
    shift: int              # frames between segment starts
    starts: list            # first frame of every segment taken
    r0: int                 # first row / column of the crop
    c0: int
    ny: int                 # rows / columns of the crop = len(ky) / len(kx)
    nx: int
    kx: np.ndarray
    ky: np.ndarray
    f: np.ndarray
    win_t: np.ndarray       # symmetric Hann per axis
    win_y: np.ndarray
    win_x: np.ndarray
    scale: float            # S = scale * sum over the segments of |fftn(x_w)|^2 (unnormalised transform)


def spectrum3d_plan(shape, du: float, dt: float) -> Spectrum3DPlan:
    """The reference's bookkeeping (:55-130, 139-151), restated.  ValueError where it would divide by zero or index nonsense."""
    count, H, W = (int(v) for v in shape)
    if count < 30:
        # below 10 the segment length is 0; from 10 to 29 it is 2, and hann(2) = [0, 0]: the window correction divides by zero
        raise ValueError(f"{count} frames: the reference takes segments of a tenth of the sequence, at least 30 are needed")
    if not (du > 0 and dt > 0):
        raise ValueError("du and dt must be positive")
    N = H * 2 // 3
    nt = int(count / 10)
    if nt % 2 > 0:
        nt += 1
    shift = int(nt / 2)
    r0, c0 = H // 2 - N // 2 - 20, W // 2 - N // 2
    Nx = Ny = (N // 2) * 2 + 1
    if Nx < 5:
        raise ValueError(f"a grid of {H} rows leaves a crop of {Nx} cells: too small")
    kx_max = (2.0 * np.pi / du) / 2.0
    ky_max = (2.0 * np.pi / du) / 2.0
    f_max = (1.0 / dt) / 2.0
    dkx = 2.0 * np.pi / (du * np.floor(Nx / 2.0) * 2.0)
    dky = 2.0 * np.pi / (du * np.floor(Ny / 2.0) * 2.0)
    df = 1.0 / (dt * np.floor(nt / 2.0) * 2.0)
    kx = np.arange(-kx_max, kx_max + dkx, dkx)          # Nx or Nx + 1 long, as the rounding falls
    ky = np.arange(-ky_max, ky_max + dky, dky)
    f = np.arange(-f_max, f_max, df)                     # nt is even
    ny, nx = len(ky), len(kx)                            # KX.shape: the window, and so the crop
    if r0 < 0 or c0 < 0 or r0 + ny > H or c0 + nx > W:
        raise ValueError(f"a {H} x {W} grid is too small for the reference's crop (rows {r0} .. {r0 + ny}, columns {c0} .. {c0 + nx})")
    dkx, dky = kx[3] - kx[2], ky[3] - ky[2]
    win_y, win_x, win_t = _hann(ny), _hann(nx), _hann(nt)
    wc2xyt = (1.0 / np.mean(win_y ** 2)) * (1.0 / np.mean(win_x ** 2)) * (1.0 / np.mean(win_t ** 2))
    starts = [ii * shift for ii in range(20)]
    for n, s in enumerate(starts):
        if s + nt > count:
            starts = starts[:n]
            break
    n3 = float(nt) * ny * nx
    # ortho-normalised transform (1 / sqrt(n3)), divided by n3, squared; per dkx dky df; window correction; mean over the segments
    scale = float(wc2xyt / (n3 ** 3 * dkx * dky * df) / len(starts))
    return Spectrum3DPlan(nt, shift, starts, r0, c0, ny, nx, kx, ky, f, win_t, win_y, win_x, scale)


class Spectrum3D:
    """wass_spec3d: one Welch accumulation of nt x ny x nx segments."""

    def __init__(self, ctx: Context, nt: int, ny: int, nx: int, win_t=None, win_y=None, win_x=None):
        self.ctx, self.nt, self.ny, self.nx = ctx, int(nt), int(ny), int(nx)
        wins = [None if w is None else np.ascontiguousarray(w, np.float64) for w in (win_t, win_y, win_x)]
        for w, n in zip(wins, (self.nt, self.ny, self.nx)):
            if w is not None and w.shape != (n,):
                raise ValueError("window length")
        h = C.c_void_p()
        ctx._check(ctx._lib.wass_spec3d_create(ctx._h, self.nt, self.ny, self.nx, *[None if w is None else w.ctypes.data for w in wins],
                                               C.byref(h)))
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self.ctx._lib.wass_spec3d_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def push(self, seg: np.ndarray, datascale: float = 1.0):
        """seg: an nt x ny x nx float32 view of host memory whose last axis is contiguous (a slice of the cube: no copy)."""
        if seg.shape != (self.nt, self.ny, self.nx):
            raise ValueError(f"segment of shape {seg.shape}, expected {(self.nt, self.ny, self.nx)}")
        if seg.dtype != np.float32 or seg.strides[2] != 4 or seg.strides[0] % 4 or seg.strides[1] % 4 or min(seg.strides) < 0:
            seg = np.ascontiguousarray(seg, np.float32)
        self.ctx._check(self.ctx._lib.wass_spec3d_push(self._h, seg.ctypes.data, seg.strides[0] // 4, seg.strides[1] // 4, float(datascale)))

    def push_dev(self, d_seg, datascale: float = 1.0):
        """d_seg: the same as a float32 device tensor (a view will do); it must stay alive until finish."""
        if tuple(d_seg.shape) != (self.nt, self.ny, self.nx) or d_seg.stride(2) != 1:
            raise ValueError("segment shape or strides")
        self.ctx._check(self.ctx._lib.wass_spec3d_push_dev(self._h, d_seg.data_ptr(), d_seg.stride(0), d_seg.stride(1), float(datascale)))

    def finish(self, scale: float = 1.0):
        """(S, n_segments, had_all_nan_cell): S = scale * sum over the pushed segments of |X|^2, fftshifted, float64."""
        S = np.empty((self.nt, self.ny, self.nx), np.float64)
        n, flag = C.c_int(), C.c_int()
        self.ctx._check(self.ctx._lib.wass_spec3d_finish(self._h, float(scale), S.ctypes.data, C.byref(n), C.byref(flag)))
        return S, n.value, bool(flag.value)


def compute_3D_spectrum(data, du: float, dt: float, segments: int = 8, datascale: float = 1.0, ctx: Context | None = None):
    """(S_welch float64 [Nt, Ny, Nx], KX, KY, f) as the reference returns them.  `segments` is accepted and ignored (the
    reference overwrites it with 10).  A cell that is NaN through a whole segment makes S NaN everywhere, as it does there."""
    p = spectrum3d_plan(data.shape, du, dt)
    if ctx is None:
        ctx = Context(0)
    with Spectrum3D(ctx, p.nt, p.ny, p.nx, p.win_t, p.win_y, p.win_x) as sp:
        for s in p.starts:
            sp.push(data[s:s + p.nt, p.r0:p.r0 + p.ny, p.c0:p.c0 + p.nx], datascale)
        S, n, had_nan = sp.finish(p.scale)
    assert n == len(p.starts)
    if had_nan:
        S[...] = np.nan
    KX, KY = np.meshgrid(p.kx, p.ky)
    return S, KX, KY, p.f


def spectrum_series(data, rangespan: int = 5) -> np.ndarray:
    """The series compute_spectrum averages, as rows: the centre cell, then the (2 rangespan + 1)^2 block around it (which
    holds the centre again: it is counted twice, :36-45)."""
    H, W = data.shape[1:3]
    ci, cj = H // 2, W // 2
    if rangespan < 0 or ci - rangespan < 0 or cj - rangespan < 0 or ci + rangespan >= H or cj + rangespan >= W:
        raise ValueError(f"rangespan {rangespan} does not fit a {H} x {W} grid")
    block = np.asarray(data[:, ci - rangespan:ci + rangespan + 1, cj - rangespan:cj + rangespan + 1], np.float32)
    n = block.shape[0]
    return np.ascontiguousarray(np.concatenate([np.asarray(data[:, ci, cj], np.float32).reshape(n, 1), block.reshape(n, -1)], axis=1).T)


def compute_spectrum(data, dt: float, nperseg: int = 512, rangespan: int = 5, scale: float = 1.0, ctx: Context | None = None):
    """(f, S, timeserie): the Welch frequency spectrum averaged over the centre of the grid, as the reference returns it."""
    count = int(data.shape[0])
    if count < 2 or nperseg < 2 or not dt > 0:
        raise ValueError("at least two frames, nperseg >= 2 and dt > 0 are needed")
    series = spectrum_series(data, rangespan)
    if not np.isfinite(series).all():
        raise ValueError("the centre block holds NaN cells (scipy.signal.csd would return NaN)")
    nps = min(int(nperseg), count)
    if ctx is None:
        ctx = Context(0)
    S = np.empty(nps // 2 + 1, np.float64)
    ctx._check(ctx._lib.wass_spec1d_welch(ctx._h, series.ctypes.data, series.shape[0], count, nps, 1.0 / dt, float(scale), S.ctypes.data))
    S /= float(series.shape[0])
    f = np.fft.rfftfreq(nps, dt)
    timeserie = scale * np.asarray(data[:, data.shape[1] // 2, data.shape[2] // 2])
    timeserie = timeserie - np.mean(timeserie)
    return f, S, timeserie


def spectrum_statistics(freq, S) -> dict:
    """Hm0, peak frequency, peak period and Tm01 as wasspost prints them (wasspost.py:405-419)."""
    freq, S = np.asarray(freq, np.float64), np.asarray(S, np.float64)
    dfreq = np.gradient(freq)
    m0 = np.sum(S * dfreq)
    m1 = np.sum(freq * S * dfreq)
    pp = float(freq[np.argmax(S)])
    return {"Hm0": float(4.0 * np.sqrt(m0)), "peak_frequency": pp, "peak_period": float(1.0 / pp) if pp != 0 else float("inf"),
            "Tm01": float(m0 / m1)}
