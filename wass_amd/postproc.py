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

from .stereo import Context, _Handle, _is_device


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


class Spectrum3D(_Handle):
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

    def _destroy(self, h):
        self.ctx._lib.wass_spec3d_destroy(h)

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

    def finish_dev(self, scale: float = 1.0, out=None):
        """finish with S left on the device: a float64 tensor of nt x ny x nx (`out`, contiguous, or a new one), the same bits."""
        import torch
        shape = (self.nt, self.ny, self.nx)
        if out is None:
            out = torch.empty(shape, dtype=torch.float64, device=f"cuda:{self.ctx.device_id}")
        elif not _is_device(out) or tuple(out.shape) != shape or out.dtype != torch.float64 or not out.is_contiguous():
            raise ValueError(f"out must be a contiguous float64 device tensor of shape {shape}")
        n, flag = C.c_int(), C.c_int()
        self.ctx._check(self.ctx._lib.wass_spec3d_finish_dev(self._h, float(scale), out.data_ptr(), C.byref(n), C.byref(flag)))
        return out, n.value, bool(flag.value)


def compute_3D_spectrum_dev(data, du: float, dt: float, datascale: float = 1.0, ctx: Context | None = None):
    """compute_3D_spectrum with the spectrum left in device memory: (S float64 tensor [Nt, Ny, Nx], kx, ky, f, had_nan) with the
    1-D axes of the reference (KX, KY = np.meshgrid(kx, ky)).  `data` is a host array (segments are uploaded) or a float32 device
    tensor (read in place).  had_nan: a cell was NaN through a whole segment, and S is NaN everywhere, as in compute_3D_spectrum."""
    p = spectrum3d_plan(data.shape, du, dt)
    if ctx is None:
        ctx = Context(0)
    dev = _is_device(data)
    if dev:
        import torch
        if data.dtype != torch.float32 or data.stride(2) != 1:
            data = data.to(torch.float32).contiguous()
        torch.cuda.current_stream(data.device).synchronize()
    with Spectrum3D(ctx, p.nt, p.ny, p.nx, p.win_t, p.win_y, p.win_x) as sp:
        for s in p.starts:
            seg = data[s:s + p.nt, p.r0:p.r0 + p.ny, p.c0:p.c0 + p.nx]
            (sp.push_dev if dev else sp.push)(seg, datascale)
        S, n, had_nan = sp.finish_dev(p.scale)
    assert n == len(p.starts)
    if had_nan:
        S.fill_(float("nan"))
    return S, p.kx, p.ky, p.f, had_nan


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


# ---- Butterworth filters of the cube: wasspost filter / filter_fast (wasspost.py:149-314) and spatial_lowpass (:318-371) --------
def _conjugate_halves(v):
    """Roots of a real polynomial as (one of every conjugate pair, imaginary part > 0; the real ones), sorted like scipy's
    _cplxreal: by real part, ties by |imaginary part|; a pair is the mean of one root and its partner's conjugate."""
    v = np.atleast_1d(np.asarray(v, np.complex128))
    tol = 100.0 * np.finfo(np.float64).eps
    v = v[np.lexsort((np.abs(v.imag), v.real))]
    is_real = np.abs(v.imag) <= tol * np.abs(v)
    reals, v = v[is_real].real, v[~is_real]
    up, dn = v[v.imag > 0], v[v.imag < 0]
    if len(up) != len(dn):
        raise ValueError("roots are not conjugate pairs")
    # runs of the same real part are ordered by |imaginary part| in both halves, so that partners meet
    same = np.diff(up.real) <= tol * np.abs(up[:-1])
    edges = np.diff(np.concatenate(([0], same.astype(int), [0])))
    for a, b in zip(np.nonzero(edges > 0)[0], np.nonzero(edges < 0)[0]):
        for half in (up, dn):
            half[a:b + 1] = half[a:b + 1][np.lexsort([np.abs(half[a:b + 1].imag)])]
    return (up + dn.conj()) / 2.0, reals


def _nearest(values, to, real):
    """Index of the element of `values` nearest to `to` among the real (or, real=False, the complex) ones."""
    order = np.argsort(np.abs(values - to))
    mask = np.isreal(values[order])
    return order[np.nonzero(mask if real else ~mask)[0][0]]


def _section(zeros, poles) -> np.ndarray:
    """[b0 b1 b2 a0 a1 a2] of one section with gain 1; a pair of conjugates gives real coefficients."""
    def poly(r):
        c = np.ones(1, np.complex128)
        for v in r:
            c = np.convolve(c, np.array([1.0, -v], np.complex128))
        return c.real
    out = np.zeros(6)
    b, a = poly(zeros), poly(poles)
    out[3 - len(b):3] = b
    out[6 - len(a):6] = a
    return out


def butter_sos(order: int, cutoff: float, btype: str = "lowpass", fs: float = 2.0) -> np.ndarray:
    """scipy.signal.butter(order, cutoff, btype=btype, output='sos', fs=fs) for 'lowpass' and 'highpass', float64 [n_sections, 6]:
    the analog prototype's poles on the unit circle, the cutoff pre-warped, the bilinear transform, then scipy's pairing
    (zpk2sos, 'nearest'): the pole nearest the unit circle is picked first and lands in the LAST section, every pole takes the
    zero nearest to it, the gain goes into section 0."""
    order = int(order)
    if order < 1:
        raise ValueError("order must be at least 1")
    if btype not in ("lowpass", "highpass"):
        raise ValueError("btype must be 'lowpass' or 'highpass'")
    wn = 2.0 * float(cutoff) / float(fs)
    if not 0.0 < wn < 1.0:
        raise ValueError("the cutoff must lie between 0 and fs / 2")
    m = np.arange(-order + 1, order, 2)
    p = -np.exp(1j * np.pi * m / (2 * order))                  # prototype: no zeros, gain 1
    warped = 4.0 * np.tan(np.pi * wn / 2.0)                    # 2 fs tan(pi wn / fs) with the design's fs = 2
    if btype == "lowpass":
        p, z, k = warped * p, np.zeros(0, np.complex128), warped ** order
    else:
        k = float(np.real(1.0 / np.prod(-p)))
        p, z = warped / p, np.zeros(order, np.complex128)
    # bilinear transform, fs2 = 2 * 2
    k = k * float(np.real(np.prod(4.0 - z) / np.prod(4.0 - p)))
    z = np.append((4.0 + z) / (4.0 - z), -np.ones(order - len(z)))
    p = (4.0 + p) / (4.0 - p)
    # sections
    n_sections = (order + 1) // 2
    if order % 2:
        p, z = np.append(p, 0.0), np.append(z, 0.0)
    z = np.concatenate(_conjugate_halves(z))
    p = np.concatenate(_conjugate_halves(p))
    worst = lambda q: int(np.argmin(np.abs(1.0 - np.abs(q))))
    sos = np.zeros((n_sections, 6))
    for si in range(n_sections - 1, -1, -1):
        i = worst(p)
        p1, p = p[i], np.delete(p, i)
        if np.isreal(p1) and np.isreal(p).sum() == 0:          # the last real pole
            i = _nearest(z, p1, True)
            z1, z = z[i], np.delete(z, i)
            sos[si] = _section([z1, 0.0], [p1, 0.0])
        elif len(p) + 1 == len(z) and not np.isreal(p1) and np.isreal(p).sum() == 1 and np.isreal(z).sum() == 1:
            i = _nearest(z, p1, False)                         # one real pole and one real zero are left: take a complex zero
            z1, z = z[i], np.delete(z, i)
            sos[si] = _section([z1, z1.conj()], [p1, p1.conj()])
        else:
            if np.isreal(p1):
                ri = np.flatnonzero(np.isreal(p))
                i = ri[worst(p[ri])]
                p2, p = p[i], np.delete(p, i)
            else:
                p2 = p1.conj()
            i = int(np.argmin(np.abs(p1 - z)))
            z1, z = z[i], np.delete(z, i)
            if not np.isreal(z1):
                sos[si] = _section([z1, z1.conj()], [p1, p2])
            else:
                i = _nearest(z, p1, True)
                z2, z = z[i], np.delete(z, i)
                sos[si] = _section([z1, z2], [p1, p2])
    assert len(p) == 0 and len(z) == 0
    sos[0, :3] *= k
    return sos


def _check_sos(sos) -> np.ndarray:
    sos = np.ascontiguousarray(sos, np.float64)
    if sos.ndim != 2 or sos.shape[1] != 6 or sos.shape[0] < 1:
        raise ValueError("sos must be n_sections x 6")
    if sos.shape[0] > 6:
        raise ValueError("at most 6 sections (order 12)")
    if not (sos[:, 3] == 1.0).all():
        raise ValueError("sos[:, 3] should be all ones")
    return sos


def sos_padlen(sos) -> int:
    """sosfiltfilt's default padlen: 3 * (2 n_sections + 1 - min(#(b2 == 0), #(a2 == 0)))."""
    sos = _check_sos(sos)
    return 3 * (2 * sos.shape[0] + 1 - int(min((sos[:, 2] == 0).sum(), (sos[:, 5] == 0).sum())))


def sosfilt_zi(sos) -> np.ndarray:
    """scipy.signal.sosfilt_zi: the state [n_sections, 2] of the step response's steady state, in closed form per section
    (zi0 = (B0 + B1) / (1 + a1 + a2), zi1 = (1 + a1) zi0 - B0 with B = b[1:] - a[1:] b0), scaled by the DC gain of the sections before."""
    sos = _check_sos(sos)
    zi = np.empty((sos.shape[0], 2))
    scale = 1.0
    for s in range(sos.shape[0]):
        b, a = sos[s, :3], sos[s, 3:]
        B = b[1:] - a[1:] * b[0]
        z0 = B.sum() / (1.0 + a[1] + a[2])
        zi[s] = scale * np.array([z0, (1.0 + a[1]) * z0 - B[0]])
        scale *= b.sum() / a.sum()
    return zi


def _scratch_bytes(name: str, args, shown: str):
    """(bytes, frames per launch or rows per slab) as the library's pure wass_<name>_scratch_bytes plans them; its refusal is a
    ValueError that shows the call"""
    from . import _lib
    b, n = C.c_size_t(), C.c_int()
    rc = getattr(_lib.load(), f"wass_{name}_scratch_bytes")(*args, C.byref(b), C.byref(n))
    if rc:
        raise ValueError(f"wass_{name}_scratch_bytes({shown}): error {rc}")
    return b.value, n.value


def sosfiltfilt_scratch_bytes(count: int, H: int, W: int, padlen: int, slab_rows: int = 0, host: bool = True):
    """(bytes of device scratch, rows per slab) of one sosfiltfilt call; no GPU needed."""
    return _scratch_bytes("sosfiltfilt", (int(count), int(H), int(W), int(padlen), int(slab_rows), int(bool(host))),
                          f"{count}, {H}, {W}, padlen {padlen}")


def _host_f32_rows(a) -> np.ndarray:
    """a count x H x W float32 host array whose last axis is contiguous and whose other strides are whole, positive elements (a
    slice or a memmap passes as it is)."""
    if not isinstance(a, np.ndarray) or a.dtype != np.float32 or a.strides[2] != 4 or a.strides[0] % 4 or a.strides[1] % 4 \
            or a.strides[0] <= 0 or a.strides[1] <= 0:
        a = np.ascontiguousarray(a, np.float32)
    return a


def _ptr_strides(a):
    """(pointer, stride_t, stride_y in elements) of a cube on either side"""
    if _is_device(a):
        return a.data_ptr(), a.stride(0), a.stride(1)
    return a.ctypes.data, a.strides[0] // a.itemsize, a.strides[1] // a.itemsize


def _cube_io(data, outs, what, dtypes=("float32",), shape=None, dense=False, alias=True):
    """A float32 cube and the outputs of an operator on it, all on one side: (data, outs, suffix, a).  `data` comes back as the
    library takes it, converted or copied only where its dtype or strides demand it.  outs[k] is the caller's, checked, or a new
    one where the caller gave None: of dtypes[k] and `shape` (default: the cube's); contiguous if `dense`, else with a contiguous
    last axis and positive whole strides (_ptr_strides gives them); with alias=False it must not share memory with the cube.
    suffix is "_dev" for device tensors, whose current stream is synchronised here (the library runs on streams of its own), and
    "" for host arrays.  a = (pointer, stride_t, stride_y, count, H, W) of the cube."""
    if len(data.shape) != 3:
        raise ValueError("data must be count x H x W")
    count, H, W = (int(v) for v in data.shape)
    shape = (count, H, W) if shape is None else tuple(shape)
    dev = _is_device(data)
    if dev:
        import torch
        lib, side = torch, "device tensor"
        if data.dtype != torch.float32 or data.stride(2) != 1 or data.stride(0) <= 0 or data.stride(1) <= 0:
            data = data.to(torch.float32).contiguous()
    else:
        lib, side = np, "host array"
        data = _host_f32_rows(data)
    outs = list(outs)
    for k, (o, name) in enumerate(zip(outs, dtypes)):
        dt = getattr(lib, name)
        if o is None:
            outs[k] = torch.empty(shape, dtype=dt, device=data.device) if dev else np.empty(shape, dt)
            continue
        if dev:
            ok = _is_device(o) and tuple(o.shape) == shape and o.dtype == dt and (alias or o.data_ptr() != data.data_ptr()) \
                and (o.is_contiguous() if dense else o.stride(2) == 1 and o.stride(0) > 0 and o.stride(1) > 0)
        else:
            ok = isinstance(o, np.ndarray) and o.shape == shape and o.dtype == dt and (alias or not np.shares_memory(o, data)) \
                and (o.flags.c_contiguous if dense else o.strides[2] == o.itemsize and min(o.strides) > 0
                     and not (o.strides[0] % o.itemsize or o.strides[1] % o.itemsize))
        if not ok:
            raise ValueError(f"{what}: an output must be {'a' if alias else 'another'} {name} {side} of shape {shape}, "
                             + ("contiguous" if dense else "with a contiguous last axis"))
    if dev:
        torch.cuda.current_stream(data.device).synchronize()
    return data, outs, "_dev" if dev else "", (*_ptr_strides(data), count, H, W)


def sosfiltfilt(sos, data, remove_mean: bool = False, ctx: Context | None = None, out=None, slab_rows: int = 0):
    """scipy.signal.sosfiltfilt(sos, data, axis=0) with scipy's defaults (odd padding of sos_padlen samples built in float32, both
    passes started from sosfilt_zi times their first sample, fp64 throughout), the result cast to float32; remove_mean=True
    subtracts the fp64 time mean of every filtered series before the cast.  `data` is count x H x W float32: a host array or
    memmap (the result is a host array, or `out`) or a device tensor (the result is a device tensor, or `out`; `out` may be
    `data`).  slab_rows > 0 caps the rows filtered at a time (the result does not depend on it)."""
    sos = _check_sos(sos)
    if len(data.shape) != 3:
        raise ValueError("data must be count x H x W")
    count, H, W = (int(v) for v in data.shape)
    padlen = sos_padlen(sos)
    if count <= padlen:
        raise ValueError(f"The length of the input vector x must be greater than padlen, which is {padlen}.")
    if H < 1 or W < 1:
        raise ValueError("empty grid")
    zi = np.ascontiguousarray(sosfilt_zi(sos))
    if ctx is None:
        ctx = Context(0)
    args = (sos.ctypes.data, sos.shape[0], zi.ctypes.data, padlen, int(bool(remove_mean)), int(slab_rows))
    data, (out,), suffix, a = _cube_io(data, (out,), "sosfiltfilt")
    ctx._check(getattr(ctx._lib, "wass_sosfiltfilt" + suffix)(ctx._h, *a, *args, *_ptr_strides(out)))
    if suffix:
        ctx.synchronize()
    return out


def butterworth_filter(data, dt: float, cutoff: float = 1.0, type: str = "lowpass", fast: bool = False, order: int = 8,
                       ctx: Context | None = None, out=None, slab_rows: int = 0):
    """wasspost filter as a function: an 8th-order zero-phase Butterworth filter along time with fs = 1 / dt; 'highpass' also
    removes the time mean.  fast=True is wasspost filter_fast: fs = round(1 / dt) and no mean removal."""
    if int(data.shape[0]) <= 10:
        raise ValueError("more than 10 frames are needed")
    if not dt > 0:
        raise ValueError("dt must be positive")
    fs = float(np.round(1.0 / dt)) if fast else 1.0 / dt
    sos = butter_sos(order, cutoff, type, fs)
    return sosfiltfilt(sos, data, remove_mean=(type == "highpass" and not fast), ctx=ctx, out=out, slab_rows=slab_rows)


class Spatial2DButterworth(_Handle):
    """The reference's class (spectra.py:176-202) on the GPU.  It is called there with W, H = XX.shape, so W is the number of ROWS
    of a surface and H the number of columns; butterworth_filter is the fftshifted transfer function [rows, cols], float64."""

    def __init__(self, W: int, H: int, du: float, cutoff_fs: float, order: int, ctx: Context | None = None, batch: int = 16):
        W, H = int(W), int(H)
        if W < 1 or H < 1 or not du > 0:
            raise ValueError("W, H >= 1 and du > 0 are needed")
        fx = np.fft.fftshift(np.fft.fftfreq(W, d=du))
        fy = np.fft.fftshift(np.fft.fftfreq(H, d=du))
        FX, FY = np.meshgrid(fy, fx)                           # [rows, cols]: FX varies along the columns
        R = np.sqrt(FX ** 2 + FY ** 2)
        with np.errstate(divide="ignore"):
            self.butterworth_filter = 1.0 / np.sqrt(1.0 + (R / cutoff_fs) ** (2 * order))
        self.rows, self.cols, self.batch = W, H, max(1, int(batch))
        self._ctx, self._h = ctx, None

    def _handle(self):
        if self._h is None:
            if self._ctx is None:
                self._ctx = Context(0)
            # the fftshift / ifftshift pair around the product is an index permutation of the transfer function
            Hu = np.ascontiguousarray(np.fft.ifftshift(self.butterworth_filter), np.float64)
            h = C.c_void_p()
            self._ctx._check(self._ctx._lib.wass_spatial_filter_create(self._ctx._h, self.rows, self.cols, Hu.ctypes.data, self.batch, C.byref(h)))
            self._h = h
        return self._h

    def _destroy(self, h):
        self._ctx._lib.wass_spatial_filter_destroy(h)

    def apply_batch(self, frames, out=None):
        """frames: n x rows x cols float32, host or device; the filtered frames, float32, on the same side.  A frame that holds a NaN
        comes out all NaN."""
        if len(frames.shape) != 3 or tuple(int(v) for v in frames.shape[1:]) != (self.rows, self.cols):
            raise ValueError(f"frames of shape {tuple(frames.shape)}, expected n x {self.rows} x {self.cols}")
        n = int(frames.shape[0])
        h, ctx = self._handle(), self._ctx
        frames, (out,), suffix, a = _cube_io(frames, (out,), "apply_batch")
        if n:
            ctx._check(getattr(ctx._lib, "wass_spatial_filter_apply" + suffix)(h, *a[:3], n, *_ptr_strides(out)))
            if suffix:
                ctx.synchronize()
        return out

    def apply(self, surface):
        """One rows x cols surface, as the reference's apply."""
        if len(surface.shape) != 2:
            raise ValueError("a 2-D surface is expected")
        return self.apply_batch(surface[None])[0]


def spatial_lowpass_filter(H: int, W: int, du: float, cutoff_in_hz: float = 1.0, order: int = 4, ctx: Context | None = None,
                           batch: int = 16) -> Spatial2DButterworth:
    """The filter wasspost spatial_lowpass builds for an H x W grid: the cutoff is the deep-water wavenumber of cutoff_in_hz,
    2 pi f^2 / 9.81, taken in cycles per metre as the reference does."""
    return Spatial2DButterworth(int(H), int(W), du, 2.0 * np.pi * cutoff_in_hz ** 2 / 9.81, order, ctx=ctx, batch=batch)


def spatial_lowpass(data, du: float, cutoff_in_hz: float = 1.0, order: int = 4, ctx: Context | None = None, out=None, batch: int = 16):
    """wasspost spatial_lowpass as a function: every frame of the count x H x W cube through spatial_lowpass_filter."""
    if len(data.shape) != 3:
        raise ValueError("data must be count x H x W")
    filt = spatial_lowpass_filter(data.shape[1], data.shape[2], du, cutoff_in_hz, order, ctx=ctx, batch=batch)
    try:
        return filt.apply_batch(data, out=out)
    finally:
        filt.close()


# ---- visibility map of the cube: wasspost visibilitymap (wasspost.py:495-621) and geometry.py -----------------------------------
def _gradient_line(f: np.ndarray, d, axis: int) -> np.ndarray:
    """np.gradient(f, d, axis=axis) with edge_order 1, restated: interior (f[k+1] - f[k-1]) / (2 d), edges (f[1] - f[0]) / d.  As
    numpy does, a float32 `f` gives float32: the differences are taken in float32 and the quotients, formed in fp64, are
    rounded to float32 (the explicit casts keep this independent of numpy's promotion rules)."""
    f = np.moveaxis(f, axis, 0)
    wide = np.float64
    out = np.empty(f.shape, f.dtype)
    d = wide(d)
    out[1:-1] = (f[2:] - f[:-2]).astype(wide) / (wide(2.0) * d)
    out[0] = (f[1] - f[0]).astype(wide) / d
    out[-1] = (f[-1] - f[-2]).astype(wide) / d
    return np.moveaxis(out, 0, axis)


def compute_slope_and_normals(XX, YY, ZZ):
    """geometry.py's function on the host: (slope [H, W, 2] = (d/dx, d/dy), unit normals [H, W, 3] = (-sx, -sy, 1) / |.|).  A
    float32 ZZ gives float32 slopes, as np.gradient does; the normals are float64."""
    XX, YY, ZZ = np.asarray(XX), np.asarray(YY), np.asarray(ZZ)
    if ZZ.ndim != 2 or XX.shape != ZZ.shape or YY.shape != ZZ.shape:
        raise ValueError("XX, YY and ZZ must be H x W")
    if ZZ.shape[0] < 2 or ZZ.shape[1] < 2:
        raise ValueError("H and W must be at least 2")
    if not np.issubdtype(ZZ.dtype, np.floating):
        ZZ = ZZ.astype(np.float64)
    dx = XX[0, 1] - XX[0, 0]
    dy = YY[1, 0] - YY[0, 0]
    if not (dx > 0.0 and dy > 0.0):
        raise ValueError("dx and dy must be positive")
    slope_y, slope_x = _gradient_line(ZZ, dy, 0), _gradient_line(ZZ, dx, 1)
    slope = np.dstack((slope_x[:, :, None], slope_y[:, :, None]))
    normals = np.dstack((slope_x[:, :, None], slope_y[:, :, None], -np.ones((ZZ.shape[0], ZZ.shape[1], 1))))
    normals = -normals / np.sqrt(np.add.reduce(normals * normals, axis=-1, keepdims=True))
    return slope, normals


def visibility_scratch_bytes(count: int, H: int, W: int, batch: int = 8, host: bool = True):
    """(bytes of device scratch, frames per launch) of one visibility_map call; no GPU needed."""
    return _scratch_bytes("visibility", (int(count), int(H), int(W), int(batch), int(bool(host))), f"{count}, {H}, {W}, batch {batch}")


def _check_grid(XX, YY, H: int, W: int):
    XX, YY = np.ascontiguousarray(XX, np.float64), np.ascontiguousarray(YY, np.float64)
    if H < 2 or W < 2:
        raise ValueError("H and W must be at least 2")
    if XX.shape != (H, W) or YY.shape != (H, W):
        raise ValueError(f"XX and YY must be {H} x {W}, like a frame")
    dx, dy = XX[0, 1] - XX[0, 0], YY[1, 0] - YY[0, 0]
    if not (dx > 0.0 and dy > 0.0):
        raise ValueError("dx and dy must be positive")
    if not np.allclose(dx, dy):
        raise ValueError("grid cells must be square")
    return XX, YY


def visibility_map(data, XX, YY, cam_to_grid, datascale: float = 1e-3, angle_limit: float = 88.0, ctx: Context | None = None,
                   out_occlusion=None, out_angles=None, batch: int = 8):
    """wasspost visibilitymap as a function: (occlusion uint8 [count, H, W], incident_angles float32 [count, H, W] in degrees,
    occluded_percent float64 [count]).  `data` is the count x H x W float32 cube in the unit that `datascale` turns into metres: a
    host array or memmap (host results) or a device tensor (device results); XX, YY are the H x W grid coordinates in metres,
    cam_to_grid the 4 x 4 Cam{n}toGrid matrix, whose last column is the camera.  A cell is occluded if its ray to the camera
    meets the surface, or if its incident angle is at least angle_limit (None, a negative or an infinite value: no such rule).
    The march is the reference's bit for bit; where the reference is undefined: NaN cells never occlude and have mask 0 and a
    NaN angle, a cell exactly under the camera is not occluded, and a finite cell at or above the camera raises ValueError."""
    if len(data.shape) != 3:
        raise ValueError("data must be count x H x W")
    count, H, W = (int(v) for v in data.shape)
    if count < 1:
        raise ValueError("no frames")
    XX, YY = _check_grid(XX, YY, H, W)
    cam = np.asarray(cam_to_grid, np.float64)
    if cam.shape != (4, 4):
        raise ValueError("cam_to_grid must be 4 x 4")
    origin = np.ascontiguousarray(cam[:3, -1])
    if int(batch) < 1:
        raise ValueError("batch must be at least 1")
    limit = -1.0 if angle_limit is None else float(angle_limit)
    if ctx is None:
        ctx = Context(0)
    counts = np.zeros(count, np.uint64)
    up = C.c_uint64()
    tail = (origin.ctypes.data, float(datascale), limit, int(batch))
    grid = [XX, YY]
    if _is_device(data):
        import torch
        grid = [torch.from_numpy(g).to(data.device) for g in grid]      # before _cube_io: it waits for the caller's stream
    data, outs, suffix, a = _cube_io(data, (out_occlusion, out_angles), "visibility_map", ("uint8", "float32"), dense=True)
    gp, op = ([_ptr_strides(v)[0] for v in vs] for vs in (grid, outs))
    ctx._check(getattr(ctx._lib, "wass_visibility" + suffix)(ctx._h, *a, *gp, *tail, *op, counts.ctypes.data, C.byref(up)))
    if up.value:
        raise ValueError(f"rays must go upward: {up.value} cells lie at or above the camera")
    return outs[0], outs[1], 100.0 * counts.astype(np.float64) / float(H * W)


def compute_occlusion_mask(ZZ, ray_d, invert_y_axis: bool = False, ctx: Context | None = None):
    """geometry.py's compute_occlusion_mask on the GPU: ZZ is an H x W surface in cell units, ray_d the H x W x 3 ray of every cell
    (ray_d[..., 2] > 0); the uint8 mask is 1 where the cell's ray, marched one cell of its dominant axis per step, meets the
    surface.  Host arrays give a host mask, device tensors a device mask.  The reference's assertions raise ValueError."""
    if len(ZZ.shape) != 2 or tuple(ray_d.shape) != (int(ZZ.shape[0]), int(ZZ.shape[1]), 3):
        raise ValueError("ray_d must be H x W x 3 for an H x W surface")
    H, W = (int(v) for v in ZZ.shape)
    if H < 1 or W < 1:
        raise ValueError("empty surface")
    if ctx is None:
        ctx = Context(0)
    up = C.c_uint64()
    if _is_device(ZZ):
        import torch
        if not _is_device(ray_d):
            raise ValueError("ZZ and ray_d must be on the same side")
        z, r = ZZ.to(torch.float64).contiguous(), ray_d.to(torch.float64).contiguous()
        mask = torch.empty((H, W), dtype=torch.uint8, device=z.device)
        torch.cuda.current_stream(z.device).synchronize()
        ctx._check(ctx._lib.wass_occlusion_rays_dev(ctx._h, z.data_ptr(), r.data_ptr(), H, W, int(bool(invert_y_axis)), mask.data_ptr(), C.byref(up)))
    else:
        z, r = np.ascontiguousarray(ZZ, np.float64), np.ascontiguousarray(ray_d, np.float64)
        mask = np.empty((H, W), np.uint8)
        ctx._check(ctx._lib.wass_occlusion_rays(ctx._h, z.ctypes.data, r.ctypes.data, H, W, int(bool(invert_y_axis)), mask.ctypes.data, C.byref(up)))
    if up.value:
        raise ValueError("rays must go upward")
    return mask


# ---- radiance of the cube: wasspost radiance (wasspost.py:813-919), bgimage (:1010-1074), radiance_threshold (:1079-1145) --------
def lanczos4_table() -> np.ndarray:
    """The fixed-point table of the Lanczos4 sampler, int16 [32, 32, 8, 8] = [fy, fx, ky, kx] (OpenCV's initInterTab2D, restated);
    no GPU needed."""
    from . import _lib
    tab = np.empty((32, 32, 8, 8), np.int16)
    rc = _lib.load().wass_lanczos4_table(tab.ctypes.data)
    if rc:
        raise ValueError(f"wass_lanczos4_table: error {rc}")
    return tab


def _check_picture(shape):
    if len(shape) != 2 or not (1 <= int(shape[0]) < 32767 and 1 <= int(shape[1]) < 32767):
        raise ValueError("a picture is Ih x Iw uint8 with sides from 1 to 32766")


def remap_lanczos4(image, mapx, mapy, ctx: Context | None = None):
    """cv.remap(image, mapx, mapy, cv.INTER_LANCZOS4) for a uint8 picture and float32 maps, constant border 0, in OpenCV's own
    fixed-point arithmetic (1/32 pixel phases, int16 weights scaled by 2^15).  Host arrays give a host result, device tensors a
    device tensor.  Where OpenCV is undefined -- a map value that is NaN, infinite or beyond +-2^26 -- the result is 0."""
    _check_picture(image.shape)
    if len(mapx.shape) != 2 or tuple(mapx.shape) != tuple(mapy.shape) or min(int(v) for v in mapx.shape) < 1:
        raise ValueError("mapx and mapy must be two h x w maps of one shape")
    sh, sw = (int(v) for v in image.shape)
    dh, dw = (int(v) for v in mapx.shape)
    if ctx is None:
        ctx = Context(0)
    if _is_device(image):
        import torch
        if not (_is_device(mapx) and _is_device(mapy)):
            raise ValueError("the picture and the maps must be on the same side")
        src = image.to(torch.uint8).contiguous()
        mx, my = mapx.to(torch.float32).contiguous(), mapy.to(torch.float32).contiguous()
        dst = torch.empty((dh, dw), dtype=torch.uint8, device=src.device)
        torch.cuda.current_stream(src.device).synchronize()
        ctx._check(ctx._lib.wass_remap_lanczos4_dev(ctx._h, src.data_ptr(), sw, sh, sw, mx.data_ptr(), my.data_ptr(), dw, dh, dst.data_ptr()))
        ctx.synchronize()
        return dst
    src = np.ascontiguousarray(image, np.uint8)
    mx, my = np.ascontiguousarray(mapx, np.float32), np.ascontiguousarray(mapy, np.float32)
    dst = np.empty((dh, dw), np.uint8)
    ctx._check(ctx._lib.wass_remap_lanczos4(ctx._h, src.ctypes.data, sw, sh, sw, mx.ctypes.data, my.ctypes.data, dw, dh, dst.ctypes.data))
    return dst


def radiance_pcam(Pplane, Iw: int, Ih: int) -> np.ndarray:
    """The 4 x 4 projection from grid coordinates into pixels of an Iw x Ih picture: inv(toNorm) @ P{cam}plane, where toNorm
    takes pixels to the square [-1, 1]^2 (x * 2 / Iw - 1, y * 2 / Ih - 1).  numpy's inv and matmul, as the reference uses them."""
    Pplane = np.asarray(Pplane, np.float64)
    if Pplane.shape != (4, 4):
        raise ValueError("Pplane must be 4 x 4")
    to_norm = np.eye(4)
    to_norm[0, 0], to_norm[0, 2] = 2.0 / Iw, -1
    to_norm[1, 1], to_norm[1, 2] = 2.0 / Ih, -1
    return np.linalg.inv(to_norm) @ Pplane


def workspace_images(wassdir: str, cam: int, count: int):
    """Yields the undistorted pictures of camera `cam` of a WASS output directory, frame by frame, as grey uint8 arrays:
    <wassdir>/%06d_wd/undistorted/%08d.png."""
    import os
    from PIL import Image
    for idx in range(int(count)):
        with Image.open(os.path.join(wassdir, "%06d_wd" % idx, "undistorted", "%08d.png" % int(cam))) as im:
            yield np.asarray(im.convert("L"), np.uint8)


def radiance_scratch_bytes(count: int, H: int, W: int, Ih: int, Iw: int, batch: int = 8, host: bool = True):
    """(bytes of device scratch, frames per launch) of one radiance call; no GPU needed."""
    return _scratch_bytes("radiance", (int(count), int(H), int(W), int(Ih), int(Iw), int(batch), int(bool(host))),
                          f"{count}, {H}, {W}, pictures {Ih} x {Iw}, batch {batch}")


def _radiance_chunk(ctx, imgs, data, XX, YY, dgrid, pcam, datascale, batch, out, levels=0):
    """frames of one picture size: imgs n x Ih x Iw (host array or device tensor), data n x H x W and out n x 2^levels H x 2^levels W
    on the cube's side"""
    n, H, W = (int(v) for v in data.shape)
    Ih, Iw = int(imgs.shape[1]), int(imgs.shape[2])
    P = np.ascontiguousarray(pcam[:3], np.float64)
    name, up = ("wass_radiance_up", (int(levels),)) if levels else ("wass_radiance", ())
    if _is_device(data):
        import torch
        if not _is_device(imgs):
            imgs = torch.from_numpy(np.ascontiguousarray(imgs, np.uint8)).to(data.device)
        imgs = imgs.to(torch.uint8).contiguous()
        torch.cuda.current_stream(data.device).synchronize()
        ctx._check(getattr(ctx._lib, name + "_dev")(ctx._h, imgs.data_ptr(), Ih * Iw, Iw, Ih, Iw, data.data_ptr(), data.stride(0), data.stride(1),
                                                    n, H, W, dgrid[0].data_ptr(), dgrid[1].data_ptr(), P.ctypes.data, float(datascale), int(batch),
                                                    *up, out.data_ptr()))
        ctx.synchronize()
        return
    if _is_device(imgs):
        imgs = imgs.cpu().numpy()
    imgs = np.ascontiguousarray(imgs, np.uint8)
    ctx._check(getattr(ctx._lib, name)(ctx._h, imgs.ctypes.data, Ih * Iw, Iw, Ih, Iw, data.ctypes.data, data.strides[0] // 4, data.strides[1] // 4,
                                       n, H, W, XX.ctypes.data, YY.ctypes.data, P.ctypes.data, float(datascale), int(batch), *up, out.ctypes.data))


def radiance(images, data, XX, YY, Pplane, datascale: float = 1e-3, upscalefactor: int = 1, ctx: Context | None = None, out=None,
             batch: int = 8):
    """wasspost radiance as a function: float32 [count, H, W], the camera picture sampled at every cell of every frame and divided
    by 255.  `images` is a count x Ih x Iw uint8 array or tensor, or an iterable of Ih x Iw frames (workspace_images); `data` the
    count x H x W float32 cube in the unit that `datascale` turns into metres, a host array or memmap (host result) or a device
    tensor (device result); XX, YY the H x W grid in metres; Pplane the 4 x 4 P{cam}plane matrix.  Per cell the height is
    data * float32(datascale) in float32, the projection ((P0 X + P1 Y) + P2 z) + P3 per row in fp64, the maps its quotients cast
    to float32, and the sampler remap_lanczos4.  Cells whose height is NaN, or that project outside the picture, are 0.
    `upscalefactor` must be 1 here: the finer grid is radiance_upscaled's."""
    if int(upscalefactor) != 1:
        raise NotImplementedError("radiance samples the grid as it is: for upscalefactor other than 1 call radiance_upscaled")
    return _radiance_frames(images, data, XX, YY, Pplane, datascale, 0, ctx, out, batch)


def _radiance_frames(images, data, XX, YY, Pplane, datascale, levels, ctx, out, batch):
    """radiance and radiance_upscaled: the checks, the outputs and the chunks of pictures of one size; `levels` of pyrUp (0: none)"""
    if len(data.shape) != 3:
        raise ValueError("data must be count x H x W")
    count, H, W = (int(v) for v in data.shape)
    if count < 1 or H < 1 or W < 1:
        raise ValueError("no frames")
    if levels and (H < 2 or W < 2):
        raise ValueError("H and W must be at least 2 to be upsampled")
    oshape = (count, H << levels, W << levels)
    XX, YY = np.ascontiguousarray(XX, np.float64), np.ascontiguousarray(YY, np.float64)
    if XX.shape != (H, W) or YY.shape != (H, W):
        raise ValueError(f"XX and YY must be {H} x {W}, like a frame")
    if np.asarray(Pplane).shape != (4, 4):
        raise ValueError("Pplane must be 4 x 4")
    if int(batch) < 1:
        raise ValueError("batch must be at least 1")
    whole = hasattr(images, "shape") and len(images.shape) == 3
    if whole:
        if int(images.shape[0]) != count:
            raise ValueError(f"{int(images.shape[0])} pictures for {count} frames")
        _check_picture(images.shape[1:])
    if ctx is None:
        ctx = Context(0)
    data, (out,), suffix, _ = _cube_io(data, (out,), "radiance", shape=oshape, dense=True)
    dgrid = None
    if suffix:
        import torch
        dgrid = (torch.from_numpy(XX).to(data.device), torch.from_numpy(YY).to(data.device))    # _radiance_chunk waits for them
    if whole:
        pcam = radiance_pcam(Pplane, int(images.shape[2]), int(images.shape[1]))
        _radiance_chunk(ctx, images, data, XX, YY, dgrid, pcam, datascale, batch, out, levels)
        return out
    t0, pending = 0, []

    def flush():
        nonlocal t0, pending
        if pending:
            stack = np.stack(pending)
            pcam = radiance_pcam(Pplane, stack.shape[2], stack.shape[1])
            _radiance_chunk(ctx, stack, data[t0:t0 + len(pending)], XX, YY, dgrid, pcam, datascale, batch, out[t0:t0 + len(pending)], levels)
            t0 += len(pending)
            pending = []

    for frame in images:
        frame = frame.cpu().numpy() if _is_device(frame) else np.asarray(frame)
        _check_picture(frame.shape)
        if t0 + len(pending) >= count:
            raise ValueError(f"more than {count} pictures")
        if pending and pending[0].shape != frame.shape:
            flush()                                     # the projection depends on the picture's size
        pending.append(np.ascontiguousarray(frame, np.uint8))
        if len(pending) == int(batch):
            flush()
    flush()
    if t0 != count:
        raise ValueError(f"{t0} pictures for {count} frames")
    return out


# ---- pyramid upsampling: cv.pyrUp, and wasspost radiance --upscalefactor N on it (wasspost.py:840-843, 880-896) --------------------
PYR_MAX_LEVELS = 4


def pyr_up_scratch_bytes(count: int, H: int, W: int, levels: int = 1, dtype=np.float32, batch: int = 8, host: bool = True):
    """(bytes of device scratch, frames per launch) of one pyr_up call; no GPU needed.  With e the element size, b the frames per
    launch and every term rounded up to 256 bytes: the levels below the last, sum over l = 1 .. levels - 1 of b 4^l H W e, and from
    the host also the input b H W e and the result b 4^levels H W e.  b is `batch` (pyr_up itself uses 8), at most count, halved
    until the sum is at most 16 GiB."""
    return _scratch_bytes("pyrup", (int(count), int(H), int(W), int(levels), int(np.dtype(dtype).itemsize), int(batch), int(bool(host))),
                          f"{count}, {H}, {W}, levels {levels}, {np.dtype(dtype)}, batch {batch}")


def _device_span(t):
    """[first byte, one past the last byte) of a device tensor with positive strides"""
    n = 1 + sum((int(s) - 1) * int(st) for s, st in zip(t.shape, t.stride()))
    return t.data_ptr(), t.data_ptr() + n * t.element_size()


def pyr_up(a, levels: int = 1, ctx: Context | None = None, out=None):
    """cv.pyrUp applied `levels` times (1 to 4): an H x W picture or a count x H x W cube of them, float32 or float64, H and W at
    least 2, becomes 2^levels H x 2^levels W per frame.  A host array or memmap gives a host array, a device tensor a device
    tensor, of the input's dtype; a strided view passes as it is where its last axis is contiguous, and so does `out`, which must
    not overlap the input.  Each level is OpenCV 4.5.5's scalar pyrUp restated (weights 1 4 6 4 1 per axis, x first, the sums
    in the element type in the order DESIGN.md states, times 1/64): bit for bit tests/pyramid_oracle.py, not pinned against
    OpenCV itself.  NaN and infinite cells spread over the cells they weigh on."""
    levels = int(levels)
    if not 1 <= levels <= PYR_MAX_LEVELS:
        raise ValueError(f"levels must be from 1 to {PYR_MAX_LEVELS}")
    if len(a.shape) not in (2, 3):
        raise ValueError("a picture is H x W, a cube count x H x W")
    single = len(a.shape) == 2
    dev = _is_device(a)
    if dev:
        import torch
        kinds = {torch.float32: ("f32", 4), torch.float64: ("f64", 8)}
    else:
        if not isinstance(a, np.ndarray):
            a = np.asarray(a)
        kinds = {np.dtype(np.float32): ("f32", 4), np.dtype(np.float64): ("f64", 8)}
    if a.dtype not in kinds:
        raise ValueError(f"pyr_up takes float32 or float64, not {a.dtype}")
    kind, e = kinds[a.dtype]
    src = a[None] if single else a
    count, H, W = (int(v) for v in src.shape)
    if count < 1:
        raise ValueError("no frames")
    if H < 2 or W < 2:
        raise ValueError("H and W must be at least 2")
    if max(H, W) << levels > 65536:
        raise ValueError("a side of the result is above 65536")
    oshape = (count, H << levels, W << levels)
    if out is not None and (_is_device(out) != dev or out.dtype != a.dtype or tuple(out.shape) != (oshape[1:] if single else oshape)):
        raise ValueError(f"out must be on the input's side, of its dtype and {' x '.join(str(v) for v in (oshape[1:] if single else oshape))}")
    if dev:
        if src.stride(2) != 1 or (count > 1 and src.stride(0) <= 0) or src.stride(1) <= 0:      # (the stride of an axis of 1 says nothing)
            src = src.contiguous()
        dst = torch.empty(oshape, dtype=a.dtype, device=a.device) if out is None else (out[None] if single else out)
        if dst.stride(2) != 1 or dst.stride(1) < oshape[2] or (count > 1 and dst.stride(0) < (oshape[1] - 1) * dst.stride(1) + oshape[2]):
            raise ValueError("out must have a contiguous last axis and rows and frames that do not overlap")
        (a0, a1), (b0, b1) = _device_span(src), _device_span(dst)
        if a0 < b1 and b0 < a1:
            raise ValueError("out must not overlap the input")
        if ctx is None:
            ctx = Context(0)
        torch.cuda.current_stream(a.device).synchronize()
        ctx._check(getattr(ctx._lib, f"wass_pyrup_{kind}_dev")(ctx._h, src.data_ptr(), src.stride(0), src.stride(1), count, H, W, levels,
                                                               dst.data_ptr(), dst.stride(0), dst.stride(1)))
        ctx.synchronize()
    else:
        if src.strides[2] != e or src.strides[1] % e or src.strides[1] <= 0 or (count > 1 and (src.strides[0] % e or src.strides[0] <= 0)):
            src = np.ascontiguousarray(src)
        dst = np.empty(oshape, a.dtype) if out is None else (out[None] if single else out)
        if dst.strides[2] != e or dst.strides[1] % e or dst.strides[1] < oshape[2] * e \
                or (count > 1 and (dst.strides[0] % e or dst.strides[0] < (oshape[1] - 1) * dst.strides[1] + oshape[2] * e)):
            raise ValueError("out must have a contiguous last axis and rows and frames that do not overlap")
        if np.shares_memory(src, dst):
            raise ValueError("out must not overlap the input")
        if ctx is None:
            ctx = Context(0)
        ctx._check(getattr(ctx._lib, f"wass_pyrup_{kind}")(ctx._h, src.ctypes.data, src.strides[0] // e, src.strides[1] // e, count, H, W, levels,
                                                           dst.ctypes.data, dst.strides[0] // e, dst.strides[1] // e))
    if out is not None:
        return out
    return dst[0] if single else dst


def radiance_upscaled_scratch_bytes(count: int, H: int, W: int, Ih: int, Iw: int, upscalefactor: int = 2, batch: int = 8, host: bool = True):
    """(bytes of device scratch, frames per launch) of one radiance_upscaled call over pictures of one size; no GPU needed.  With
    L = upscalefactor - 1 levels, b frames per launch and every term rounded up to 256 bytes: per call the upsampled grid
    2 x 4^L H W 8 and its lower levels, sum over l = 1 .. L - 1 of 4^l H W 8; per launch the scaled heights b H W 4, their lower
    levels, sum of b 4^l H W 4, and the upsampled heights b 4^L H W 4.  From the host also XX and YY 2 x H W 8, the pictures
    b Ih Iw, the heights b H W 4 and the result b 4^L H W 4.  b is `batch`, at most count, halved until the sum is at most 16 GiB.
    upscalefactor 1 is radiance_scratch_bytes."""
    levels = int(upscalefactor) - 1
    if levels == 0:
        return radiance_scratch_bytes(count, H, W, Ih, Iw, batch, host)
    return _scratch_bytes("radiance_up", (int(count), int(H), int(W), int(Ih), int(Iw), levels, int(batch), int(bool(host))),
                          f"{count}, {H}, {W}, pictures {Ih} x {Iw}, levels {levels}, batch {batch}")


def radiance_upscaled(images, data, XX, YY, Pplane, upscalefactor: int = 2, datascale: float = 1e-3, ctx: Context | None = None, out=None,
                      batch: int = 8):
    """wasspost radiance --upscalefactor N as a function: the radiance on a grid finer than the cube's.  `upscalefactor` has the
    reference's meaning: the grid XX, YY (fp64) and every frame's heights (float32, already multiplied by float32(datascale)) go
    through pyr_up upscalefactor - 1 times, so 2 doubles H and W, 3 quadruples them, up to 5; 1 is radiance itself.  The result is
    float32 [count, 2^(N-1) H, 2^(N-1) W].  images, data, XX, YY, Pplane, out, batch and the host / device split are radiance's."""
    levels = int(upscalefactor) - 1
    if not 0 <= levels <= PYR_MAX_LEVELS:
        raise ValueError(f"upscalefactor must be from 1 to {PYR_MAX_LEVELS + 1}")
    return _radiance_frames(images, data, XX, YY, Pplane, datascale, levels, ctx, out, batch)


def bgimage_scratch_bytes(count: int, H: int, W: int, filtersize: int = 2000, slab_rows: int = 0, host: bool = True):
    """(bytes of device scratch, rows per slab) of one bgimage call; no GPU needed."""
    return _scratch_bytes("bgimage", (int(count), int(H), int(W), int(filtersize), int(slab_rows), int(bool(host))),
                          f"{count}, {H}, {W}, size {filtersize}")


def bgimage(data, filtersize: int = 2000, ctx: Context | None = None, out=None, slab_rows: int = 0):
    """wasspost bgimage as a function: scipy.ndimage.uniform_filter1d(data, filtersize, axis=0, mode='reflect') of the count x H x W
    float32 cube, bit for bit (the whole series in one run: no chunks, so no restart of the running sum).  A host array or memmap
    gives a host array, a device tensor a device tensor; `out` must not be `data`.  slab_rows > 0 caps the rows filtered at a
    time (the result does not depend on it)."""
    if len(data.shape) != 3:
        raise ValueError("data must be count x H x W")
    count, H, W = (int(v) for v in data.shape)
    if count < 1 or H < 1 or W < 1:
        raise ValueError("empty cube")
    if int(filtersize) < 1:
        raise ValueError("filtersize must be at least 1")
    if ctx is None:
        ctx = Context(0)
    data, (out,), suffix, a = _cube_io(data, (out,), "bgimage", alias=False)
    ctx._check(getattr(ctx._lib, "wass_bgimage" + suffix)(ctx._h, *a, int(filtersize), int(slab_rows), *_ptr_strides(out)))
    if suffix:
        ctx.synchronize()
    return out


VATS_BINS = 30


def radiance_threshold_scratch_bytes(count: int, H: int, W: int, batch: int = 8, host: bool = True):
    """(bytes of device scratch, frames per launch) of one pass of radiance_threshold; no GPU needed."""
    return _scratch_bytes("radiance_threshold", (int(count), int(H), int(W), int(batch), int(bool(host))), f"{count}, {H}, {W}, batch {batch}")


def vats_threshold(counts, bin_edges):
    """The threshold wasspost derives from the histogram of a frame (density=True): among the bins from the peak on, the one
    farthest from the straight line through the peak and the last bin, in (bin number, density) coordinates; its right edge."""
    counts, bin_edges = np.asarray(counts), np.asarray(bin_edges)
    density = counts / np.array(np.diff(bin_edges), float) / counts.sum()          # np.histogram's own expression
    nbins = density.shape[0]
    pts = np.vstack((np.arange(nbins), density, np.ones(nbins)))                    # homogeneous points, one per column
    peak = int(np.argmax(density))
    line = np.cross(pts[:, peak], pts[:, -1])
    far = int(np.argmax(np.abs(line @ pts)[peak:])) + peak
    return bin_edges[far + 1]


def _threshold_sides(radiance, radiance_bg):
    if len(radiance.shape) != 3 or tuple(radiance.shape) != tuple(radiance_bg.shape):
        raise ValueError("radiance and radiance_bg must be two count x H x W cubes of one shape")
    if min(int(v) for v in radiance.shape) < 1:
        raise ValueError("empty cube")
    if _is_device(radiance) != _is_device(radiance_bg):
        raise ValueError("radiance and radiance_bg must be on the same side")
    if _is_device(radiance):
        import torch
        both = []
        for a in (radiance, radiance_bg):
            if a.dtype != torch.float32 or a.stride(2) != 1 or a.stride(0) <= 0 or a.stride(1) <= 0:
                a = a.to(torch.float32).contiguous()
            both.append(a)
        torch.cuda.current_stream(both[0].device).synchronize()
        return both[0], both[1], "_dev", [v for a in both for v in (a.data_ptr(), a.stride(0), a.stride(1))]
    a, b = _host_f32_rows(radiance), _host_f32_rows(radiance_bg)
    return a, b, "", [v for x in (a, b) for v in (x.ctypes.data, x.strides[0] // 4, x.strides[1] // 4)]


def radiance_histogram(radiance, radiance_bg, ctx: Context | None = None, batch: int = 8):
    """What the VATS rule sees, per frame: (counts int64 [count, 30], bin_edges float32 [count, 31], min(Ibg) float32 [count]) of
    Isub = I - (Ibg - min(Ibg)), equal to np.histogram(Isub, bins=30).  ValueError if Isub holds a value that is not finite."""
    I, B, suffix, ptrs = _threshold_sides(radiance, radiance_bg)
    count, H, W = (int(v) for v in I.shape)
    if ctx is None:
        ctx = Context(0)
    lib = ctx._lib
    m, lo, hi = (np.empty(count, np.float32) for _ in range(3))
    bad = np.zeros(count, np.uint32)
    ctx._check(getattr(lib, "wass_radiance_range" + suffix)(ctx._h, *ptrs, count, H, W, int(batch), m.ctypes.data, lo.ctypes.data, hi.ctypes.data,
                                                           bad.ctypes.data))
    if bad.any():
        t = int(np.flatnonzero(bad)[0])
        raise ValueError(f"frame {t}: {int(bad[t])} cells of the background-subtracted radiance are not finite; the histogram has no range")
    edges = np.stack([np.histogram_bin_edges(np.array([lo[t], hi[t]], np.float32), bins=VATS_BINS) for t in range(count)])
    edges = np.ascontiguousarray(edges, np.float32)
    counts = np.zeros((count, VATS_BINS), np.uint32)
    ctx._check(getattr(lib, "wass_radiance_hist" + suffix)(ctx._h, *ptrs, count, H, W, int(batch), m.ctypes.data, edges.ctypes.data, counts.ctypes.data))
    return counts.astype(np.int64), edges, m


def radiance_threshold(radiance, radiance_bg, threshold_val: float = 0.35, use_vats: bool = False, ctx: Context | None = None, batch: int = 8):
    """wasspost radiance_threshold as a function: (mask uint8 [count, H, W], thresholds float32 [count]).  Per frame, in float32,
    Isub = I - (Ibg - min(Ibg)) and mask = Isub > threshold, the threshold being threshold_val or, with use_vats, the one
    vats_threshold derives from the 30-bin histogram of Isub (counted on the device, equal to np.histogram's).  Host arrays or
    memmaps give a host mask, device tensors a device mask; the thresholds are a host array.  With use_vats a frame with a value
    that is not finite raises ValueError, as numpy's histogram does; without, such cells compare false."""
    if int(batch) < 1:
        raise ValueError("batch must be at least 1")
    I, B, suffix, ptrs = _threshold_sides(radiance, radiance_bg)
    count, H, W = (int(v) for v in I.shape)
    if ctx is None:
        ctx = Context(0)
    lib = ctx._lib
    if use_vats:
        counts, edges, m = radiance_histogram(I, B, ctx=ctx, batch=batch)
        thr = np.array([vats_threshold(counts[t], edges[t]) for t in range(count)], np.float32)
    else:
        m, lo, hi = (np.empty(count, np.float32) for _ in range(3))
        bad = np.zeros(count, np.uint32)
        ctx._check(getattr(lib, "wass_radiance_range" + suffix)(ctx._h, *ptrs, count, H, W, int(batch), m.ctypes.data, lo.ctypes.data,
                                                               hi.ctypes.data, bad.ctypes.data))
        thr = np.full(count, np.float32(threshold_val), np.float32)
    if suffix:
        import torch
        mask = torch.empty((count, H, W), dtype=torch.uint8, device=I.device)
        ctx._check(lib.wass_radiance_mask_dev(ctx._h, *ptrs, count, H, W, int(batch), m.ctypes.data, thr.ctypes.data, mask.data_ptr()))
    else:
        mask = np.empty((count, H, W), np.uint8)
        ctx._check(lib.wass_radiance_mask(ctx._h, *ptrs, count, H, W, int(batch), m.ctypes.data, thr.ctypes.data, mask.ctypes.data))
    return mask, thr


# ---- polarimetric set-up of the cube: wasspost polarimetric_setup (wasspost.py:627-805), clip and zeromean ------------------------
POL_OUTPUTS = ("S", "occlusion", "angles", "dolp", "normals", "rays_cam")       # bit k of the C entry's `outputs` is POL_OUTPUTS[k]


def bilinear_table() -> np.ndarray:
    """The weights of the bilinear sampler, float32 [32, 32, 2, 2] = [fy, fx, ky, kx] (OpenCV's initInterTab2D for INTER_LINEAR,
    restated): ty[ky] * tx[kx] with t = (1 - f / 32, f / 32); no GPU needed."""
    from . import _lib
    tab = np.empty((32, 32, 2, 2), np.float32)
    rc = _lib.load().wass_bilinear_table_f32(tab.ctypes.data)
    if rc:
        raise ValueError(f"wass_bilinear_table_f32: error {rc}")
    return tab


def remap_linear_f32(image, mapx, mapy, ctx: Context | None = None):
    """cv.remap(image, mapx, mapy, cv.INTER_LINEAR) for a float32 picture and float32 maps, constant border 0, in OpenCV's float
    pipeline: 1/32 pixel phases, the four float32 weights of bilinear_table(), ((v00 w00 + v01 w01) + v10 w10) + v11 w11 in float32.
    Host arrays give a host result, device tensors a device tensor.  Each tap outside the picture counts 0; NaN and infinite
    samples propagate; a map value that is NaN, infinite or beyond +-2^26 gives 0."""
    if len(image.shape) != 2 or not (1 <= int(image.shape[0]) < 32767 and 1 <= int(image.shape[1]) < 32767):
        raise ValueError("a picture is Ih x Iw float32 with sides from 1 to 32766")
    if len(mapx.shape) != 2 or tuple(mapx.shape) != tuple(mapy.shape) or min(int(v) for v in mapx.shape) < 1:
        raise ValueError("mapx and mapy must be two h x w maps of one shape")
    sh, sw = (int(v) for v in image.shape)
    dh, dw = (int(v) for v in mapx.shape)
    if ctx is None:
        ctx = Context(0)
    if _is_device(image):
        import torch
        if not (_is_device(mapx) and _is_device(mapy)):
            raise ValueError("the picture and the maps must be on the same side")
        src = image.to(torch.float32).contiguous()
        mx, my = mapx.to(torch.float32).contiguous(), mapy.to(torch.float32).contiguous()
        dst = torch.empty((dh, dw), dtype=torch.float32, device=src.device)
        torch.cuda.current_stream(src.device).synchronize()
        ctx._check(ctx._lib.wass_remap_linear_f32_dev(ctx._h, src.data_ptr(), sw, sh, sw, mx.data_ptr(), my.data_ptr(), dw, dh, dst.data_ptr()))
        ctx.synchronize()
        return dst
    src = np.ascontiguousarray(image, np.float32)
    mx, my = np.ascontiguousarray(mapx, np.float32), np.ascontiguousarray(mapy, np.float32)
    dst = np.empty((dh, dw), np.float32)
    ctx._check(ctx._lib.wass_remap_linear_f32(ctx._h, src.ctypes.data, sw, sh, sw, mx.ctypes.data, my.ctypes.data, dw, dh, dst.ctypes.data))
    return dst


def _pol_outputs(outputs) -> int:
    outputs = tuple(outputs)
    for name in outputs:
        if name not in POL_OUTPUTS:
            raise ValueError(f"unknown output {name!r}: choose among {POL_OUTPUTS}")
    return sum(1 << k for k, name in enumerate(POL_OUTPUTS) if name in outputs)


def polarimetric_scratch_bytes(count: int, H: int, W: int, Ih: int, Iw: int, batch: int = 8, host: bool = True,
                               outputs=("S", "occlusion")):
    """(bytes of device scratch, frames per launch) of one polarimetric_setup call; no GPU needed."""
    return _scratch_bytes("polarimetric", (int(count), int(H), int(W), int(Ih), int(Iw), int(batch), int(bool(host)), _pol_outputs(outputs)),
                          f"{count}, {H}, {W}, pictures {Ih} x {Iw}, batch {batch}")


@dataclass
class PolarimetricResult:
    """What polarimetric_setup returns.  The per-frame arrays are None unless named in `outputs`."""
    Savg: object                    # float64 [H, W, 3]: the mean Stokes vector over the frames in which the cell is visible
    Navg: object                    # float64 [H, W, 3]: the mean normal, unit length
    Zavg: object                    # float64 [H, W]: the mean height in metres (not NaN-aware)
    valid: object                   # float64 [H, W]: in how many frames the cell is visible
    occluded_percent: np.ndarray    # float64 [count]
    S: object = None                # float32 [count, H, W, 3], NaN in occluded cells
    occlusion: object = None        # uint8 [count, H, W]
    angles: object = None           # float32 [count, H, W], degrees
    dolp: object = None             # float32 [count, H, W]
    normals: object = None          # float64 [count, H, W, 3]
    rays_cam: object = None         # float64 [count, 3, H * W]


_POL_SHAPES = {"S": (lambda H, W: (H, W, 3), "float32"), "occlusion": (lambda H, W: (H, W), "uint8"),
               "angles": (lambda H, W: (H, W), "float32"), "dolp": (lambda H, W: (H, W), "float32"),
               "normals": (lambda H, W: (H, W, 3), "float64"), "rays_cam": (lambda H, W: (3, H * W), "float64")}


def polarimetric_setup(stokes, data, XX, YY, Pplane, cam_to_grid, K, datascale: float = 1e-3, angle_limit: float = 85.0,
                       outputs=("S", "occlusion"), total_frames: int | None = None, ctx: Context | None = None, batch: int = 8):
    """wasspost polarimetric_setup as a function.  `stokes` holds the float32 pictures S0, S1, S2 of every frame: a
    count x 3 x Ih x Iw host array, memmap or device tensor, or an iterable of (S0, S1, S2) triples; `data` is the count x H x W
    float32 cube in the unit that `datascale` turns into metres, a host array or memmap (host results) or a device tensor (device
    results); XX, YY the H x W grid in metres; Pplane, cam_to_grid and K the matrices P{cam}plane (4 x 4), Cam{cam}toGrid (4 x 4)
    and intr{cam} (3 x 3).  Per frame and cell: the projection of `radiance`, the camera-frame viewing ray, the normals of
    compute_slope_and_normals, the mask and angles of visibility_map(..., angle_limit), the three pictures sampled with
    remap_linear_f32 and blanked (NaN) in occluded cells, DOLP = sqrt(S1^2 + S2^2) / S0 in float32.  The averages are fp64 sums in
    frame order: Savg = sum(nan_to_num(S)) / valid, Navg = sum(normals), normalised, Zavg = sum(z) / total_frames (default: the
    number of frames), valid = sum(1 - mask).  Only the per-frame arrays named in `outputs` are produced (normals and rays_cam
    are 48 bytes per cell and frame).  A finite cell at or above the camera raises ValueError."""
    if len(data.shape) != 3:
        raise ValueError("data must be count x H x W")
    count, H, W = (int(v) for v in data.shape)
    if count < 1:
        raise ValueError("no frames")
    XX, YY = _check_grid(XX, YY, H, W)
    cam = np.asarray(cam_to_grid, np.float64)
    if cam.shape != (4, 4):
        raise ValueError("cam_to_grid must be 4 x 4")
    K = np.asarray(K, np.float64)
    if K.shape != (3, 3):
        raise ValueError("K must be 3 x 3")
    if np.asarray(Pplane).shape != (4, 4):
        raise ValueError("Pplane must be 4 x 4")
    if int(batch) < 1:
        raise ValueError("batch must be at least 1")
    if total_frames is None:
        total_frames = count
    if int(total_frames) < 1:
        raise ValueError("total_frames must be at least 1")
    bits = _pol_outputs(outputs)
    whole = hasattr(stokes, "shape")
    if whole:
        if len(stokes.shape) != 4 or int(stokes.shape[0]) != count or int(stokes.shape[1]) != 3:
            raise ValueError(f"stokes must be {count} x 3 x Ih x Iw")
    Kinv = np.linalg.inv(K)
    if ctx is None:
        ctx = Context(0)
    data, _, dev, _ = _cube_io(data, (), "polarimetric_setup")
    if dev:
        import torch
        new = lambda shape, dt: torch.empty(shape, dtype=getattr(torch, dt), device=data.device)
        acc = torch.zeros(8 * H * W, dtype=torch.float64, device=data.device)
        grid = (torch.tensor(XX).to(data.device), torch.tensor(YY).to(data.device))      # a copy: the caller's may be read-only
        ptr = lambda a: a.data_ptr()
        entry = ctx._lib.wass_polarimetric_dev
    else:
        new = lambda shape, dt: np.empty(shape, getattr(np, dt))
        acc = np.zeros(8 * H * W, np.float64)
        grid = (XX, YY)
        ptr = lambda a: a.ctypes.data
        entry = ctx._lib.wass_polarimetric
    per_frame = {name: new((count,) + _POL_SHAPES[name][0](H, W), _POL_SHAPES[name][1])
                 for k, name in enumerate(POL_OUTPUTS) if bits >> k & 1}
    counts = np.zeros(count, np.uint64)
    from ._lib import PolOut, PolParams

    def run(pics, t0, n):
        """frames t0 .. t0 + n - 1 from pics, n x 3 x Ih x Iw on any side"""
        Ih, Iw = int(pics.shape[2]), int(pics.shape[3])
        if not (1 <= Ih < 32767 and 1 <= Iw < 32767):
            raise ValueError("a picture is Ih x Iw float32 with sides from 1 to 32766")
        pcam = radiance_pcam(Pplane, Iw, Ih)
        p = PolParams()
        p.Pcam[:] = [float(v) for v in pcam[:3].ravel()]
        p.Kinv[:] = [float(v) for v in Kinv.ravel()]
        p.origin[:] = [float(v) for v in cam[:3, -1]]
        p.datascale = float(datascale)
        p.angle_limit = -1.0 if angle_limit is None else float(angle_limit)
        p.batch = int(batch)
        p.total_frames = int(total_frames) if t0 + n == count else 0
        o = PolOut()
        for name, a in per_frame.items():
            setattr(o, name, ptr(a[t0:t0 + n]))
        up = C.c_uint64()
        cube = data[t0:t0 + n]
        if dev:
            if not _is_device(pics):
                pics = torch.from_numpy(np.ascontiguousarray(pics, np.float32)).to(data.device)
            if pics.dtype != torch.float32 or pics.stride(3) != 1 or min(pics.stride(k) for k in range(3)) <= 0:
                pics = pics.to(torch.float32).contiguous()
            torch.cuda.current_stream(data.device).synchronize()
            ss = [pics.stride(k) for k in range(3)]
            cs = (cube.stride(0), cube.stride(1))
        else:
            if _is_device(pics):
                pics = pics.cpu().numpy()
            if not isinstance(pics, np.ndarray) or pics.dtype != np.float32 or pics.strides[3] != 4 or any(s % 4 or s <= 0 for s in pics.strides[:3]):
                pics = np.ascontiguousarray(pics, np.float32)
            ss = [s // 4 for s in pics.strides[:3]]
            cs = (cube.strides[0] // 4, cube.strides[1] // 4)
        ctx._check(entry(ctx._h, ptr(pics), ss[0], ss[1], ss[2], Ih, Iw, ptr(cube), cs[0], cs[1], n, H, W, ptr(grid[0]), ptr(grid[1]),
                         C.byref(p), ptr(acc), C.byref(o), counts[t0:].ctypes.data, C.byref(up)))
        if up.value:
            raise ValueError(f"rays must go upward: {up.value} cells lie at or above the camera")

    if whole:
        run(stokes, 0, count)
    else:
        t0, pending = 0, []

        def flush():
            nonlocal t0, pending
            if pending:
                if dev and all(_is_device(a) for tr in pending for a in tr):
                    import torch
                    stack = torch.stack([torch.stack(list(tr)) for tr in pending])
                else:
                    stack = np.stack([np.stack([a.cpu().numpy() if _is_device(a) else np.asarray(a, np.float32) for a in tr]) for tr in pending])
                run(stack, t0, len(pending))
                t0 += len(pending)
                pending = []

        for triple in stokes:
            triple = tuple(triple)
            if len(triple) != 3 or any(len(a.shape) != 2 or tuple(a.shape) != tuple(triple[0].shape) for a in triple):
                raise ValueError("every frame needs three pictures S0, S1, S2 of one shape")
            if t0 + len(pending) >= count:
                raise ValueError(f"more than {count} frames of pictures")
            if pending and tuple(pending[0][0].shape) != tuple(triple[0].shape):
                flush()                                 # the projection depends on the picture's size
            pending.append(triple)
            if len(pending) == int(batch) and t0 + len(pending) < count:
                flush()                                 # the last chunk is flushed below: it ends the sequence
        if t0 + len(pending) != count:
            raise ValueError(f"{t0 + len(pending)} frames of pictures for {count} frames")
        flush()
    if dev:
        ctx.synchronize()
    HW = H * W
    return PolarimetricResult(Savg=acc[:3 * HW].reshape(H, W, 3), Navg=acc[3 * HW:6 * HW].reshape(H, W, 3), Zavg=acc[6 * HW:7 * HW].reshape(H, W),
                              valid=acc[7 * HW:].reshape(H, W), occluded_percent=100.0 * counts.astype(np.float64) / float(HW), **per_frame)


def clip_cube(data, minval: float, maxval: float, out=None, ctx: Context | None = None):
    """wasspost clip as a function: (np.clip(data, float32(minval), float32(maxval)) in float32 with NaN kept, vmin, vmax), vmin
    and vmax the smallest and largest value of the result that is not NaN (NaN if there is none).  A host array or memmap gives
    a host array, a device tensor a device tensor; `out` may be `data`."""
    lo, hi = np.float32(minval), np.float32(maxval)
    if np.isnan(lo) or np.isnan(hi):
        raise ValueError("minval and maxval must be numbers")
    if min(data.shape, default=0) < 1:
        raise ValueError("empty cube")
    data, (out,), suffix, a = _cube_io(data, (out,), "clip_cube")
    if ctx is None:
        ctx = Context(0)
    vmin, vmax = C.c_float(), C.c_float()
    ctx._check(getattr(ctx._lib, "wass_clip_cube" + suffix)(ctx._h, *a, float(lo), float(hi), *_ptr_strides(out), C.byref(vmin), C.byref(vmax)))
    return out, np.float32(vmin.value), np.float32(vmax.value)


def zeromean(data, out=None, ctx: Context | None = None):
    """wasspost zeromean as a function: float32(double(data) - mean), the mean of every cell over time an fp64 sum in frame order
    divided by the number of frames.  A cell that is NaN in any frame is NaN in all.  A host array or memmap gives a host
    array, a device tensor a device tensor; `out` may be `data`."""
    if min(data.shape, default=0) < 1:
        raise ValueError("empty cube")
    data, (out,), suffix, a = _cube_io(data, (out,), "zeromean")
    if ctx is None:
        ctx = Context(0)
    ctx._check(getattr(ctx._lib, "wass_zeromean" + suffix)(ctx._h, *a, *_ptr_strides(out)))
    if suffix:
        ctx.synchronize()
    return out


# ---- wave-by-wave statistics of the cube: zero crossings, H1/3, moments (beyond the reference; DESIGN.md has the definitions) ----
WAVE_FIELDS = ("mean", "m2", "m3", "m4", "eta_max", "eta_min", "h_mean", "h_sqmean", "h_max", "t_hmax", "t_z", "h_13", "t_13")
_CROSSINGS = {"up": 0, "down": 1}


def _wave_args(count, H, W, dt, datascale, crossing, hist_bins, hist_width, slab_rows):
    if crossing not in _CROSSINGS:
        raise ValueError("crossing must be 'up' or 'down'")
    count, H, W, hist_bins, slab_rows = int(count), int(H), int(W), int(hist_bins), int(slab_rows)
    dt, datascale, hist_width = float(dt), float(datascale), float(hist_width)
    if count < 1 or H < 1 or W < 1:
        raise ValueError("empty cube")
    if not (dt > 0 and np.isfinite(dt)):
        raise ValueError("dt must be positive and finite")
    if not np.isfinite(datascale):
        raise ValueError("datascale must be finite")
    if hist_bins < 0 or (hist_bins > 0 and not hist_width > 0):
        raise ValueError("hist_bins > 0 needs hist_width > 0")
    if slab_rows < 0:
        raise ValueError("slab_rows must not be negative")
    return count, H, W, dt, datascale, _CROSSINGS[crossing], hist_bins, hist_width, slab_rows


def _wave_strides(st, sy, count, H, W):
    """the stride of an axis of length 1 is never used, and numpy and torch may report anything for it (0 for a new axis)"""
    sy = W if H == 1 else int(sy)
    return (H * sy if count == 1 else int(st)), sy


def wave_statistics_scratch_bytes(count: int, H: int, W: int, dt: float = 1.0, datascale: float = 1.0, crossing: str = "up",
                                  hist_bins: int = 0, hist_width: float = 0.0, slab_rows: int = 0, host: bool = True):
    """(bytes of device scratch, rows per slab) of one wave_statistics call; no GPU needed.  Per slab of `rows` rows:
    2 * (count // 2) * rows * W * 8 bytes for the waves and, for a host cube, count * rows * W * 4 for the cube, 13 * rows * W * 8
    and rows * W * 4 for the results and hist_bins * 8, each part rounded up to 256 bytes."""
    count, H, W, dt, datascale, cr, hist_bins, hist_width, slab_rows = _wave_args(count, H, W, dt, datascale, crossing, hist_bins, hist_width, slab_rows)
    return _scratch_bytes("wavestats", (count, H, W, dt, datascale, cr, hist_bins, hist_width, slab_rows, int(bool(host))), f"{count}, {H}, {W}")


@dataclass
class WaveStatistics:
    """What wave_statistics returns: H x W maps, numpy arrays for a host cube and tensors for a device cube.  The floating maps
    are float64 and NaN where the cell's series holds a sample that is not finite; the wave maps are NaN where the cell has no wave."""
    mean: object            # time mean of the cell, times datascale
    m2: object              # mean of eta^2 (the variance with demean=True), eta^3, eta^4
    m3: object
    m4: object
    eta_max: object
    eta_min: object
    h_mean: object          # mean of the wave heights H_k, and of H_k^2
    h_sqmean: object
    h_max: object           # the highest wave and the period of the first wave that high
    t_hmax: object
    t_z: object             # mean zero-crossing period: first crossing to last, over the number of waves
    h_13: object            # mean height and period of the highest third of the waves
    t_13: object
    n_cross: object         # int32: zero crossings of the kind asked for; -1 in an invalid cell
    n_waves: object         # int32: max(n_cross - 1, 0); -1 in an invalid cell
    sigma: object           # sqrt(m2)
    hs_m0: object           # 4 sigma
    skewness: object        # m3 / (m2 sigma)
    kurtosis: object        # m4 / m2^2
    h_rms: object           # sqrt(h_sqmean)
    hist: np.ndarray | None = None      # uint64 [hist_bins]: the heights of all waves of all valid cells, bins of hist_width, the last open
    hist_width: float = 0.0
    dt: float = 0.0
    crossing: str = "up"

    def _host(self, name) -> np.ndarray:
        v = getattr(self, name)
        return v.cpu().numpy() if _is_device(v) else np.asarray(v)

    def summary(self) -> dict:
        """Scalars over the valid cells, NaN-aware: their number, the number of waves, the medians of h_13, t_13, t_z and hs_m0,
        the largest h_max and eta_max and their cells (row, column; None if there is none)."""
        n_cross = self._host("n_cross")
        valid = n_cross >= 0
        out = {"valid_cells": int(valid.sum()), "n_waves": int(self._host("n_waves")[valid].sum())}
        for name in ("h_13", "t_13", "t_z", "hs_m0"):
            v = self._host(name)
            v = v[np.isfinite(v)]
            out["median_" + name] = float(np.median(v)) if v.size else float("nan")
        for name in ("h_max", "eta_max"):
            v = self._host(name)
            if np.isnan(v).all():
                out[name], out[name + "_cell"] = float("nan"), None
            else:
                at = int(np.nanargmax(v))
                out[name], out[name + "_cell"] = float(v.flat[at]), (at // v.shape[1], at % v.shape[1])
        return out


def wave_statistics(data, dt: float, datascale: float = 1.0, crossing: str = "up", demean: bool = True, hist_bins: int = 0,
                    hist_width: float = 0.0, ctx: Context | None = None, slab_rows: int = 0) -> WaveStatistics:
    """The time-domain half of the wave product, for every cell of a count x H x W float32 cube: the individual waves between the
    zero up-crossings (crossing="down": down-crossings) of eta = (z - time mean) * datascale (demean=False: z * datascale), their
    heights H_k (crest minus trough) and periods T_k (crossings linearly interpolated, times dt), and from them the significant
    height h_13 and its period t_13 (the means over the highest third, (Nw + 2) // 3 waves), h_max and its period, the mean
    zero-crossing period t_z, h_mean and h_rms; and the surface moments: sigma, hs_m0 = 4 sigma, skewness, kurtosis, eta_max,
    eta_min.  Pass datascale=1e-3 for GridSequenceResult.Z (millimetres) to get metres.  `data` is a host array or memmap (numpy
    maps come back) or a device tensor (tensors come back); strided views whose last axis is contiguous are taken as they are.
    All arithmetic is fp64 in a fixed order ("Wave-by-wave statistics"): the result is the same bits on every run and
    does not depend on slab_rows, which caps the rows worked on at a time.  sigma, hs_m0, skewness, kurtosis and h_rms are
    computed with numpy from the device's maps.  hist_bins > 0 also pools the heights of all waves into hist_bins bins of
    hist_width (the last one open).  A cell with a NaN or an infinity in any frame is invalid: NaN maps, n_cross = n_waves = -1."""
    if len(data.shape) != 3:
        raise ValueError("data must be count x H x W")
    count, H, W, dt, datascale, cr, hist_bins, hist_width, slab_rows = _wave_args(*data.shape, dt, datascale, crossing, hist_bins, hist_width, slab_rows)
    if ctx is None:
        ctx = Context(0)
    nf = len(WAVE_FIELDS)
    hist = np.zeros(hist_bins, np.uint64) if hist_bins else None
    args = (count, H, W, dt, datascale, cr, int(bool(demean)), hist_bins, hist_width, slab_rows)
    data, _, dev, a = _cube_io(data, (), "wave_statistics")
    if dev:
        import torch
        d_fields = torch.empty((nf, H, W), dtype=torch.float64, device=data.device)
        d_ncross = torch.empty((H, W), dtype=torch.int32, device=data.device)
        d_hist = torch.empty(hist_bins, dtype=torch.int64, device=data.device) if hist_bins else None    # the call zeroes it
        ctx._check(ctx._lib.wass_wavestats_dev(ctx._h, a[0], *_wave_strides(a[1], a[2], count, H, W), *args,
                                               d_fields.data_ptr(), d_ncross.data_ptr(), d_hist.data_ptr() if hist_bins else None))
        fields, n_cross = d_fields.cpu().numpy(), d_ncross.cpu().numpy()
        if hist_bins:
            hist = d_hist.cpu().numpy().view(np.uint64)
    else:
        fields, n_cross = np.empty((nf, H, W), np.float64), np.empty((H, W), np.int32)
        ctx._check(ctx._lib.wass_wavestats(ctx._h, a[0], *_wave_strides(a[1], a[2], count, H, W), *args,
                                           fields.ctypes.data, n_cross.ctypes.data, hist.ctypes.data if hist_bins else None))
    m2, m3, m4, h_sqmean = (fields[WAVE_FIELDS.index(n)] for n in ("m2", "m3", "m4", "h_sqmean"))
    with np.errstate(invalid="ignore", divide="ignore"):
        sigma = np.sqrt(m2)
        derived = {"n_waves": np.where(n_cross < 0, n_cross, np.maximum(n_cross - 1, 0)).astype(np.int32), "sigma": sigma, "hs_m0": 4.0 * sigma,
                   "skewness": m3 / (m2 * sigma), "kurtosis": m4 / (m2 * m2), "h_rms": np.sqrt(h_sqmean)}
    if dev:
        maps = {n: d_fields[k] for k, n in enumerate(WAVE_FIELDS)}
        maps["n_cross"] = d_ncross
        maps.update({n: torch.from_numpy(np.ascontiguousarray(v)).to(data.device) for n, v in derived.items()})
    else:
        maps = {n: fields[k] for k, n in enumerate(WAVE_FIELDS)}
        maps["n_cross"] = n_cross
        maps.update(derived)
    return WaveStatistics(hist=hist, hist_width=hist_width, dt=dt, crossing=crossing, **maps)


# ---- spectral products of S(f, ky, kx): directional spectra and the surface current (beyond the reference; DESIGN.md, "Spectral
# products", has the definitions).  Everything that needs atan2, sqrt or tanh is evaluated here in numpy fp64; the device gets label
# maps and sums (specprod.hip).
_TWO_PI = 2.0 * np.pi
CURRENT_SUMS = ("Axx", "Axy", "Ayy", "bx", "by", "sw", "sr2")


def dft_axes(nt: int, ny: int, nx: int, du: float, dt: float):
    """(kx, ky, f): the exact bins of np.fft.fftn after np.fft.fftshift, as angular wavenumbers 2 pi m / (n du) and frequencies
    m / (nt dt), m = -(n // 2) .. .  The reference's wavenumber axes (spectrum3d_plan) are spaced 2 pi / (du (n - 1)) instead; the
    functions below take either."""
    def ax(n, d):
        return (np.arange(n) - n // 2) * (1.0 / (n * d))            # np.fft.fftfreq's rounding
    return _TWO_PI * ax(int(nx), du), _TWO_PI * ax(int(ny), du), ax(int(nt), dt)


def _spacing(a) -> float:
    return float((a[-1] - a[0]) / (len(a) - 1)) if len(a) > 1 else 1.0


def _spec_axes(shape, kx, ky, f):
    """the axes as float64, checked against the cube; the positive half as (p0, nf)"""
    if len(shape) != 3:
        raise ValueError("S must be nt x ny x nx")
    nt, ny, nx = (int(v) for v in shape)
    kx, ky, f = (np.ascontiguousarray(a, np.float64) for a in (kx, ky, f))
    if kx.shape != (nx,) or ky.shape != (ny,) or f.shape != (nt,):
        raise ValueError(f"axes of {len(f)}, {len(ky)}, {len(kx)} bins for a spectrum of shape {(nt, ny, nx)}")
    for a in (kx, ky, f):
        if not np.isfinite(a).all() or (len(a) > 1 and not (np.diff(a) > 0).all()):
            raise ValueError("every axis must be finite and ascending")
    P = np.flatnonzero(f > 0.5 * _spacing(f))            # not f > 0: np.arange may leave the reference's zero bin a rounding error above zero
    if not len(P):
        raise ValueError("no frequency above zero")
    return kx, ky, f, int(P[0]), len(P)


def spectral_label_maps(kx, ky, ndir: int, dk: float | None = None, k_min: float = 0.0, k_max: float = np.inf):
    """(L_dir, L_k, nk, kmod) for wavenumber axes kx, ky: int32 ny x nx maps, -1 = unused.  The propagation vector of cell (i, j) is
    kappa = (-kx[j], -ky[i]) (numpy's forward transform puts cos(k0 . r - w0 t) at (+f0, -k0)); theta = atan2(kappa_y, kappa_x) mod
    2 pi, counter-clockwise from +x of the grid.  L_dir = floor(theta / dtheta + 0.5) mod ndir: bins centred on b * dtheta.
    L_k = floor(kmod / dk + 0.5) with dk = max(dkx, dky) by default; rings from nk = floor(min(max|kx|, max|ky|) / dk) + 1 on (the
    corners) are unused, as are kmod == 0 and everything outside [k_min, k_max]."""
    ndir = int(ndir)
    if ndir < 1:
        raise ValueError("ndir must be at least 1")
    kx, ky = np.asarray(kx, np.float64), np.asarray(ky, np.float64)
    dk = max(_spacing(kx), _spacing(ky)) if dk is None else float(dk)
    if not (dk > 0 and np.isfinite(dk)) or not k_min >= 0 or not k_max >= k_min:
        raise ValueError("dk must be positive and 0 <= k_min <= k_max")
    KX, KY = np.meshgrid(-kx, -ky)
    kmod = np.sqrt(KX * KX + KY * KY)
    theta = np.mod(np.arctan2(KY, KX), _TWO_PI)
    used = (kmod != 0) & (kmod >= k_min) & (kmod <= k_max)
    L_dir = np.where(used, np.mod(np.floor(theta / (_TWO_PI / ndir) + 0.5), ndir), -1).astype(np.int32)
    ring = np.floor(kmod / dk + 0.5)
    nk = int(np.floor(min(np.abs(kx).max(), np.abs(ky).max()) / dk)) + 1
    L_k = np.where(used & (ring < nk), ring, -1).astype(np.int32)
    return L_dir, L_k, nk, kmod


def spectrum_products_scratch_bytes(nt: int, ny: int, nx: int, nf: int | None = None, ndir: int = 72, nk: int | None = None, slab: int = 0,
                                    host: bool = True):
    """(bytes of device scratch, frequencies per slab) of one spectrum_products call; no GPU needed.  nf: the frequencies above zero
    (default (nt - 1) // 2, the DFT's); nk: the rings (default min(ny, nx) // 2 + 1).  The label maps, their cell lists, the two
    tables, E2 and the peak's partials, and for a host S a slab of `slab` frequencies (0: as many as fit 16 GiB), each part rounded
    up to 256 bytes."""
    nt, ny, nx = int(nt), int(ny), int(nx)
    nf = (nt - 1) // 2 if nf is None else int(nf)
    nk = min(ny, nx) // 2 + 1 if nk is None else int(nk)
    return _scratch_bytes("specprod", (nt, ny, nx, nt - nf, int(ndir), nk, int(slab), int(bool(host))), f"{nt}, {ny}, {nx}, nf {nf}")


def _check_spec(ctx, rc):
    """the library's refusal of a bin that is negative or not finite is a ValueError, like the host's argument checks"""
    from . import _lib
    if rc == _lib.WASS_ERR_INVALID_ARG:
        raise ValueError(ctx._lib.wass_last_error(ctx._h).decode())
    ctx._check(rc)


def _device_spectrum(S, ctx):
    """S as a dense float64 device tensor: a host array is uploaded once, a device tensor is taken as it is"""
    import torch
    if _is_device(S):
        if S.dtype != torch.float64 or not S.is_contiguous():
            S = S.to(torch.float64).contiguous()
        torch.cuda.current_stream(S.device).synchronize()
        return S
    S = np.ascontiguousarray(S, np.float64)
    S = torch.from_numpy(S if S.flags.writeable else S.copy()).to(torch.device("cuda", ctx.device_id))
    torch.cuda.current_stream(S.device).synchronize()
    return S


@dataclass
class SpectralProducts:
    """What spectrum_products returns: numpy fp64.  With dkx, dky, df the spacings of the axes, dtheta = 2 pi / ndir and the factor 2
    for the half of the spectrum that is left out (S is even under (f, k) -> (-f, -k))."""
    freq: np.ndarray                # f[P], the frequencies above zero
    theta: np.ndarray               # b * dtheta, the centres of the direction bins (towards, counter-clockwise from +x of the grid)
    k: np.ndarray                   # b * dk, the centres of the wavenumber rings
    D: np.ndarray                   # [nf][ndir] frequency-direction spectrum: 2 T_dir dkx dky / dtheta
    S_f: np.ndarray                 # [nf] frequency spectrum: 2 dkx dky sum_b T_dir
    F_fk: np.ndarray                # [nf][nk] frequency-wavenumber spectrum: 2 T_k dkx dky / dk
    S_k: np.ndarray                 # [nk] wavenumber spectrum: sum_p F_fk df
    E_k2: np.ndarray                # [ny][nx] 2-D wavenumber spectrum: 2 E2 df, on the axes given (propagation is towards -k)
    mean_direction: np.ndarray      # [nf] atan2(b1, a1)
    spread: np.ndarray              # [nf] sqrt(2 (1 - hypot(a1, b1)))
    m0: float                       # sum_p S_f df
    peak_value: float               # the largest bin of the positive half over the used cells, and where it is
    peak_index: tuple               # (p, i, j) into S, or None
    T_dir: np.ndarray               # the device's sums
    T_k: np.ndarray
    E2: np.ndarray
    kx: np.ndarray
    ky: np.ndarray
    f: np.ndarray
    dk: float

    def summary(self) -> dict:
        """m0, Hm0 = 4 sqrt(m0), the peak frequency (of S_f), the peak direction (the bin of the largest D), the energy-weighted
        mean direction atan2(sum D sin, sum D cos) mod 2 pi, and the peak bin as (f, kappa_x, kappa_y)."""
        pf, pd = np.unravel_index(int(np.argmax(self.D)), self.D.shape)
        c, s = float((self.D * np.cos(self.theta)).sum()), float((self.D * np.sin(self.theta)).sum())
        out = {"m0": self.m0, "Hm0": float(4.0 * np.sqrt(self.m0)), "peak_frequency": float(self.freq[int(np.argmax(self.S_f))]),
               "peak_direction": float(self.theta[pd]), "mean_direction": float(np.mod(np.arctan2(s, c), _TWO_PI)), "peak": None}
        if self.peak_index is not None:
            p, i, j = self.peak_index
            out["peak"] = (float(self.f[p]), float(-self.kx[j]), float(-self.ky[i]))
        return out


def _derive_products(T_dir, T_k, E2, dkx, dky, df, dk, dtheta):
    nf, ndir = T_dir.shape
    D = 2.0 * T_dir * dkx * dky / dtheta
    srow = np.zeros(nf)
    for b in range(ndir):                                # sequential in b: the stated order
        srow = srow + T_dir[:, b]
    S_f = 2.0 * dkx * dky * srow
    F_fk = 2.0 * T_k * dkx * dky / dk
    S_k = np.zeros(T_k.shape[1])
    for p in range(nf):
        S_k = S_k + F_fk[p] * df
    theta = np.arange(ndir) * dtheta
    c, s = np.cos(theta), np.sin(theta)
    sa, sb, sd = np.zeros(nf), np.zeros(nf), np.zeros(nf)
    for b in range(ndir):
        sa, sb, sd = sa + D[:, b] * c[b], sb + D[:, b] * s[b], sd + D[:, b]
    with np.errstate(invalid="ignore", divide="ignore"):
        a1, b1 = sa / sd, sb / sd
        mean_direction = np.arctan2(b1, a1)
        spread = np.sqrt(2.0 * (1.0 - np.hypot(a1, b1)))
    m0 = 0.0
    for p in range(nf):
        m0 = m0 + S_f[p] * df
    return dict(theta=theta, D=D, S_f=S_f, F_fk=F_fk, S_k=S_k, E_k2=2.0 * E2 * df, mean_direction=mean_direction, spread=spread, m0=float(m0))


def spectrum_tables(S, p0: int, L_dir, ndir: int, L_k, nk: int, scale: float = 1.0, ctx: Context | None = None, slab: int = 0):
    """(T_dir [nf][ndir], T_k [nf][nk], E2 [ny][nx], peak value, peak flat index) of the frequencies p0 .. nt - 1 of S for label
    maps given as they are (int32 ny x nx, -1 = unused): what spectrum_products hands to the device after it has made the maps."""
    if len(S.shape) != 3:
        raise ValueError("S must be nt x ny x nx")
    nt, ny, nx = (int(v) for v in S.shape)
    p0, ndir, nk = int(p0), int(ndir), int(nk)
    L_dir, L_k = np.ascontiguousarray(L_dir, np.int32), np.ascontiguousarray(L_k, np.int32)
    if L_dir.shape != (ny, nx) or L_k.shape != (ny, nx) or not 0 <= p0 < nt or ndir < 1 or nk < 1:
        raise ValueError("label maps of ny x nx, 0 <= p0 < nt and at least one label of each kind are needed")
    if ctx is None:
        ctx = Context(0)
    nf = nt - p0
    T_dir, T_k, E2 = np.empty((nf, ndir)), np.empty((nf, nk)), np.empty((ny, nx))
    pv, pi = C.c_double(), C.c_int64()
    outs = (T_dir.ctypes.data, T_k.ctypes.data, E2.ctypes.data, C.byref(pv), C.byref(pi))
    if _is_device(S):
        d_S = _device_spectrum(S, ctx)
        _check_spec(ctx, ctx._lib.wass_specprod_tables_dev(ctx._h, d_S.data_ptr(), nt, ny, nx, p0, float(scale), L_dir.ctypes.data, ndir,
                                                           L_k.ctypes.data, nk, *outs))
    else:
        S = np.ascontiguousarray(S, np.float64)
        _check_spec(ctx, ctx._lib.wass_specprod_tables(ctx._h, S.ctypes.data, nt, ny, nx, p0, float(scale), L_dir.ctypes.data, ndir,
                                                       L_k.ctypes.data, nk, int(slab), *outs))
    return T_dir, T_k, E2, pv.value, int(pi.value)


def spectrum_products(S, kx, ky, f, ndir: int = 72, dk: float | None = None, k_min: float = 0.0, k_max: float = np.inf, scale: float = 1.0,
                      ctx: Context | None = None, slab: int = 0) -> SpectralProducts:
    """The spectral half of the wave product: the frequency-direction spectrum, mean direction and spread, the frequency-wavenumber
    and wavenumber spectra and the peak of S(f, ky, kx), an nt x ny x nx float64 spectrum with ascending uniform axes f, ky, kx
    (compute_3D_spectrum[_dev]'s, or dft_axes').  S is a host array (staged in slabs of at most `slab` frequencies; 0: as many as fit
    16 GiB) or a device tensor (read in place: nothing of S is downloaded).  Only the frequencies above half a bin, f > df / 2, are read (the
    reference's zero bin is a rounding error above zero); a bin there that is negative or not finite is a ValueError.  The sums run on the GPU in fp64 in a fixed order ("Spectral
    products"): the same bits on every run, for host and device input and for every slab.
    scale multiplies S on the way in.  compute_3D_spectrum leaves sum S dkx dky df at the variance of the (window-corrected) surface
    divided by nt * ny * nx of the window, so scale = nt * ny * nx makes m0 that variance (less the bins at f = 0, at the Nyquist
    frequency and at k = 0, which are left out) and Hm0 the significant wave height in the units of the data."""
    nt, ny, nx = (int(v) for v in S.shape) if len(S.shape) == 3 else (0, 0, 0)
    kx, ky, f, p0, nf = _spec_axes(S.shape, kx, ky, f)
    scale = float(scale)
    if not (scale > 0 and np.isfinite(scale)):
        raise ValueError("scale must be positive and finite")
    L_dir, L_k, nk, _ = spectral_label_maps(kx, ky, ndir, dk, k_min, k_max)
    ndir = int(ndir)
    dkx, dky, df = _spacing(kx), _spacing(ky), _spacing(f)
    dk = max(dkx, dky) if dk is None else float(dk)
    T_dir, T_k, E2, pv, pi = spectrum_tables(S, p0, L_dir, ndir, L_k, nk, scale, ctx, slab)
    at = None if pi < 0 else (pi // (ny * nx), pi % (ny * nx) // nx, pi % nx)
    return SpectralProducts(freq=f[p0:], k=np.arange(nk) * dk, peak_value=pv, peak_index=at, T_dir=T_dir, T_k=T_k, E2=E2, kx=kx, ky=ky, f=f,
                            dk=dk, **_derive_products(T_dir, T_k, E2, dkx, dky, df, dk, _TWO_PI / ndir))


def spectrum_peak(S, labels, pa: int, pb: int, p0: int, scale: float = 1.0, ctx: Context | None = None):
    """(value, flat index (p ny + i) nx + j): the largest S * scale over the frequencies pa <= p < pb and the cells with labels >= 0, the
    lowest index among equals; (NaN, -1) without a used bin.  p0 is the first frequency above zero: all bins from there on are
    checked, and one that is negative or not finite is a ValueError."""
    if ctx is None:
        ctx = Context(0)
    d_S = _device_spectrum(S, ctx)
    nt, ny, nx = (int(v) for v in d_S.shape)
    labels = np.ascontiguousarray(labels, np.int32)
    if labels.shape != (ny, nx):
        raise ValueError("labels must be ny x nx")
    pv, pi = C.c_double(), C.c_int64()
    _check_spec(ctx, ctx._lib.wass_specprod_peak_dev(ctx._h, d_S.data_ptr(), nt, ny, nx, int(p0), int(pa), int(pb), float(scale), labels.ctypes.data,
                                                     C.byref(pv), C.byref(pi)))
    return pv.value, int(pi.value)


def current_sums(S, omega, kappa_x, kappa_y, sigma0, labels, U: float, V: float, threshold_value: float, gate_value: float = np.inf,
                 pa: int = 0, pb: int | None = None, scale: float = 1.0, ctx: Context | None = None):
    """(sums, n): the weighted normal equations of the current fit over the bins (p, i, j) with labels[i][j] >= 0, pa <= p < pb,
    w = S * scale >= threshold_value and |r| <= gate_value, r = d - (kappa_x[j] U + kappa_y[i] V), d = omega[p] - sigma0[i][j]:
    sums = {Axx: sum (w kx) kx, Axy: sum (w kx) ky, Ayy: sum (w ky) ky, bx: sum (w kx) d, by: sum (w ky) d, sw: sum w,
    sr2: sum (w r) r}, n the bins taken.  Every map is taken as given, so a probe can use values that are exact in binary.  S is a
    device tensor, or a host array that is uploaded whole."""
    if ctx is None:
        ctx = Context(0)
    d_S = _device_spectrum(S, ctx)
    nt, ny, nx = (int(v) for v in d_S.shape)
    pb = nt if pb is None else int(pb)
    omega, kappa_x, kappa_y, sigma0 = (np.ascontiguousarray(a, np.float64) for a in (omega, kappa_x, kappa_y, sigma0))
    labels = np.ascontiguousarray(labels, np.int32)
    if omega.shape != (nt,) or kappa_x.shape != (nx,) or kappa_y.shape != (ny,) or sigma0.shape != (ny, nx) or labels.shape != (ny, nx):
        raise ValueError("omega[nt], kappa_x[nx], kappa_y[ny], sigma0[ny][nx] and labels[ny][nx] are needed")
    sums, n = np.empty(len(CURRENT_SUMS)), C.c_int64()
    _check_spec(ctx, ctx._lib.wass_specprod_current_sums_dev(ctx._h, d_S.data_ptr(), nt, ny, nx, int(pa), pb, float(scale), labels.ctypes.data,
                                                             omega.ctypes.data, kappa_x.ctypes.data, kappa_y.ctypes.data, sigma0.ctypes.data,
                                                             float(U), float(V), float(threshold_value), float(gate_value), sums.ctypes.data,
                                                             C.byref(n)))
    return dict(zip(CURRENT_SUMS, (float(v) for v in sums))), int(n.value)


def solve_current(s: dict, n: int):
    """(U, V, singular) of [Axx Axy; Axy Ayy] (U, V) = (bx, by) by Cramer's rule: det = Axx Ayy - Axy Axy, U = (bx Ayy - by Axy) / det,
    V = (Axx by - Axy bx) / det.  Fewer than two bins or a determinant that is not positive: NaN and singular."""
    det = s["Axx"] * s["Ayy"] - s["Axy"] * s["Axy"]
    if n < 2 or not det > 0:
        return float("nan"), float("nan"), True
    return (s["bx"] * s["Ayy"] - s["by"] * s["Axy"]) / det, (s["Axx"] * s["by"] - s["Axy"] * s["bx"]) / det, False


@dataclass
class CurrentFit:
    """What dispersion_current returns.  (U, V) is the current along +x and +y of the grid, in the units of 2 pi f / k."""
    U: float
    V: float
    speed: float            # hypot(U, V)
    direction: float        # atan2(V, U) mod 2 pi: where the current goes, counter-clockwise from +x
    n_bins: int             # the bins of the last round
    rms: float              # sqrt(sr2 / sw) of the last round: the weighted residual, at the current that round started from
    singular: bool
    trace: list             # one dict per round: round, U, V, n_bins, singular and the seven sums


def dispersion_current(S, kx, ky, f, depth: float = np.inf, g: float = 9.81, threshold: float = 0.1, f_min: float = 0.0, f_max: float = np.inf,
                       k_min: float = 0.0, k_max: float = np.inf, iterations: int = 3, gate: float = 2.0, scale: float = 1.0,
                       ctx: Context | None = None) -> CurrentFit:
    """The surface current that Doppler-shifts the dispersion shell of S(f, ky, kx): the weighted least-squares fit of
    omega = sigma0(k) + kappa . (U, V) over the bins at or above threshold * (the largest bin), sigma0 = sqrt(g k tanh(k depth)),
    weights S.  Round 0 takes all those bins with U = V = 0; each of the `iterations` rounds after it takes those with
    |omega - sigma0 - kappa . (U, V)| <= gate * domega at the current of the round before and solves again.  A round that is
    singular (fewer than two bins, or all kappa on one line) ends the fit with NaN.  The used cells are those with k_min <= |k| <=
    k_max and k != 0, the used frequencies those above half a bin with f_min <= f <= f_max.  S: a device tensor (read in place) or a host
    array (uploaded once).  The sums run on the GPU in a fixed order; the 2 x 2 solve is Cramer's rule on the host."""
    kx, ky, f, p0, nf = _spec_axes(S.shape, kx, ky, f)
    if not (g > 0 and depth > 0 and threshold >= 0 and gate >= 0 and iterations >= 0):
        raise ValueError("g, depth > 0 and threshold, gate, iterations >= 0 are needed")
    if ctx is None:
        ctx = Context(0)
    labels, _, _, kmod = spectral_label_maps(kx, ky, 1, None, k_min, k_max)
    sigma0 = np.sqrt(g * kmod) if np.isinf(depth) else np.sqrt(g * kmod * np.tanh(kmod * depth))
    omega, domega = _TWO_PI * f, _TWO_PI * _spacing(f)
    Pu = p0 + np.flatnonzero((f[p0:] >= f_min) & (f[p0:] <= f_max))
    pa, pb = (int(Pu[0]), int(Pu[-1]) + 1) if len(Pu) else (p0, p0)
    d_S = _device_spectrum(S, ctx)
    smax, _ = spectrum_peak(d_S, labels, pa, pb, p0, scale, ctx)
    thr = threshold * smax
    U = V = 0.0
    trace, singular = [], bool(np.isnan(smax))
    sums, n = dict.fromkeys(CURRENT_SUMS, 0.0), 0
    for m in range(int(iterations) + 1):
        if singular:
            break
        sums, n = current_sums(d_S, omega, -kx, -ky, sigma0, labels, U, V, thr, gate * domega if m else np.inf, pa, pb, scale, ctx)
        U, V, singular = solve_current(sums, n)
        trace.append({"round": m, "U": U, "V": V, "n_bins": n, "singular": singular, **sums})
    if singular:
        U = V = float("nan")
    with np.errstate(invalid="ignore", divide="ignore"):
        rms = float(np.sqrt(np.float64(sums["sr2"]) / np.float64(sums["sw"])))
    return CurrentFit(U=U, V=V, speed=float(np.hypot(U, V)), direction=float(np.mod(np.arctan2(V, U), _TWO_PI)), n_bins=n, rms=rms,
                      singular=bool(singular), trace=trace)


# ---- the wavenumber-frequency filter of the cube: a 3-D Fourier mask and its inverse (beyond the reference; DESIGN.md, "Dispersion
# filter", is the specification).  As above, sqrt, tanh and atan2 are evaluated here; the device gets maps and compares.
KFILTER_SCRATCH_CAP = 16 << 30
_KF_RESTORE_MEAN, _KF_KEEP_NAN, _KF_NO_CENTRE = 1, 2, 4


def fourier_filter_scratch_bytes(nt: int, ny: int, nx: int) -> int:
    """Bytes of device scratch a Fourier3DFilter of nt x ny x nx holds, for host and device input alike; no GPU needed.  Above
    KFILTER_SCRATCH_CAP the filter cannot be made (MemoryError)."""
    from . import _lib
    return _lib.scratch_bytes("kfilter", (int(nt), int(ny), int(nx)), f"a cube of {nt} x {ny} x {nx}: every axis must be 1 .. 8192")


@dataclass
class KFilterStats:
    """What a filter run measured.  var_in and var_out are the mean squares of the prepared (centred, NaN at 0) cube and of the
    filtered field before the mean is put back, over the samples that were not NaN; kept = var_out / var_in."""
    var_in: float
    var_out: float
    kept: float
    n_pass: int | None          # bins of the full cube with H = 1 (set_shell), None for an explicit mask
    n_nan: int
    n_empty_cells: int


def check_even_mask(H, nx: int):
    """ValueError unless H [nt][ny][nx // 2 + 1] is finite and even on the columns that stand alone: H[f, ky, kx] == H[-f, -ky, kx]
    for kx = 0 and, nx even, kx = nx // 2."""
    if not np.isfinite(H).all():
        raise ValueError("the mask must be finite")
    for kx in {0, nx // 2} if nx % 2 == 0 else {0}:
        col = H[:, :, kx]
        mirror = np.roll(col[::-1, ::-1], (1, 1), (0, 1))             # [f][ky] -> [-f][-ky]
        if not np.array_equal(col, mirror):
            raise ValueError(f"the mask is not even: H[f, ky, {kx}] != H[-f, -ky, {kx}] somewhere")


class Fourier3DFilter(_Handle):
    """wass_kfilter: out = real(ifftn(fftn(p) * H)) over nt x ny x nx cubes, p the cube minus every cell's time mean with NaN at 0.
    Set H with set_mask or set_shell, then apply as often as needed; .stats holds the KFilterStats of the last apply."""

    def __init__(self, nt: int, ny: int, nx: int, ctx: Context | None = None):
        from . import _lib
        self.nt, self.ny, self.nx = int(nt), int(ny), int(nx)
        self.ch = self.nx // 2 + 1
        if fourier_filter_scratch_bytes(self.nt, self.ny, self.nx) > KFILTER_SCRATCH_CAP:
            raise MemoryError(f"a {self.nt} x {self.ny} x {self.nx} cube needs more than {KFILTER_SCRATCH_CAP} bytes of scratch")
        self.ctx = Context(0) if ctx is None else ctx
        h = C.c_void_p()
        rc = self.ctx._lib.wass_kfilter_create(self.ctx._h, self.nt, self.ny, self.nx, C.byref(h))
        if rc == _lib.WASS_ERR_NO_MEMORY:
            raise MemoryError(self.ctx._lib.wass_last_error(self.ctx._h).decode())
        self.ctx._check(rc)
        self._h = h
        self.stats, self.n_pass = None, None

    def _destroy(self, h):
        self.ctx._lib.wass_kfilter_destroy(h)

    def set_mask(self, H):
        """H: real, [nt][ny][nx // 2 + 1] in the un-shifted order of np.fft.rfftn, taken as float32; it must be even (check_even_mask)."""
        H = np.ascontiguousarray(H, np.float32)
        if H.shape != (self.nt, self.ny, self.ch):
            raise ValueError(f"a mask of shape {H.shape}, expected {(self.nt, self.ny, self.ch)}")
        check_even_mask(H, self.nx)
        self.ctx._check(self.ctx._lib.wass_kfilter_set_mask(self._h, H.ctypes.data))
        self.n_pass = None

    def set_shell(self, omega, kappa_x, kappa_y, sigma0, used, U: float = 0.0, V: float = 0.0, G: float = 0.0, f_lo: float = -np.inf,
                  f_hi: float = np.inf, complement: bool = False) -> int:
        """The shell mask from maps on the fftshifted axes, all taken as given (a probe can use numbers that are exact in binary):
        omega[nt], kappa_x[nx], kappa_y[ny], sigma0[ny][nx] float64, used[ny][nx] uint8.  f_lo and f_hi bound omega, in its units.
        Returns the number of bins of the full cube that pass."""
        omega, kappa_x, kappa_y, sigma0 = (np.ascontiguousarray(a, np.float64) for a in (omega, kappa_x, kappa_y, sigma0))
        used = np.ascontiguousarray(used, np.uint8)
        if omega.shape != (self.nt,) or kappa_x.shape != (self.nx,) or kappa_y.shape != (self.ny,) or sigma0.shape != (self.ny, self.nx) \
                or used.shape != (self.ny, self.nx):
            raise ValueError("omega[nt], kappa_x[nx], kappa_y[ny], sigma0[ny][nx] and used[ny][nx] are needed")
        if not (np.isfinite(U) and np.isfinite(V) and G >= 0):
            raise ValueError("U and V must be finite and G >= 0")
        n = C.c_uint64()
        _check_spec(self.ctx, self.ctx._lib.wass_kfilter_set_shell(self._h, omega.ctypes.data, kappa_x.ctypes.data, kappa_y.ctypes.data,
                                                                   sigma0.ctypes.data, used.ctypes.data, float(U), float(V), float(G), float(f_lo),
                                                                   float(f_hi), int(bool(complement)), C.byref(n)))
        self.n_pass = int(n.value)
        return self.n_pass

    def mask(self) -> np.ndarray:
        """The mask in use, float32 [nt][ny][nx // 2 + 1]."""
        H = np.empty((self.nt, self.ny, self.ch), np.float32)
        _check_spec(self.ctx, self.ctx._lib.wass_kfilter_get_mask(self._h, H.ctypes.data))
        return H

    STAGES = ("prepare", "x", "y", "t", "mul", "t_inv", "y_inv", "full_close_stage", "close", "copy_out")

    def set_timing(self, on: bool = True):
        """Bracket the stages of every apply with events (and run the full closing stage beside k_dft_close, as a yardstick)."""
        self.ctx._check(self.ctx._lib.wass_kfilter_set_timing(self._h, int(bool(on))))

    def last_timings(self) -> dict:
        """{stage: milliseconds} of the last apply made with set_timing on."""
        ms = (C.c_float * 10)()
        self.ctx._check(self.ctx._lib.wass_kfilter_last_timings(self._h, C.byref(ms)))
        return dict(zip(self.STAGES, (float(v) for v in ms)))

    def apply(self, data, out=None, restore_mean: bool = True, keep_nan: bool = True, centre: bool = True):
        """The filtered cube: a host array or memmap gives a host array, a device tensor a device tensor; strided views pass as they
        are and `out` may be `data`.  An infinite sample is a ValueError.  centre=False takes every cell's mean as 0."""
        if tuple(int(v) for v in data.shape) != (self.nt, self.ny, self.nx):
            raise ValueError(f"a cube of shape {tuple(data.shape)}, expected {(self.nt, self.ny, self.nx)}")
        from . import _lib
        data, (out,), suffix, a = _cube_io(data, (out,), "Fourier3DFilter.apply")
        flags = (_KF_RESTORE_MEAN if restore_mean else 0) | (_KF_KEEP_NAN if keep_nan else 0) | (0 if centre else _KF_NO_CENTRE)
        st = _lib.KFilterStatsC()
        _check_spec(self.ctx, getattr(self.ctx._lib, "wass_kfilter_apply" + suffix)(self._h, *a[:3], *_ptr_strides(out), flags, C.byref(st)))
        if suffix:
            self.ctx.synchronize()
        with np.errstate(invalid="ignore", divide="ignore"):
            kept = float(np.float64(st.var_out) / np.float64(st.var_in))
        self.stats = KFilterStats(float(st.var_in), float(st.var_out), kept, self.n_pass, int(st.n_nan), int(st.n_empty_cells))
        return out


def dispersion_mask_maps(nt: int, ny: int, nx: int, du: float, dt: float, depth: float = np.inf, g: float = 9.81, k_min: float = 0.0,
                         k_max: float = np.inf, sector=None) -> dict:
    """The host maps of the shell mask on the fftshifted axes of dft_axes(nt, ny, nx, du, dt), with dispersion_current's quantities:
    f, omega = 2 pi f, domega = 2 pi df, kappa_x = -kx, kappa_y = -ky, kmod, theta (spectral_label_maps'), sigma0 = sqrt(g kmod
    tanh(kmod depth)) or sqrt(g kmod), and used (uint8 ny x nx): kmod != 0, k_min <= kmod <= k_max and, with sector = (direction,
    half_width) in radians, the direction of travel theta within half_width of direction (the difference folded into [-pi, pi])."""
    if not (du > 0 and dt > 0 and g > 0 and depth > 0):
        raise ValueError("du, dt, g and depth must be positive")
    kx, ky, f = dft_axes(nt, ny, nx, du, dt)
    labels, _, _, kmod = spectral_label_maps(kx, ky, 1, 1.0, k_min, k_max)
    KX, KY = np.meshgrid(-kx, -ky)
    theta = np.mod(np.arctan2(KY, KX), _TWO_PI)
    used = labels >= 0
    if sector is not None:
        direction, half_width = (float(v) for v in sector)
        if not (np.isfinite(direction) and half_width >= 0):
            raise ValueError("sector = (direction, half_width >= 0) in radians")
        used &= np.abs(np.mod(theta - direction + np.pi, _TWO_PI) - np.pi) <= half_width
    sigma0 = np.sqrt(g * kmod) if np.isinf(depth) else np.sqrt(g * kmod * np.tanh(kmod * depth))
    df = 1.0 / (int(nt) * dt)
    return {"f": f, "df": df, "omega": _TWO_PI * f, "domega": _TWO_PI * df, "kappa_x": -kx, "kappa_y": -ky, "kmod": kmod, "theta": theta,
            "sigma0": sigma0, "used": used.astype(np.uint8)}


def shell_band(maps: dict, f_min: float = 0.0, f_max: float = np.inf):
    """(f_lo, f_hi) for set_shell: the omega of the first and last frequency above half a bin with f_min <= f <= f_max, so that the
    device's comparison of omega decides exactly what a comparison of f decides; (inf, -inf) for a band without a bin."""
    f = maps["f"]
    P = np.flatnonzero((f > 0.5 * maps["df"]) & (f >= f_min) & (f <= f_max))
    return (float(maps["omega"][P[0]]), float(maps["omega"][P[-1]])) if len(P) else (np.inf, -np.inf)


def fourier_filter_3d(data, H, restore_mean: bool = True, keep_nan: bool = True, ctx: Context | None = None, out=None):
    """real(ifftn(fftn(p) * H)) of a count x H x W float32 cube for an explicit real, even mask H [count][H][W // 2 + 1] in
    np.fft.rfftn's order; p, the undoing, inputs and outputs as Fourier3DFilter.apply has them."""
    if len(data.shape) != 3 or min(data.shape) < 1:
        raise ValueError("data must be a count x H x W cube")
    with Fourier3DFilter(*data.shape, ctx=ctx) as filt:
        filt.set_mask(H)
        return filt.apply(data, out=out, restore_mean=restore_mean, keep_nan=keep_nan)


def dispersion_filter(data, du: float, dt: float, depth: float = np.inf, current=(0.0, 0.0), width: float = 2.0, f_min: float = 0.0,
                      f_max: float = np.inf, k_min: float = 0.0, k_max: float = np.inf, sector=None, complement: bool = False, g: float = 9.81,
                      restore_mean: bool = True, keep_nan: bool = True, ctx: Context | None = None, out=None):
    """(cube, KFilterStats): the cube with everything removed that lies more than `width` frequency bins off the dispersion shell
    omega = sigma0(k) + kappa . (U, V), or outside the band f_min .. f_max, k_min .. k_max and the sector (direction, half_width) of
    directions of travel (radians, counter-clockwise from +x).  current is (U, V) or the CurrentFit of dispersion_current; a singular
    fit is a ValueError.  complement=True returns what the filter removes instead.  keep_nan=False fills the NaN samples with the
    filtered field (all-NaN cells stay NaN).  Inputs and outputs as Fourier3DFilter.apply has them."""
    if len(data.shape) != 3 or min(data.shape) < 1:
        raise ValueError("data must be a count x H x W cube")
    if isinstance(current, CurrentFit):
        if current.singular or not (np.isfinite(current.U) and np.isfinite(current.V)):
            raise ValueError("the current fit is singular")
        U, V = current.U, current.V
    else:
        U, V = (float(v) for v in current)
        if not (np.isfinite(U) and np.isfinite(V)):
            raise ValueError("the current must be finite")
    if not width >= 0:
        raise ValueError("width must be >= 0")
    nt, ny, nx = (int(v) for v in data.shape)
    maps = dispersion_mask_maps(nt, ny, nx, du, dt, depth, g, k_min, k_max, sector)
    with Fourier3DFilter(nt, ny, nx, ctx=ctx) as filt:
        filt.set_shell(maps["omega"], maps["kappa_x"], maps["kappa_y"], maps["sigma0"], maps["used"], U, V, width * maps["domega"],
                       *shell_band(maps, f_min, f_max), complement)
        res = filt.apply(data, out=out, restore_mean=restore_mean, keep_nan=keep_nan)
        return res, filt.stats
