"""numpy restatements of the reference's postproc/wasspost/spectra.py (compute_3D_spectrum :53-171, compute_spectrum :9-49)
for the spectrum tests, the generator of their input cubes and the error bound the GPU result is held to.  Test
infrastructure only: nothing here is imported by the package.

The 3-D restatement runs the reference's own numpy operations on the same dtypes (the float32 cube stays float32 up to the
subtraction of the mean, the window makes it float64, np.fft.fftn), so it equals the reference to the last bits; the window
is scipy.signal.windows.hann restated (general_cosine on linspace(-pi, pi)).  The 1-D restatement is an fp64 Welch estimate
with scipy.signal.csd's defaults (the reference itself runs csd on float32 data).
"""
import numpy as np


# ---- the input cubes: closed form, no random-number stream ---------------------------------------------------------------------
def _hash01(idx, seed):
    """An integer hash of uint64 indices (splitmix64's finaliser) mapped to [0, 1)."""
    with np.errstate(over="ignore"):
        h = (idx + np.uint64(seed)) * np.uint64(0x9E3779B97F4A7C15)
        h ^= h >> np.uint64(30)
        h *= np.uint64(0xBF58476D1CE4E5B9)
        h ^= h >> np.uint64(27)
        h *= np.uint64(0x94D049BB133111EB)
        h ^= h >> np.uint64(31)
    return (h >> np.uint64(40)).astype(np.float64) / float(1 << 24)


# amplitude (mm), cycles per frame, per row, per column, phase
WAVES = ((400.0, 0.083, 0.031, 0.017, 0.3), (150.0, 0.127, -0.043, 0.052, 1.1), (60.0, 0.21, 0.09, -0.075, 2.0),
         (25.0, 0.31, 0.004, 0.16, 4.0))


def make_cube(count, H, W, seed=1, noise=20.0, nan_fraction=0.0, waves=WAVES, offset=0.0):
    """count x H x W float32 millimetres: a sum of plane waves + noise * (hash - 0.5) + offset, NaN where a second hash falls below
    nan_fraction.  Frame by frame, so that a large cube needs no large temporaries."""
    out = np.empty((count, H, W), np.float32)
    yy = np.arange(H, dtype=np.float64)[:, None]
    xx = np.arange(W, dtype=np.float64)[None, :]
    cell = np.arange(H * W, dtype=np.uint64).reshape(H, W)
    sp = [a * np.exp(1j * (2 * np.pi * (cy * yy + cx * xx) + ph)) for a, ct, cy, cx, ph in waves]
    for t in range(count):
        z = np.full((H, W), float(offset))
        for (a, ct, cy, cx, ph), e in zip(waves, sp):
            z += (e * np.exp(2j * np.pi * ct * t)).real
        idx = cell + np.uint64(t) * np.uint64(H * W)
        if noise:
            z += noise * (_hash01(idx, seed) - 0.5)
        if nan_fraction:
            z[_hash01(idx, seed + 7919) < nan_fraction] = np.nan
        out[t] = z
    return out


# ---- compute_3D_spectrum -------------------------------------------------------------------------------------------------------
def hann(n, sym=True):
    if n <= 1:
        return np.ones(max(n, 0))
    m = n if sym else n + 1
    w = 0.5 + 0.5 * np.cos(np.linspace(-np.pi, np.pi, m))
    return w if sym else w[:-1]


def axes3d(count, H, W, du, dt):
    """dict: Nt, shift, r_start, c_start, Nx (the nominal crop), kx, ky, f as the reference derives them."""
    N = H * 2 // 3
    Nt = int(count / 10)
    if Nt % 2 > 0:
        Nt += 1
    mr, mc = H // 2, W // 2
    r_start, r_end = mr - N // 2 - 20, mr + N // 2 - 20 + 1
    c_start, c_end = mc - N // 2, mc + N // 2 + 1
    Nx, Ny = r_end - r_start, c_end - c_start
    kx_max = (2.0 * np.pi / du) / 2.0
    ky_max = (2.0 * np.pi / du) / 2.0
    f_max = (1.0 / dt) / 2.0
    dkx = 2.0 * np.pi / (du * np.floor(Nx / 2.0) * 2.0)
    dky = 2.0 * np.pi / (du * np.floor(Ny / 2.0) * 2.0)
    df = 1.0 / (dt * np.floor(Nt / 2.0) * 2.0)
    kx = np.arange(-kx_max, kx_max + dkx, dkx)
    ky = np.arange(-ky_max, ky_max + dky, dky)
    f = np.arange(-f_max, f_max, df)
    return {"Nt": Nt, "shift": int(Nt / 2), "r_start": r_start, "c_start": c_start, "Nx": Nx, "Ny": Ny, "kx": kx, "ky": ky, "f": f, "df": df}


def _setup3d(shape, du, dt):
    a = axes3d(shape[0], shape[1], shape[2], du, dt)
    kx, ky = a["kx"], a["ky"]
    KX, KY = np.meshgrid(kx, ky)
    a["KX"], a["KY"] = KX, KY
    a["dkx"], a["dky"] = kx[3] - kx[2], ky[3] - ky[2]
    hx, hy, ht = hann(KX.shape[0]), hann(KX.shape[1]), hann(a["Nt"])
    a["win"] = (hx[:, None] * hy)[None, :, :] * ht[:, None, None]
    a["wc"] = (1.0 / np.mean(hx ** 2)) * (1.0 / np.mean(hy ** 2)) * (1.0 / np.mean(ht ** 2))
    n3 = float(a["win"].size)
    a["K"] = a["wc"] / (n3 ** 3 * a["dkx"] * a["dky"] * a["df"])
    return a


def segments3d(data, du, dt, datascale=1.0):
    """Yields (Zcube_w, K) per Welch segment: the windowed, centred fp64 segment the reference transforms, and the factor K with
    S_segment = K * |fftn(Zcube_w)|^2 (unnormalised transform)."""
    import warnings
    a = _setup3d(data.shape, du, dt)
    Nt, win = a["Nt"], a["win"]
    r0, c0 = a["r_start"], a["c_start"]
    r1, c1 = r0 + win.shape[1], c0 + win.shape[2]
    for ii in range(20):
        z = np.array(data[ii * a["shift"]:ii * a["shift"] + Nt, r0:r1, c0:c1]) * datascale
        if z.shape[0] != Nt:
            break
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)            # "Mean of empty slice" for a cell that is NaN throughout
            z = np.where(np.isnan(z), np.nanmean(z, axis=0), z)
        yield (z - np.mean(z)) * win, a["K"]


def compute_3D_spectrum(data, du, dt, segments=8, datascale=1.0):
    a = _setup3d(data.shape, du, dt)
    S_welch = np.zeros_like(a["win"])
    n = 0
    for zw, _ in segments3d(data, du, dt, datascale):
        S = np.fft.fftshift(np.fft.fftn(zw, norm="ortho"))
        S /= (S.shape[0] * S.shape[1] * S.shape[2])
        S = np.abs(S) ** 2 / (a["dkx"] * a["dky"] * a["df"])
        S *= a["wc"]
        S_welch += S
        n += 1
    S_welch /= n
    return S_welch, a["KX"], a["KY"], a["f"]


def bound3d(data, du, dt, datascale=1.0):
    """e2 of the element-wise check |S - S_ref| <= 2 sqrt(S_ref e2) + e2, and the per-segment Parseval sums.
    Three chained length-n inner products in f32 with f32-rounded twiddles and an f32-rounded input move a coefficient by at most
    (nx + ny + nt + 6) 2^-24 ||x_w||_1; e2 is that amplitude squared, scaled like S, the largest over the segments.  With
    dX_s the error of segment s, |mean_s K (|X_s + dX_s|^2 - |X_s|^2)| <= 2 sqrt(K) max|dX| mean_s sqrt(K) |X_s| + K max|dX|^2, and
    mean_s sqrt(K) |X_s| <= sqrt(S_ref) (Cauchy-Schwarz)."""
    e2, energy = 0.0, []
    for zw, K in segments3d(data, du, dt, datascale):
        nt, ny, nx = zw.shape
        dX = (nx + ny + nt + 6) * 2.0 ** -24 * float(np.abs(zw).sum())
        e2 = max(e2, K * dX * dX)
        energy.append(float((zw * zw).sum()) * zw.size)          # Parseval: sum |X|^2 = N sum x^2
    return e2, energy


# ---- compute_spectrum ----------------------------------------------------------------------------------------------------------
def welch(x, fs, nperseg):
    """scipy.signal.csd(x, x, fs, nperseg=nperseg) in fp64: hann (periodic), overlap nperseg // 2, detrend='constant', one-sided
    density, mean over the segments; nperseg > len(x) shrinks to len(x)."""
    x = np.asarray(x, np.float64)
    nps = min(int(nperseg), x.shape[0])
    nov = nps // 2
    step = nps - nov
    nseg = (x.shape[0] - nov) // step
    w = hann(nps, sym=False)
    P = np.zeros(nps // 2 + 1)
    for s in range(nseg):
        seg = x[s * step:s * step + nps]
        X = np.fft.rfft((seg - seg.mean()) * w)
        P += (X.real ** 2 + X.imag ** 2)
    P *= 1.0 / (fs * (w * w).sum()) / nseg
    if nps % 2:
        P[1:] *= 2
    else:
        P[1:-1] *= 2
    return np.fft.rfftfreq(nps, 1.0 / fs), P


def compute_spectrum(data, dt, nperseg=512, rangespan=5, scale=1.0):
    ci, cj = data.shape[1] // 2, data.shape[2] // 2
    ts = scale * np.asarray(data[:, ci, cj], np.float64)
    ts = ts - np.mean(ts)
    f, S = welch(ts, 1.0 / dt, nperseg)
    n = 0
    for ii in range(ci - rangespan, ci + rangespan + 1):
        for jj in range(cj - rangespan, cj + rangespan + 1):
            tn = scale * np.asarray(data[:, ii, jj], np.float64)
            S = S + welch(tn - np.mean(tn), 1.0 / dt, nperseg)[1]
            n += 1
    return np.fft.rfftfreq(min(int(nperseg), data.shape[0]), dt), S / float(n + 1), ts
