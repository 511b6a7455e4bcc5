"""Inputs of the spectral-product tests: closed-form spectra (no random-number stream), the shape table of the GPU suite with the
launch arithmetic of specprod.hip restated, and hand-built probes, each there to catch one mistake.  tests/test_specprod.py shows on
the CPU which mistake each probe catches; tests/test_specprod_gpu.py runs them on the GPU."""
import functools

import numpy as np

import specprod_oracle as O
import spectrum_oracle as SO


def random_spectrum(nt, ny, nx, seed=1, span=40):
    """positive doubles with full mantissas over 2^-span .. 2: sums of them round differently in every order"""
    idx = np.arange(nt * ny * nx, dtype=np.uint64)
    u, v, e = SO._hash01(idx, seed), SO._hash01(idx, seed + 101), SO._hash01(idx, seed + 202)
    return ((1.0 + u) * (1.0 + v * 2.0 ** -24) * 2.0 ** np.floor(-span * e)).reshape(nt, ny, nx)


def integer_spectrum(nt, ny, nx, seed=1):
    """integer-valued: every order of a sum agrees, so a wrong or a missing cell shows as a wrong integer"""
    idx = np.arange(nt * ny * nx, dtype=np.uint64)
    return np.floor(1000.0 * SO._hash01(idx, seed)).reshape(nt, ny, nx)


# ---- the shape table of the GPU suite, and the launch arithmetic it has to reach ----------------------------------------------------
NTS = (3, 4, 5, 6, 10, 34)
GRIDS = ((2, 2), (3, 5), (1, 7), (7, 1), (63, 65), (64, 64), (65, 129), (129, 257))
NDIRS = (1, 2, 3, 36, 72, 360, 40000)                       # 40000: more than there are cells
# label maps given directly, all cells one label: the list lengths around one, two and three trips of a thread of k_sp_label, and
# the cell counts around the workgroups of k_sp_cells; 300 x 300 makes 352 workgroups, more than one trip of k_sp_best / k_sp_fold
DIRECT_GRIDS = ((1, 255), (1, 256), (1, 257), (3, 171), (2, 256), (300, 300))


def label_trips(n_cells_of_label):
    """k_sp_label: thread t of 256 takes q = t, t + 256, .. below the list's length: the trips of thread 0"""
    return -(-n_cells_of_label // 256)


def cell_groups(cells):
    """k_sp_cells, k_sp_current: (workgroups, lanes of the last one that have a cell); k_sp_best and k_sp_fold take the workgroups
    t, t + 256, .."""
    return -(-cells // 256), (cells - 1) % 256 + 1


def axes_for(nt, ny, nx):
    return O.dft_axes(nt, ny, nx, 0.5, 0.25)


# ---- probes of spectrum_products: name -> (S, kx, ky, f, kwargs) -------------------------------------------------------------------
def _one_cell(nt, ny, nx, p, kap_x, kap_y, value=3.0):
    """energy in the one bin whose propagation vector is (kap_x, kap_y) bins: kappa = -k"""
    S = np.zeros((nt, ny, nx))
    S[p, ny // 2 - kap_y, nx // 2 - kap_x] = value
    return S


@functools.lru_cache(maxsize=None)
def product_probes():
    out = {}
    # nt = 4: f = (-2, -1, 0, 1) df.  Energy at f = 0 and at the Nyquist bin (index 0, on the negative side) must not be counted.
    S = integer_spectrum(4, 5, 5, seed=3) + 1.0
    S[0] *= 64.0
    S[2] *= 32.0
    out["half"] = (S, *axes_for(4, 5, 5), dict(ndir=4))
    # kappa = (1, 2) bins: theta = 63.4 degrees, bin 1 of four centred bins; bin 0 if the bins start at their edge; bin 3 for kappa = +k
    out["direction"] = (_one_cell(3, 7, 7, 2, 1, 2), *axes_for(3, 7, 7), dict(ndir=4))
    # kappa = (3, -1) bins: theta = 341.6 degrees rounds to bin 4 of four, which is bin 0
    out["wrap"] = (_one_cell(3, 7, 7, 2, 3, -1), *axes_for(3, 7, 7), dict(ndir=4))
    # kappa = (2, 2) bins on a 5 x 5 grid: ring 3, and only rings 0 .. 2 are whole
    out["corner"] = (_one_cell(3, 5, 5, 2, 2, 2), *axes_for(3, 5, 5), dict(ndir=4))
    # 900 cells in one direction bin: several trips per thread and a tree whose result a left-to-right or a pairwise sum misses
    out["fold"] = (random_spectrum(10, 30, 30, seed=5, span=3), *axes_for(10, 30, 30), dict(ndir=1))
    # every bin the same: the peak is the first of them
    out["tie"] = (np.full((5, 4, 6), 0.75), *axes_for(5, 4, 6), dict(ndir=3))
    # two equal peaks, the later one in a lower row of a later frequency
    S = integer_spectrum(6, 9, 8, seed=9)
    S[4, 7, 2] = S[5, 1, 1] = 5000.0
    out["tie2"] = (S, *axes_for(6, 9, 8), dict(ndir=5))
    for v in out.values():
        v[0].setflags(write=False)
    return out


# ---- probes of current_sums: name -> kwargs, every value exact in binary where a comparison is probed ---------------------------
def _dyadic_maps(nt, ny, nx):
    return dict(omega=0.25 * np.arange(nt), kappa_x=np.arange(nx) - 1.0, kappa_y=2.0 - np.arange(ny), sigma0=np.zeros((ny, nx)),
                labels=np.zeros((ny, nx), np.int32), U=0.0, V=0.0, threshold_value=0.0, gate_value=np.inf)


@functools.lru_cache(maxsize=None)
def current_probes():
    out = {}
    # threshold 0.5: one bin exactly at it (taken), one an ulp below (not taken), one above
    S = np.full((4, 2, 3), 0.25)
    S[1, 0, 2], S[2, 1, 0], S[3, 1, 1] = 0.5, np.nextafter(0.5, 0.0), 1.0
    out["threshold"] = dict(S=S, **{**_dyadic_maps(4, 2, 3), "threshold_value": 0.5})
    # gate 0.5: r = omega - sigma0 is exactly 0.5 at p = 2 (taken) but for the cell whose sigma0 puts it an ulp beyond
    m = _dyadic_maps(5, 2, 3)
    m["sigma0"][0, 1] = -2.0 ** -53
    out["gate"] = dict(S=np.ones((5, 2, 3)), **{**m, "gate_value": 0.5})
    # the same with a current: r = d - (kx U + ky V) with dyadic U, V
    m = _dyadic_maps(5, 2, 3)
    out["gate_current"] = dict(S=np.ones((5, 2, 3)), **{**m, "U": 0.125, "V": -0.25, "gate_value": 0.25})
    # nothing reaches the threshold; one bin does; bins on one line through the origin
    out["empty"] = dict(S=np.full((3, 2, 3), 0.25), **{**_dyadic_maps(3, 2, 3), "threshold_value": 0.5})
    S = np.full((3, 2, 3), 0.25)
    S[2, 0, 0] = 1.0
    out["one_bin"] = dict(S=S, **{**_dyadic_maps(3, 2, 3), "threshold_value": 0.5})
    m = _dyadic_maps(3, 5, 5)
    m["kappa_x"], m["kappa_y"] = np.arange(5) - 2.0, np.arange(5) - 2.0
    m["labels"] = np.where(np.eye(5) > 0, 0, -1).astype(np.int32)
    m["labels"][2, 2] = -1
    out["collinear"] = dict(S=np.ones((3, 5, 5)), **m)
    # values with full mantissas: (w kx) kx and w (kx kx) differ, and so does every other order of the sums; 352 workgroups
    for name, (nt, ny, nx) in (("full", (4, 9, 31)), ("many_groups", (3, 300, 300))):
        idx = np.arange(ny * nx, dtype=np.uint64)
        m = dict(omega=1.0 + SO._hash01(np.arange(nt, dtype=np.uint64), 11), kappa_x=SO._hash01(np.arange(nx, dtype=np.uint64), 12) - 0.5,
                 kappa_y=SO._hash01(np.arange(ny, dtype=np.uint64), 13) - 0.5, sigma0=1.0 + SO._hash01(idx, 14).reshape(ny, nx),
                 labels=np.where(SO._hash01(idx, 15) < 0.9, 0, -1).astype(np.int32).reshape(ny, nx), U=0.3, V=-0.2, threshold_value=0.25,
                 gate_value=0.75)
        out[name] = dict(S=random_spectrum(nt, ny, nx, seed=21, span=3), pa=1, **m)
    for v in out.values():
        v["S"].setflags(write=False)
    return out


# ---- a synthetic dispersion shell ---------------------------------------------------------------------------------------------
def shell_spectrum(nt, ny, nx, du, dt, U0, V0, depth=np.inf, g=9.81, outlier=False):
    """(S, kx, ky, f): for every cell with k != 0 the energy 1 / (1 + kmod) in the bin of the positive half nearest to
    (sigma0 + kappa . (U0, V0)) / 2 pi, where that lies inside the half.  outlier: one more bin, as strong as the strongest, far
    off the shell."""
    kx, ky, f = O.dft_axes(nt, ny, nx, du, dt)
    labels, _, _, kmod, _ = O.label_maps(kx, ky, 1)
    kapx, kapy = O.kappa(kx, ky)
    KX, KY = np.meshgrid(kapx, kapy)
    fs = (O.sigma0_map(kmod, depth, g) + KX * U0 + KY * V0) / O.TWO_PI
    P = O.positive_half(f)
    df = O.spacing(f)
    q = np.rint((fs - f[P[0]]) / df).astype(np.int64)
    S = np.zeros((nt, ny, nx))
    ii, jj = np.nonzero((labels >= 0) & (q >= 0) & (q < len(P)))
    S[P[0] + q[ii, jj], ii, jj] = 1.0 / (1.0 + kmod[ii, jj])
    if outlier:
        i, j = ny // 2 + 1, nx // 2 + 2
        S[P[-1], i, j] = S.max()
    return S, kx, ky, f


def advected_cube(count, H, W, du, dt, U0, V0, g=9.81):
    """count x H x W float32: plane waves with omega = sqrt(g k) + k . (U0, V0), their wavenumbers on the bins of the reference's
    crop (2 pi m / (Nx du), Nx the crop's width), a hash for noise"""
    n = (H * 2 // 3 // 2) * 2 + 1
    waves = ((3, 0, 1.0, 0.3), (0, -3, 0.8, 1.1), (2, 2, 0.9, 2.0), (-3, 1, 0.7, 4.0), (8, -7, 0.5, 0.7), (10, 3, 0.5, 5.0), (-6, -9, 0.4, 3.3))
    yy, xx = np.meshgrid(np.arange(H) * du, np.arange(W) * du, indexing="ij")
    out = np.empty((count, H, W), np.float32)
    cell = np.arange(H * W, dtype=np.uint64).reshape(H, W)
    for t in range(count):
        z = 0.02 * (SO._hash01(cell + np.uint64(t * H * W), 77) - 0.5)
        for mx, my, a, ph in waves:
            k0x, k0y = O.TWO_PI * mx / (n * du), O.TWO_PI * my / (n * du)
            w0 = np.sqrt(g * np.hypot(k0x, k0y)) + k0x * U0 + k0y * V0
            z = z + a * np.cos(k0x * xx + k0y * yy - w0 * (t * dt) + ph)
        out[t] = z
    return out


def fit_rows(S, pa, pb, labels, omega, kapx, kapy, sig0, thr):
    """the weighted rows of the fit, one per bin taken with U = V = 0 and no gate"""
    KX, KY = np.meshgrid(kapx, kapy)
    A, b, w = [], [], []
    for p in range(pa, pb):
        take = (labels >= 0) & (S[p] >= thr)
        A.append(np.stack([KX[take], KY[take]], 1))
        b.append(omega[p] - sig0[take])
        w.append(S[p][take])
    return np.concatenate(A), np.concatenate(b), np.concatenate(w)


def shell_bound(S, kx, ky, f, fit):
    """(domega / 2) ||A^-1|| sum w |kappa| from the bins the fit's round 0 took: every such bin of a synthetic shell lies within half a
    frequency bin of the shell, b - A u0 = sum w kappa (d - kappa . u0), and u - u0 = A^-1 (b - A u0)"""
    A, _, w = fit_rows(S, fit["pa"], fit["pb"], fit["labels"], 2 * np.pi * f, *O.kappa(kx, ky), fit["sigma0"], fit["threshold_value"])
    N = (A * w[:, None]).T @ A
    return np.pi * O.spacing(f) * np.linalg.norm(np.linalg.inv(N), 2) * float((w * np.hypot(A[:, 0], A[:, 1])).sum())
