"""The oracle of the dispersion filter (wass_amd.postproc: Fourier3DFilter, fourier_filter_3d, dispersion_filter; the kernels
k_kf_prepare, k_kf_shell, k_kf_mul and k_dft_close of wass_amd/csrc/spectrum.hip): an fp64 numpy restatement of DESIGN.md,
"Dispersion filter" (preparation, mask rule, product with w, inverse, undoing) that can be broken on purpose, a staged model with
the kernels' structure in float32 or fp64 (the stages of tests/dft_oracle.py), the case table, the launch arithmetic, the bounds.
Test infrastructure only: nothing here is imported by the package."""
import numpy as np

import dft_oracle as DO

U32 = 2.0 ** -24                   # unit round-off of float32
U64 = 2.0 ** -53
TWO_PI = 2.0 * np.pi

# what can be broken, one at a time: the oracle's answer to each probe of tests/kfilter_probes.py must move by 5 tolerances
VARIANTS = ("no_mirror", "kappa_sign", "w_none", "w_all", "nyquist_doubled", "no_inv", "no_mean", "no_nan", "close_drop_k", "gate_lt")

# (nt, ny, nx).  What each is there for is asserted by tests/test_kfilter.py::test_case_table_reaches from launch_plan below.
CASES = [(1, 1, 1), (2, 1, 1), (1, 2, 3), (3, 2, 2), (4, 3, 1), (5, 13, 28), (4, 16, 30), (7, 9, 33), (3, 5, 125), (2, 7, 126),
         (3, 4, 127), (2, 33, 128), (5, 6, 129), (6, 11, 64), (9, 8, 65), (8, 10, 63), (20, 129, 131)]


# ---- the launch arithmetic ------------------------------------------------------------------------------------------------------
def launch_plan(nt, ny, nx):
    """What kfilter_apply launches for a cube: the seven DFT launches (k_dft_stage's as tests/dft_oracle.py describes them, then
    k_dft_close: M = nx, N = nt ny, K = ch), the bitmap's words and the partial sums."""
    ch = nx // 2 + 1
    st = DO._stage_plan
    return {"ch": ch, "cells": ny * nx, "wpf": -(-(ny * nx) // 64), "nprep": -(-(ny * nx) // 256),
            "stages": [st("x", False, True, ch, nt * ny, nx, 1), st("y", True, False, ny, ch, ny, nt), st("t", True, False, nt, ny * ch, nt, 1),
                       st("ti", True, False, nt, ny * ch, nt, 1), st("yi", True, False, ny, ch, ny, nt),
                       st("close", True, True, nx, nt * ny, ch, 1)]}


# ---- preparation and undoing ----------------------------------------------------------------------------------------------------
def prepare(cube, centre=True):
    """(p float32, m_c float64 [ny][nx], nan bool [nt][ny][nx], empty bool [ny][nx]): the cell mean is the fp64 sum of the samples
    that are not NaN in frame order, divided by their count (0 for an empty cell, and everywhere without `centre`)."""
    v = np.asarray(cube, np.float32)
    nan = np.isnan(v)
    s = np.zeros(v.shape[1:], np.float64)
    for t in range(v.shape[0]):
        s = np.where(nan[t], s, s + np.where(nan[t], 0.0, v[t].astype(np.float64)))
    cnt = (~nan).sum(axis=0)
    with np.errstate(invalid="ignore", divide="ignore"):
        m = np.where(cnt > 0, s / cnt.astype(np.float64), 0.0)
    if not centre:
        m = np.zeros_like(m)
    with np.errstate(invalid="ignore"):
        p = np.where(nan, np.float32(0), (v.astype(np.float64) - m[None]).astype(np.float32))
    return p, m, nan, cnt == 0


def undo(y, m, nan, empty, restore_mean=True, keep_nan=True, variant=None):
    """out float32 of the filtered field y (float32 or float64: its float32 value is taken)."""
    y = np.asarray(y).astype(np.float32)
    out = (y.astype(np.float64) + m[None]).astype(np.float32) if restore_mean and variant != "no_mean" else y.copy()
    if keep_nan and variant != "no_nan":
        out[nan] = np.nan
    out[:, empty] = np.nan
    return out


# ---- the mask -------------------------------------------------------------------------------------------------------------------
def mask_maps(nt, ny, nx, du, dt, depth=np.inf, g=9.81, k_min=0.0, k_max=np.inf, sector=None, variant=None):
    """dispersion_mask_maps restated with spectral_label_maps' and dispersion_current's own expressions.  variant 'kappa_sign'
    takes kappa with the sign of k."""
    ax = lambda n, d: (np.arange(n) - n // 2) * (1.0 / (n * d))
    kx, ky, f = TWO_PI * ax(nx, du), TWO_PI * ax(ny, du), ax(nt, dt)
    sgn = 1.0 if variant == "kappa_sign" else -1.0
    KX, KY = np.meshgrid(sgn * kx, sgn * ky)
    kmod = np.sqrt(KX * KX + KY * KY)
    theta = np.mod(np.arctan2(KY, KX), TWO_PI)
    used = (kmod != 0) & (kmod >= k_min) & (kmod <= k_max)
    if sector is not None:
        used &= np.abs(np.mod(theta - sector[0] + np.pi, TWO_PI) - np.pi) <= sector[1]
    sigma0 = np.sqrt(g * kmod) if np.isinf(depth) else np.sqrt(g * kmod * np.tanh(kmod * depth))
    df = 1.0 / (nt * dt)
    return {"f": f, "df": df, "omega": TWO_PI * f, "domega": TWO_PI * df, "kappa_x": sgn * kx, "kappa_y": sgn * ky, "kmod": kmod,
            "theta": theta, "sigma0": sigma0, "used": used.astype(np.uint8)}


def band(maps, f_min=0.0, f_max=np.inf):
    f = maps["f"]
    P = np.flatnonzero((f > 0.5 * maps["df"]) & (f >= f_min) & (f <= f_max))
    return (float(maps["omega"][P[0]]), float(maps["omega"][P[-1]])) if len(P) else (np.inf, -np.inf)


def shell_mask(omega, kappa_x, kappa_y, sigma0, used, U=0.0, V=0.0, G=0.0, f_lo=-np.inf, f_hi=np.inf, complement=False, variant=None):
    """The full mask [nt][ny][nx], float32, un-shifted (np.fft.fftn's order), from maps on the fftshifted axes.  variant 'no_mirror'
    decides a bin of negative frequency at its own indices, 'gate_lt' gates with < instead of <=."""
    nt, ny, nx = len(omega), len(kappa_y), len(kappa_x)
    a, b, c = np.indices((nt, ny, nx))                               # un-shifted indices
    nyq = ((nt % 2 == 0) & (a == nt // 2)) | ((ny % 2 == 0) & (b == ny // 2)) | ((nx % 2 == 0) & (c == nx // 2))
    neg = a > nt // 2
    if variant != "no_mirror":
        a, b, c = np.where(neg, (nt - a) % nt, a), np.where(neg, (ny - b) % ny, b), np.where(neg, (nx - c) % nx, c)
    p, i, j = (a + nt // 2) % nt, (b + ny // 2) % ny, (c + nx // 2) % nx
    w = np.asarray(omega, np.float64)[p]
    d = w - np.asarray(sigma0, np.float64)[i, j]
    r = d - (np.asarray(kappa_x, np.float64)[j] * U + np.asarray(kappa_y, np.float64)[i] * V)
    gate = np.abs(r) < G if variant == "gate_lt" else np.abs(r) <= G
    ok = (np.asarray(used)[i, j] != 0) & (w >= f_lo) & (w <= f_hi) & gate
    if complement:
        ok = ~ok
    decided = (np.indices((nt, ny, nx))[0] != 0) & ~nyq
    return np.where(decided & ok, np.float32(1), np.float32(0))


def half(Hfull):
    return np.ascontiguousarray(Hfull[:, :, :Hfull.shape[2] // 2 + 1])


def full(Hhalf, nx):
    """The full mask an even half mask stands for: column kx > nx / 2 is column nx - kx read at (-f, -ky)."""
    nt, ny, ch = Hhalf.shape
    a, b, c = np.indices((nt, ny, nx))
    mir = c > nx // 2
    return Hhalf[np.where(mir, (nt - a) % nt, a), np.where(mir, (ny - b) % ny, b), np.where(mir, nx - c, c)]


def is_even(Hfull):
    return np.array_equal(Hfull, np.roll(Hfull[::-1, ::-1, ::-1], (1, 1, 1), (0, 1, 2)))


# ---- the filter -----------------------------------------------------------------------------------------------------------------
def weights(nt, ny, nx, variant=None):
    """w / (nt ny nx) per column of the half layout."""
    kx = np.arange(nx // 2 + 1)
    alone = (kx == 0) | ((nx % 2 == 0) & (kx == nx // 2))
    if variant == "w_none":
        alone = np.ones_like(alone)
    if variant == "w_all":
        alone = np.zeros_like(alone)
    if variant == "nyquist_doubled":
        alone = kx == 0
    inv = 1.0 if variant == "no_inv" else 1.0 / (float(nt) * float(ny) * float(nx))
    return np.where(alone, 1.0, 2.0) * inv


def field(p, Hhalf, variant=None):
    """y float64 = real(ifftn(fftn(p) * H)), restated the way the chain computes it: the half spectrum, conj(X) H w / N, the
    forward t and y transforms, and the closing x stage's real part, all in fp64 with numpy's FFT."""
    nt, ny, nx = p.shape
    X = np.fft.rfftn(np.asarray(p, np.float64))
    Z = np.conj(X) * (np.asarray(Hhalf, np.float64) * weights(nt, ny, nx, variant)[None, None, :])
    Z = np.fft.fft(np.fft.fft(Z, axis=0), axis=1)
    k, x = np.arange(nx // 2 + 1, dtype=np.int64)[:, None], np.arange(nx, dtype=np.int64)[None, :]
    E = np.exp(-2j * np.pi * ((k * x) % nx) / nx)
    if variant == "close_drop_k":
        E[DO.TK * ((len(k) - 1) // DO.TK):] = 0
    return np.real(Z @ E)


def staged_field(p, Hhalf, variant=None, dtype=np.float64):
    """The same with the kernels' structure: DO.dft_stage per launch (f32-rounded twiddles and f32 products for dtype float32),
    k_kf_mul's fp64 product with one rounding, and k_dft_close as the real part of the <true, true> stage."""
    nt, ny, nx = p.shape
    ch = nx // 2 + 1
    re, im = DO.dft_stage(np.asarray(p, dtype), None, 2, nx, ch, dtype)
    re, im = DO.dft_stage(re, im, 1, ny, ny, dtype)
    re, im = DO.dft_stage(re, im, 0, nt, nt, dtype)
    hw = np.asarray(Hhalf, np.float32).astype(np.float64) * weights(nt, ny, nx, variant)[None, None, :]
    re, im = (re.astype(np.float64) * hw).astype(dtype), (-(im.astype(np.float64) * hw)).astype(dtype)
    re, im = DO.dft_stage(re, im, 0, nt, nt, dtype)
    re, im = DO.dft_stage(re, im, 1, ny, ny, dtype)
    return DO.dft_stage(re, im, 2, nx, nx, dtype, "drop_k" if variant == "close_drop_k" else None)[0]


def filter_cube(cube, Hhalf, restore_mean=True, keep_nan=True, centre=True, variant=None):
    """{'out', 'y', 'p', 'var_in', 'var_out', 'n_nan', 'n_empty'}: the whole operator in fp64."""
    p, m, nan, empty = prepare(cube, centre)
    y = field(p, Hhalf, variant)
    ok = ~nan
    n = int(ok.sum())
    sq = lambda a: float((np.asarray(a, np.float64)[ok] ** 2).sum()) / n if n else float("nan")
    return {"out": undo(y, m, nan, empty, restore_mean, keep_nan, variant), "y": y, "p": p, "m": m, "nan": nan, "empty": empty,
            "var_in": sq(p), "var_out": sq(y.astype(np.float32)), "n_nan": int(nan.sum()), "n_empty": int(empty.sum())}


# ---- bounds ---------------------------------------------------------------------------------------------------------------------
def bound(p, Hhalf):
    """|y - oracle| <= 2 (nt + ny + nx + 8) 2^-24 max|H| ||p||_1 per element ("Dispersion filter", derives it)."""
    nt, ny, nx = p.shape
    return 2.0 * (nt + ny + nx + 8) * U32 * float(np.abs(Hhalf).max(initial=0.0)) * float(np.abs(np.asarray(p, np.float64)).sum())


def out_tolerance(ref_out, b, restore_mean):
    """The bound on out: that of y, and half an ulp of the result where the mean was added (the cast after the fp64 addition)."""
    return b + (U32 * np.abs(np.nan_to_num(ref_out.astype(np.float64))) if restore_mean else 0.0)


def gamma(n, u=U64):
    return n * u / (1.0 - n * u)


# tile limit = bound * sqrt(elements) / sqrt(ntiles) * TILE_MARGIN: the Frobenius norm of the element-wise bound shared out over the
# 64 x 64 tiles of DO.tile_errors, so that one wrong tile cannot hide in the budget of the others.  TILE_MARGIN is 8 x the worst
# ratio  tile error / (bound sqrt(elements) / sqrt(ntiles))  of staged_field in float32 against field in fp64, measured on the CPU
# over CASES on dense_input (tests/test_kfilter.py::test_tile_margin_is_measured repeats the measurement).  The factor 8 is the one
# tests/dft_oracle.py grants a k-ordered fma chain over numpy's blocked sums.  Measured worst ratios: 0.006715 at (2, 1, 1), 0.0039 at
# (3, 2, 2), 0.0018 at (4, 3, 1), 2e-5 and less from (5, 13, 28) on: ||p||_1 grows with the cube and the bound with it, so on the larger
# shapes this limit is loose too.  There the GPU test also holds every tile to 8 x the LARGEST tile error of the float32 staged
# model on the same input (model_tile_limit): the model's own error, not a bound on it.
TILE_MEASURED = (0.006715, (2, 1, 1))
TILE_MARGIN = 8 * TILE_MEASURED[0]


def tile_limit(b, elements, ntiles):
    return b * np.sqrt(elements) / np.sqrt(ntiles) * TILE_MARGIN


def model_tile_limit(p, Hhalf, y_ref):
    """8 x the largest 64 x 64 tile error (Frobenius) of the float32 staged model against the fp64 oracle y_ref, and no less than
    one float32 rounding of the largest |y| on every element of a tile (a model that happens to be exact leaves that much)."""
    err, _ = DO.tile_errors(staged_field(p, Hhalf, dtype=np.float32), y_ref)
    return 8.0 * max(float(err.max()), 64.0 * U32 * float(np.abs(y_ref).max(initial=0.0)))


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
def dense_input(case, seed=0):
    """(cube float32 with an offset, 1 % NaN samples and, from 4 cells on, one all-NaN cell; an even half mask of values in [0, 1])
    for a case: what the bounded GPU tests and the tile margin use."""
    nt, ny, nx = case
    rng = np.random.default_rng(1000 * nt + 10 * ny + nx + seed)
    t, y, x = np.indices(case)
    cube = (50.0 + np.cos(0.7 * x + 0.4 * y - 0.9 * t) + 0.5 * np.sin(0.3 * x - 1.1 * y + 0.5 * t) + 0.1 * rng.standard_normal(case)).astype(np.float32)
    cube[rng.random(case) < 0.01] = np.nan
    if ny * nx >= 4:
        cube[:, ny // 2, nx // 3] = np.nan
    Hf = rng.random(case).astype(np.float32)
    Hf = np.maximum(Hf, np.roll(Hf[::-1, ::-1, ::-1], (1, 1, 1), (0, 1, 2)))            # even
    return cube, half(Hf)
