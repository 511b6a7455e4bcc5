"""Variational refinement, without a GPU: the calculus of tests/vref_oracle.py (whose float32 form the kernels are held to bit for
bit in tests/test_vref_gpu.py) against torch autograd of an independently written model and against central differences; its parts
against direct formulas; the probes' conditions; each probe against the mistake it is there to catch; the end-to-end scene; and
the argument checks that need no device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import test_grid_setup as TS
import vref_oracle as V
from wass_amd import _lib, gridding, refinement

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps
TIE_MARGIN = 1e-3


# ---------------------------------------------------------------------------------------------------------------- scenes
def clear_probe(ny, nx, ih, iw, Z_of, dt=np.float64, **kw):
    """the first seed whose queries all stay TIE_MARGIN away from an integer pixel and a clamp (the sampler's ties)"""
    for seed in range(200):
        S, args = V.probe(ny, nx, ih, iw, seed=seed, dt=dt, **kw)
        Z = Z_of(ny, nx)
        if V.all_inside(S, Z) and V.distance_to_ties(S, Z) > TIE_MARGIN:
            return S, args, Z
    raise AssertionError("no seed keeps the queries off the ties")


def flat(ny, nx):
    return np.full((ny, nx), 0.07)


def sloped(ny, nx):
    y, x = np.mgrid[0:ny, 0:nx]
    return 0.02 * x - 0.015 * y + 0.01


CALCULUS = {"flat": (8, 10, 40, 36, flat), "sloped": (10, 8, 36, 40, sloped), "13x9": (13, 9, 40, 36, sloped)}


def calculus_scene(name):
    """(Scene fp64, Zc): the named surface at the coarse size, so that resize(Zc) is a like surface"""
    ny, nx, ih, iw, Z_of = CALCULUS[name]
    coarse = lambda a, b: Z_of(a // 2, b // 2) * (2.0 if Z_of is sloped else 1.0)  # noqa: E731
    for seed in range(200):
        S, _ = V.probe(ny, nx, ih, iw, seed=seed, dt=np.float64)
        Zc = coarse(ny, nx)
        Z = V.resize(S, Zc)
        if V.all_inside(S, Z) and V.distance_to_ties(S, Z) > TIE_MARGIN:
            return S, Zc
    raise AssertionError("no seed keeps the queries off the ties")


# ---------------------------------------------------------------------------------------------------------------- an independent model
def torch_energy(S, Zc, alpha):
    """data + alpha * smoothness of resize(Zc), written apart from the oracle: dense resize matrices, matrix products for the
    projection, the four-pixel form of the sampler from gathers by index, torch's conv2d for the correlation.  fp64."""
    import torch
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float64))  # noqa: E731
    ny, nx = S.shape
    Wy, Wx = t(dense_resize_matrix(ny // 2, ny)), t(dense_resize_matrix(nx // 2, nx))
    Z = Wy @ Zc @ Wx.T
    pts = torch.stack([t(S.Xb).reshape(-1), t(S.Yb).reshape(-1), Z.reshape(-1)])
    cam = t(S.R) @ pts + t(S.T)[:, None]
    hom = torch.cat([cam, torch.ones((1, cam.shape[1]), dtype=torch.float64)])
    samples = []
    for P, I in zip(S.P, (S.I0, S.I1)):
        s = t(P) @ hom
        u, v = s[0] / s[2], s[1] / s[2]
        H, W = I.shape
        fx = u.detach().floor().clamp(0, W - 2).long()
        fy = v.detach().floor().clamp(0, H - 2).long()
        ax, ay = (u - fx).clamp(0, 1), (v - fy).clamp(0, 1)
        flat_I = t(I).reshape(-1)
        at = lambda yy, xx: flat_I[yy * W + xx]  # noqa: E731
        val = (1 - ax) * (1 - ay) * at(fy, fx) + ax * (1 - ay) * at(fy, fx + 1) + (1 - ax) * ay * at(fy + 1, fx) + ax * ay * at(fy + 1, fx + 1)
        samples.append(val * t(S.mask).reshape(-1))
    data = (((samples[0] - samples[1]) / 255.0) ** 2).mean()
    kernels = torch.stack([t(S.kx), t(S.ky)])[:, None]
    slopes = torch.nn.functional.conv2d(Z[None, None], kernels, padding=3)[0]
    return data + alpha * (slopes[0] ** 2 + slopes[1] ** 2).mean()


def dense_resize_matrix(n_in, n_out):
    """tf.image.resize's bilinear rule with half-pixel centres as an n_out x n_in matrix, fp64"""
    W = np.zeros((n_out, n_in))
    for d in range(n_out):
        src = (d + 0.5) * (n_in / n_out) - 0.5
        lo, hi, t = max(int(np.floor(src)), 0), min(int(np.ceil(src)), n_in - 1), src - np.floor(src)
        W[d, lo] += 1 - t
        W[d, hi] += t
    return W


@pytest.mark.parametrize("name", sorted(CALCULUS))
def test_gradient_against_autograd_and_central_differences(name):
    """Bounds.  Autograd: both sides are the same derivative in fp64, each entry a sum of at most n = 2 * 49 * 25 + 25 products
    (taps times gathered nodes) of a few operations each, so they agree within gamma_n * (sum of the absolute terms) <= 8 n eps
    times the largest entry of the data part plus that of the smoothness part.  Central differences with step h: rounding at most
    (N + 100) eps E / h (E is a sum of N squares, evaluated twice, divided by 2 h) and truncation h^2 |E'''| / 6, which is measured
    as 4/3 of the difference between the quotients at h and h / 2; h = eps^(1/3) balances the two."""
    import torch
    S, Zc = calculus_scene(name)
    alpha = 10.0
    g, gZ = V.gradient(S, Zc, alpha)
    assert g.shape == (S.shape[0] // 2, S.shape[1] // 2) and gZ.shape == S.shape and np.abs(g).max() > 0
    zc = torch.from_numpy(Zc.copy()).requires_grad_(True)
    e = torch_energy(S, zc, alpha)
    e.backward()
    assert abs(e.item() - V.energy(S, Zc, alpha)) <= (S.Xb.size + 100) * EPS * e.item()
    scale = np.abs(V.gradient(S, Zc, 0.0)[0]).max() + np.abs(g - V.gradient(S, Zc, 0.0)[0]).max()
    n = 2 * 49 * 25 + 25
    err = np.abs(g - zc.grad.numpy()).max()
    print(f"{name}: autograd max difference {err:.3g} (bound {8 * n * EPS * scale:.3g}), largest entry {np.abs(g).max():.3g}")
    assert err <= 8 * n * EPS * scale
    # the data part alone must be there too: alpha = 0
    zc0 = torch.from_numpy(Zc.copy()).requires_grad_(True)
    torch_energy(S, zc0, 0.0).backward()
    g0 = V.gradient(S, Zc, 0.0)[0]
    assert np.abs(g0).max() > 0 and np.abs(g0 - zc0.grad.numpy()).max() <= 8 * n * EPS * np.abs(g0).max()
    h = EPS ** (1.0 / 3.0)
    N, E = S.Xb.size, V.energy(S, Zc, alpha)
    rng = np.random.default_rng(3)
    cells = {(0, 0), (Zc.shape[0] - 1, Zc.shape[1] - 1), (0, Zc.shape[1] - 1)} | {(int(rng.integers(Zc.shape[0])), int(rng.integers(Zc.shape[1]))) for _ in range(6)}
    for cy, cx in sorted(cells):
        def quotient(step):
            a, b = Zc.copy(), Zc.copy()
            a[cy, cx] += step
            b[cy, cx] -= step
            return (V.energy(S, a, alpha) - V.energy(S, b, alpha)) / (2 * step)
        q1, q2 = quotient(h), quotient(h / 2)
        bound = (N + 100) * EPS * E / h + (N + 100) * EPS * E / (h / 2) + 4.0 / 3.0 * abs(q1 - q2)
        assert abs(g[cy, cx] - q2) <= bound, (name, cy, cx, g[cy, cx], q2, bound)


# ---------------------------------------------------------------------------------------------------------------- the parts
def test_sampler_against_the_four_pixel_formula():
    rng = np.random.default_rng(5)
    I = V.texture(9, 12, 1)
    u = rng.uniform(-3, 14, 4000); v = rng.uniform(-3, 11, 4000)
    val, gx, gy = V.bilinear(I, u, v, np.float64)
    fx = np.clip(np.floor(u), 0, 10).astype(int); fy = np.clip(np.floor(v), 0, 7).astype(int)
    ax, ay = np.clip(u - fx, 0, 1), np.clip(v - fy, 0, 1)
    want = (1 - ax) * (1 - ay) * I[fy, fx] + ax * (1 - ay) * I[fy, fx + 1] + (1 - ax) * ay * I[fy + 1, fx] + ax * ay * I[fy + 1, fx + 1]
    assert np.abs(val - want).max() <= 8 * EPS * 255
    # the derivative, where the query is inside: against the formula's own
    inside = (u > 0) & (u < 11) & (v > 0) & (v < 8)
    dwx = (1 - ay) * (I[fy, fx + 1] - I[fy, fx]) + ay * (I[fy + 1, fx + 1] - I[fy + 1, fx])
    dwy = (1 - ax) * (I[fy + 1, fx] - I[fy, fx]) + ax * (I[fy + 1, fx + 1] - I[fy, fx + 1])
    assert np.abs(gx - dwx)[inside].max() <= 16 * EPS * 255 and np.abs(gy - dwy)[inside].max() <= 16 * EPS * 255
    # outside along an axis the value does not depend on that coordinate
    assert (gx[(u < 0) | (u > 11)] == 0).all() and (gy[(v < 0) | (v > 8)] == 0).all() and inside.sum() > 500


@pytest.mark.parametrize("n_out", [2, 3, 5, 8, 9, 13, 64, 65, 130])
def test_resize_and_its_adjoint_against_a_dense_matrix(n_out):
    n_in = n_out // 2
    S, _ = V.probe(n_out, max(2, n_out - 3), 8, 8, dt=np.float64)
    ny, nx = S.shape
    Wy, Wx = dense_resize_matrix(ny // 2, ny), dense_resize_matrix(nx // 2, nx)
    assert np.allclose(Wy.sum(axis=1), 1) and Wy.shape == (n_out, n_in)
    rng = np.random.default_rng(n_out)
    Zc, g = rng.normal(size=(ny // 2, nx // 2)), rng.normal(size=(ny, nx))
    assert np.abs(V.resize(S, Zc) - Wy @ Zc @ Wx.T).max() <= 16 * EPS * np.abs(Zc).max()
    assert np.abs(V.resize_adjoint(S, g) - Wy.T @ g @ Wx).max() <= 64 * EPS * np.abs(g).max() * 6
    # the float32 tables hold the same indices
    for n_i, n_o in ((ny // 2, ny), (nx // 2, nx)):
        lo32, hi32, t32 = V.axis_tables(n_i, n_o, np.float32)
        lo64, hi64, t64 = V.axis_tables(n_i, n_o, np.float64)
        assert np.array_equal(lo32, lo64) and np.array_equal(hi32, hi64) and np.abs(t32 - t64).max() < 1e-5


def test_correlation_against_scipy():
    import scipy.signal
    rng = np.random.default_rng(8)
    for ny, nx in ((2, 2), (3, 5), (7, 7), (6, 8), (13, 9), (20, 17)):
        S, _ = V.probe(ny, nx, 8, 8, dt=np.float64)
        Z = rng.normal(size=(ny, nx))
        zdx, zdy = V.zgrad(S, Z)
        for got, K in ((zdx, S.kx), (zdy, S.ky)):
            want = scipy.signal.correlate2d(Z, K, mode="same", boundary="fill", fillvalue=0)
            assert np.abs(got - want).max() <= 49 * 4 * EPS * np.abs(Z).max()
        # the adjoint: <corr(Z, K), A> = <Z, corr(A, flipped K)>
        A = rng.normal(size=(ny, nx))
        lhs = (zdx * A).sum()
        rhs = (Z * V.correlate(S, A, S.kx[::-1, ::-1])).sum()
        assert abs(lhs - rhs) <= 1e-12 * max(1.0, abs(lhs))


def test_kernels_are_the_references_expression():
    import scipy.signal
    for N, sigma in ((7, 0.8), (5, 1.0), (9, 2.5)):
        x = np.expand_dims(np.array(scipy.signal.windows.gaussian(N, sigma)), axis=0).astype(np.double)
        x = x.T @ x
        dx, dy = np.gradient(x, axis=1), np.gradient(x, axis=0)
        for got in (refinement.derivative_of_gaussian_win(N, sigma), V.derivative_of_gaussian_win(N, sigma)):
            assert np.array_equal(got[0], dx) and np.array_equal(got[1], dy)
    dx, dy = refinement.derivative_of_gaussian_win(7, 0.8)
    assert np.array_equal(dx, -dx[:, ::-1]) and np.array_equal(dx, dy.T) and dx[3, 2] > 0 > dx[3, 4]
    with pytest.raises(ValueError):
        refinement.derivative_of_gaussian_win(6, 1.0)


def test_initial_downsampling_rule():
    """cv.resize's INTER_LINEAR at an exact halving is the mean of each 2 x 2 block; in general a dense fp64 form of the same rule"""
    rng = np.random.default_rng(2)
    Z = rng.normal(size=(12, 10)).astype(np.float32)
    got = refinement.downsample_linear(Z, 6, 5)
    assert got.dtype == np.float32 and np.array_equal(got, V.cv_resize_linear(Z, 6, 5))
    assert np.abs(got - Z.reshape(6, 2, 5, 2).mean(axis=(1, 3))).max() <= 4 * np.finfo(np.float32).eps * np.abs(Z).max()
    Z = rng.normal(size=(13, 9)).astype(np.float32)
    got = refinement.downsample_linear(Z, 6, 4)
    assert got.shape == (6, 4) and np.array_equal(got, V.cv_resize_linear(Z, 6, 4))

    def dense(n_in, n_out):
        W = np.zeros((n_out, n_in))
        for d in range(n_out):
            f = (d + 0.5) * (n_in / n_out) - 0.5
            s = int(np.floor(f)); f -= s
            if s < 0:
                s, f = 0, 0.0
            if s >= n_in - 1:
                s, f = n_in - 1, 0.0
            W[d, s] += 1 - f
            W[d, min(s + 1, n_in - 1)] += f
        return W
    assert np.abs(got - dense(13, 6) @ Z.astype(np.float64) @ dense(9, 4).T).max() <= 1e-5


def test_one_adam_step_by_hand():
    S, _ = V.probe(4, 4, 8, 8, dt=np.float64)
    g = np.array([[0.5, -2.0], [1e-9, 0.0]])
    Zc = np.array([[1.0, 2.0], [3.0, 4.0]])
    z1, m1, v1 = V.adam_step(S, Zc, np.zeros_like(g), np.zeros_like(g), g, 1)
    assert np.allclose(m1, 0.1 * g, rtol=1e-12) and np.allclose(v1, 0.001 * g * g, rtol=1e-12)
    # the first step of Adam moves by lr * g / (|g| + eps * sqrt(1 - b2) ...): lr_1 = lr * sqrt(0.001) / 0.1
    lr1 = 1e-3 * np.sqrt(1 - 0.999) / (1 - 0.9)
    assert np.allclose(Zc - z1, lr1 * 0.1 * g / (np.sqrt(0.001) * np.abs(g) + 1e-7), rtol=1e-12)
    assert abs((Zc - z1)[0, 0] - 1e-3) < 1e-8 and abs((Zc - z1)[0, 1] + 1e-3) < 1e-8 and (Zc - z1)[1, 1] == 0
    # second step, t = 2
    z2, m2, v2 = V.adam_step(S, z1, m1, v1, g, 2)
    assert np.allclose(m2, 0.19 * g, rtol=1e-12) and np.allclose(v2, 0.001999 * g * g, rtol=1e-12)
    lr2 = 1e-3 * np.sqrt(1 - 0.999 ** 2) / (1 - 0.9 ** 2)
    assert np.allclose(z1 - z2, lr2 * m2 / (np.sqrt(v2) + 1e-7), rtol=1e-12)
    # float32 state stays float32
    S32 = V.as_dtype(S, np.float32)
    z, m, v = V.adam_step(S32, Zc.astype(np.float32), np.zeros((2, 2), np.float32), np.zeros((2, 2), np.float32), g.astype(np.float32), 1)
    assert z.dtype == m.dtype == v.dtype == np.float32


# ---------------------------------------------------------------------------------------------------------------- probes
def test_probe_conditions():
    for name in CALCULUS:
        S, Zc = calculus_scene(name)
        Z = V.resize(S, Zc)
        assert V.distance_to_ties(S, Z) > TIE_MARGIN and V.all_inside(S, Z) and V.min_depth(S, Z) > 1.0
    S, _, Z = clear_probe(13, 9, 64, 48, lambda ny, nx: V.surface(ny, nx, 1, amp=0.1), dt=np.float32)
    assert V.distance_to_ties(S, Z) > TIE_MARGIN and V.min_depth(S, Z) > 1.0
    # the scenes whose queries are MEANT to leave the picture do, on every side, in both pictures
    S, _ = V.probe(13, 9, 5, 7, spread=1.6)
    cams, ok = V.project(S, np.zeros(S.shape, np.float32))
    for (u, v, _), I in zip(cams, (S.I0, S.I1)):
        assert u.min() < 0 and u.max() > I.shape[1] - 1 and v.min() < 0 and v.max() > I.shape[0] - 1 and ok.all()


def _changes(a, b):
    return a.shape != b.shape or not np.array_equal(a, b)


@pytest.mark.parametrize("mistake", V.MISTAKES)
def test_each_probe_changes_under_its_mistake(mistake):
    """float32, as on the device: the quantity the GPU tests compare bit for bit differs when the oracle makes the mistake"""
    S, args = V.probe(13, 9, 64, 48, seed=2, mask="checkerboard")
    bad = V.scene(mistake=mistake, **args)
    rng = np.random.default_rng(4)
    Z = V.surface(13, 9, 3).astype(np.float32)
    Zc = rng.normal(0, 0.05, S.coarse).astype(np.float32)
    if mistake == "convolution":
        assert _changes(V.zgrad(S, Z)[0], V.zgrad(bad, Z)[0]) and _changes(V.zgrad(S, Z)[1], V.zgrad(bad, Z)[1])
    elif mistake == "transposed":
        assert S.coarse == (6, 4) and bad.coarse == (4, 6)
        assert _changes(V.gradient(S, Zc, 10.0)[0], V.gradient(bad, np.zeros(bad.coarse, np.float32), 10.0)[0])
    elif mistake == "corner_aligned":
        assert _changes(V.resize(S, Zc), V.resize(bad, Zc)) and _changes(V.gradient(S, Zc, 10.0)[0], V.gradient(bad, Zc, 10.0)[0])
    elif mistake == "no_mask":
        assert _changes(V.sample(S, Z)[0], V.sample(bad, Z)[0]) and (V.sample(S, Z)[0][S.mask == 0] == 0).all()
        assert V.loss(S, Z)[0] != V.loss(bad, Z)[0]
    elif mistake == "eps_in_sqrt":
        a, b = V.optimize(S, Zc, 1), V.optimize(bad, Zc, 1)
        assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and _changes(a[0], b[0])
    elif mistake == "xy_swapped":
        assert _changes(V.sample(S, Z)[0], V.sample(bad, Z)[0]) and _changes(V.sample(S, Z)[1], V.sample(bad, Z)[1])
    else:
        raise AssertionError(mistake)


# ---------------------------------------------------------------------------------------------------------------- end to end
def e2e_setup():
    f = TS.rig_files()
    N = V.E2E["N"]
    return gridding.setup_algebra(f["K0"], f["K1"], f["R"], f["T"], f["P0cam"], f["P1cam"], TS.PLANE, TS.BASELINE, Nx=N, Ny=N, Iw=TS.IW, Ih=TS.IH,
                                  z_q02=-0.3, z_q98=0.3, **V.E2E["area"])


def test_end_to_end_on_a_synthetic_rig():
    """The rig of tests/test_grid_setup.py looks at the plane z = c0 (plane units) carrying an analytic texture; from Zinit = 0 the
    float32 oracle alone brings the masked RMS error below half of its start (vref_oracle.E2E says why alpha is small here)."""
    S, _ = V.e2e_scene(e2e_setup(), TS.IH, TS.IW)
    c0, N = V.E2E["c0"], V.E2E["N"]
    zero = np.zeros((N, N), np.float32)
    assert V.all_inside(S, zero) and V.all_inside(S, zero + np.float32(c0)) and S.mask.sum() == (N - 2 * V.E2E["margin"]) ** 2
    start = V.masked_rms(zero, c0, S.mask)
    assert abs(start - c0) < 1e-9
    d0, d1 = V.loss(S, zero)[0], V.loss(S, zero + np.float32(c0))[0]
    assert d1 < 0.02 * d0                                      # the pictures agree at the true plane
    Zc, m, v, step = V.optimize(S, refinement.downsample_linear(zero, N // 2, N // 2), V.E2E["iters"], alpha=V.E2E["alpha"])
    Z = V.resize(S, Zc) * S.mask
    end = V.masked_rms(Z, c0, S.mask)
    print(f"masked rms {start:.4f} -> {end:.4f}; data loss {d0:.3g} -> {V.loss(S, Z)[0]:.3g}")
    assert end < 0.5 * start and step == V.E2E["iters"]
    # and it went the right way, not merely somewhere
    assert Z[S.mask != 0].mean() > 0.5 * c0


# ---------------------------------------------------------------------------------------------------------------- arguments
def test_python_argument_errors_come_before_any_device_work():
    S, a = V.probe(6, 8, 8, 8, dt=np.float64)
    ok = dict(a)
    for key, val in (("XX", a["XX"][:, :-1]), ("mask", a["mask"][:-1]), ("XX", np.zeros((1, 8))), ("I0", np.zeros((1, 8))), ("I1", np.zeros(8)),
                     ("baseline", 0.0), ("baseline", np.nan), ("Rp2c", np.eye(4)), ("P0cam", np.full((3, 4), np.nan)), ("Tp2c", np.zeros(2))):
        bad = dict(ok)
        bad[key] = val
        if key == "XX" and val.shape[0] == 1:
            bad["YY"], bad["mask"] = val, val
        with pytest.raises(ValueError):
            refinement.VariationalRefinement(**bad)


def test_library_refusals_without_a_device():
    lib = _lib.load()
    n = C.c_size_t(0)
    assert lib.wass_vref_scratch_bytes(1024, 1024, 2058, 2456, 2058, 2456, C.byref(n)) == 0
    assert n.value >= 8 * 1024 * 1024 * 4 + 2 * 2058 * 2456 * 4
    for dims in ((1, 8, 8, 8, 8, 8), (8, 1, 8, 8, 8, 8), (8, 8, 1, 8, 8, 8), (8, 8, 8, 1, 8, 8), (8, 8, 8, 8, 1, 8), (8, 8, 8, 8, 8, 1), (0, 0, 0, 0, 0, 0),
                 (-4, 8, 8, 8, 8, 8), (40000, 8, 8, 8, 8, 8)):
        assert lib.wass_vref_scratch_bytes(*dims, C.byref(n)) == -1, dims
    assert lib.wass_vref_scratch_bytes(8, 8, 8, 8, 8, 8, None) == -1
    assert lib.wass_vref_scratch_bytes(2, 2, 2, 2, 2, 2, C.byref(n)) == 0 and n.value > 0
    h = C.c_void_p()
    dp = C.POINTER(C.c_double)
    zeros = (C.c_double * 12)()
    assert lib.wass_vref_create(None, 8, 8, None, None, None, C.cast(zeros, dp), C.cast(zeros, dp), C.cast(zeros, dp), C.cast(zeros, dp), None, 8, 8,
                                None, 8, 8, None, C.byref(h)) == -1 and not h.value
    st = C.c_int64(0)
    assert lib.wass_vref_sample(None, None, None, None, None) == -1 and lib.wass_vref_zgrad(None, None, None, None) == -1
    assert lib.wass_vref_loss(None, None, None, None) == -1 and lib.wass_vref_gradient(None, None, 10.0, None, None) == -1
    assert lib.wass_vref_optimize(None, None, None, None, C.byref(st), 1, 10.0, 1e-3, 1e-7, 10, None, 0, None, None) == -1
    lib.wass_vref_destroy(None)


def test_header_with_the_new_entries_is_plain_c99(tmp_path):
    src = tmp_path / "vref_abi.c"
    src.write_text('#include "wass_gpu.h"\n'
                   "int main(void) { wass_vref* h = 0; size_t n = 0; double a = 0, b = 0; int64_t step = 0; int rows = 0;\n"
                   "  int rc = wass_vref_scratch_bytes(2, 2, 2, 2, 2, 2, &n);\n"
                   "  rc += wass_vref_create(0, 2, 2, 0, 0, 0, 0, 0, 0, 0, 0, 2, 2, 0, 2, 2, 0, &h);\n"
                   "  rc += wass_vref_sample(h, 0, 0, 0, 0) + wass_vref_zgrad(h, 0, 0, 0) + wass_vref_loss(h, 0, &a, &b);\n"
                   "  rc += wass_vref_gradient(h, 0, 10.0, 0, 0);\n"
                   "  rc += wass_vref_optimize(h, 0, 0, 0, &step, 0, 10.0, 1e-3, 1e-7, 10, 0, 0, &rows, 0);\n"
                   "  wass_vref_destroy(h); return rc; }\n")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-fsyntax-only", str(src)])
