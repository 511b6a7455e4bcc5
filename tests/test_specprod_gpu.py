"""Spectral products on the GPU: every table, sum and fit bit for bit against the numpy oracle (tests/specprod_oracle.py).  The
exactness rests on fp64 add and multiply alone, each rounded on its own, in the fold order the oracle restates; atan2, sqrt and tanh
run in numpy on both sides."""
import functools

import numpy as np
import pytest

import specprod_oracle as O
import specprod_probes as SP
from wass_amd import postproc as P

pytestmark = pytest.mark.gpu

FIELDS = ("freq", "D", "S_f", "F_fk", "S_k", "E_k2", "mean_direction", "spread", "T_dir", "T_k", "E2")


def assert_products(got, ref, where=""):
    for name in FIELDS:
        g = getattr(got, name)
        assert g.dtype == np.float64 and g.shape == ref[name].shape, (name, where)
        if not np.array_equal(g, ref[name], equal_nan=True):
            bad = np.argwhere(~((g == ref[name]) | (np.isnan(g) & np.isnan(ref[name]))))
            pytest.fail(f"{where}: {name} differs in {len(bad)} places, first at {tuple(bad[0])}: {g[tuple(bad[0])]!r} for {ref[name][tuple(bad[0])]!r}")
    assert got.m0 == ref["m0"], where
    ny, nx = ref["E2"].shape
    flat = -1 if got.peak_index is None else (got.peak_index[0] * ny + got.peak_index[1]) * nx + got.peak_index[2]
    assert flat == ref["peak_index"] and (got.peak_value == ref["peak_value"] or (flat < 0 and np.isnan(got.peak_value))), where


@functools.lru_cache(maxsize=None)
def _cube(ny, nx):
    S = SP.random_spectrum(max(SP.NTS), ny, nx, seed=ny * 1000 + nx, span=3)
    S.setflags(write=False)
    return S


@pytest.mark.parametrize("ny, nx", SP.GRIDS)
def test_shapes(gpu_ctx, ny, nx):
    """every nt of the table with two direction counts each, so that every count meets every parity of nt over the grids"""
    for a, nt in enumerate(SP.NTS):
        # the middle frequencies of the widest cube: any nt x ny x nx block of positive doubles will do
        S = np.ascontiguousarray(_cube(ny, nx)[:nt])
        kx, ky, f = SP.axes_for(nt, ny, nx)
        for ndir in (SP.NDIRS[(a + SP.GRIDS.index((ny, nx))) % len(SP.NDIRS)], SP.NDIRS[(a + 3 + ny) % len(SP.NDIRS)]):
            assert_products(P.spectrum_products(S, kx, ky, f, ndir=ndir, ctx=gpu_ctx), O.products(S, kx, ky, f, ndir=ndir), f"{nt} x {ny} x {nx}, {ndir}")


def test_every_direction_count(gpu_ctx):
    S = np.ascontiguousarray(_cube(63, 65)[:6])
    kx, ky, f = SP.axes_for(6, 63, 65)
    for ndir in SP.NDIRS:
        assert_products(P.spectrum_products(S, kx, ky, f, ndir=ndir, ctx=gpu_ctx), O.products(S, kx, ky, f, ndir=ndir), f"ndir {ndir}")
    kw = dict(ndir=36, dk=1.7 * O.spacing(kx), k_min=2.0, k_max=5.5, scale=3.0)
    assert_products(P.spectrum_products(S, kx, ky, f, ctx=gpu_ctx, **kw), O.products(S, kx, ky, f, **kw), "k band, dk and scale")


def _direct_maps(ny, nx):
    cells = ny * nx
    raster = np.arange(cells, dtype=np.int32).reshape(ny, nx)
    last = np.full((ny, nx), -1, np.int32)
    last[:, :] = 0
    last[-1, -1] = 1                                        # label 1's only cell is the last of the map
    return {"one": (np.zeros((ny, nx), np.int32), 1), "none": (np.full((ny, nx), -1, np.int32), 3), "each": (raster, cells),
            "reverse": (raster[::-1, ::-1].copy(), cells), "last": (last, 2), "thirds": ((raster % 3 - 1).astype(np.int32), 2)}


@pytest.mark.parametrize("ny, nx", SP.DIRECT_GRIDS)
def test_label_maps_given_directly(gpu_ctx, ny, nx):
    nt, p0 = 5, 2
    maps = _direct_maps(ny, nx)
    for S in (SP.random_spectrum(nt, ny, nx, seed=31, span=3), SP.integer_spectrum(nt, ny, nx, seed=32)):
        Pz = np.arange(p0, nt)
        # one label per cell costs the oracle a loop over the cells: on the small maps only
        pairs = (("one", "each"), ("none", "reverse"), ("last", "thirds"), ("thirds", "one")) if ny * nx <= 1024 else (("one", "thirds"), ("last", "none"))
        for a, b in pairs:
            (La, na), (Lb, nb) = maps[a], maps[b]
            T_a, T_b, E2, pv, pi = P.spectrum_tables(S, p0, La, na, Lb, nb, ctx=gpu_ctx)
            assert np.array_equal(T_a, O.label_sums(S, Pz, La, na)), (a, ny, nx)
            assert np.array_equal(T_b, O.label_sums(S, Pz, Lb, nb)), (b, ny, nx)
            assert np.array_equal(E2, O.e2_sum(S, Pz))
            rv, ri = O.peak(S, Pz, La)
            assert pi == ri and (pv == rv or (ri < 0 and np.isnan(pv))), (a, ny, nx)
    S = SP.integer_spectrum(nt, ny, nx, seed=32)
    assert np.array_equal(P.spectrum_tables(S, p0, *maps["one"], *maps["none"], ctx=gpu_ctx)[0][:, 0], S[p0:].sum((1, 2)))


@pytest.mark.parametrize("name", sorted(SP.product_probes()))
def test_product_probe(gpu_ctx, name):
    S, kx, ky, f, kw = SP.product_probes()[name]
    assert_products(P.spectrum_products(S, kx, ky, f, ctx=gpu_ctx, **kw), O.products(S, kx, ky, f, **kw), name)


def test_refusals(gpu_ctx):
    import torch
    nt, ny, nx = 6, 9, 11
    kx, ky, f = SP.axes_for(nt, ny, nx)
    clean = SP.random_spectrum(nt, ny, nx, seed=41, span=3)
    ref = O.products(clean, kx, ky, f, ndir=8)
    for bad in (np.nan, np.inf, -1.0, -np.inf):
        S = clean.copy()
        S[4, 4, 5] = bad                                    # k = 0, an unused cell of the positive half: refused all the same
        for inp in (S, torch.from_numpy(S).cuda()):
            with pytest.raises(ValueError):
                P.spectrum_products(inp, kx, ky, f, ndir=8, ctx=gpu_ctx)
            with pytest.raises(ValueError):
                P.dispersion_current(inp, kx, ky, f, ctx=gpu_ctx)
        S = clean.copy()
        S[:4, 2, 3] = bad                                   # the negative half, f = 0 and the Nyquist bin are never read
        assert_products(P.spectrum_products(S, kx, ky, f, ndir=8, ctx=gpu_ctx), ref, f"{bad} in the other half")
    with pytest.raises(ValueError):
        P.spectrum_tables(clean, 4, np.full((ny, nx), 2, np.int32), 2, np.zeros((ny, nx), np.int32), 1, ctx=gpu_ctx)


def test_host_device_slabs_and_repeats(gpu_ctx):
    import torch
    nt, ny, nx = 34, 63, 65
    S = np.ascontiguousarray(_cube(ny, nx)[:nt])
    kx, ky, f = SP.axes_for(nt, ny, nx)
    ref = O.products(S, kx, ky, f, ndir=36)
    d_S = torch.from_numpy(S.copy()).cuda()
    for inp, kw in ((S, {}), (d_S, {}), (S, dict(slab=1)), (S, dict(slab=5)), (S, dict(slab=16)), (d_S, {})):
        assert_products(P.spectrum_products(inp, kx, ky, f, ndir=36, ctx=gpu_ctx, **kw), ref, f"{type(inp).__name__} {kw}")
    assert np.array_equal(d_S.cpu().numpy(), S)            # read in place and left alone


def test_finish_dev_is_finish(gpu_ctx):
    from spectrum_oracle import make_cube
    seg = make_cube(12, 21, 23, seed=3)
    out = []
    for dev in (False, True):
        with P.Spectrum3D(gpu_ctx, 4, 21, 23) as sp:
            for s in (0, 4, 8):
                sp.push(seg[s:s + 4], 1e-3)
            S, n, flag = (sp.finish_dev if dev else sp.finish)(0.37)
            assert n == 3 and not flag
            out.append(S.cpu().numpy() if dev else S)
            if dev:
                sp.push(seg[:4], 1e-3)                      # the handle has started over
                again = sp.finish_dev(1.0, out=S)[0]
                assert again is S
    assert out[0].dtype == out[1].dtype == np.float64 and np.array_equal(out[0], out[1]) and out[0].max() > 0


# ---- the current sums ----------------------------------------------------------------------------------------------------------------
def _oracle_sums(kw):
    kw = dict(kw)
    S = kw.pop("S")
    return O.current_sums(S, kw.pop("pa", 0), S.shape[0], kw["labels"], kw["omega"], kw["kappa_x"], kw["kappa_y"], kw["sigma0"], kw["U"], kw["V"],
                          kw["threshold_value"], kw["gate_value"])


@pytest.mark.parametrize("name", sorted(SP.current_probes()))
def test_current_probe(gpu_ctx, name):
    kw = SP.current_probes()[name]
    got, ref = P.current_sums(ctx=gpu_ctx, **kw), _oracle_sums(kw)
    assert got == ref, name
    assert P.current_sums(ctx=gpu_ctx, **kw) == got          # the same bits again


def test_peak_ties_and_ranges(gpu_ctx):
    S = np.full((6, 5, 7), 0.5)
    labels = np.zeros((5, 7), np.int32)
    labels[0, :3] = -1
    assert P.spectrum_peak(S, labels, 3, 6, 3, ctx=gpu_ctx) == O.peak(S, np.arange(3, 6), labels) == (0.5, 3 * 35 + 3)
    assert P.spectrum_peak(S, labels, 4, 5, 3, ctx=gpu_ctx) == O.peak(S, np.arange(4, 5), labels) == (0.5, 4 * 35 + 3)
    S2 = SP.integer_spectrum(6, 300, 300, seed=51)
    S2[5, 299, 299] = S2[4, 100, 17] = S2[4, 250, 3] = 7777.0
    lab2 = np.zeros((300, 300), np.int32)
    assert P.spectrum_peak(S2, lab2, 3, 6, 3, ctx=gpu_ctx) == O.peak(S2, np.arange(3, 6), lab2) == (7777.0, (4 * 300 + 100) * 300 + 17)
    lab2[100, 17] = -1
    assert P.spectrum_peak(S2, lab2, 3, 6, 3, ctx=gpu_ctx)[1] == (4 * 300 + 250) * 300 + 3
    v, i = P.spectrum_peak(S, np.full((5, 7), -1, np.int32), 3, 6, 3, ctx=gpu_ctx)
    assert np.isnan(v) and i == -1


def assert_fit(got, ref, where=""):
    for name in ("U", "V", "speed", "direction", "rms"):
        assert np.array_equal(getattr(got, name), ref[name], equal_nan=True), (name, where)
    assert got.n_bins == ref["n_bins"] and got.singular == ref["singular"] and len(got.trace) == len(ref["trace"]), where
    for a, b in zip(got.trace, ref["trace"]):
        assert a.keys() == b.keys() and all(np.array_equal(a[k], b[k], equal_nan=True) for k in a), (a, b, where)


def test_singular_fits(gpu_ctx):
    kx, ky, f = SP.axes_for(6, 5, 5)
    S = np.zeros((6, 5, 5))
    fit = P.dispersion_current(S + 1.0, kx, ky, f, threshold=2.0, ctx=gpu_ctx)      # nothing reaches twice the peak
    assert fit.singular and np.isnan(fit.U) and fit.n_bins == 0 and len(fit.trace) == 1
    S[5, 1, 3] = 1.0
    assert_fit(P.dispersion_current(S, kx, ky, f, ctx=gpu_ctx), O.dispersion_current(S, kx, ky, f), "one bin")
    S[4, 1, 3] = S[5, 0, 4] = 1.0                           # kappa = (-1, 1) and (-2, 2): on one line
    fit = P.dispersion_current(S, kx, ky, f, ctx=gpu_ctx)
    assert_fit(fit, O.dispersion_current(S, kx, ky, f), "collinear")
    assert fit.singular and fit.n_bins == 3


# ---- every product of one mid-size spectrum, and the chain from the cube ------------------------------------------------------------------
def test_mid_size(gpu_ctx):
    import torch
    nt, ny, nx = 20, 129, 131
    shell, kx, ky, f = SP.shell_spectrum(nt, ny, nx, 1.5, 0.5, 0.35, 0.2)
    S = shell * (1.0 + SP.random_spectrum(nt, ny, nx, seed=61, span=2)) + 1e-3 * SP.random_spectrum(nt, ny, nx, seed=62, span=3)
    d_S = torch.from_numpy(S).cuda()
    ref = O.products(S, kx, ky, f, ndir=72)
    for inp in (d_S, S):
        got = P.spectrum_products(inp, kx, ky, f, ndir=72, ctx=gpu_ctx)
        assert_products(got, ref, "20 x 129 x 131")
    s = got.summary()
    assert s["m0"] == ref["m0"] and s["Hm0"] == 4 * np.sqrt(ref["m0"]) and s["peak"][0] == f[ref["peak_index"] // (ny * nx)]
    for kw in (dict(), dict(depth=7.0, threshold=0.02, f_min=0.2, f_max=0.8, k_min=0.1, k_max=1.5, iterations=2, gate=1.5, scale=2.0)):
        fit = P.dispersion_current(d_S, kx, ky, f, ctx=gpu_ctx, **kw)
        assert_fit(fit, O.dispersion_current(S, kx, ky, f, **kw), str(kw))
        assert not fit.singular and fit.n_bins > 1000
    print("fit", fit.U, fit.V, "bins", [t["n_bins"] for t in fit.trace])


def test_end_to_end(gpu_ctx):
    """cube -> compute_3D_spectrum_dev -> products and current, against the oracle fed the downloaded S.  The reference's crop needs
    120 rows, so the cube is 60 x 120 x 120: six frames a segment, two frequencies above zero."""
    du, dt, U0, V0 = 2.0, 1.0, 0.3, -0.2
    cube = SP.advected_cube(60, 120, 120, du, dt, U0, V0)
    S, kx, ky, f, had_nan = P.compute_3D_spectrum_dev(cube, du, dt, ctx=gpu_ctx)
    assert not had_nan and tuple(S.shape) == (6, 81, 81) and str(S.dtype) == "torch.float64"
    S_host = P.compute_3D_spectrum(cube, du, dt, ctx=gpu_ctx)[0]
    Sh = S.cpu().numpy()
    assert np.array_equal(Sh, S_host)                       # finish_dev gives finish's bits through the whole chain
    import torch
    S2 = P.compute_3D_spectrum_dev(torch.from_numpy(cube).cuda(), du, dt, ctx=gpu_ctx)[0]
    assert torch.equal(S, S2)                               # a device cube: push_dev
    scale = float(Sh.size)
    assert_products(P.spectrum_products(S, kx, ky, f, ndir=24, scale=scale, ctx=gpu_ctx), O.products(Sh, kx, ky, f, ndir=24, scale=scale), "end to end")
    fit, ref = P.dispersion_current(S, kx, ky, f, ctx=gpu_ctx), O.dispersion_current(Sh, kx, ky, f)
    assert_fit(fit, ref, "end to end")
    bound = SP.shell_bound(Sh, kx, ky, f, ref)
    err = np.hypot(fit.U - U0, fit.V - V0)
    print("fit", fit.U, fit.V, "error", err, "bound", bound, "bins", [t["n_bins"] for t in fit.trace])
    assert not fit.singular and err <= bound
