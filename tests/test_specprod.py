"""Spectral products without a GPU: the numpy oracle (tests/specprod_oracle.py) checked by independent means, the argument errors
and the scratch formula of the library, the conditions every GPU input must meet, and every hand-built probe
(tests/specprod_probes.py) against the mistake it is there to catch: a deliberately broken model must differ from the
specification on it."""
import ctypes as C

import numpy as np
import pytest

import specprod_oracle as O
import specprod_probes as SP
import spectrum_oracle as SO
from wass_amd import postproc as P

EPS = np.finfo(np.float64).eps


def gamma(n):
    return n * (EPS / 2) / (1 - n * (EPS / 2))


# ---- the oracle, by independent means ------------------------------------------------------------------------------------------
def test_dft_axes_against_fftfreq():
    for nt, ny, nx in ((6, 5, 8), (7, 4, 9), (100, 684, 683)):
        for axes in (O.dft_axes(nt, ny, nx, 0.25, 0.5), P.dft_axes(nt, ny, nx, 0.25, 0.5)):
            kx, ky, f = axes
            assert np.array_equal(kx, 2 * np.pi * np.fft.fftshift(np.fft.fftfreq(nx, 0.25)))
            assert np.array_equal(ky, 2 * np.pi * np.fft.fftshift(np.fft.fftfreq(ny, 0.25)))
            assert np.array_equal(f, np.fft.fftshift(np.fft.fftfreq(nt, 0.5)))


def test_label_maps_of_the_package_are_the_oracles():
    for ny, nx, ndir, kw in ((7, 9, 8, {}), (33, 32, 72, dict(k_min=1.0, k_max=9.0)), (5, 5, 360, dict(dk=0.7)), (1, 7, 3, {}), (7, 1, 3, {})):
        kx, ky, _ = O.dft_axes(4, ny, nx, 0.5, 1.0)
        got, ref = P.spectral_label_maps(kx, ky, ndir, **kw), O.label_maps(kx, ky, ndir, **kw)
        assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]) and got[2] == ref[2]
        assert got[0].dtype == np.int32 and got[0].max() < ndir and got[1].max() < got[2]


def test_label_sums_against_bincount():
    S = SP.random_spectrum(6, 33, 35, seed=2, span=20)
    kx, ky, f = SP.axes_for(6, 33, 35)
    Pz = O.positive_half(f)
    assert list(Pz) == [4, 5]
    for ndir in (1, 5, 72):
        L_dir, L_k, nk, _, _ = O.label_maps(kx, ky, ndir)
        for L, n in ((L_dir, ndir), (L_k, nk)):
            T = O.label_sums(S, Pz, L, n)
            used = L.ravel() >= 0
            for q, p in enumerate(Pz):
                ref = np.bincount(L.ravel()[used], weights=S[p].ravel()[used], minlength=n)
                count = np.bincount(L.ravel()[used], minlength=n)
                mag = np.bincount(L.ravel()[used], weights=np.abs(S[p]).ravel()[used], minlength=n)
                assert (np.abs(T[q] - ref) <= 2 * gamma(np.maximum(count, 1)) * mag).all()
    assert np.array_equal(O.e2_sum(S, Pz), S[4] + S[5])
    assert np.abs(O.e2_sum(S, Pz) - S[Pz].sum(0)).max() <= gamma(2) * S[Pz].sum(0).max()


def _plane_wave_cube(count, H, W, mt, my, mx, nt, n):
    """cos(k0 . r - w0 t) with (w0, k0) on bin (mt, my, mx) of an nt x n x n window"""
    t = np.arange(count)[:, None, None]
    y = np.arange(H)[None, :, None]
    x = np.arange(W)[None, None, :]
    return (1000.0 * np.cos(2 * np.pi * (mx * x + my * y) / n - 2 * np.pi * mt * t / nt)).astype(np.float32)


def test_plane_wave_peak_direction_and_time_reversal():
    count, H, W, du, dt = 60, 126, 126, 0.5, 0.25
    a = SO.axes3d(count, H, W, du, dt)
    nt, n = a["Nt"], len(a["kx"])
    assert nt == 6 and n == 85
    mt, my, mx = 1, -7, 4
    kx, ky, f = O.dft_axes(nt, n, n, du, dt)
    for sign in (1, -1):
        cube = _plane_wave_cube(count, H, W, sign * mt, my, mx, nt, n)
        S = SO.compute_3D_spectrum(cube, du, dt)[0]
        r = O.products(S, kx, ky, f, ndir=72)
        p, c = divmod(r["peak_index"], n * n)
        i, j = divmod(c, n)
        # travelling along sign * k0: the peak's propagation vector is exactly the wave's bin
        assert (p, i, j) == (nt // 2 + mt, n // 2 - sign * my, n // 2 - sign * mx)
        assert (-kx[j], -ky[i]) == (sign * kx[n // 2 + mx], sign * ky[n // 2 + my])
        theta0 = np.mod(np.arctan2(sign * my, sign * mx), 2 * np.pi)
        b = int(np.floor(theta0 / (2 * np.pi / 72) + 0.5)) % 72
        pf, pd = np.unravel_index(np.argmax(r["D"]), r["D"].shape)
        assert pd == b and r["freq"][pf] == f[p]
        if sign == 1:
            first = b
        else:
            assert (b - first) % 72 == 36                   # reversing time turns the direction by pi


def test_m0_against_the_windowed_variance():
    """Parseval: the reference's normalisation leaves sum S dkx dky df = wc mean(x_w^2) / N, N = nt ny nx; m0 takes twice the
    positive half of the used cells with the spacings of the axes it is given, so m0 N less what it leaves out is that variance."""
    count, H, W, du, dt = 60, 126, 126, 0.5, 0.25
    cube = SO.make_cube(count, H, W, seed=4)
    S, KX, KY, f = SO.compute_3D_spectrum(cube, du, dt)
    a = SO._setup3d(cube.shape, du, dt)
    kx, ky = a["kx"], a["ky"]
    N = float(S.size)
    cell = a["dkx"] * a["dky"] * a["df"]
    var_w = np.mean([a["wc"] * np.mean(zw * zw) for zw, _ in SO.segments3d(cube, du, dt)])
    assert S.sum() * cell * N == pytest.approx(var_w, rel=1e-10)
    r = O.products(S, kx, ky, f, ndir=36, scale=N)
    Pz = O.positive_half(f)
    used = r["L_dir"] >= 0
    direct = 2.0 * (S[Pz][:, used].sum() * N) * O.spacing(kx) * O.spacing(ky) * O.spacing(f)
    assert r["m0"] == pytest.approx(direct, rel=1e-11)
    # the half taken is the mirror image of the half left out, but for f = 0, the Nyquist bin and k = 0
    assert list(Pz) == [4, 5] and 0 < abs(f[3]) < 1e-15      # the reference's zero bin is not exactly zero, and is left out all the same
    left_out = S[3].sum() + S[0].sum() + S[Pz][:, ~used].sum() * 2
    assert direct / (O.spacing(kx) * O.spacing(ky) * O.spacing(f)) == pytest.approx((S.sum() - left_out) * N, rel=1e-9)
    print("m0", r["m0"], "windowed variance", var_w, "Hm0", 4 * np.sqrt(r["m0"]))


def test_current_fit_against_lstsq():
    S, kx, ky, f = SP.shell_spectrum(24, 21, 23, 2.0, 0.5, 0.4, -0.25)
    S = S * (1.0 + 0.5 * SP.random_spectrum(24, 21, 23, seed=8, span=1))
    fit = O.dispersion_current(S, kx, ky, f, iterations=0, threshold=0.05)
    A, b, w = SP.fit_rows(S, fit["pa"], fit["pb"], fit["labels"], 2 * np.pi * f, *O.kappa(kx, ky), fit["sigma0"], fit["threshold_value"])
    assert len(w) == fit["n_bins"] > 50
    sw = np.sqrt(w)
    ref = np.linalg.lstsq(A * sw[:, None], b * sw, rcond=None)[0]
    cond = np.linalg.cond(A * sw[:, None]) ** 2             # of the normal equations
    tol = 64 * cond * EPS * np.linalg.norm(ref)
    print("fit", fit["U"], fit["V"], "lstsq", ref, "tolerance", tol)
    assert abs(fit["U"] - ref[0]) <= tol and abs(fit["V"] - ref[1]) <= tol


def test_current_of_a_synthetic_shell():
    U0, V0 = 0.4, -0.25
    S, kx, ky, f = SP.shell_spectrum(32, 33, 31, 2.0, 0.5, U0, V0)
    for depth, it in ((np.inf, 0), (np.inf, 3)):
        fit = O.dispersion_current(S, kx, ky, f, depth=depth, iterations=it, threshold=0.05)
        bound = SP.shell_bound(S, kx, ky, f, fit)
        err = np.hypot(fit["U"] - U0, fit["V"] - V0)
        print("iterations", it, "fit", fit["U"], fit["V"], "error", err, "bound", bound, "bins", [t["n_bins"] for t in fit["trace"]])
        assert not fit["singular"] and len(fit["trace"]) == it + 1
        assert len({t["n_bins"] for t in fit["trace"]}) == 1     # the gate of two bins drops nothing of a clean shell
        assert err <= bound
    S5, kx, ky, f = SP.shell_spectrum(32, 33, 31, 2.0, 0.5, U0, V0, depth=5.0)
    fit = O.dispersion_current(S5, kx, ky, f, depth=5.0, iterations=0, threshold=0.05)
    assert np.hypot(fit["U"] - U0, fit["V"] - V0) <= SP.shell_bound(S5, kx, ky, f, fit)
    last = fit["trace"][-1]
    assert fit["direction"] == np.mod(np.arctan2(fit["V"], fit["U"]), 2 * np.pi) and fit["rms"] == np.sqrt(last["sr2"] / last["sw"])


def test_singular_fits():
    pr = SP.current_probes()
    for name, n in (("empty", 0), ("one_bin", 1), ("collinear", 12)):
        kw = dict(pr[name])
        s, got = O.current_sums(kw.pop("S"), kw.pop("pa", 0), 3, kw["labels"], kw["omega"], kw["kappa_x"], kw["kappa_y"], kw["sigma0"], kw["U"], kw["V"],
                                kw["threshold_value"], kw["gate_value"])
        assert got == n and O.solve(s, got)[2] and P.solve_current(s, got)[2]
    s = dict(Axx=2.0, Axy=0.5, Ayy=1.0, bx=1.0, by=-1.0, sw=1.0, sr2=0.0)
    assert O.solve(s, 5) == P.solve_current(s, 5) == ((1.0 * 1.0 - -1.0 * 0.5) / 1.75, (2.0 * -1.0 - 0.5 * 1.0) / 1.75, False)


# ---- the library without a GPU ---------------------------------------------------------------------------------------------------
def test_argument_errors_and_the_scratch_formula():
    from wass_amd import _lib
    lib = _lib.load()
    b, n = C.c_size_t(), C.c_int()

    def a256(v):
        return (v + 255) // 256 * 256
    for (nt, ny, nx, p0, nd, nk, slab, host) in ((100, 684, 684, 51, 72, 343, 0, 1), (100, 684, 684, 51, 72, 343, 0, 0), (10, 65, 129, 6, 360, 33, 3, 1),
                                                  (3, 1, 7, 2, 1, 1, 0, 1)):
        assert lib.wass_specprod_scratch_bytes(nt, ny, nx, p0, nd, nk, slab, host, C.byref(b), C.byref(n)) == 0
        cells, nf = ny * nx, nt - p0
        freqs = min(nf, slab) if slab else nf
        assert n.value == freqs
        want = (a256(freqs * cells * 8) if host else 0) + 3 * a256(cells * 4) + a256((nd + 1) * 4) + a256((nk + 1) * 4) + a256(nf * nd * 8) \
            + a256(nf * nk * 8) + a256(cells * 8) + a256((cells + 255) // 256 * 16) + 256
        assert b.value == want, (nt, ny, nx)
    assert P.spectrum_products_scratch_bytes(100, 684, 684, 49, 72, 343, host=False)[0] < 20e6
    big = P.spectrum_products_scratch_bytes(8192, 8192, 8192, host=True)            # 512 MiB a frequency: slabs under the cap
    assert big[0] <= 16 << 30 and 1 <= big[1] < 4095
    for bad in ((0, 5, 5, 0, 4, 3, 0, 1), (4, 0, 5, 3, 4, 3, 0, 1), (4, 5, 5, 4, 4, 3, 0, 1), (4, 5, 5, -1, 4, 3, 0, 1), (4, 5, 5, 3, 0, 3, 0, 1),
                (4, 5, 5, 3, 4, 0, 0, 1), (4, 5, 5, 3, 4, 3, -1, 1)):
        assert lib.wass_specprod_scratch_bytes(*bad, C.byref(b), C.byref(n)) == -1, bad
    assert lib.wass_specprod_scratch_bytes(4, 5, 5, 3, 4, 3, 0, 1, None, C.byref(n)) == -1
    assert lib.wass_specprod_scratch_bytes(4, 50000, 50000, 3, 4, 3, 0, 1, C.byref(b), C.byref(n)) == -2      # a cell is indexed with 32 bits
    with pytest.raises(ValueError):
        P.spectrum_products_scratch_bytes(4, 5, 5, nf=0)


def test_python_argument_errors():
    S = np.ones((4, 5, 6))
    kx, ky, f = O.dft_axes(4, 5, 6, 1.0, 1.0)
    for call in (lambda: P.spectrum_products(S[0], kx, ky, f), lambda: P.spectrum_products(S, ky, kx, f), lambda: P.spectrum_products(S, kx[::-1], ky, f),
                 lambda: P.spectrum_products(S, kx, ky, -np.abs(f) - 1), lambda: P.spectrum_products(S, kx, ky, f, ndir=0),
                 lambda: P.spectrum_products(S, kx, ky, f, dk=0.0), lambda: P.spectrum_products(S, kx, ky, f, scale=0.0),
                 lambda: P.spectrum_products(S, kx, ky, f, k_min=2.0, k_max=1.0), lambda: P.dispersion_current(S, kx, ky, f, depth=0.0),
                 lambda: P.dispersion_current(S, kx, ky, f, iterations=-1), lambda: P.spectrum_tables(S, 4, np.zeros((5, 6)), 1, np.zeros((5, 6)), 1)):
        with pytest.raises(ValueError):
            call()


# ---- what every GPU input must meet, and that the shape table reaches the edges of the launches -----------------------------------
def test_the_shape_table_reaches_the_launch_edges():
    trips, groups, tails = set(), set(), set()
    for ny, nx in SP.GRIDS + SP.DIRECT_GRIDS:
        g, tail = SP.cell_groups(ny * nx)
        groups.add(min(g, 257) if g <= 256 else 257)
        tails.add(tail)
    for ny, nx in SP.DIRECT_GRIDS:
        trips.add(SP.label_trips(ny * nx))                   # all cells one label
    for ny, nx in SP.GRIDS:
        kx, ky, _ = SP.axes_for(4, ny, nx)
        for ndir in SP.NDIRS:
            L_dir, L_k, nk, _, _ = O.label_maps(kx, ky, ndir)
            for L, n in ((L_dir, ndir), (L_k, nk)):
                trips.update(SP.label_trips(int(c)) for c in np.bincount(L[L >= 0], minlength=n))
    assert {0, 1, 2, 3} <= trips and max(trips) > 256        # empty labels; one, two, three trips; 90000 cells: 352
    assert {1, 2, 257} <= groups and {1, 255, 256} <= tails  # one workgroup, two, more than one trip of the folds; a lane alone, all but one, all
    assert {O.positive_half(SP.axes_for(nt, 2, 2)[2]).size for nt in SP.NTS} == {1, 2, 4, 16}
    assert max(SP.NDIRS) > max(ny * nx for ny, nx in SP.GRIDS)


def test_gpu_inputs_are_what_they_claim():
    for name, (S, kx, ky, f, kw) in SP.product_probes().items():
        Pz = O.positive_half(f)
        assert S.dtype == np.float64 and np.isfinite(S).all() and (S[Pz] >= 0).all() and len(Pz) >= 1, name
    S = SP.random_spectrum(3, 30, 30, seed=5)
    assert S.min() > 0 and len(np.unique(np.frexp(S)[1])) > 30 and (np.frexp(S)[0] * 2.0 ** 53 % 2.0 ** 20 != 0).mean() > 0.9     # full mantissas
    S = SP.integer_spectrum(4, 9, 9)
    assert np.array_equal(S, np.floor(S)) and S.max() < 1000 and len(np.unique(S)) > 100
    pr = SP.current_probes()
    kw = pr["gate"]
    r = kw["omega"][2] - kw["sigma0"]
    assert (r == 0.5).sum() == 5 and r[0, 1] == np.nextafter(0.5, 1.0)
    assert pr["threshold"]["S"][2, 1, 0] < 0.5 == pr["threshold"]["S"][1, 0, 2]


# ---- every probe against the broken model it is there to catch --------------------------------------------------------------------
def _differs(a, b, keys):
    return any(np.shape(a[k]) != np.shape(b[k]) or not np.array_equal(a[k], b[k], equal_nan=True) for k in keys)


@pytest.mark.parametrize("probe, broken, keys", [
    ("half", "f0_in_P", ("freq", "S_f")), ("half", "nyquist_in_P", ("freq", "S_f")),
    ("direction", "kappa_plus", ("T_dir",)), ("direction", "dir_edge", ("T_dir",)), ("wrap", "no_mod", ("T_dir",)), ("corner", "corners", ("T_k",)),
    ("fold", "pairwise", ("T_dir",)), ("fold", "sequential", ("T_dir",)), ("tie", "tie_high", ("peak_index",)), ("tie2", "tie_high", ("peak_index",))])
def test_product_probe_catches(probe, broken, keys):
    S, kx, ky, f, kw = SP.product_probes()[probe]
    assert _differs(O.products(S, kx, ky, f, **kw), O.products(S, kx, ky, f, broken=(broken,), **kw), keys)


def _sums(kw, broken=()):
    kw = dict(kw)
    S = kw.pop("S")
    return O.current_sums(S, kw.pop("pa", 0), S.shape[0], kw["labels"], kw["omega"], kw["kappa_x"], kw["kappa_y"], kw["sigma0"], kw["U"], kw["V"],
                          kw["threshold_value"], kw["gate_value"], broken=broken)


@pytest.mark.parametrize("probe, broken", [("threshold", "gt_threshold"), ("gate", "lt_gate"), ("gate_current", "lt_gate"), ("full", "fused"),
                                           ("many_groups", "pairwise"), ("many_groups", "sequential")])
def test_current_probe_catches(probe, broken):
    kw = SP.current_probes()[probe]
    assert _sums(kw) != _sums(kw, (broken,))


def test_threshold_and_gate_probes_count_what_they_should():
    pr = SP.current_probes()
    assert _sums(pr["threshold"])[1] == 2 and _sums(pr["threshold"], ("gt_threshold",))[1] == 1
    # p = 0, 1 of all six cells, p = 2 of the five whose residual is exactly the gate
    assert _sums(pr["gate"])[1] == 17 and _sums(pr["gate"], ("lt_gate",))[1] == 12


def test_the_gate_is_not_applied_in_round_0():
    S, kx, ky, f = SP.shell_spectrum(32, 33, 31, 2.0, 0.5, 0.4, -0.25, outlier=True)
    a, b = O.dispersion_current(S, kx, ky, f, threshold=0.05), O.dispersion_current(S, kx, ky, f, threshold=0.05, broken=("gate_round0",))
    assert a["trace"][0]["n_bins"] > b["trace"][0]["n_bins"] and a["trace"][0]["U"] != b["trace"][0]["U"]
    assert a["trace"][1]["n_bins"] == a["trace"][0]["n_bins"] - 1      # the first gated round drops the outlier
