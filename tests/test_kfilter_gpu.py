"""The dispersion filter on the GPU (wass_amd.postproc: Fourier3DFilter, fourier_filter_3d, dispersion_filter) against the oracle
of tests/kfilter_oracle.py, over its case table (tests/test_kfilter.py asserts what the table reaches) and on the probes of
tests/kfilter_probes.py.  Masks and everything a flag decides are compared bit for bit, the filtered field within the bound that
DESIGN.md, "Dispersion filter", derives and within the tile limits of kfilter_oracle."""
import functools

import numpy as np
import pytest

import dft_oracle as DO
import kfilter_oracle as KO
import kfilter_probes as KP
from guarded import Guarded, host
from wass_amd import postproc as P

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _ref(case):
    """the dense input of a case and the oracle's answers to it, computed once and left unchanged"""
    cube, H = KO.dense_input(case)
    r = KO.filter_cube(cube, H)
    r.update(cube=cube, H=H, b=KO.bound(r["p"], H))
    for v in r.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return r


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _fields(stats):
    return np.array([stats.var_in, stats.var_out, stats.kept, stats.n_nan, stats.n_empty_cells], np.float64)


def _exact_shell(case):
    """maps exact in binary for a shape, and a gate G that some bin meets exactly: (maps, U, V, G)"""
    m = KP.exact_maps(case)
    U, V = 0.25, -0.5
    p, i, j = np.indices(case)
    r = np.abs((m["omega"][p] - m["sigma0"][i, j]) - (m["kappa_x"][j] * U + m["kappa_y"][i] * V))
    nyq = [(n % 2 == 0) & (q == 0) for n, q in zip(case, (p, i, j))]              # the shifted index 0 of an even axis
    r = np.unique(r[(m["used"][i, j] != 0) & (m["omega"][p] > 0) & ~(nyq[0] | nyq[1] | nyq[2])])
    r = r[r > 0]
    return m, U, V, (float(r[len(r) // 3]) if len(r) else None)


# ---- the mask -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", KO.CASES, ids=str)
def test_shell_mask_is_the_oracles(gpu_ctx, case):
    m, U, V, G = _exact_shell(case)
    edge, G = G is not None, G or 1.0
    maps = (m["omega"], m["kappa_x"], m["kappa_y"], m["sigma0"], m["used"])
    top = float(m["omega"][-1])
    settings = [(U, V, G, -np.inf, np.inf, False), (U, V, np.nextafter(G, 0.0), -np.inf, np.inf, False), (U, V, np.nextafter(G, np.inf), -np.inf, np.inf, False),
                (U, V, G, -np.inf, np.inf, True), (U, V, G, np.inf, -np.inf, False), (U, V, G, np.inf, -np.inf, True), (0.0, 0.0, 1e9, -np.inf, np.inf, False),
                (U, V, 2.0, 1.0, max(top - 1.0, 1.0), False)]
    sums = []
    with P.Fourier3DFilter(*case, ctx=gpu_ctx) as filt:
        for s in settings:
            n = filt.set_shell(*maps, *s)
            want = KO.shell_mask(*maps, *s)
            got = filt.mask()
            assert got.dtype == np.float32 and np.array_equal(got, KO.half(want)), (case, s)
            assert n == int(want.sum()) and KO.is_even(want)
            sums.append(n)
    assert edge == (case[0] >= 3 and max(case[1:]) >= 3), "a cube with a decidable bin off k = 0 has a gate to put a bin on"
    if edge:
        assert sums[1] < sums[0] == sums[2], "no bin sits at |r| == G"
    assert sums[4] == 0 and sums[5] == sums[0] + sums[3] and sums[6] >= sums[0]


def test_physical_maps_and_sector_edges(gpu_ctx):
    case, du, dt = (9, 10, 10), 0.5, 0.25
    for sector in (None, (0.0, np.pi / 4), (np.pi, np.pi / 4), (np.pi / 2, 0.0)):
        maps = KO.mask_maps(*case, du, dt, 4.0, 9.81, 0.0, np.inf, sector)
        if sector == (0.0, np.pi / 4):                               # the diagonals kappa = (m, m) and (m, -m) are the two edges, and inside
            d = maps["used"][np.arange(10), np.arange(10)].sum() + maps["used"][np.arange(10), 9 - np.arange(10)].sum()
            assert d > 0 and maps["used"].sum() < 99
        want = KO.shell_mask(maps["omega"], maps["kappa_x"], maps["kappa_y"], maps["sigma0"], maps["used"], 0.2, -0.1, 2.0 * maps["domega"],
                             *KO.band(maps, 0.3, 1.7))
        mine = P.dispersion_mask_maps(*case, du, dt, 4.0, 9.81, 0.0, np.inf, sector)
        with P.Fourier3DFilter(*case, ctx=gpu_ctx) as filt:
            n = filt.set_shell(mine["omega"], mine["kappa_x"], mine["kappa_y"], mine["sigma0"], mine["used"], 0.2, -0.1, 2.0 * mine["domega"],
                               *P.shell_band(mine, 0.3, 1.7))
            assert np.array_equal(filt.mask(), KO.half(want)) and n == int(want.sum())
        assert sector is not None or n > 0


# ---- exact results --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", KO.CASES, ids=str)
def test_exact_results(gpu_ctx, case):
    import torch
    r = _ref(case)
    cube, H = r["cube"], r["H"]
    nan, empty, m32 = r["nan"], r["empty"], r["m"].astype(np.float32)
    with P.Fourier3DFilter(*case, ctx=gpu_ctx) as filt:
        # nothing passes: the mean comes back, bit for bit
        filt.set_mask(np.zeros_like(H))
        out = filt.apply(cube)
        want = np.where(nan | empty[None], np.float32(np.nan), np.broadcast_to(m32[None], case))
        assert _same(out, want.astype(np.float32))
        assert (filt.stats.n_nan, filt.stats.n_empty_cells) == (r["n_nan"], r["n_empty"]) and filt.stats.var_out == 0.0
        zeros = filt.apply(cube, restore_mean=False, keep_nan=False)
        assert np.isnan(zeros[:, empty]).all() and not zeros[:, ~empty].any()
        # the dense mask: NaN where it was, twice the same bits, the same bits from device memory and in place
        filt.set_mask(H)
        out = filt.apply(cube)
        assert np.array_equal(np.isnan(out), nan | empty[None])
        assert _same(filt.apply(cube), out)
        filled = filt.apply(cube, keep_nan=False)
        assert np.array_equal(np.isnan(filled), np.broadcast_to(empty[None], case)) and _same(np.where(nan, np.float32(np.nan), filled), out)
        stats = filt.stats
        d = torch.from_numpy(cube.copy()).cuda()
        dout = filt.apply(d)
        assert _same(dout.cpu().numpy(), out) and np.array_equal(_fields(filt.stats), _fields(stats), equal_nan=True)
        assert filt.apply(d, out=d) is d and _same(d.cpu().numpy(), out)
        h = cube.copy()
        assert filt.apply(h, out=h) is h and _same(h, out)


def test_strided_views_and_guards(gpu_ctx):
    import torch
    case = (5, 13, 28)
    r = _ref(case)
    clean = np.nan_to_num(r["cube"], nan=49.0)                    # Guarded compares with ==: no NaN in what it holds
    with P.Fourier3DFilter(*case, ctx=gpu_ctx) as filt:
        filt.set_mask(r["H"])
        base, base_nan = filt.apply(clean), filt.apply(r["cube"])
        for dev in (False, True):
            g = Guarded(dev)
            out = g.out(case, np.float32)
            assert filt.apply(g.input(clean), out=out) is out
            g.check(f"Fourier3DFilter.apply, {'device' if dev else 'host'}")
            assert _same(np.ascontiguousarray(host(out)), base)
            # the same with the NaN samples, the parent compared byte for byte
            parent = np.full((2 * case[0], case[1] + 3, case[2] + 5), 3.0e30, np.float32)
            parent[::2, 2:-1, 3:-2] = r["cube"]
            before = parent.tobytes()
            if dev:
                parent = torch.from_numpy(parent).cuda()
            assert _same(np.ascontiguousarray(host(filt.apply(parent[::2, 2:-1, 3:-2]))), base_nan)
            assert host(parent).tobytes() == before


def test_timing_mode_changes_nothing(gpu_ctx):
    case = (6, 11, 64)
    r = _ref(case)
    with P.Fourier3DFilter(*case, ctx=gpu_ctx) as filt:
        filt.set_mask(r["H"])
        plain = filt.apply(r["cube"])
        filt.set_timing(True)
        timed = filt.apply(r["cube"])
        ms = filt.last_timings()
        filt.set_timing(False)
        assert _same(timed, plain) and _same(filt.apply(r["cube"]), plain)
    assert list(ms) == list(P.Fourier3DFilter.STAGES) and all(v >= 0 for v in ms.values()) and sum(ms.values()) > 0


def test_set_mask_of_the_shell_mask(gpu_ctx):
    for case in ((7, 9, 33), (4, 16, 30)):
        m, U, V, G = _exact_shell(case)
        cube = _ref(case)["cube"]
        with P.Fourier3DFilter(*case, ctx=gpu_ctx) as filt:
            assert filt.set_shell(m["omega"], m["kappa_x"], m["kappa_y"], m["sigma0"], m["used"], U, V, 2.0 * G + 1.0) > 0
            a, Hs = filt.apply(cube), filt.mask()
            assert filt.stats.n_pass == int(KO.full(Hs, case[2]).sum())
        assert _same(P.fourier_filter_3d(cube, Hs, ctx=gpu_ctx), a)


SPATIAL = [c for c in DO.CASES_SPATIAL if max(c) <= 130]


@pytest.mark.parametrize("rows,cols", SPATIAL, ids=str)
def test_close_is_the_real_part_of_the_stage(gpu_ctx, rows, cols):
    """The witness is the spatial filter, whose last launch is k_dft_stage<true, true> on the same half spectrum: with one frame, a
    mask that is its transfer function and no centring, the chain before k_dft_close is the spatial filter's launch for launch (the
    t stages of length 1 multiply by one and add zero)."""
    Hs = DO.butterworth_transfer(rows, cols).astype(np.float32).astype(np.float64)          # what a float32 mask can hold
    _, view = DO.dense_frames_spatial((rows, cols))
    frame = np.ascontiguousarray(view[:1])
    sp = P.Spatial2DButterworth(rows, cols, DO.SPATIAL_DU, DO.SPATIAL_CUTOFF, DO.SPATIAL_ORDER, ctx=gpu_ctx, batch=1)
    sp.butterworth_filter = Hs
    with sp:
        want = sp.apply_batch(frame)
    with P.Fourier3DFilter(1, rows, cols, ctx=gpu_ctx) as filt:
        filt.set_mask(np.fft.ifftshift(Hs)[None, :, :cols // 2 + 1])
        got = filt.apply(frame, restore_mean=False, centre=False)
    assert np.isfinite(want).all() and np.abs(want).max() > 1.0
    assert np.array_equal(got, want), f"{int((got != want).sum())} of {want.size} cells differ"


# ---- bounded results ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", KO.CASES, ids=str)
def test_bounded_results(gpu_ctx, case):
    r = _ref(case)
    cube, H, b, ok = r["cube"], r["H"], r["b"], ~r["nan"]
    with P.Fourier3DFilter(*case, ctx=gpu_ctx) as filt:
        filt.set_mask(H)
        out = filt.apply(cube)
        st = filt.stats
        y = filt.apply(cube, restore_mean=False, keep_nan=False)
    live = np.broadcast_to(~r["empty"][None], case)
    ey = np.where(live, np.abs(y.astype(np.float64) - r["y"]), 0.0)
    eo = np.where(ok, np.abs(out.astype(np.float64) - r["out"].astype(np.float64)), 0.0)
    el_y, el_o = DO.ratio(ey, np.full(case, b)), DO.ratio(eo, np.broadcast_to(KO.out_tolerance(r["out"], b, True), case))
    terr, ntiles = DO.tile_errors(np.where(live, y, 0), np.where(live, r["y"], 0))
    t_table = DO.ratio(terr, np.full(terr.shape, KO.tile_limit(b, y.size, ntiles)))
    t_model = DO.ratio(terr, np.full(terr.shape, KO.model_tile_limit(r["p"], H, r["y"])))
    n = int(ok.sum())
    y2 = float((y.astype(np.float64)[ok] ** 2).sum()) / n if n else float("nan")
    rel = lambda got, want: abs(got - want) / want if want else abs(got)
    v_in, v_out = rel(st.var_in, r["var_in"]), rel(st.var_out, y2)
    print(f"{case}: |y - oracle| / bound {el_y:.4g}, |out - oracle| / tolerance {el_o:.4g}, tile error / table limit {t_table:.4g}, / model limit "
          f"{t_model:.4g}; var_in off by {v_in:.3g}, var_out by {v_out:.3g} (gamma_N {KO.gamma(n + 2):.3g}); kept {st.kept:.4f}")
    assert el_y <= 1.0 and el_o <= 1.0 and t_table <= 1.0 and t_model <= 1.0
    if n:
        assert v_in <= KO.gamma(n + 2) and v_out <= KO.gamma(n + 2)
        assert st.var_in == 0 or st.kept == st.var_out / st.var_in
    else:
        assert np.isnan(st.var_in) and np.isnan(st.var_out)


# ---- the probes -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("probe", KP.probes(), ids=lambda p: p.name)
def test_probe_on_the_device(gpu_ctx, probe):
    good = KP.model(probe)
    with P.Fourier3DFilter(*probe.cube.shape, ctx=gpu_ctx) as filt:
        if probe.H is not None:
            filt.set_mask(probe.H)
        else:
            filt.set_shell(*KP.shell_args(probe))
            assert np.array_equal(filt.mask(), good["H"])
        out = filt.apply(probe.cube, restore_mean=probe.restore_mean, keep_nan=probe.keep_nan)
    off = 5.0 * KP.miss(out, good["out"], good["tol"])
    print(f"{probe.name}: |out - oracle| / tolerance = {off:.4g}")
    assert off <= 1.0
    for v in probe.catches:
        assert KP.miss(out, KP.model(probe, v)["out"], good["tol"]) >= 1.0, v


# ---- physics: the sign conventions ----------------------------------------------------------------------------------------------
SEA = (16, 12, 20)
DU, G0 = 0.5, 9.81


def _on_shell(mx, my, mf, shape=SEA):
    """dt that puts the deep-water wave towards kappa = 2 pi (mx / (nx du), my / (ny du)) exactly on frequency bin mf"""
    nt, ny, nx = shape
    k0 = 2.0 * np.pi * np.hypot(mx / (nx * DU), my / (ny * DU))
    return 2.0 * np.pi * mf / (nt * np.sqrt(G0 * k0))


def _kept(gpu_ctx, cube, dt, **kw):
    out, st = P.dispersion_filter(cube, DU, dt, ctx=gpu_ctx, restore_mean=False, **kw)
    nt, ny, nx = cube.shape
    maps = KO.mask_maps(nt, ny, nx, DU, dt, kw.get("depth", np.inf), G0, kw.get("k_min", 0.0), kw.get("k_max", np.inf), kw.get("sector"))
    U, V = kw.get("current", (0.0, 0.0))
    H = KO.half(KO.shell_mask(maps["omega"], maps["kappa_x"], maps["kappa_y"], maps["sigma0"], maps["used"], U, V, kw.get("width", 2.0) * maps["domega"],
                              *KO.band(maps, kw.get("f_min", 0.0), kw.get("f_max", np.inf)), kw.get("complement", False)))
    ref = KO.filter_cube(cube, H, restore_mean=False)
    b = KO.bound(ref["p"], H)
    assert np.abs(out.astype(np.float64) - ref["y"]).max() <= b, "the device is off the oracle"
    assert st.n_pass == int(KO.full(H, nx).sum())
    return st.kept, out, b


def test_wave_on_the_shell(gpu_ctx):
    mx, my, mf = 3, 2, 4
    dt = _on_shell(mx, my, mf)
    w = KP.wave(SEA, mf, my, mx, offset=20.0)
    kept, out, b = _kept(gpu_ctx, w, dt, width=0.5)
    assert kept >= 0.999 and np.abs(out - (w - np.float32(20.0))).max() <= b + 1e-5
    assert _kept(gpu_ctx, w, dt, width=0.5, complement=True)[0] <= 1e-9
    # the direction of travel is that of kappa = (mx, my): a sector around it keeps the wave, the opposite one removes it
    th = float(np.arctan2(my / (SEA[1] * DU), mx / (SEA[2] * DU)))
    assert _kept(gpu_ctx, w, dt, width=0.5, sector=(th, 0.3))[0] >= 0.999
    assert _kept(gpu_ctx, w, dt, width=0.5, sector=(th + np.pi, 0.3))[0] <= 1e-9
    # the same wave run backwards in time travels the other way: cos(k . r + w t)
    back = KP.wave(SEA, -mf, my, mx)
    assert _kept(gpu_ctx, back, dt, width=0.5, sector=(th, 0.3))[0] <= 1e-9 and _kept(gpu_ctx, back, dt, width=0.5, sector=(th + np.pi, 0.3))[0] >= 0.999
    # three bins off the shell
    assert _kept(gpu_ctx, KP.wave(SEA, mf + 3, my, mx), dt, width=2.0)[0] <= 1e-9
    assert _kept(gpu_ctx, KP.wave(SEA, mf + 3, my, mx), dt, width=3.5)[0] >= 0.999


def test_wave_on_a_current(gpu_ctx):
    mx, my, mf, shift = 3, 0, 3, 2
    dt = _on_shell(mx, my, mf)
    domega = 2.0 * np.pi / (SEA[0] * dt)
    cur = (shift * domega / (2.0 * np.pi * mx / (SEA[2] * DU)), 0.7)            # kappa . (U, V) = shift bins; V does nothing to kappa_y = 0
    moved, still = KP.wave(SEA, mf + shift, my, mx), KP.wave(SEA, mf, my, mx)
    assert _kept(gpu_ctx, moved, dt, width=1.0, current=cur)[0] >= 0.999
    assert _kept(gpu_ctx, still, dt, width=1.0, current=cur)[0] <= 1e-9
    assert _kept(gpu_ctx, still, dt, width=1.0)[0] >= 0.999 and _kept(gpu_ctx, moved, dt, width=1.0)[0] <= 1e-9
    # against the current the wave towards -x is shifted down
    assert _kept(gpu_ctx, KP.wave(SEA, mf - shift, -my, -mx), dt, width=1.0, current=cur)[0] >= 0.999


def test_current_fit_then_filter(gpu_ctx):
    shape, dt = (32, 16, 16), 0.5
    nt, ny, nx = shape
    rng = np.random.default_rng(5)
    Utrue = (0.3, -0.2)
    t, y, x = np.indices(shape)
    sea = np.zeros(shape)
    for mx, my in ((1, 0), (2, 1), (1, 2), (0, 2), (2, -1), (3, 1), (1, -2), (2, 2)):
        kx, ky = 2.0 * np.pi * mx / (nx * DU), 2.0 * np.pi * my / (ny * DU)
        w = np.sqrt(G0 * np.hypot(kx, ky)) + kx * Utrue[0] + ky * Utrue[1]
        sea += rng.uniform(0.5, 1.0) * np.cos(kx * x * DU + ky * y * DU - w * t * dt + rng.uniform(0, 6.28))
    noise = 0.3 * rng.standard_normal(shape)
    cube = (sea + noise).astype(np.float32)
    kxa, kya, fa = P.dft_axes(nt, ny, nx, DU, dt)
    S = np.fft.fftshift(np.abs(np.fft.fftn(cube.astype(np.float64) - cube.mean(axis=0, dtype=np.float64))) ** 2)
    fit = P.dispersion_current(S, kxa, kya, fa, threshold=0.05, ctx=gpu_ctx)
    assert not fit.singular and abs(fit.U - Utrue[0]) < 0.1 and abs(fit.V - Utrue[1]) < 0.1
    out, st = P.dispersion_filter(cube, DU, dt, current=fit, width=2.0, ctx=gpu_ctx)
    maps = KO.mask_maps(nt, ny, nx, DU, dt)
    H = KO.half(KO.shell_mask(maps["omega"], maps["kappa_x"], maps["kappa_y"], maps["sigma0"], maps["used"], fit.U, fit.V, 2.0 * maps["domega"],
                              *KO.band(maps)))
    ref = KO.filter_cube(cube, H)
    b = KO.bound(ref["p"], H)
    want = ref["var_out"] / ref["var_in"]
    slack = (2.0 * np.sqrt(ref["var_out"]) * b + b * b) / ref["var_in"]
    print(f"fit ({fit.U:.3f}, {fit.V:.3f}) for {Utrue}; kept {st.kept:.4f}, the oracle {want:.4f}, slack {slack:.2g}; the sea alone is "
          f"{sea.var() / cube.astype(np.float64).var():.4f} of the variance")
    assert st.kept >= want - slack and 0.5 < st.kept < 1.0
    assert np.abs(out.astype(np.float64) - ref["out"]).max() <= np.max(KO.out_tolerance(ref["out"], b, True))


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals(gpu_ctx):
    import torch
    case = (4, 3, 5)
    cube = DO.probe_cube(*case)
    H = np.ones((4, 3, 3), np.float32)
    bad = cube.copy()
    bad[2, 1, 3] = -np.inf
    with P.Fourier3DFilter(*case, ctx=gpu_ctx) as filt:
        with pytest.raises(ValueError, match="no mask"):
            filt.apply(cube)
        filt.set_mask(H)
        out = np.full(case, 7.0, np.float32)
        with pytest.raises(ValueError, match="infinite"):
            filt.apply(bad, out=out)
        assert (out == 7.0).all()                                          # refused before anything was written
        with pytest.raises(ValueError, match="infinite"):
            filt.apply(torch.from_numpy(bad).cuda())
        assert np.isfinite(filt.apply(cube)).all()                         # the handle is as good as before
        uneven = H.copy()
        uneven[1, 2, 0] = 0.0
        with pytest.raises(ValueError, match="not even"):
            filt.set_mask(uneven)
        with pytest.raises(ValueError):
            filt.set_mask(H[:, :, :2])
        with pytest.raises(ValueError):
            filt.apply(cube[:3])
        m = KP.exact_maps(case)
        with pytest.raises(ValueError):
            filt.set_shell(m["omega"], m["kappa_x"], m["kappa_y"], m["sigma0"], m["used"], np.nan, 0.0, 1.0)
        with pytest.raises(ValueError):
            filt.set_shell(m["omega"][:-1], m["kappa_x"], m["kappa_y"], m["sigma0"], m["used"], 0.0, 0.0, 1.0)
    with pytest.raises(ValueError, match="not even"):
        P.fourier_filter_3d(cube, uneven, ctx=gpu_ctx)
    singular = P.CurrentFit(U=float("nan"), V=float("nan"), speed=float("nan"), direction=float("nan"), n_bins=1, rms=float("nan"), singular=True,
                            trace=[])
    with pytest.raises(ValueError, match="singular"):
        P.dispersion_filter(cube, 1.0, 1.0, current=singular, ctx=gpu_ctx)
    # above the cap: the plan function alone decides, nothing is allocated
    assert P.fourier_filter_scratch_bytes(1200, 1024, 1024) > P.KFILTER_SCRATCH_CAP
    with pytest.raises(MemoryError):
        P.Fourier3DFilter(1200, 1024, 1024, ctx=gpu_ctx)
