"""The dispersion filter without a GPU: the oracle of tests/kfilter_oracle.py against numpy's own transforms, the mask rule against
a brute-force loop, the host maps against the expressions of spectral_label_maps and dispersion_current, the scratch plan against
its golden table, argument errors, every probe of tests/kfilter_probes.py against the broken model it is there to catch, and a
restatement of the launch arithmetic that asserts what the case table reaches."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import dft_oracle as DO
import kfilter_oracle as KO
import kfilter_probes as KP
from wass_amd import _lib
from wass_amd import postproc as P

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kfilter_plans.json")
SMALL = [c for c in KO.CASES if c[0] * c[1] * c[2] <= 40000]
DU, DT = 0.5, 0.25


# ---- the oracle -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", KO.CASES, ids=str)
def test_oracle_is_numpy_irfftn(case):
    cube, H = KO.dense_input(case)
    p, m, nan, empty = KO.prepare(cube)
    y = KO.field(p, H)
    X = np.fft.rfftn(p.astype(np.float64))
    ref = np.fft.irfftn(X * H.astype(np.float64), s=case, axes=(0, 1, 2))
    full = np.real(np.fft.ifftn(np.fft.fftn(p.astype(np.float64)) * KO.full(H, case[2]).astype(np.float64)))
    top = max(float(np.abs(ref).max()), 1e-300)
    assert np.abs(y - ref).max() <= 1e-12 * top and np.abs(y - full).max() <= 1e-12 * top
    staged = KO.staged_field(p, H)
    assert np.abs(staged - ref).max() <= 1e-12 * top


def test_preparation_and_undoing():
    cube = np.array([[[1, 2, np.nan]], [[3, np.nan, np.nan]], [[8, 4, np.nan]]], np.float32)
    p, m, nan, empty = KO.prepare(cube)
    assert m.tolist() == [[4.0, 3.0, 0.0]] and empty.tolist() == [[False, False, True]]
    assert p[:, 0, 0].tolist() == [-3, -1, 4] and p[:, 0, 1].tolist() == [-1, 0, 1] and p[:, 0, 2].tolist() == [0, 0, 0]
    y = np.zeros_like(p)
    out = KO.undo(y, m, nan, empty)
    assert np.array_equal(out, np.where(nan, np.nan, np.float32(1) * m[None].astype(np.float32)), equal_nan=True)
    out = KO.undo(y, m, nan, empty, keep_nan=False)
    assert out[1, 0, 1] == 3 and np.isnan(out[:, 0, 2]).all()
    assert not KO.undo(y, m, nan, empty, restore_mean=False, keep_nan=False)[:, 0, :2].any()
    # the zeromean rule: the sum runs in frame order in fp64
    big = np.array([1e8, 1, -1e8, 1], np.float32).reshape(4, 1, 1)
    assert KO.prepare(big)[1][0, 0] == ((1e8 + 1 - 1e8) + 1) / 4


# ---- the mask -------------------------------------------------------------------------------------------------------------------
def _brute_mask(nt, ny, nx, du, dt, depth, g, U, V, width, f_min, f_max, k_min, k_max, sector, complement):
    """The rule of DESIGN.md read literally, bin by bin over the full cube, on np.fft.fftfreq's axes."""
    f = np.fft.fftfreq(nt, dt)
    kx, ky = 2.0 * np.pi * np.fft.fftfreq(nx, du), 2.0 * np.pi * np.fft.fftfreq(ny, du)
    df = 1.0 / (nt * dt)
    G = width * (2.0 * np.pi * df)

    def decide(a, b, c):
        kapx, kapy = -kx[c], -ky[b]
        kmod = np.sqrt(kapx * kapx + kapy * kapy)
        used = kmod != 0 and k_min <= kmod <= k_max
        if used and sector is not None:
            theta = np.mod(np.arctan2(kapy, kapx), 2.0 * np.pi)
            used = abs(np.mod(theta - sector[0] + np.pi, 2.0 * np.pi) - np.pi) <= sector[1]
        sigma0 = np.sqrt(g * kmod) if np.isinf(depth) else np.sqrt(g * kmod * np.tanh(kmod * depth))
        omega = 2.0 * np.pi * f[a]
        d = omega - sigma0
        r = d - (kapx * U + kapy * V)
        ok = bool(used and f_min <= f[a] <= f_max and abs(r) <= G)
        return (not ok) if complement else ok

    H = np.zeros((nt, ny, nx), np.float32)
    for a in range(nt):
        for b in range(ny):
            for c in range(nx):
                if a == 0 or (nt % 2 == 0 and a == nt // 2) or (ny % 2 == 0 and b == ny // 2) or (nx % 2 == 0 and c == nx // 2):
                    continue
                if f[a] > df / 2:
                    H[a, b, c] = decide(a, b, c)
                elif f[a] < -df / 2:
                    H[a, b, c] = decide(-a % nt, -b % ny, -c % nx)
    return H


MASK_SETTINGS = [dict(), dict(U=0.3, V=-0.2, width=1.0), dict(depth=2.0, sector=(0.7, 0.9), width=3.0), dict(complement=True, f_min=0.3, f_max=1.2),
                 dict(k_min=1.0, k_max=4.0, U=-0.1, V=0.4)]


@pytest.mark.parametrize("case", SMALL, ids=str)
def test_mask_is_the_rule_and_even(case):
    nt, ny, nx = case
    for n, kw in enumerate(MASK_SETTINGS):
        s = dict(depth=np.inf, g=9.81, U=0.0, V=0.0, width=2.0, f_min=0.0, f_max=np.inf, k_min=0.0, k_max=np.inf, sector=None, complement=False)
        s.update(kw)
        maps = KO.mask_maps(nt, ny, nx, DU, DT, s["depth"], s["g"], s["k_min"], s["k_max"], s["sector"])
        H = KO.shell_mask(maps["omega"], maps["kappa_x"], maps["kappa_y"], maps["sigma0"], maps["used"], s["U"], s["V"], s["width"] * maps["domega"],
                          *KO.band(maps, s["f_min"], s["f_max"]), s["complement"])
        assert KO.is_even(H), (case, kw)
        assert np.array_equal(KO.full(KO.half(H), nx), H)
        if nt * ny * nx <= 12000 or n == 1:
            assert np.array_equal(H, _brute_mask(nt, ny, nx, DU, DT, **s)), (case, kw)
        if s["complement"] and not (nt <= 2):
            plain = KO.shell_mask(maps["omega"], maps["kappa_x"], maps["kappa_y"], maps["sigma0"], maps["used"], s["U"], s["V"],
                                  s["width"] * maps["domega"], *KO.band(maps, s["f_min"], s["f_max"]), False)
            decided = (H + plain) == 1
            assert not (H * plain).any() and not decided[0].any() and (nt % 2 or not decided[nt // 2].any())


def test_maps_are_the_packages_own_expressions():
    for (nt, ny, nx), depth, sector in (((8, 6, 10), np.inf, None), ((7, 9, 33), 3.5, (2.0, 0.6)), ((1, 1, 1), 1.0, None), ((4, 1, 5), np.inf, (0.0, 0.1))):
        got = P.dispersion_mask_maps(nt, ny, nx, DU, DT, depth, 9.81, 0.5, 6.0, sector)
        want = KO.mask_maps(nt, ny, nx, DU, DT, depth, 9.81, 0.5, 6.0, sector)
        for k, v in want.items():
            assert np.array_equal(got[k], v), k
        kx, ky, f = P.dft_axes(nt, ny, nx, DU, DT)
        L_dir, _, _, kmod = P.spectral_label_maps(kx, ky, 1, 1.0, 0.5, 6.0)
        assert np.array_equal(got["kmod"], kmod) and np.array_equal(got["kappa_x"], -kx) and np.array_equal(got["omega"], 2.0 * np.pi * f)
        if sector is None:
            assert np.array_equal(got["used"], (L_dir >= 0).astype(np.uint8))
        sig = np.sqrt(9.81 * kmod) if np.isinf(depth) else np.sqrt(9.81 * kmod * np.tanh(kmod * depth))      # dispersion_current's
        assert np.array_equal(got["sigma0"], sig)
        assert P.shell_band(got, 0.2, 1.5) == KO.band(want, 0.2, 1.5)
    # theta is the direction of travel: counter-clockwise from +x, of kappa = -k
    m = P.dispersion_mask_maps(4, 5, 5, 1.0, 1.0)
    i, j = 2 + 1, 2 - 1                                          # ky > 0, kx < 0: kappa points to +x, -y
    assert m["kappa_x"][j] > 0 and m["kappa_y"][i] < 0 and np.isclose(m["theta"][i, j], 2.0 * np.pi - np.pi / 4)
    assert P.shell_band(m, 5.0, 6.0) == (np.inf, -np.inf)


# ---- the plan -------------------------------------------------------------------------------------------------------------------
def test_plans_match_golden():
    with open(GOLDEN) as f:
        entries = json.load(f)
    lib = _lib.load()
    bad = []
    for e in entries:
        b = C.c_size_t()
        rc = lib.wass_kfilter_scratch_bytes(*e["args"], C.byref(b))
        got = {"error": rc} if rc else b.value
        if got != e["result"]:
            bad.append((e["args"], e["result"], got))
    assert not bad, f"{len(bad)} of {len(entries)} plans differ, the first: {bad[0]}"
    res = [e["result"] for e in entries]
    assert any(isinstance(r, dict) for r in res) and any(isinstance(r, int) and r > 16 << 30 for r in res)


def test_production_size_fits_the_cap():
    assert P.KFILTER_SCRATCH_CAP == 16 << 30
    b = P.fourier_filter_scratch_bytes(1000, 1024, 1024)          # the same plan serves host and device input
    cube = 1000 * 1024 * 1024 * 4
    assert b <= P.KFILTER_SCRATCH_CAP and 3.5 * cube < b < 3.7 * cube
    assert P.fourier_filter_scratch_bytes(1200, 1024, 1024) > P.KFILTER_SCRATCH_CAP
    with pytest.raises(MemoryError):                              # refused before a context is made or anything is allocated
        P.Fourier3DFilter(1200, 1024, 1024)
    with pytest.raises(ValueError):
        P.fourier_filter_scratch_bytes(0, 4, 4)
    with pytest.raises(ValueError):
        P.fourier_filter_scratch_bytes(4, 4, 8193)


# ---- argument errors ------------------------------------------------------------------------------------------------------------
def test_argument_errors():
    H = np.ones((4, 3, 3), np.float32)
    P.check_even_mask(H, 5)
    bad = H.copy()
    bad[1, 1, 0] = 0.5                                            # its mirror image (3, 2, 0) is still 1
    with pytest.raises(ValueError, match="not even"):
        P.check_even_mask(bad, 5)
    bad[3, 2, 0] = 0.5
    P.check_even_mask(bad, 5)
    ny_col = np.ones((4, 3, 3), np.float32)
    ny_col[1, 0, 2] = 0.0                                         # column 2 is the Nyquist column of nx = 4, not of nx = 5
    P.check_even_mask(ny_col, 5)
    with pytest.raises(ValueError, match="not even"):
        P.check_even_mask(ny_col, 4)
    with pytest.raises(ValueError, match="finite"):
        P.check_even_mask(np.full((1, 1, 1), np.nan, np.float32), 1)
    for kw in (dict(du=0.0), dict(dt=-1.0), dict(depth=0.0), dict(g=0.0), dict(k_min=-1.0), dict(k_min=2.0, k_max=1.0), dict(sector=(0.0, -1.0)),
               dict(sector=(np.nan, 1.0))):
        args = dict(nt=4, ny=4, nx=4, du=1.0, dt=1.0)
        args.update(kw)
        with pytest.raises(ValueError):
            P.dispersion_mask_maps(**args)
    cube = np.zeros((4, 4, 4), np.float32)
    singular = P.CurrentFit(U=float("nan"), V=float("nan"), speed=float("nan"), direction=float("nan"), n_bins=0, rms=float("nan"), singular=True,
                            trace=[])
    with pytest.raises(ValueError, match="singular"):             # before any context is made
        P.dispersion_filter(cube, 1.0, 1.0, current=singular)
    with pytest.raises(ValueError):
        P.dispersion_filter(cube, 1.0, 1.0, current=(np.inf, 0.0))
    with pytest.raises(ValueError):
        P.dispersion_filter(cube, 1.0, 1.0, width=-1.0)
    with pytest.raises(ValueError):
        P.dispersion_filter(cube[0], 1.0, 1.0)
    with pytest.raises(ValueError):
        P.fourier_filter_3d(cube[0], H)


# ---- the probes -----------------------------------------------------------------------------------------------------------------
def test_every_variant_has_a_probe():
    caught = {v for p in KP.probes() for v in p.catches}
    assert caught == set(KO.VARIANTS)


@pytest.mark.parametrize("probe", KP.probes(), ids=lambda p: p.name)
def test_probe_catches_its_broken_model(probe):
    good = KP.model(probe)
    if "out = input" in probe.expect or "passes whole" in probe.expect:
        assert KP.miss(good["out"], probe.cube, good["tol"]) <= 0.2, "the right model does not give what the probe expects"
    if probe.expect.startswith("out = (float) m_c"):
        assert np.array_equal(good["out"], good["m"].astype(np.float32)[None] + 0 * probe.cube)
    for v in probe.catches:
        bad = KP.model(probe, v)
        ratio = KP.miss(bad["out"], good["out"], good["tol"])
        print(f"{probe.name}: {v} misses by {ratio:.3g} x (5 x tolerance)")
        assert ratio >= 1.0, f"{probe.name} does not catch {v}: it misses by {ratio:.3g} x (5 x tolerance)"
    # the staged model in float32 is inside the tolerance: the probe's tolerance is one the device can meet
    y32 = KO.staged_field(good["p"], good["H"], dtype=np.float32)
    out32 = KO.undo(y32, good["m"], good["nan"], good["empty"], probe.restore_mean, probe.keep_nan)
    assert KP.miss(out32, good["out"], good["tol"]) <= 0.2


def test_gate_probe_sits_on_the_edge():
    pr = next(p for p in KP.probes() if p.name == "gate_edge")
    args = list(KP.shell_args(pr))
    on = KO.shell_mask(*args)
    args[7] = np.nextafter(pr.shell["G"], 0.0)
    below = KO.shell_mask(*args)
    args[7] = np.nextafter(pr.shell["G"], 2.0)
    above = KO.shell_mask(*args)
    assert on.sum() > below.sum() and np.array_equal(on, above)
    assert np.array_equal(KO.shell_mask(*KP.shell_args(pr), variant="gate_lt"), below)


# ---- the tile margin ------------------------------------------------------------------------------------------------------------
def test_tile_margin_is_measured():
    worst, at = 0.0, None
    for case in KO.CASES:
        cube, H = KO.dense_input(case)
        p = KO.prepare(cube)[0]
        err, ntiles = DO.tile_errors(KO.staged_field(p, H, dtype=np.float32), KO.field(p, H))
        b = KO.bound(p, H)
        assert np.abs(KO.staged_field(p, H, dtype=np.float32) - KO.field(p, H)).max() <= b
        r = DO.ratio(err, np.full(err.shape, b * np.sqrt(p.size) / np.sqrt(ntiles)))
        if r > worst:
            worst, at = r, case
    print(f"worst tile ratio of the float32 staged model: {worst:.4g} at {at}")
    assert at == KO.TILE_MEASURED[1] and abs(worst - KO.TILE_MEASURED[0]) <= 0.02 * KO.TILE_MEASURED[0]
    assert KO.TILE_MARGIN == 8 * KO.TILE_MEASURED[0] and KO.TILE_MARGIN < 1.0


# ---- the launch arithmetic ------------------------------------------------------------------------------------------------------
def test_case_table_reaches():
    plans = {c: KO.launch_plan(*c) for c in KO.CASES}
    assert KO.CASES[:4] == [(1, 1, 1), (2, 1, 1), (1, 2, 3), (3, 2, 2)]
    nxs = {c[2] for c in KO.CASES}
    assert {1, 2, 3} <= nxs                                                         # the columns that stand alone
    chs = {p["ch"] for p in plans.values()}
    assert {0, 1, 15} <= {ch % 16 for ch in chs} and {63, 64, 65} <= chs             # the k tiles of k_dft_close
    assert {0, 1, 63} <= {nx % 64 for nx in nxs}                                    # its M edge
    assert {0, 1, 63} <= {(c[0] * c[1]) % 64 for c in KO.CASES}                     # its N edge
    close = [p["stages"][-1] for p in plans.values()]
    assert all(s["stage"] == "close" and s["inst"] == (True, True) for s in close)
    assert {1} <= {s["grid"][0] for s in close} and max(s["grid"][0] for s in close) > 1       # one and several tiles in N ...
    assert {1} <= {s["grid"][1] for s in close} and max(s["grid"][1] for s in close) > 1       # ... and in M
    assert {1} <= {s["nk"] for s in close} and max(s["nk"] for s in close) >= 5
    assert {c[0] % 2 for c in KO.CASES} == {0, 1} and any(c[1] != c[2] for c in KO.CASES)
    assert any(p["cells"] % 32 for p in plans.values()) and any(p["cells"] % 64 == 0 for p in plans.values())
    assert any(p["wpf"] > 1 for p in plans.values()) and any(p["nprep"] > 1 for p in plans.values())
    big = [c for c in KO.CASES if max(c) > 130]
    assert big == [(20, 129, 131)]
    # the plan function agrees on the sizes the arithmetic gives: the bitmap and the partial sums are in the byte count
    for c, p in plans.items():
        nt, ny, nx = c
        a = lambda v: (v + 255) & ~255
        tw = lambda n: a(2 * (-(-n // 16) * 16) * (-(-n // 64) * 64) * 4)
        half_ = nt * ny * p["ch"]
        nclose = p["stages"][-1]["grid"][0] * p["stages"][-1]["grid"][1]
        want = a(nt * ny * nx * 4) + 2 * a(2 * half_ * 4) + a(half_ * 4) + a(nt * p["wpf"] * 8) + a(ny * nx * 8) + a(max(4 * p["nprep"], nclose) * 8) \
            + a(64) + a(256) + tw(nx) + tw(ny) + tw(nt)
        assert P.fourier_filter_scratch_bytes(*c) == want, c
