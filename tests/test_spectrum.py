"""Wave spectra, the parts that need no GPU: the numpy restatements (tests/spectrum_oracle.py) against what the reference's own
spectra.py returned (tests/golden/spectra_*.npz, written by tests/golden/make_golden_spectra.py) and against scipy, the axis
bookkeeping of wass_amd.postproc, the statistics, the argument errors and the scratch the C ABI states."""
import ctypes
import os
import warnings

import numpy as np
import pytest

import spectrum_oracle as SO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _golden_cube(g, **kw):
    return SO.make_cube(*[int(v) for v in g["shape"]], seed=int(g["seed"]), **kw)


@pytest.mark.parametrize("name,width", [("nx", 81), ("nx1", 84)])
def test_oracle_3d_equals_the_reference(name, width):
    """Both sides are fp64 with the same operations: rtol 1e-9 on every bin, the axes bit for bit."""
    g = np.load(os.path.join(GOLDEN, f"spectra_3d_{name}.npz"))
    cube = _golden_cube(g, nan_fraction=float(g["nan_fraction"]))
    S, KX, KY, f = SO.compute_3D_spectrum(cube, float(g["du"]), float(g["dt"]), datascale=float(g["datascale"]))
    assert S.shape == g["S"].shape == (4, width, width)
    np.testing.assert_allclose(S, g["S"], rtol=1e-9, atol=0)
    assert np.array_equal(KX, g["KX"]) and np.array_equal(KY, g["KY"]) and np.array_equal(f, g["f"])


def test_oracle_1d_equals_the_reference():
    """The reference runs scipy.signal.csd on float32 data: 1e-5 of the peak."""
    g = np.load(os.path.join(GOLDEN, "spectra_1d.npz"))
    cube = _golden_cube(g)
    f, S, ts = SO.compute_spectrum(cube, float(g["dt"]), int(g["nperseg"]), int(g["rangespan"]), float(g["scale"]))
    assert S.shape == g["S"].shape
    assert np.max(np.abs(S - g["S"])) <= 1e-5 * g["S"].max()
    np.testing.assert_allclose(f, g["f"], rtol=1e-12)
    np.testing.assert_allclose(ts, g["timeserie"], atol=1e-6 * np.abs(g["timeserie"]).max())


@pytest.mark.parametrize("nperseg", [64, 128, 63, 512])
def test_welch_restatement_equals_scipy_csd(nperseg):
    sig = pytest.importorskip("scipy.signal")
    x = SO.make_cube(300, 1, 1, seed=11)[:, 0, 0].astype(np.float64)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)             # nperseg = 512 is greater than input length
        f1, P1 = sig.csd(x, x, 12.5, nperseg=nperseg)
    f2, P2 = SO.welch(x, 12.5, nperseg)
    assert P1.shape == P2.shape
    np.testing.assert_allclose(P2, np.real(P1), rtol=1e-10, atol=1e-14 * P2.max())
    np.testing.assert_allclose(f2, f1, rtol=1e-12)


def test_hann_restatement_equals_scipy():
    win = pytest.importorskip("scipy.signal.windows")
    from wass_amd.postproc import _hann
    for n in (1, 2, 4, 22, 83, 84, 683, 684):
        assert np.array_equal(SO.hann(n), win.hann(n)) and np.array_equal(_hann(n), win.hann(n))
        assert np.array_equal(SO.hann(n, sym=False), win.hann(n, sym=False))


def test_axis_lengths_of_the_two_golden_shapes():
    from wass_amd.postproc import spectrum3d_plan
    p = spectrum3d_plan((40, 120, 126), 0.25, 0.1)
    assert (p.nt, p.ny, p.nx, len(p.starts)) == (4, 81, 81, 19) and (p.r0, p.c0) == (0, 23)
    p = spectrum3d_plan((40, 123, 130), 0.1, 0.1)
    assert (p.nt, p.ny, p.nx) == (4, 84, 84)                      # the nominal crop is 83
    assert SO.axes3d(40, 123, 130, 0.1, 0.1)["Nx"] == 83
    assert spectrum3d_plan((40, 123, 130), 0.2, 0.1).nx == 84 and spectrum3d_plan((40, 135, 140), 1 / 3, 0.1).nx == 92
    assert spectrum3d_plan((40, 1024, 1024), 0.2, 0.1).nx == 684


def test_segment_counts():
    from wass_amd.postproc import spectrum3d_plan
    for count, nt, nseg in ((200, 20, 19), (400, 40, 19), (210, 22, 18), (130, 14, 17), (1000, 100, 19), (30, 4, 14), (39, 4, 18)):
        p = spectrum3d_plan((count, 150, 160), 0.2, 0.1)
        assert (p.nt, len(p.starts)) == (nt, nseg) and p.starts[1] == nt // 2
        a = SO.axes3d(count, 150, 160, 0.2, 0.1)
        assert a["Nt"] == nt and len(a["f"]) == len(p.f)


def test_crop_size_is_the_axis_length_over_a_sweep_of_grids():
    """H from 120 to 1300: the window (and so the crop) is len(kx) x len(ky), which is one longer than the nominal crop on a
    good part of the grid sizes; the plan agrees with the restatement of the reference's expressions everywhere."""
    from wass_amd.postproc import spectrum3d_plan
    longer = 0
    for du in (0.1, 0.2, 0.25, 1 / 3):
        for H in range(120, 1301):
            a = SO.axes3d(40, H, H + 4, du, 0.1)
            if a["r_start"] < 0:
                with pytest.raises(ValueError):
                    spectrum3d_plan((40, H, H + 4), du, 0.1)
                continue
            p = spectrum3d_plan((40, H, H + 4), du, 0.1)
            assert p.nx == len(p.kx) == len(a["kx"]) and p.ny == len(p.ky) == len(a["ky"])
            assert p.nx in (a["Nx"], a["Nx"] + 1) and a["Nx"] % 2 == 1
            assert (p.r0, p.c0) == (a["r_start"], a["c_start"]) and p.r0 + p.ny <= H
            assert p.win_y.shape == (p.ny,) and p.win_x.shape == (p.nx,)
            longer += p.nx != a["Nx"]
    assert longer > 300


def test_plan_scale_equals_the_oracle_factor():
    from wass_amd.postproc import spectrum3d_plan
    p = spectrum3d_plan((210, 123, 130), 0.1, 0.08)
    a = SO._setup3d((210, 123, 130), 0.1, 0.08)
    assert p.scale == pytest.approx(a["K"] / 18, rel=1e-14)


def test_spectrum_statistics_on_a_known_spectrum():
    from wass_amd.postproc import spectrum_statistics
    f = np.linspace(0.0, 2.0, 201)
    S = np.where((f >= 0.5) & (f <= 1.0), 2.0, 0.0)
    S[60] = 3.0                                                   # the peak, at 0.6 Hz
    st = spectrum_statistics(f, S)
    d = np.gradient(f)
    m0, m1 = np.sum(S * d), np.sum(f * S * d)
    assert st["Hm0"] == pytest.approx(4 * np.sqrt(m0)) and st["Tm01"] == pytest.approx(m0 / m1)
    assert st["peak_frequency"] == pytest.approx(0.6) and st["peak_period"] == pytest.approx(1 / 0.6)
    assert 0.98 < m0 < 1.04                                       # a band of 0.5 Hz at density 2


def test_series_block_counts_the_centre_twice():
    from wass_amd.postproc import spectrum_series
    data = np.arange(3 * 41 * 43, dtype=np.float32).reshape(3, 41, 43)
    s = spectrum_series(data, 2)
    assert s.shape == (26, 3) and s.flags.c_contiguous
    assert np.array_equal(s[0], data[:, 20, 21]) and np.array_equal(s[1], data[:, 18, 19]) and np.array_equal(s[13], data[:, 20, 21])
    assert spectrum_series(data, 0).shape == (2, 3)


def test_value_errors():
    from wass_amd import postproc as P
    z = np.zeros((9, 150, 160), np.float32)
    with pytest.raises(ValueError):
        P.compute_3D_spectrum(z, 0.2, 0.1)                        # fewer than 10 frames: segments of length 0
    with pytest.raises(ValueError):
        P.compute_3D_spectrum(np.zeros((29, 150, 160), np.float32), 0.2, 0.1)     # segments of 2 frames: hann(2) is all zero
    with pytest.raises(ValueError):
        P.compute_3D_spectrum(np.zeros((40, 100, 160), np.float32), 0.2, 0.1)     # 50 - 33 - 20 < 0
    with pytest.raises(ValueError):
        P.compute_3D_spectrum(np.zeros((40, 150, 90), np.float32), 0.2, 0.1)      # too narrow for the square crop
    with pytest.raises(ValueError):
        P.compute_3D_spectrum(np.zeros((40, 150, 160), np.float32), 0.0, 0.1)
    with pytest.raises(ValueError):
        P.compute_spectrum(np.zeros((50, 8, 8), np.float32), 0.1, rangespan=5)
    with pytest.raises(ValueError):
        P.compute_spectrum(np.full((50, 20, 20), np.nan, np.float32), 0.1)


def test_scratch_is_stated_and_capped():
    from wass_amd import _lib, build
    build.build()
    lib = _lib.load()
    n = ctypes.c_size_t()
    assert lib.wass_spec3d_scratch_bytes(100, 684, 684, ctypes.byref(n)) == 0
    real = 100 * 684 * 684 * 4
    assert 5.9 * real < n.value < 6.2 * real                     # about six f32 copies of the window: 1.1 GB
    assert lib.wass_spec3d_scratch_bytes(300, 684, 684, ctypes.byref(n)) == 0 and n.value < 3.5e9
    assert lib.wass_spec3d_scratch_bytes(0, 684, 684, ctypes.byref(n)) == -1
    assert lib.wass_spec3d_scratch_bytes(100, 9000, 684, ctypes.byref(n)) == -1
