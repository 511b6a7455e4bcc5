"""The filter design and the filter oracle, without a GPU: wass_amd.postproc.butter_sos against scipy.signal.butter (where scipy
imports) and against its recorded coefficients (always), the numpy restatement of sosfiltfilt (tests/filter_oracle.py) against
scipy.signal.sosfiltfilt and its recorded outputs, the spatial oracle against the recorded outputs of the reference's class,
the stated scratch and the argument errors.  tests/golden/filters.npz comes from tests/golden/make_golden_filters.py."""
import os

import numpy as np
import pytest

import filter_oracle as FO
import spectrum_oracle as SO
from wass_amd import postproc as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FS = 12.0
CUTOFFS = (1.0, 0.3, 0.05, 0.02, 5.9)          # the four of the oracle test and one near Nyquist (6 Hz)
TEMPORAL = {"lp0": ("lowpass", 1.0), "lp1": ("lowpass", 0.3), "hp0": ("highpass", 0.05), "hp1": ("highpass", 0.02)}


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "filters.npz"))


def _same_structure(a, b):
    assert a.shape == b.shape and a.dtype == np.float64
    assert np.array_equal(a == 0, b == 0), "zeros (first-order sections) differ"
    # the same order of the sections: rising pole radius, the gain in section 0
    assert np.array_equal(np.argsort(a[:, 5], kind="stable"), np.argsort(b[:, 5], kind="stable"))
    assert np.array_equal(a[1:, 0], b[1:, 0]) and np.all(a[:, 3] == 1.0)


def _rel(a, b):
    nz = b != 0
    return float(np.max(np.abs(a[nz] - b[nz]) / np.abs(b[nz]))) if nz.any() else 0.0


def test_butter_sos_against_recorded_scipy(golden):
    """The recorded coefficients are scipy's for exactly these arguments; the tolerance per coefficient is the recorded spread of
    scipy's own result between cutoff * (1 -+ 2^-52), plus 4 ulps."""
    assert float(golden["fs"]) == FS and tuple(golden["cutoffs"]) == CUTOFFS
    worst, worst_ratio = 0.0, 0.0
    for order in range(1, 11):
        for bt in ("lowpass", "highpass"):
            for i, fc in enumerate(CUTOFFS):
                a, b = P.butter_sos(order, fc, bt, FS), golden[f"sos_{order}_{bt}_{i}"]
                _same_structure(a, b)
                nz = b != 0
                err = np.abs(a - b)[nz] / np.abs(b[nz])
                tol = golden[f"spread_{order}_{bt}_{i}"][nz] / np.abs(b[nz]) + 4 * 2.0 ** -52
                worst, worst_ratio = max(worst, float(err.max())), max(worst_ratio, float((err / tol).max()))
    print(f"butter_sos against the recorded coefficients: worst relative difference {worst:.3e}, worst difference / (scipy's spread + 4 ulps) "
          f"{worst_ratio:.3f}")
    assert worst_ratio <= 1.0


def test_butter_sos_against_scipy():
    """Against scipy.signal.butter: equal structure; coefficients within scipy's own spread between cutoff * (1 -+ 2^-52) plus 4
    ulps."""
    signal = pytest.importorskip("scipy.signal")
    worst, worst_ratio = 0.0, 0.0
    for order in range(1, 11):
        for bt in ("lowpass", "highpass"):
            for fc in CUTOFFS:
                a = P.butter_sos(order, fc, bt, FS)
                b = signal.butter(order, fc, btype=bt, output="sos", fs=FS)
                _same_structure(a, b)
                lo = signal.butter(order, fc * (1 - 2.0 ** -52), btype=bt, output="sos", fs=FS)
                hi = signal.butter(order, fc * (1 + 2.0 ** -52), btype=bt, output="sos", fs=FS)
                nz = b != 0
                spread = np.maximum(np.abs(lo - b), np.abs(hi - b))[nz] / np.abs(b[nz])
                err = np.abs(a - b)[nz] / np.abs(b[nz])
                tol = spread + 4 * 2.0 ** -52
                worst = max(worst, float(err.max()))
                worst_ratio = max(worst_ratio, float((err / tol).max()))
    print(f"butter_sos against scipy: worst relative difference {worst:.3e}, worst difference / (scipy's spread + 4 ulps) {worst_ratio:.3f}")
    assert worst_ratio <= 1.0


def test_wasspost_filter_sections():
    sos = P.butter_sos(8, 1.0, "lowpass", FS)
    assert sos.shape == (4, 6)
    np.testing.assert_allclose(sos[:, 5], [0.342, 0.413, 0.565, 0.822], atol=5e-4)
    assert np.all(sos[1:, :3] == [1.0, 2.0, 1.0]) and sos[0, 0] < 1e-5
    hp = P.butter_sos(8, 0.05, "highpass", FS)
    assert np.all(hp[1:, :3] == [1.0, -2.0, 1.0]) and np.all(np.diff(hp[:, 5]) > 0)
    odd = P.butter_sos(3, 1.0, "highpass", FS)
    assert odd.shape == (2, 6) and odd[0, 2] == 0 and odd[0, 5] == 0
    with pytest.raises(ValueError):
        P.butter_sos(8, 6.0, "lowpass", FS)
    with pytest.raises(ValueError):
        P.butter_sos(8, 1.0, "bandpass", FS)
    with pytest.raises(ValueError):
        P.butter_sos(0, 1.0, "lowpass", FS)


def test_padlen_and_zi(golden):
    assert P.sos_padlen(P.butter_sos(8, 1.0, "lowpass", FS)) == 27 == FO.padlen(P.butter_sos(8, 1.0, "lowpass", FS))
    for order in range(1, 11):
        for bt in ("lowpass", "highpass"):
            sos = P.butter_sos(order, 0.3, bt, FS)
            want = 3 * (2 * ((order + 1) // 2) + 1 - order % 2)
            assert P.sos_padlen(sos) == FO.padlen(sos) == want
    assert P.sos_padlen(P.butter_sos(7, 1.0, "lowpass", FS)) == 24
    for bt in ("lowpass", "highpass"):
        for i in range(len(CUTOFFS)):
            sos, zi = golden[f"sos_8_{bt}_{i}"], golden[f"zi_{bt}_{i}"]
            # sosfilt_zi solves a 2 x 2 system whose determinant 1 + a1 + a2 cancels for poles near z = 1: relative to that cancellation
            cond = np.max((1 + np.abs(sos[:, 4]) + np.abs(sos[:, 5])) / np.abs(1 + sos[:, 4] + sos[:, 5]))
            for got in (P.sosfilt_zi(sos), FO.sosfilt_zi(sos)):
                assert np.max(np.abs(got - zi)) <= 16 * cond * 2.0 ** -52 * np.max(np.abs(zi))
            assert np.array_equal(P.sosfilt_zi(sos), FO.sosfilt_zi(sos))


def test_too_short_raises_like_scipy():
    sos = P.butter_sos(8, 1.0, "lowpass", FS)
    x = np.zeros((27, 2, 2), np.float32)
    with pytest.raises(ValueError, match="padlen"):
        FO.sosfiltfilt(sos, x)
    with pytest.raises(ValueError, match="padlen"):
        P.sosfiltfilt(sos, x)                      # raised before a context is needed
    with pytest.raises(ValueError):
        P.sosfiltfilt(sos, np.zeros((40, 4), np.float32))
    with pytest.raises(ValueError):
        P.sosfiltfilt(np.ones((2, 5)), np.zeros((40, 2, 2), np.float32))
    bad = sos.copy(); bad[0, 3] = 2.0
    with pytest.raises(ValueError, match="ones"):
        P.sosfiltfilt(bad, np.zeros((40, 2, 2), np.float32))
    with pytest.raises(ValueError):
        P.butterworth_filter(np.zeros((10, 2, 2), np.float32), 0.1)
    with pytest.raises(ValueError):
        P.butterworth_filter(np.zeros((40, 2, 2), np.float32), 0.0)
    with pytest.raises(ValueError):
        P.spatial_lowpass(np.zeros((4, 4), np.float32), 0.2)
    with pytest.raises(ValueError):
        P.Spatial2DButterworth(0, 4, 0.2, 0.5, 4)


def _oracle_case(golden, name):
    c = {k: int(v) for k, v in zip(("count", "H", "W", "seed"), golden["cube"])}
    if name == "hp2":
        return FO.series_cube(**c, offset=5000.0, drift=0.7), P.butter_sos(8, 0.05, "highpass", FS)
    bt, fc = TEMPORAL[name]
    return FO.series_cube(**c), P.butter_sos(8, fc, bt, FS)


@pytest.mark.parametrize("name", ["lp0", "lp1", "hp0", "hp1", "hp2"])
def test_oracle_against_recorded_scipy(golden, name):
    """|oracle64 - scipy| <= 4 n, n = max |oracle64 - oracle_longdouble| on the same input."""
    cube, sos = _oracle_case(golden, name)
    o64, n = FO.noise(sos, cube)
    ref = golden[f"tf_{name}"]
    assert o64.shape == ref.shape and n > 0
    err = float(np.max(np.abs(o64 - ref)))
    print(f"{name}: max |oracle64 - scipy (recorded)| = {err:.3e}, n = {n:.3e}, ratio {err / n:.2f}; max |out| = {np.abs(ref).max():.3e}")
    assert err <= 4 * n


@pytest.mark.parametrize("name", ["lp0", "lp1", "hp0", "hp1"])
def test_oracle_against_scipy(golden, name):
    signal = pytest.importorskip("scipy.signal")
    cube, sos = _oracle_case(golden, name)
    o64, n = FO.noise(sos, cube)
    ref = signal.sosfiltfilt(signal.butter(8, TEMPORAL[name][1], btype=TEMPORAL[name][0], output="sos", fs=FS), cube, axis=0)
    err = float(np.max(np.abs(o64 - ref)))
    print(f"{name}: max |oracle64 - scipy| = {err:.3e}, n = {n:.3e}, ratio {err / n:.2f}")
    assert err <= 4 * n
    # the padding quirk: the same with the padding built in fp64 is off by about a third of a float32 ulp of the largest output
    edge = FO.padlen(sos)
    x = cube.astype(np.float64)
    ext = np.concatenate((2 * x[:1] - x[edge:0:-1], x, 2 * x[-1:] - x[-2:-(edge + 2):-1]), axis=0)
    zi = FO.sosfilt_zi(sos).reshape(sos.shape[0], 2, 1, 1)
    y = FO._sosfilt(sos, ext.copy(), zi * ext[:1])[::-1].copy()
    y = FO._sosfilt(sos, y, zi * y[:1])[::-1][edge:-edge]
    assert np.max(np.abs(y - ref)) > 100 * n


def test_oracle_nan_and_mean():
    sos = P.butter_sos(8, 0.05, "highpass", FS)
    cube = FO.series_cube(80, 2, 3, seed=5, offset=100.0)
    cube[40, 1, 1] = np.nan
    o = FO.sosfiltfilt(sos, cube, remove_mean=True)
    assert np.isnan(o[:, 1, 1]).all() and np.isfinite(np.delete(o.reshape(80, 6), 4, axis=1)).all()
    assert np.max(np.abs(np.delete(o.reshape(80, 6), 4, axis=1).mean(axis=0))) < 1e-12 * np.nanmax(np.abs(o))


@pytest.mark.parametrize("name", ["square", "nonsquare"])
def test_spatial_oracle_against_the_reference_class(golden, name):
    rows, cols, du, cutoff, order, seed = golden[f"sp_{name}_args"]
    rows, cols, order, seed = int(rows), int(cols), int(order), int(seed)
    Hs = FO.transfer_function(rows, cols, du, cutoff, order)
    assert np.array_equal(Hs, golden[f"sp_{name}_H"])
    filt = P.Spatial2DButterworth(rows, cols, du, cutoff, order)          # no GPU is touched before apply
    assert np.array_equal(filt.butterworth_filter, golden[f"sp_{name}_H"])
    surf = SO.make_cube(1, rows, cols, seed=seed)[0]
    ref = golden[f"sp_{name}_out"]
    got = FO.spatial_apply(surf, Hs)
    tol = 64 * 2.0 ** -52 * np.log2(rows * cols) * np.abs(ref).max()      # two fp64 FFT pairs with different factorisations
    err = float(np.max(np.abs(got - ref)))
    print(f"{name}: max |oracle - reference class| = {err:.3e}, tolerance {tol:.3e}, max |out| = {np.abs(ref).max():.3e}")
    assert got.shape == ref.shape == (rows, cols) and err <= tol
    if rows != cols:
        # the transfer function of the swapped arguments (W taken for the columns) is cols x rows: read with the frame's pitch it is
        # far off.  (Its transpose is the right array again: the filter is radial and du is the same on both axes.)
        Ht = FO.transfer_function(cols, rows, du, cutoff, order)
        assert np.array_equal(Ht.T, Hs)
        wrong = FO.spatial_apply(surf, Ht.reshape(rows, cols))
        print(f"{name}: the transfer function of swapped arguments is off by {np.max(np.abs(wrong - ref)):.3e}")
        assert np.max(np.abs(wrong - ref)) > 1e6 * tol
    else:
        assert np.array_equal(FO.transfer_function(cols, rows, du, cutoff, order).T, Hs)     # ... and hides on a square grid


def test_spatial_lowpass_cutoff():
    """spatial_lowpass's filter at cutoffs where f and f^2 differ: the reference's formula, its argument order and order 4."""
    for hz in (0.7, 1.0, 1.6):
        fc = 2.0 * np.pi * hz ** 2 / 9.81          # the reference's expression
        filt = P.spatial_lowpass_filter(30, 44, 0.2, cutoff_in_hz=hz)           # no GPU is touched before apply
        Hs = filt.butterworth_filter
        assert Hs.shape == (30, 44) and np.array_equal(Hs, FO.transfer_function(30, 44, 0.2, fc, 4))
        assert Hs[15, 22] == 1.0 and Hs.max() == 1.0 and Hs.min() > 0
        # half power at the cutoff, along the columns' axis: bin j of 44 columns is j / (44 * 0.2) cycles per metre
        f_col = np.fft.fftshift(np.fft.fftfreq(44, d=0.2))
        j = int(np.argmin(np.abs(f_col - fc)))
        assert Hs[15, j] == pytest.approx(1.0 / np.sqrt(1.0 + (f_col[j] / fc) ** 8), rel=1e-12)
        # even: H(-k) = H(k) where both exist
        assert np.array_equal(Hs[1:, 1:], Hs[1:, 1:][::-1, ::-1])
    assert not np.array_equal(P.spatial_lowpass_filter(30, 44, 0.2, 0.7).butterworth_filter, P.spatial_lowpass_filter(30, 44, 0.2, 0.7 ** 0.5).butterworth_filter)


def test_stated_scratch():
    from wass_amd import build
    build.build()
    b, rows = P.sosfiltfilt_scratch_bytes(600, 257, 64, 27)
    al = lambda v: (v + 255) // 256 * 256
    assert rows == 257 and b == al(654 * 257 * 64 * 8) + al(600 * 257 * 64 * 4)
    b, rows = P.sosfiltfilt_scratch_bytes(600, 257, 64, 27, slab_rows=100, host=False)
    assert rows == 100 and b == al(654 * 100 * 64 * 8)
    # 1000 x 1024 x 1024 from device memory: one slab, 8.8 GB; 3000 frames: slabs
    b, rows = P.sosfiltfilt_scratch_bytes(1000, 1024, 1024, 27, host=False)
    assert rows == 1024 and b == 1054 * 1024 * 1024 * 8
    b, rows = P.sosfiltfilt_scratch_bytes(3000, 1024, 1024, 27, host=True)
    assert 1 <= rows < 1024 and b <= 16 << 30 and (rows + 1) * (3054 * 1024 * 8 + 3000 * 1024 * 4) > (16 << 30) - 512
    with pytest.raises(ValueError):
        P.sosfiltfilt_scratch_bytes(27, 8, 8, 27)
    with pytest.raises(ValueError):
        P.sosfiltfilt_scratch_bytes(100, 0, 8, 27)
    from wass_amd import _lib
    import ctypes as C
    n = C.c_size_t()
    assert _lib.load().wass_spatial_filter_scratch_bytes(1024, 1024, 16, C.byref(n)) == 0
    assert 16 * 1024 * 1024 * 4 * 4 < n.value < 16 * 1024 * 1024 * 4 * 5
    assert _lib.load().wass_spatial_filter_scratch_bytes(0, 1024, 16, C.byref(n)) != 0


def test_postproc_does_not_import_scipy():
    txt = open(os.path.join(ROOT, "wass_amd", "postproc.py")).read()
    assert "import scipy" not in txt and "from scipy" not in txt
