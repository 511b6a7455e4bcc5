"""wass_amd.postproc's Butterworth filters on the GPU against the fp64 restatements of tests/filter_oracle.py.

Temporal, element-wise, no exempt elements: |gpu_f32 - oracle64| <= 0.5 ulp_f32(|oracle64|) + 4 n, where n = the largest
|oracle64 - oracle_longdouble| of the case (the recurrence's own fp64 noise, measured from the oracle alone): the first term is
the output cast, the second allows for any re-association of the three-term updates; and, beyond that bound, the bits of the rounded
oracle (every kernel instance, the short series and the probes that tell a subtly wrong update are in tests/test_filter_edges_gpu.py).  Spatial: the Frobenius norm of a frame's error (and so
every element's) within filter_oracle.spatial_bound, a 2-norm bound that carries the inverse's 1 / (rows cols); every shape also
shows that an output of zeros, the unfiltered frame, four times the cutoff and a shifted or swapped transfer function miss that
bound by far.
Every test prints its largest error in units of the bound before it asserts."""
import os

import numpy as np
import pytest

import filter_oracle as FO
import spectrum_oracle as SO
import wass_amd
from wass_amd import postproc as P

pytestmark = pytest.mark.gpu

FS = 12.0


def _check_temporal(got, sos, cube, remove_mean=False, what=""):
    o64, n = FO.noise(sos, cube, remove_mean)
    assert got.shape == o64.shape and got.dtype == np.float32
    nan = np.isnan(o64)
    assert np.array_equal(np.isnan(got), nan), "NaN pattern"
    bound = FO.temporal_bound(o64, n)
    err = np.abs(got.astype(np.float64) - o64)
    ok = ~nan
    worst = float(np.max(err[ok] / bound[ok])) if ok.any() else 0.0
    exact = float(np.mean(got[ok] == o64[ok].astype(np.float32))) if ok.any() else 1.0
    print(f"{what}: n = {n:.3e}, max |out| = {np.nanmax(np.abs(o64)):.3e}, largest error / bound = {worst:.4f}, "
          f"equal to the rounded oracle in {100 * exact:.4f} % of the elements")
    assert worst <= 1.0
    # the kernel's contract is stronger than the bound: scipy's order of operations in fp64, nothing contracted, the padding rounded
    # in float32, so the result is the oracle's, rounded (tests/test_filter_edges_gpu.py holds every instance to that at short series)
    assert np.array_equal(got, o64.astype(np.float32), equal_nan=True)
    return o64, n


FILTERS = {"lp1.0": (8, 1.0, "lowpass"), "hp0.05": (8, 0.05, "highpass"), "lp0.02": (8, 0.02, "lowpass"), "hp0.02": (8, 0.02, "highpass"),
           "odd7": (7, 0.5, "lowpass"), "odd3hp": (3, 0.1, "highpass")}


@pytest.mark.parametrize("name", list(FILTERS))
def test_filters_at_600_frames(gpu_ctx, name):
    order, fc, bt = FILTERS[name]
    sos = P.butter_sos(order, fc, bt, FS)
    cube = FO.series_cube(600, 37, 53, seed=order + len(name), offset=40.0)
    _check_temporal(P.sosfiltfilt(sos, cube, ctx=gpu_ctx), sos, cube, what=f"{name} 600 x 37 x 53")


@pytest.mark.parametrize("shape", [(28, 5, 300), (600, 1, 1), (1500, 5, 300), (600, 257, 64), (100, 512, 512)])
@pytest.mark.parametrize("bt,fc", [("lowpass", 1.0), ("highpass", 0.05)])
def test_shapes(gpu_ctx, shape, bt, fc):
    """count = padlen + 1 = 28, 600, 1500 (and 100 on the large grid, to keep the long-double oracle short)."""
    sos = P.butter_sos(8, fc, bt, FS)
    assert P.sos_padlen(sos) == 27
    cube = FO.series_cube(*shape, seed=shape[0] + shape[2], offset=-15.0)
    _check_temporal(P.sosfiltfilt(sos, cube, ctx=gpu_ctx), sos, cube, what=f"{bt} {fc} {shape}")


def test_too_short(gpu_ctx):
    sos = P.butter_sos(8, 1.0, "lowpass", FS)
    with pytest.raises(ValueError, match="padlen"):
        P.sosfiltfilt(sos, np.zeros((27, 4, 4), np.float32), ctx=gpu_ctx)
    zi = P.sosfilt_zi(sos)
    x = np.zeros((27, 4, 4), np.float32)
    rc = gpu_ctx._lib.wass_sosfiltfilt(gpu_ctx._h, x.ctypes.data, 16, 4, 27, 4, 4, sos.ctypes.data, 4, zi.ctypes.data, 27, 0, 0, x.ctypes.data, 16, 4)
    assert rc != 0


def test_slabs_views_device_and_repeats(gpu_ctx, tmp_path):
    import torch
    sos = P.butter_sos(8, 0.05, "highpass", FS)
    cube = FO.series_cube(120, 37, 53, seed=77, offset=900.0, drift=0.3)
    for rm in (False, True):
        one = P.sosfiltfilt(sos, cube, remove_mean=rm, ctx=gpu_ctx)
        _check_temporal(one, sos, cube, rm, what=f"one slab, remove_mean {rm}")
        assert P.sosfiltfilt_scratch_bytes(120, 37, 53, 27, slab_rows=5)[1] == 5         # 7 slabs of 5 rows and a ragged one of 2
        for rows in (5, 1, 36):
            assert P.sosfiltfilt(sos, cube, remove_mean=rm, ctx=gpu_ctx, slab_rows=rows).tobytes() == one.tobytes()
        assert P.sosfiltfilt(sos, cube, remove_mean=rm, ctx=gpu_ctx).tobytes() == one.tobytes()            # repeat
        big = np.full((120, 40, 60), np.float32(7.0))
        big[:, 2:39, 4:57] = cube
        view = big[:, 2:39, 4:57]
        assert not view.flags.c_contiguous
        assert P.sosfiltfilt(sos, view, remove_mean=rm, ctx=gpu_ctx).tobytes() == one.tobytes()
        mm = np.memmap(tmp_path / f"cube{int(rm)}.f32", np.float32, "w+", shape=cube.shape)
        mm[:] = cube
        mm.flush()
        out_mm = np.memmap(tmp_path / f"out{int(rm)}.f32", np.float32, "w+", shape=cube.shape)
        assert P.sosfiltfilt(sos, mm, remove_mean=rm, ctx=gpu_ctx, out=out_mm) is out_mm
        assert np.asarray(out_mm).tobytes() == one.tobytes()
        d = torch.from_numpy(big).to(f"cuda:{gpu_ctx.device_id}")
        dv = d[:, 2:39, 4:57]
        got = P.sosfiltfilt(sos, dv, remove_mean=rm, ctx=gpu_ctx, slab_rows=9)
        assert got.cpu().numpy().tobytes() == one.tobytes()
        assert P.sosfiltfilt(sos, dv, remove_mean=rm, ctx=gpu_ctx, out=dv) is dv                            # in place, strided
        back = d.cpu().numpy()
        assert back[:, 2:39, 4:57].tobytes() == one.tobytes()
        back[:, 2:39, 4:57] = 7.0
        assert (back == 7.0).all()                                                                          # nothing outside the view


def test_nan_series(gpu_ctx):
    sos = P.butter_sos(8, 1.0, "lowpass", FS)
    clean = FO.series_cube(90, 9, 70, seed=5)
    base = P.sosfiltfilt(sos, clean, ctx=gpu_ctx)
    cube = clean.copy()
    cube[0, 0, 0] = cube[89, 8, 69] = cube[45, 3, 33] = cube[1, 4, 64] = np.nan
    cube[10:20, 5, 5] = np.nan
    for rm in (False, True):
        got = P.sosfiltfilt(sos, cube, remove_mean=rm, ctx=gpu_ctx)
        _check_temporal(got, sos, cube, rm, what=f"NaN series, remove_mean {rm}")
        bad = np.isnan(cube).any(axis=0)
        assert bad.sum() == 5 and np.isnan(got[:, bad]).all()
        want = base if not rm else P.sosfiltfilt(sos, clean, remove_mean=True, ctx=gpu_ctx)
        assert got[:, ~bad].tobytes() == want[:, ~bad].tobytes()


def test_remove_mean_and_constant(gpu_ctx):
    hp = P.butter_sos(8, 0.05, "highpass", FS)
    cube = FO.series_cube(600, 5, 300, seed=12, offset=5000.0, drift=0.7)
    got = P.butterworth_filter(cube, 1 / FS, cutoff=0.05, type="highpass", ctx=gpu_ctx)
    _check_temporal(got, hp, cube, True, what="wasspost filter --highpass (mean removed)")
    fast = P.butterworth_filter(cube, 1 / 12.3, cutoff=0.05, type="highpass", fast=True, ctx=gpu_ctx)
    _check_temporal(fast, hp, cube, False, what="filter_fast: fs rounded to 12, mean kept")
    low = P.butterworth_filter(cube, 1 / FS, ctx=gpu_ctx)
    _check_temporal(low, P.butter_sos(8, 1.0, "lowpass", FS), cube, False, what="wasspost filter (low-pass 1 Hz)")
    lowm = P.sosfiltfilt(P.butter_sos(8, 1.0, "lowpass", FS), cube, remove_mean=True, ctx=gpu_ctx)
    _check_temporal(lowm, P.butter_sos(8, 1.0, "lowpass", FS), cube, True, what="low-pass with a large mean removed")
    # a constant through the high-pass: 0 within the absolute part of the bound
    const = np.full((600, 3, 70), np.float32(1234.5))
    for rm in (False, True):
        out = P.sosfiltfilt(hp, const, remove_mean=rm, ctx=gpu_ctx)
        o64, n = _check_temporal(out, hp, const, rm, what=f"constant 1234.5 through the high-pass, remove_mean {rm}")
        assert np.max(np.abs(out)) <= np.max(np.abs(o64)) + np.max(FO.temporal_bound(o64, n))
        print(f"   largest |output| {np.max(np.abs(out)):.3e}")
        assert np.max(np.abs(out)) < 1e-6


# ---- the spatial filter ------------------------------------------------------------------------------------------------------------
SPATIAL_WAVES = ((300.0, 0.0, 0.03, 0.02, 0.3), (250.0, 0.0, 0.21, -0.17, 1.1), (150.0, 0.0, -0.05, 0.11, 2.0))   # long, short, near the cutoff


def _fro(a):
    return float(np.sqrt(np.sum(np.asarray(a, np.float64) ** 2)))


def _check_spatial(got, frames, Hs, what=""):
    """||got - oracle||_F <= spatial_bound per frame; returns the oracle's frames."""
    assert got.shape == frames.shape and got.dtype == np.float32
    worst, rel, refs = 0.0, 0.0, []
    for g, x in zip(got, frames):
        ref = FO.spatial_apply(x, Hs)
        refs.append(ref)
        err = g.astype(np.float64) - ref
        worst = max(worst, _fro(err) / FO.spatial_bound(x))
        rel = max(rel, float(np.max(np.abs(err))) / float(np.abs(ref).max()))
    print(f"{what}: largest ||error||_F / bound = {worst:.3e}; largest |error| / max |out| = {rel:.3e}")
    assert worst <= 1.0
    return refs


def _wrong_answers_miss(x, ref, rows, cols, du, fc, order, what=""):
    """What a broken filter would return misses the bound by far: the check above can fail."""
    B = FO.spatial_bound(x)
    Hs = FO.transfer_function(rows, cols, du, fc, order)
    wrong = {"zeros": np.zeros_like(ref), "unfiltered": x.astype(np.float64),
             "4 x cutoff": FO.spatial_apply(x, FO.transfer_function(rows, cols, du, 4 * fc, order)),
             "H not un-shifted": FO.spatial_apply(x, np.fft.ifftshift(Hs))}
    if rows != cols:
        wrong["H of swapped arguments"] = FO.spatial_apply(x, FO.transfer_function(cols, rows, du, fc, order).reshape(rows, cols))
    ratios = {k: _fro(v - ref) / B for k, v in wrong.items()}
    print(f"{what}: ||wrong - oracle||_F / bound: " + ", ".join(f"{k} {v:.1f}" for k, v in ratios.items()))
    assert min(ratios.values()) >= 5.0


@pytest.mark.parametrize("rows,cols,n", [(64, 64, 3), (333, 257, 3), (683, 684, 2), (1024, 1024, 2)])
def test_spatial_shapes(gpu_ctx, rows, cols, n):
    du, hz = 0.2, (1.0 if rows != 333 else 0.9)
    frames = SO.make_cube(n, rows, cols, seed=rows + cols, offset=500.0, waves=SPATIAL_WAVES)
    fc = 2.0 * np.pi * hz ** 2 / 9.81
    got = P.spatial_lowpass(frames, du, cutoff_in_hz=hz, ctx=gpu_ctx, batch=2)
    Hs = FO.transfer_function(rows, cols, du, fc, 4)
    refs = _check_spatial(got, frames, Hs, what=f"spatial_lowpass {rows} x {cols}, {hz} Hz")
    _wrong_answers_miss(frames[0], refs[0], rows, cols, du, fc, 4, what=f"{rows} x {cols}")
    # the mean is the DC coefficient, H(0) = 1: |mean error| <= ||error||_F / sqrt(N) (Cauchy-Schwarz); the offset is 500
    for g, x in zip(got, frames):
        tol = FO.spatial_bound(x) / np.sqrt(rows * cols)
        assert tol < 50.0 and abs(float(g.astype(np.float64).mean()) - float(x.astype(np.float64).mean())) <= tol
    filt = P.Spatial2DButterworth(rows, cols, du, fc, 4, ctx=gpu_ctx)
    one = filt.apply(frames[1])
    assert one.shape == (rows, cols) and one.tobytes() == got[1].tobytes()            # apply == apply_batch, whatever the batch
    assert filt.apply_batch(frames).tobytes() == got.tobytes()
    filt.close()


def test_on_bin_cosine_non_square(gpu_ctx):
    """cos at bin (p, q), p != q, rows != cols: comes back scaled by H(p, q).  No oracle: axes and shift by themselves."""
    rows, cols, p, q, du, A = 48, 80, 3, 11, 0.25, 100.0
    r, c = np.arange(rows)[:, None], np.arange(cols)[None, :]
    x = (A * np.cos(2 * np.pi * (p * r / rows + q * c / cols) + 0.3)).astype(np.float32)
    R = lambda a, b: np.hypot(a / (rows * du), b / (cols * du))                       # cycles per metre of bin (a, b)
    fcut = R(p, q) * 1.05
    h = lambda a, b: 1.0 / np.sqrt(1.0 + (R(a, b) / fcut) ** 8)
    filt = P.Spatial2DButterworth(rows, cols, du, fcut, 4, ctx=gpu_ctx)
    got = filt.apply(x).astype(np.float64)
    bound = FO.spatial_bound(x)
    err = _fro(got - h(p, q) * x.astype(np.float64))
    print(f"on-bin cosine: H(p, q) = {h(p, q):.4f}, H(q, p) = {h(q, p):.4f}, ||error||_F {err:.3e}, bound {bound:.3e}, ||x||_F {_fro(x):.3e}")
    assert err <= bound
    # the bound separates the right answer from the swapped axes
    assert abs(h(p, q) - h(q, p)) * _fro(x) > 20 * bound
    filt.close()


def test_spatial_nan_frame_device_and_repeats(gpu_ctx):
    import torch
    rows, cols = 123, 130
    frames = SO.make_cube(7, rows, cols, seed=3)
    filt = P.Spatial2DButterworth(rows, cols, 0.2, 0.5, 4, ctx=gpu_ctx, batch=3)
    base = filt.apply_batch(frames)
    assert filt.apply_batch(frames).tobytes() == base.tobytes()
    bad = frames.copy()
    bad[4, 77, 5] = np.nan
    got = filt.apply_batch(bad)
    assert np.isnan(got[4]).all()
    keep = [0, 1, 2, 3, 5, 6]
    assert got[keep].tobytes() == base[keep].tobytes()
    d = torch.from_numpy(frames).to(f"cuda:{gpu_ctx.device_id}")
    assert filt.apply_batch(d).cpu().numpy().tobytes() == base.tobytes()
    pad = torch.zeros((7, rows + 3, cols + 5), dtype=torch.float32, device=d.device)
    pad[:, 1:1 + rows, 2:2 + cols] = d
    view = pad[:, 1:1 + rows, 2:2 + cols]
    assert filt.apply_batch(view, out=view) is view
    assert view.cpu().numpy().tobytes() == base.tobytes()
    filt.close()


# ---- end to end ------------------------------------------------------------------------------------------------------------------------
def test_grid_sequence_through_both_filters_into_the_spectrum(gpu_ctx, oracle, tmp_path):
    """GridSequenceResult.Z -> butterworth_filter -> spatial_lowpass -> compute_spectrum; every stage against its oracle on the
    stage's own input, so that each bound stays the stage's own."""
    from test_grid_seq_gpu import _sequence_on_disk
    from wass_amd.gridding import grid_sequence
    plane = np.array([0.02, 0.81, 0.586, -11.0]); plane[:3] /= np.linalg.norm(plane[:3])
    dirs = _sequence_on_disk(tmp_path, oracle, 30, plane)
    R, T, _, _ = wass_amd.RT_from_plane(plane)
    W, H = 132, 126
    setup = {"Rpl": R, "Tpl": T.reshape(3, 1), "CAM_BASELINE": np.array([[2.5]]), "xmin": np.array([[-12.0]]), "xmax": np.array([[12.0]]),
             "ymin": np.array([[-30.0]]), "ymax": np.array([[-5.0]]), "XX": np.zeros((H, W)), "fps": np.array([[12.5]])}
    res = grid_sequence(dirs, setup, alg_options={"Nfreqs": 30, "MAX_ITERS": 60}, force_zero_mean=True, batch=8, ctx=gpu_ctx)
    Z = res.Z
    assert Z.shape == (30, H, W) and np.isfinite(Z).all()
    dt, du = 1 / 12.5, 24.0 / W
    Zf = P.butterworth_filter(Z, dt, cutoff=1.0, ctx=gpu_ctx)
    _check_temporal(Zf, P.butter_sos(8, 1.0, "lowpass", 12.5), np.asarray(Z, np.float32), what="grid_sequence cube, low-pass 1 Hz")
    Zs = P.spatial_lowpass(Zf, du, cutoff_in_hz=0.7, ctx=gpu_ctx)
    refs = _check_spatial(Zs, Zf, FO.transfer_function(H, W, du, 2.0 * np.pi * 0.7 ** 2 / 9.81, 4), what="... spatial_lowpass at 0.7 Hz")
    B = FO.spatial_bound(Zf[0])
    print(f"... ||unfiltered - oracle||_F / bound = {_fro(Zf[0] - refs[0]) / B:.1f}, ||oracle||_F / bound = {_fro(refs[0]) / B:.1f}")
    assert _fro(Zf[0] - refs[0]) >= 5 * B
    f, S1, _ = P.compute_spectrum(Zs, dt, nperseg=16, rangespan=2, scale=0.001, ctx=gpu_ctx)
    S1r = SO.compute_spectrum(Zs, dt, nperseg=16, rangespan=2, scale=0.001)[1]
    assert S1.max() > 0 and np.max(np.abs(S1 - S1r)) <= 1e-5 * S1r.max()


def test_hm0_of_a_high_passed_sea(gpu_ctx):
    """A 0.75 m sinusoid at 0.625 Hz on a 3 m swing at 0.004 Hz and a 5 m offset (millimetres): the high-pass at 0.05 Hz leaves the
    wave.  Hm0 of the GPU chain against Hm0 of the oracle chain within the propagated bound: the filtered amplitudes differ by at
    most max(bound) (Hm0 is 4 times an rms amplitude, scale 1 / 1000), and compute_spectrum's own check allows 1e-5 of the peak
    per bin."""
    a, dt = 0.75, 0.1
    waves = ((1000.0 * a, 0.0625, 0.01, 0.02, 0.4), (3000.0, 0.0004, 0.0, 0.0, 1.0))
    cube = SO.make_cube(2048, 24, 24, noise=0.0, waves=waves, offset=5000.0)
    hp = P.butter_sos(8, 0.05, "highpass", 1 / dt)
    got = P.butterworth_filter(cube, dt, cutoff=0.05, type="highpass", ctx=gpu_ctx)
    o64, n = _check_temporal(got, hp, cube, True, what="synthetic sea, high-pass 0.05 Hz")
    f, S, _ = P.compute_spectrum(got, dt, nperseg=512, rangespan=5, scale=0.001, ctx=gpu_ctx)
    fr, Sr, _ = SO.compute_spectrum(o64.astype(np.float32), dt, nperseg=512, rangespan=5, scale=0.001)
    st, sr = P.spectrum_statistics(f, S), P.spectrum_statistics(fr, Sr)
    m0 = (sr["Hm0"] / 4.0) ** 2
    dm0 = 1e-5 * Sr.max() * float(np.sum(np.gradient(fr)))
    tol = 4.0 * 0.001 * float(np.max(FO.temporal_bound(o64, n))) + 4.0 * dm0 / (2.0 * np.sqrt(m0))
    print(f"Hm0 {st['Hm0']:.6f} (GPU chain), {sr['Hm0']:.6f} (oracle chain), difference {abs(st['Hm0'] - sr['Hm0']):.3e}, bound {tol:.3e}; "
          f"expected {4 * a / np.sqrt(2):.5f}; unfiltered the estimate is {P.spectrum_statistics(*SO.compute_spectrum(cube, dt, 512, 5, 0.001)[:2])['Hm0']:.3f}")
    assert abs(st["Hm0"] - sr["Hm0"]) <= tol
    assert st["Hm0"] == pytest.approx(4 * a / np.sqrt(2), rel=0.01)
    assert st["peak_frequency"] == pytest.approx(0.625, abs=1e-9)
