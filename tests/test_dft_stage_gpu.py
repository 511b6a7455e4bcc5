"""k_dft_stage of wass_amd/csrc/spectrum.hip on the GPU, through its three callers, at the shapes of tests/dft_oracle.py: every
kernel instance, one and several tiles in M and N, ragged edges in M, N and K, axes of length 1 and 2.

  probes   windows that are 0 except at one or two positions per axis leave at most eight cells of a small-integer cube: the
           prepared segment is known exactly, the expected |X|^2 is a direct fp64 sum, and the bound (dft_oracle.probe_bound)
           has a constant that does not grow with the axis lengths
  dense    element-wise with spectrum_oracle.bound3d's formula, per 64 x 64 tile (dft_oracle.TILE_MARGIN), Parseval, the sum of
           two segments
  Welch    the existing 1e-5 of the peak and a derived element-wise bound (dft_oracle.welch_tolerance)
  spatial  filter_oracle.spatial_bound per frame and per tile, injected transfer functions, delta frames
tests/test_dft_stage.py shows on the CPU that each of these checks fails for a model with one thing broken.  Every test prints
its worst error in units of its bound before it asserts."""
import numpy as np
import pytest

import dft_oracle as D
import filter_oracle as FO
import spectrum_oracle as SO
from wass_amd import postproc as P

pytestmark = pytest.mark.gpu

ids = lambda c: "x".join(str(v) for v in c)


def _dev(ctx, a):
    import torch
    d = torch.from_numpy(np.ascontiguousarray(a)).to(f"cuda:{ctx.device_id}")
    torch.cuda.synchronize()
    return d


# ---- a. probes ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", D.CASES_3D, ids=ids)
def test_probes_3d(gpu_ctx, case):
    nt, ny, nx = case
    cube = D.probe_cube(*case)
    a, b = D.mirror_pairs(*case)
    worst = 0.0
    for pr in D.probes(*case):
        cells = D.probe_cells(pr, cube)
        ref, e2 = D.probe_expected(cells, *case), D.probe_bound(cells)
        with P.Spectrum3D(gpu_ctx, nt, ny, nx, *D.probe_windows(pr, *case)) as sp:
            sp.push(cube)
            S, n, flag = sp.finish(1.0)
        r = D.ratio(np.abs(S - ref), D.tol_of(ref, e2)) if S.shape == case else np.inf
        print(f"{case} probe {pr}: {len(cells)} cells, peak {ref.max():.4g}, largest error / bound = {r:.4f}, n {n}, flag {flag}")
        worst = max(worst, r)
        assert n == 1 and not flag and S.shape == case and np.isfinite(S).all()
        assert r <= 1.0, pr
        assert S.ravel()[a].tobytes() == S.ravel()[b].tobytes(), pr         # both halves of kx read the same stored coefficient
    print(f"{case}: worst probe error / bound = {worst:.4f}")


# ---- b. dense segments ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", D.CASES_3D, ids=ids)
def test_dense_3d(gpu_ctx, case):
    nt, ny, nx = case
    wins = D.dense_windows(*case)
    cube, view = D.dense_cube_3d(case)
    cube2, view2 = D.dense_cube_3d(case, seed=1)
    refs = []
    for v in (view, view2):
        prep, flag = D.prepare3d(v, *wins)
        xw = prep.astype(np.float64)
        ref = np.fft.fftshift(np.abs(np.fft.fftn(xw)) ** 2)
        refs.append((xw, ref, D.tol_of(ref, D.bound3d_e2(xw)), flag))
    d = _dev(gpu_ctx, cube)
    with P.Spectrum3D(gpu_ctx, nt, ny, nx, *wins) as sp:
        sp.push(view)
        S, n, flag = sp.finish(1.0)
        sp.push_dev(d[:, 2:2 + ny, 3:3 + nx])
        Sd, nd, flagd = sp.finish(1.0)
        sp.push(view2)
        S2, _, flag2 = sp.finish(1.0)
        sp.push(view)
        sp.push(view2)
        S12, n12, flag12 = sp.finish(1.0)
    xw, ref, tol, want_flag = refs[0]
    assert S.shape == case
    el = D.ratio(np.abs(S - ref), tol)
    te, ntiles = D.tile_errors(S, ref)
    tl = D.ratio(te.max(), D.tile_limit(float(np.linalg.norm(tol)), ntiles, "3d"))
    want = float((xw * xw).sum()) * xw.size
    pv = D.ratio(abs(float(S.sum()) - want), (nx + ny + nt + 6) * 2.0 ** -23 * want)
    both = D.ratio(np.abs(S12 - (ref + refs[1][1])), tol + refs[1][2])
    print(f"{case}: element-wise error / bound = {el:.4f}, worst of {ntiles} tiles / its limit = {tl:.4f}, Parseval / bound = {pv:.4f}, "
          f"two segments / bound = {both:.4f}; host and device pushes {'equal' if Sd.tobytes() == S.tobytes() else 'DIFFER'}, segments {n} {nd} {n12}, "
          f"flags {flag} {flagd} {flag2} {flag12} (expected {want_flag} {want_flag} {refs[1][3]} {want_flag or refs[1][3]})")
    assert n == 1 and nd == 1 and n12 == 2 and Sd.tobytes() == S.tobytes()
    assert flag == flagd == want_flag and flag2 == refs[1][3] and flag12 == (flag or flag2)
    assert np.isfinite(S).all()
    assert el <= 1.0 and tl <= 1.0 and pv <= 1.0 and both <= 1.0
    assert D.ratio(np.abs(S2 - refs[1][1]), refs[1][2]) <= 1.0
    assert S12.tobytes() == (S + S2).tobytes()                            # += in the order of the pushes; finish starts the handle over
    a, b = D.mirror_pairs(*case)
    assert S12.ravel()[a].tobytes() == S12.ravel()[b].tobytes()


# ---- c. the 1-D Welch estimate --------------------------------------------------------------------------------------------------
def _welch_case(ctx, cube, nperseg, rangespan, what):
    dt, scale = 0.1, D.WELCH_SCALE
    f, S, ts = P.compute_spectrum(cube, dt, nperseg=nperseg, rangespan=rangespan, scale=scale, ctx=ctx)
    fr, Sr, tsr = SO.compute_spectrum(cube, dt, nperseg=nperseg, rangespan=rangespan, scale=scale)
    series = P.spectrum_series(cube, rangespan).astype(np.float64) * scale
    tol = D.welch_tolerance(D.staged_welch(series, 1.0 / dt, nperseg), 1.0 / dt, nperseg, cube.shape[0])
    assert S.shape == Sr.shape == (min(nperseg, cube.shape[0]) // 2 + 1,) and S.dtype == np.float64
    flat = float(np.max(np.abs(S - Sr)) / Sr.max())
    el = D.ratio(np.abs(S - Sr), tol)
    print(f"{what}: max error / peak = {flat:.3e}, element-wise error / bound = {el:.4f}")
    assert np.isfinite(S).all() and flat <= 1e-5
    assert el <= 1.0
    assert np.array_equal(f, fr)
    np.testing.assert_allclose(ts, tsr, atol=1e-6 * np.abs(tsr).max())
    S2 = P.compute_spectrum(cube, dt, nperseg=nperseg, rangespan=rangespan, scale=scale, ctx=ctx)[1]
    assert S2.tobytes() == S.tobytes()
    return S, Sr, tol


@pytest.mark.parametrize("case", D.CASES_WELCH, ids=ids)
def test_welch(gpu_ctx, case):
    n_samples, nperseg, rangespan = case
    cube = SO.make_cube(n_samples, *D.WELCH_GRID, seed=n_samples + nperseg)
    _welch_case(gpu_ctx, cube, nperseg, rangespan, f"compute_spectrum {case}")
    # all of every series' first segment in its last sample: the last k tile, whatever the window leaves of it elsewhere
    _welch_case(gpu_ctx, D.impulse_cube(n_samples, nperseg), nperseg, rangespan, f"compute_spectrum {case}, impulse at frame nps - 1")


@pytest.mark.parametrize("nps", [48, 49])
def test_welch_on_bin_sinusoid(gpu_ctx, nps):
    """p cycles per segment, no noise: with the periodic Hann window the exact spectrum is 0 more than one bin from p."""
    p = 5
    cube = SO.make_cube(200, *D.WELCH_GRID, noise=0.0, waves=((300.0, p / nps, 0.01, 0.02, 0.4),))
    S, Sr, tol = _welch_case(gpu_ctx, cube, nps, 1, f"on-bin sinusoid, nps {nps}")
    out = np.abs(np.arange(S.size) - p) > 2
    print(f"   largest bin outside the lobe {S[out].max():.3e}, its bound {tol[out][np.argmax(S[out])]:.3e}, peak {S.max():.3e}")
    assert int(np.argmax(S)) == p and Sr[out].max() < 1e-12 * Sr.max()
    assert (S[out] <= Sr[out] + tol[out]).all()


# ---- d. the spatial filter ------------------------------------------------------------------------------------------------------
def _frames_within(got, frames, Hs, what, tiles):
    worst_n = worst_t = 0.0
    for g, x in zip(got, frames):
        ref, B = FO.spatial_apply(x, Hs), FO.spatial_bound(x)
        worst_n = max(worst_n, D.ratio(np.linalg.norm(g.astype(np.float64) - ref), B))
        if tiles:
            te, n = D.tile_errors(g, ref)
            worst_t = max(worst_t, D.ratio(te.max(), D.tile_limit(B, n, "spatial")))
    print(f"{what}: largest ||error||_F / bound = {worst_n:.4f}" + (f", worst tile / its limit = {worst_t:.4f}" if tiles else ""))
    assert np.isfinite(got).all() and worst_n <= 1.0 and worst_t <= 1.0


@pytest.mark.parametrize("case", D.CASES_SPATIAL, ids=ids)
def test_spatial(gpu_ctx, case):
    rows, cols = case
    cube, view = D.dense_frames_spatial(case)
    host = np.ascontiguousarray(view)
    dview = _dev(gpu_ctx, cube)[:, 1:1 + rows, 2:2 + cols]
    deltas = D.delta_frames(rows, cols)
    transfers = {"butterworth": None}
    transfers.update(D.injected_transfers(rows, cols))
    for name, Hs in transfers.items():
        filt = P.Spatial2DButterworth(rows, cols, D.SPATIAL_DU, D.SPATIAL_CUTOFF, D.SPATIAL_ORDER, ctx=gpu_ctx, batch=D.SPATIAL_BATCH)
        if Hs is None:
            Hs = D.butterworth_transfer(rows, cols)
            np.testing.assert_allclose(filt.butterworth_filter, Hs, rtol=1e-14)
        else:
            filt.butterworth_filter = Hs                                   # read when the handle is made, at the first apply
        try:
            got = filt.apply_batch(host)
            same = filt.apply_batch(dview).cpu().numpy().tobytes() == got.tobytes()
            assert got.shape == host.shape and got.dtype == np.float32
            _frames_within(got, host, Hs, f"{case} {name}, dense (device view {'equal' if same else 'DIFFERS'})", tiles=(name == "butterworth"))
            assert same
            if name == "ones":
                for g, x in zip(got, host):
                    assert np.linalg.norm(g.astype(np.float64) - x) <= FO.spatial_bound(x)
            _frames_within(filt.apply_batch(deltas), deltas, Hs, f"{case} {name}, {len(deltas)} delta frames", tiles=False)
        finally:
            filt.close()


def test_spatial_nan_frame_in_a_batch(gpu_ctx):
    rows, cols = 63, 65
    _, view = D.dense_frames_spatial((rows, cols))
    frames = np.ascontiguousarray(view)
    filt = P.Spatial2DButterworth(rows, cols, D.SPATIAL_DU, D.SPATIAL_CUTOFF, D.SPATIAL_ORDER, ctx=gpu_ctx, batch=D.SPATIAL_BATCH)
    try:
        base = filt.apply_batch(frames)
        for k in range(len(frames)):
            bad = frames.copy()
            bad[k, 62, 64] = np.nan
            got = filt.apply_batch(bad)
            keep = [i for i in range(len(frames)) if i != k]
            print(f"NaN in frame {k}: {int(np.isnan(got[k]).sum())} of {rows * cols} cells of it are NaN, {int(np.isnan(got[keep]).sum())} of the others; "
                  f"the others {'equal' if got[keep].tobytes() == base[keep].tobytes() else 'DIFFER from'} the clean run")
            assert np.isnan(got[k]).all()
            assert got[keep].tobytes() == base[keep].tobytes()
    finally:
        filt.close()
