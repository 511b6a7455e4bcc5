"""The staging of the operators of csrc/spectrum.hip that keep their scratch in a handle (Spectrum3D, Spatial2DButterworth) and of
compute_spectrum, which go through csrc/cube.h's arena, upload_rows and download_rows: the smallest shapes that cross a tile
edge and leave a ragged batch.  Rows of 67 cells (one 64-wide tile and three columns), 5 rows, segments of 3 frames; the
spatial filter takes 5 frames 2 at a time (batches of 2, 2 and 1); the Welch estimate 130 samples of a 3 x 5 grid in segments
of 64 (three segments and a remainder).

Inputs and outputs are views inside parents filled with guard values (tests/guarded.py): every second frame and an inner
window of rows and columns.  Every such run gives the bits of the same call on contiguous copies, the host form the bits of
the device form, no guard cell of any parent changes, and the contiguous result keeps the bounds of tests/test_dft_stage_gpu.py
(dft_oracle.tol_of / bound3d_e2, filter_oracle.spatial_bound, dft_oracle.welch_tolerance and the 1e-5 of the peak).  The
spectrum is finished twice on one handle, after two segments and after one more: the Welch sum and the reset."""
import functools

import numpy as np
import pytest

import dft_oracle as D
import filter_oracle as FO
import spectrum_oracle as SO
from guarded import Guarded
from wass_amd import postproc as P

pytestmark = pytest.mark.gpu

NT, NY, NX = 3, 5, 67
ROWS, COLS, FRAMES, BATCH = 5, 67, 5, 2
SAMPLES, GRID, NPERSEG, RANGESPAN, DT = 130, (3, 5), 64, 1, 0.1


def _give(a, dev, g):
    """`a` as the operator gets it: a view into a guarded parent, or (g None) a contiguous copy; on the device if `dev`"""
    if g is not None:
        v = g.input(a)
    elif dev:
        import torch
        v = torch.from_numpy(a.copy()).cuda()
    else:
        v = a.copy()
    if dev:
        import torch
        torch.cuda.synchronize()                # the library runs on streams of its own
    return v


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def _segments():
    return _frozen(SO.make_cube(NT, NY, NX, seed=11), SO.make_cube(NT, NY, NX, seed=12))


def run_spectrum3d(ctx, dev, g):
    """two segments, finish, the second segment again, finish"""
    a, b = (_give(s, dev, g) for s in _segments())
    with P.Spectrum3D(ctx, NT, NY, NX, *D.dense_windows(NT, NY, NX)) as sp:
        push = sp.push_dev if dev else sp.push
        push(a)
        push(b)
        S12, n12, flag12 = sp.finish(1.0)
        push(b)
        S2, n2, flag2 = sp.finish(1.0)
    return {"S12": S12, "S2": S2, "n": np.array([n12, n2]), "flag": np.array([flag12, flag2])}


@functools.lru_cache(maxsize=None)
def _frames():
    return _frozen(SO.make_cube(FRAMES, ROWS, COLS, seed=ROWS + 2 * COLS, offset=50.0, waves=D.SPATIAL_WAVES))[0]


def run_spatial(ctx, dev, g):
    x = _give(_frames(), dev, g)
    out = None if g is None else g.out(_frames().shape, np.float32)
    with P.Spatial2DButterworth(ROWS, COLS, D.SPATIAL_DU, D.SPATIAL_CUTOFF, D.SPATIAL_ORDER, ctx=ctx, batch=BATCH) as filt:
        got = filt.apply_batch(x, out=out)
    assert out is None or got is out
    return {"out": got.cpu().numpy() if dev else np.array(got)}


@functools.lru_cache(maxsize=None)
def _welch_cube():
    return _frozen(SO.make_cube(SAMPLES, *GRID, seed=SAMPLES + NPERSEG))[0]


def run_welch(ctx, dev, g):
    f, S, ts = P.compute_spectrum(_give(_welch_cube(), False, g), DT, nperseg=NPERSEG, rangespan=RANGESPAN, scale=D.WELCH_SCALE, ctx=ctx)
    return {"f": f, "S": S, "timeserie": ts}


def _runs(ctx, run, name, sides):
    """{(dev, guarded): result}; the guards are checked, and every run has the bits of the host's on contiguous copies"""
    results = {}
    for dev in sides:
        for guarded in (False, True):
            g = Guarded(dev) if guarded else None
            results[dev, guarded] = run(ctx, dev, g)
            if g is not None:
                g.check(f"{name}, {'device' if dev else 'host'}")
    base = results[False, False]
    for (dev, guarded), r in results.items():
        assert set(r) == set(base)
        for k in base:
            assert r[k].dtype == base[k].dtype and r[k].shape == base[k].shape and r[k].tobytes() == base[k].tobytes(), \
                f"{name}: {k}, {'device' if dev else 'host'}, {'views into guarded parents' if guarded else 'contiguous'}, against the host's contiguous run"
    return base


def test_spectrum3d_staging(gpu_ctx):
    got = _runs(gpu_ctx, run_spectrum3d, "Spectrum3D", (False, True))
    refs = []
    for seg in _segments():
        prep, flag = D.prepare3d(seg, *D.dense_windows(NT, NY, NX))
        assert not flag
        xw = prep.astype(np.float64)
        ref = np.fft.fftshift(np.abs(np.fft.fftn(xw)) ** 2)
        refs.append((ref, D.tol_of(ref, D.bound3d_e2(xw))))
    both = D.ratio(np.abs(got["S12"] - (refs[0][0] + refs[1][0])), refs[0][1] + refs[1][1])
    again = D.ratio(np.abs(got["S2"] - refs[1][0]), refs[1][1])
    print(f"Spectrum3D {NT} x {NY} x {NX}: two segments, error / bound = {both:.4f}; the second alone after the reset = {again:.4f}; "
          f"segments {got['n']}, flags {got['flag']}")
    assert got["S12"].shape == (NT, NY, NX) and np.isfinite(got["S12"]).all() and np.isfinite(got["S2"]).all()
    assert got["n"].tolist() == [2, 1] and not got["flag"].any()
    assert both <= 1.0 and again <= 1.0


def test_spatial_filter_staging(gpu_ctx):
    got = _runs(gpu_ctx, run_spatial, "Spatial2DButterworth", (False, True))["out"]
    assert got.shape == (FRAMES, ROWS, COLS) and got.dtype == np.float32 and np.isfinite(got).all()
    Hs = D.butterworth_transfer(ROWS, COLS)
    worst = max(D.ratio(np.linalg.norm(g.astype(np.float64) - FO.spatial_apply(x, Hs)), FO.spatial_bound(x)) for g, x in zip(got, _frames()))
    print(f"Spatial2DButterworth {ROWS} x {COLS}, {FRAMES} frames {BATCH} at a time: largest ||error||_F / bound = {worst:.4f}")
    assert worst <= 1.0


def test_compute_spectrum_staging(gpu_ctx):
    got = _runs(gpu_ctx, run_welch, "compute_spectrum", (False,))
    cube = _welch_cube()
    fr, Sr, tsr = SO.compute_spectrum(cube, DT, nperseg=NPERSEG, rangespan=RANGESPAN, scale=D.WELCH_SCALE)
    series = P.spectrum_series(cube, RANGESPAN).astype(np.float64) * D.WELCH_SCALE
    tol = D.welch_tolerance(D.staged_welch(series, 1.0 / DT, NPERSEG), 1.0 / DT, NPERSEG, SAMPLES)
    S = got["S"]
    assert S.shape == Sr.shape == (NPERSEG // 2 + 1,) and S.dtype == np.float64 and np.isfinite(S).all()
    flat, el = float(np.max(np.abs(S - Sr)) / Sr.max()), D.ratio(np.abs(S - Sr), tol)
    print(f"compute_spectrum {SAMPLES} samples of {GRID}, nperseg {NPERSEG}: max error / peak = {flat:.3e}, element-wise error / bound = {el:.4f}")
    assert flat <= 1e-5 and el <= 1.0
    assert np.array_equal(got["f"], fr)
    np.testing.assert_allclose(got["timeserie"], tsr, atol=1e-6 * np.abs(tsr).max())
