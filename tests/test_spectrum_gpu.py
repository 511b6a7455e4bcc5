"""wass_amd.postproc on the GPU against the fp64 restatement of the reference (tests/spectrum_oracle.py).

The element-wise bound is derived, not tuned (spectrum_oracle.bound3d): three chained length-n inner products in f32 with
f32-rounded twiddles move a Fourier coefficient by at most (nx + ny + nt + 6) 2^-24 ||x_w||_1; e2 is that amplitude squared,
scaled like S, and |S - S_ref| <= 2 sqrt(S_ref e2) + e2 follows.  Every test prints the largest observed error in units of
that bound before it asserts."""
import os

import numpy as np
import pytest

import spectrum_oracle as SO
import wass_amd
from wass_amd import postproc as P

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _check_bound(S, S_ref, e2, what):
    assert S.shape == S_ref.shape and S.dtype == np.float64
    tol = 2.0 * np.sqrt(S_ref * e2) + e2
    err = np.abs(S - S_ref)
    worst = float(np.max(err / tol))
    print(f"{what}: max |S - S_ref| / max S_ref = {err.max() / S_ref.max():.3e}, sqrt(e2 / max S_ref) = {np.sqrt(e2 / S_ref.max()):.3e}, "
          f"largest error / bound = {worst:.4f}")
    assert np.isfinite(S).all() and worst <= 1.0
    return worst


def _run_case(ctx, cube, du, dt, datascale=1.0, what=""):
    S, KX, KY, f = P.compute_3D_spectrum(cube, du, dt, datascale=datascale, ctx=ctx)
    Sr, KXr, KYr, fr = SO.compute_3D_spectrum(cube, du, dt, datascale=datascale)
    assert np.array_equal(KX, KXr) and np.array_equal(KY, KYr) and np.array_equal(f, fr)
    e2, _ = SO.bound3d(cube, du, dt, datascale)
    _check_bound(S, Sr, e2, what)
    return S, Sr, e2


@pytest.mark.parametrize("name", ["nx", "nx1"])
def test_golden_shapes(gpu_ctx, name):
    """The two cubes of tests/golden: against the oracle within the bound, and against the reference's own recorded output."""
    g = np.load(os.path.join(ROOT, "tests", "golden", f"spectra_3d_{name}.npz"))
    cube = SO.make_cube(*[int(v) for v in g["shape"]], seed=int(g["seed"]), nan_fraction=float(g["nan_fraction"]))
    S, Sr, e2 = _run_case(gpu_ctx, cube, float(g["du"]), float(g["dt"]), float(g["datascale"]), name)
    _check_bound(S, g["S"], e2, name + " (recorded)")


@pytest.mark.parametrize("shape,du,nt,nseg,width", [((200, 150, 160), 0.2, 20, 19, None), ((400, 384, 400), 0.2, 40, 19, 257),
                                                     ((210, 123, 128), 0.1, 22, 18, 84), ((130, 123, 128), 0.1, 14, 17, 84)])
def test_sequences(gpu_ctx, shape, du, nt, nseg, width):
    p = P.spectrum3d_plan(shape, du, 0.1)
    assert (p.nt, len(p.starts)) == (nt, nseg) and (width is None or p.nx == width)
    cube = SO.make_cube(*shape, seed=shape[0], nan_fraction=0.002)
    _run_case(gpu_ctx, cube, du, 0.1, what=str(shape))


def _du_for_width(H, want):
    for du in (0.2, 0.1, 0.25, 0.3, 0.15, 0.4, 0.5, 1 / 3, 0.125, 0.35):
        if len(SO.axes3d(40, H, H, du, 0.1)["kx"]) == want:
            return du
    raise AssertionError(f"no du gives axes {want} long")


@pytest.mark.parametrize("width", [684, 683])
def test_production_window(gpu_ctx, width):
    """40 x 1024 x 1024: the production window (684 wide, even; 683, prime and odd, with another du), ragged against the 16 x 16
    tiles, many tiles, cheap in t."""
    du = _du_for_width(1024, width)
    assert width != 684 or du == 0.2
    cube = SO.make_cube(40, 1024, 1024, seed=width, nan_fraction=0.001)
    S, Sr, e2 = _run_case(gpu_ctx, cube, du, 0.1, what=f"1024^2 window {width} du {du}")
    assert S.shape == (4, width, width)


def test_parseval_per_segment(gpu_ctx):
    """Independent of the FFT oracle: per segment, sum |X|^2 = N sum x_w^2 (fp64) within (nx + ny + nt + 6) 2^-23 relative."""
    cube = SO.make_cube(200, 150, 160, seed=21, nan_fraction=0.01)
    p = P.spectrum3d_plan(cube.shape, 0.2, 0.1)
    _, energy = SO.bound3d(cube, 0.2, 0.1)
    worst = 0.0
    with P.Spectrum3D(gpu_ctx, p.nt, p.ny, p.nx, p.win_t, p.win_y, p.win_x) as sp:
        for s, want in zip(p.starts, energy):
            sp.push(cube[s:s + p.nt, p.r0:p.r0 + p.ny, p.c0:p.c0 + p.nx])
            S, n, flag = sp.finish(1.0)
            assert n == 1 and not flag
            worst = max(worst, abs(S.sum() - want) / want)
    tol = (p.nx + p.ny + p.nt + 6) * 2.0 ** -23
    print(f"Parseval: largest relative difference {worst:.3e}, bound {tol:.3e}")
    assert worst <= tol


def _circ(a, b, n):
    d = np.abs(a - b)
    return np.minimum(d, n - d)


def test_on_bin_plane_wave(gpu_ctx):
    """Integer cycles on all three axes of the 4 x 84 x 84 window, no noise.  The two largest bins are the stated (f, ky, kx) and its
    mirror, with equal value.  With the reference's symmetric Hann window the true spectrum itself leaks outside the main lobe
    (the oracle has 2.8e-7 there against e2 = 2.2e-11: the window's period is n - 1, not n), so "nothing outside the main lobe" is
    asserted where it is true of the exact result: with periodic Hann windows through the same kernels everything more than 2
    bins away on any axis is below e2; with the reference's window the region is held to the oracle within the bound."""
    W, nt, p_, q, r = 84, 4, 1, 5, 9
    cube = SO.make_cube(40, 123, 130, noise=0.0, waves=((300.0, p_ / nt, q / W, r / W, 0.7),))
    S, Sr, e2 = _run_case(gpu_ctx, cube, 0.1, 0.1, what="on-bin wave")
    peak, mirror = (p_ + nt // 2, q + W // 2, r + W // 2), (-p_ + nt // 2, -q + W // 2, -r + W // 2)
    top = [tuple(int(v) for v in np.unravel_index(i, S.shape)) for i in np.argsort(S.ravel())[::-1][:2]]
    assert sorted(top) == sorted([peak, mirror])
    assert S[peak] == S[mirror]
    it, iy, ix = np.indices(S.shape)
    lobe = np.zeros(S.shape, bool)
    for pk in (peak, mirror):
        lobe |= (_circ(it, pk[0], nt) <= 2) & (_circ(iy, pk[1], W) <= 2) & (_circ(ix, pk[2], W) <= 2)
    assert (~lobe).sum() > 0.9 * S.size
    # periodic windows: the exact spectrum is 0 outside the lobe
    pl = P.spectrum3d_plan(cube.shape, 0.1, 0.1)
    wt, wy, wx = SO.hann(nt, sym=False), SO.hann(W, sym=False), SO.hann(W, sym=False)
    seg = cube[0:nt, pl.r0:pl.r0 + W, pl.c0:pl.c0 + W]
    xw = (seg.astype(np.float64) - float(np.mean(seg))) * (wy[:, None] * wx)[None] * wt[:, None, None]
    e2p = ((2 * W + nt + 6) * 2.0 ** -24 * np.abs(xw).sum()) ** 2
    with P.Spectrum3D(gpu_ctx, nt, W, W, wt, wy, wx) as sp:
        sp.push(seg)
        Sp, _, _ = sp.finish(1.0)
    exact = np.abs(np.fft.fftshift(np.fft.fftn(xw))) ** 2
    assert exact[~lobe].max() < 1e-12 * exact.max()
    print(f"periodic Hann: largest bin outside the main lobe {Sp[~lobe].max():.3e}, e2 {e2p:.3e}, peak {Sp.max():.3e}")
    assert Sp[~lobe].max() <= e2p
    assert Sp[peak] == Sp[mirror] == Sp.max()


def test_all_nan_cell_and_scattered_nans(gpu_ctx):
    cube = SO.make_cube(40, 123, 130, seed=31, nan_fraction=0.01)
    _run_case(gpu_ctx, cube, 0.1, 0.1, what="1 % NaN")
    p = P.spectrum3d_plan(cube.shape, 0.1, 0.1)
    bad = cube.copy()
    bad[6:10, p.r0 + 17, p.c0 + 40] = np.nan                     # NaN throughout the segment that starts at frame 6
    S, _, _, _ = P.compute_3D_spectrum(bad, 0.1, 0.1, ctx=gpu_ctx)
    assert S.shape == (4, 84, 84) and np.isnan(S).all()
    assert np.isnan(SO.compute_3D_spectrum(bad, 0.1, 0.1)[0]).all()
    with P.Spectrum3D(gpu_ctx, p.nt, p.ny, p.nx) as sp:
        sp.push(bad[6:10, p.r0:p.r0 + p.ny, p.c0:p.c0 + p.nx])
        S1, n, flag = sp.finish(1.0)
        assert flag and n == 1 and np.isfinite(S1).all()          # no NaN went through the MFMA
        sp.push(bad[0:4, p.r0:p.r0 + p.ny, p.c0:p.c0 + p.nx])     # the handle starts over, the flag with it
        assert not sp.finish(1.0)[2]
    bad[5, p.r0 + 17, p.c0 + 40] = 1.0                            # outside that segment: nothing changes
    assert np.isnan(P.compute_3D_spectrum(bad, 0.1, 0.1, ctx=gpu_ctx)[0]).all()
    bad[7, p.r0 + 17, p.c0 + 40] = 1.0                            # one frame of every segment has data again
    assert np.isfinite(P.compute_3D_spectrum(bad, 0.1, 0.1, ctx=gpu_ctx)[0]).all()


def test_determinism_and_device_push(gpu_ctx):
    import torch
    cube = SO.make_cube(200, 150, 160, seed=41, nan_fraction=0.005)
    S1 = P.compute_3D_spectrum(cube, 0.2, 0.1, ctx=gpu_ctx)[0]
    S2 = P.compute_3D_spectrum(cube, 0.2, 0.1, ctx=gpu_ctx)[0]
    assert S1.tobytes() == S2.tobytes()
    p = P.spectrum3d_plan(cube.shape, 0.2, 0.1)
    d = torch.from_numpy(cube).to(f"cuda:{gpu_ctx.device_id}")
    torch.cuda.synchronize()
    with P.Spectrum3D(gpu_ctx, p.nt, p.ny, p.nx, p.win_t, p.win_y, p.win_x) as sp:
        for s in p.starts:
            sp.push_dev(d[s:s + p.nt, p.r0:p.r0 + p.ny, p.c0:p.c0 + p.nx])
        S3, n, flag = sp.finish(p.scale)
    assert n == 19 and not flag and S3.tobytes() == S1.tobytes()
    # a datascale goes through the same way on both sides
    _run_case(gpu_ctx, cube, 0.2, 0.1, datascale=0.001, what="datascale 0.001")


@pytest.mark.parametrize("shape,nperseg,rangespan", [((700, 40, 40), 64, 5), ((700, 40, 40), 512, 5), ((700, 40, 40), 512, 0),
                                                     ((300, 41, 43), 512, 5), ((300, 41, 43), 64, 0), ((333, 41, 43), 128, 3)])
def test_compute_spectrum(gpu_ctx, shape, nperseg, rangespan):
    cube = SO.make_cube(*shape, seed=shape[0] + nperseg)
    f, S, ts = P.compute_spectrum(cube, 0.1, nperseg=nperseg, rangespan=rangespan, scale=0.001, ctx=gpu_ctx)
    fr, Sr, tsr = SO.compute_spectrum(cube, 0.1, nperseg=nperseg, rangespan=rangespan, scale=0.001)
    assert S.shape == Sr.shape == (min(nperseg, shape[0]) // 2 + 1,) and S.dtype == np.float64
    err = float(np.max(np.abs(S - Sr)) / Sr.max())
    print(f"compute_spectrum {shape} nperseg {nperseg} rangespan {rangespan}: max error / peak = {err:.3e}")
    assert err <= 1e-5
    assert np.array_equal(f, fr)
    np.testing.assert_allclose(ts, tsr, atol=1e-6 * np.abs(tsr).max())
    S2 = P.compute_spectrum(cube, 0.1, nperseg=nperseg, rangespan=rangespan, scale=0.001, ctx=gpu_ctx)[1]
    assert S2.tobytes() == S.tobytes()


def test_hm0_of_a_sinusoid(gpu_ctx):
    a = 0.75                                                      # metres; the cube is in millimetres
    cube = SO.make_cube(2048, 24, 24, noise=0.0, waves=((1000.0 * a, 0.0625, 0.01, 0.02, 0.4),))
    f, S, _ = P.compute_spectrum(cube, 0.1, nperseg=512, rangespan=5, scale=0.001, ctx=gpu_ctx)
    st = P.spectrum_statistics(f, S)
    print(f"Hm0 {st['Hm0']:.5f}, expected {4 * a / np.sqrt(2):.5f}; peak at {st['peak_frequency']:.4f} Hz")
    assert st["Hm0"] == pytest.approx(4 * a / np.sqrt(2), rel=0.01)
    assert st["peak_frequency"] == pytest.approx(0.625, abs=1e-9) and st["Tm01"] == pytest.approx(1.6, rel=0.01)


def test_grid_sequence_into_the_spectrum(gpu_ctx, oracle, tmp_path):
    """End to end: grid_sequence on synthetic work directories, its cube into compute_3D_spectrum, against the oracle on the same Z."""
    from test_grid_seq_gpu import _sequence_on_disk
    from wass_amd.gridding import grid_sequence
    plane = np.array([0.02, 0.81, 0.586, -11.0]); plane[:3] /= np.linalg.norm(plane[:3])
    dirs = _sequence_on_disk(tmp_path, oracle, 30, plane)
    R, T, _, _ = wass_amd.RT_from_plane(plane)
    W, H = 132, 126
    setup = {"Rpl": R, "Tpl": T.reshape(3, 1), "CAM_BASELINE": np.array([[2.5]]), "xmin": np.array([[-12.0]]), "xmax": np.array([[12.0]]),
             "ymin": np.array([[-30.0]]), "ymax": np.array([[-5.0]]), "XX": np.zeros((H, W)), "fps": np.array([[12.5]])}
    res = grid_sequence(dirs, setup, alg_options={"Nfreqs": 30, "MAX_ITERS": 60}, force_zero_mean=True, batch=8, ctx=gpu_ctx)
    assert res.Z.shape == (30, H, W) and np.isfinite(res.Z).all()
    du = 24.0 / W
    S, Sr, e2 = _run_case(gpu_ctx, res.Z, du, 1 / 12.5, datascale=0.001, what="grid_sequence cube")
    assert S.shape[0] == 4 and S.shape[1] == S.shape[2] and S.max() > 0
    f, S1, _ = P.compute_spectrum(res.Z, 1 / 12.5, nperseg=16, rangespan=2, scale=0.001, ctx=gpu_ctx)
    S1r = SO.compute_spectrum(res.Z, 1 / 12.5, nperseg=16, rangespan=2, scale=0.001)[1]
    assert np.max(np.abs(S1 - S1r)) <= 1e-5 * S1r.max()
