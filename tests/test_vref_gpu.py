"""Variational refinement on the GPU (wass_amd/csrc/vref.hip, wass_amd/refinement.py) against the float32 form of
tests/vref_oracle.py, bit for bit: projection, samples, slopes, the gradient (coarse and full resolution), k-hot probes whose
footprints are known by hand, whole Adam trajectories; the two loss sums within gamma_N of the oracle's fp64 sums; the
end-to-end scene of tests/test_vref.py; refine_surface on a work directory; refusals through the C ABI."""
import ctypes as C

import numpy as np
import pytest

import test_grid_setup as TS
import test_vref as TV
import vref_oracle as V
from wass_amd import gridding, refinement

pytestmark = pytest.mark.gpu

EPS64 = np.finfo(np.float64).eps
GRIDS = ((2, 2), (3, 5), (7, 7), (6, 8), (13, 9), (64, 64), (65, 67), (130, 34))
PICTURES = ((2, 2), (5, 7), (64, 48), (200, 150))
MASKS = ("ones", "zeros", "checkerboard")


def gamma(n):
    return n * EPS64 / (1.0 - n * EPS64)


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b)


def check_forward(ctx, ny, nx, ih, iw, mask, spread, seed, uint8=False, behind=True):
    S, args = V.probe(ny, nx, ih, iw, seed=seed, spread=spread, mask=mask, uint8=uint8)
    Z = V.surface(ny, nx, seed).astype(np.float32)
    if behind:
        Z[ny // 2, nx // 2] = -6.0                             # behind both cameras (they stand at z = 4 looking down)
    rng = np.random.default_rng(seed)
    Zc = rng.normal(0, 0.05, S.coarse).astype(np.float32)
    with refinement.VariationalRefinement(ctx=ctx, **args) as vr:
        i0, i1, p0, p1 = vr.sample_images(Z)
        w0, w1, uv = V.sample(S, Z)
        if behind:
            cams, ok = V.project(S, Z)
            assert not ok[ny // 2, nx // 2] and ok.sum() == ny * nx - 1 and w0[ny // 2, nx // 2] == 0 == w1[ny // 2, nx // 2]
        assert same(i0, w0) and same(i1, w1), (ny, nx, ih, iw, mask, spread)
        assert same(p0, np.stack([uv[0].ravel(), uv[1].ravel()], axis=1)) and same(p1, np.stack([uv[2].ravel(), uv[3].ravel()], axis=1))
        zdx, zdy = vr.compute_Z_gradient(Z)
        wdx, wdy = V.zgrad(S, Z)
        assert same(zdx, wdx) and same(zdy, wdy), (ny, nx)
        got, want = vr.compute_loss(Z), V.loss(S, Z)
        for g, w in zip(got, want):
            assert abs(g - w) <= gamma(ny * nx) * w, (g, w)
        for alpha in (10.0, 0.0):
            gC, gZ = vr.energy_gradient(Zc, alpha, full=True)
            wC, wZ = V.gradient(S, Zc, alpha)
            assert same(gZ, wZ), (ny, nx, alpha, np.abs(gZ - wZ).max())
            assert same(gC, wC), (ny, nx, alpha, np.abs(gC - wC).max())
        assert same(vr.energy_gradient(Zc, 10.0), wC if alpha == 10.0 else V.gradient(S, Zc, 10.0)[0])
    return S


@pytest.mark.parametrize("k", range(len(GRIDS)))
def test_every_grid_against_the_oracle(gpu_ctx, k):
    """each grid with two of the pictures, every mask; queries inside the picture and, with spread 1.6, clamped on every side"""
    ny, nx = GRIDS[k]
    for j, mask in enumerate(MASKS):
        ih, iw = PICTURES[(k + j) % 4]
        S = check_forward(gpu_ctx, ny, nx, ih, iw, mask, 0.7 if j != 1 else 1.6, seed=10 * k + j)
        if mask == "ones" and min(ny, nx) > 2:
            assert np.abs(V.sample(S, np.zeros((ny, nx), np.float32))[0]).max() > 0
    check_forward(gpu_ctx, ny, nx, *PICTURES[(k + 3) % 4], "ones", 1.6, seed=10 * k + 5)


@pytest.mark.parametrize("k", range(len(PICTURES)))
def test_every_picture_against_the_oracle(gpu_ctx, k):
    ih, iw = PICTURES[k]
    for spread in (0.7, 1.6, 3.0):
        S = check_forward(gpu_ctx, 13, 9, ih, iw, "checkerboard", spread, seed=50 + k, uint8=(spread == 0.7), behind=(spread != 3.0))
    # with spread 1.6 the queries leave the picture on every side, in both cameras
    S, _ = V.probe(13, 9, ih, iw, seed=50 + k, spread=1.6)
    cams, _ = V.project(S, np.zeros((13, 9), np.float32))
    for u, v, _ in cams:
        assert u.min() < 0 and u.max() > iw - 1 and v.min() < 0 and v.max() > ih - 1


# ---------------------------------------------------------------------------------------------------------------- k-hot probes
def _khot_rig(ctx, ny, nx, mask=None):
    S, args = V.probe(ny, nx, 64, 48, seed=3)
    if mask is not None:
        args = dict(args, mask=mask)
        S = V.scene(**args)
    return S, refinement.VariationalRefinement(ctx=ctx, **args)


def test_one_slope_cell_has_the_flipped_kernels_footprint(gpu_ctx):
    """A single non-zero cell of Zdx (then of Zdy), value 1, with gd = 0: gZ is cS * K[jy - iy + 3][jx - ix + 3] over the 7 x 7 nodes
    about it that lie inside the grid and 0 elsewhere -- one product per node, so exactly.  At a corner, on an edge, and on each
    side of the 64 x 16 tile's boundaries."""
    ny, nx, alpha = 65, 67, 10.0
    S, vr = _khot_rig(gpu_ctx, ny, nx)
    cS = np.float32(2.0 * alpha / (ny * nx))
    zero = np.zeros((ny, nx), np.float32)
    with vr:
        for iy, ix in ((0, 0), (ny - 1, nx - 1), (0, nx // 2), (ny // 2, 0), (15, 63), (16, 64), (15, 64), (16, 63), (31, 64), (32, 63)):
            for which, K in ((0, S.kx), (1, S.ky)):
                hot = zero.copy()
                hot[iy, ix] = 1.0
                gC, gZ = vr.adjoint(hot if which == 0 else zero, hot if which == 1 else zero, zero, alpha)
                want = np.zeros((ny, nx), np.float32)
                for jy in range(max(0, iy - 3), min(ny, iy + 4)):
                    for jx in range(max(0, ix - 3), min(nx, ix + 4)):
                        want[jy, jx] = K[jy - iy + 3, jx - ix + 3] * cS
                assert np.array_equal(gZ, want), (iy, ix, which)
                assert np.count_nonzero(gZ) == np.count_nonzero(want) > 0
                assert same(gC, V.resize_adjoint(S, want))


def test_one_data_cell_has_the_resizes_footprint(gpu_ctx):
    """gd with a single non-zero node (a node with a picture difference), Zdx = Zdy = 0: gZ = gd, and gC is wy * wx * value on the at
    most 2 x 2 coarse nodes that node reads (tf.image.resize's two taps per axis), 0 elsewhere.  Then the same through the public
    gradient: a mask with a single 1 leaves one node with a picture difference."""
    ny, nx = 65, 67
    S, vr = _khot_rig(gpu_ctx, ny, nx)
    (yl, yh, ty), (xl, xh, tx) = V.axis_tables(ny // 2, ny, np.float32), V.axis_tables(nx // 2, nx, np.float32)
    zero = np.zeros((ny, nx), np.float32)
    one = np.float32(1)
    with vr:
        for iy, ix in ((0, 0), (ny - 1, nx - 1), (0, 33), (15, 63), (16, 64), (40, 21)):
            hot = zero.copy()
            hot[iy, ix] = 0.75
            gC, gZ = vr.adjoint(zero, zero, hot, 10.0)
            assert np.array_equal(gZ, hot)
            want = np.zeros((ny // 2, nx // 2), np.float32)
            wy = {}
            for c, w in ((yl[iy], one - ty[iy]), (yh[iy], ty[iy])):
                wy[c] = wy.get(c, np.float32(0)) + w
            wx = {}
            for c, w in ((xl[ix], one - tx[ix]), (xh[ix], tx[ix])):
                wx[c] = wx.get(c, np.float32(0)) + w
            for cy, a in wy.items():
                for cx, b in wx.items():
                    want[cy, cx] = a * (b * np.float32(0.75))
            assert np.array_equal(gC, want), (iy, ix)
            assert 1 <= np.count_nonzero(want) <= 4
    rng = np.random.default_rng(12)
    Zc = rng.normal(0, 0.05, (ny // 2, nx // 2)).astype(np.float32)
    for iy, ix in ((0, 0), (15, 63), (16, 64), (ny - 1, nx - 1)):
        mask = np.zeros((ny, nx)); mask[iy, ix] = 1
        S1, vr1 = _khot_rig(gpu_ctx, ny, nx, mask=mask)
        with vr1:
            gC, gZ = vr1.energy_gradient(Zc, 0.0, full=True)
        wC, wZ = V.gradient(S1, Zc, 0.0)
        assert same(gZ, wZ) and same(gC, wC)
        assert np.count_nonzero(gZ) == 1 and gZ[iy, ix] != 0 and 1 <= np.count_nonzero(gC) <= 4


# ---------------------------------------------------------------------------------------------------------------- trajectories
TRAJ = {"13x9": (13, 9, 64, 48), "65x67": (65, 67, 64, 48)}


@pytest.fixture(scope="module")
def trajectories():
    """per scene: the oracle's (Zc, m, v) after 1, 2, 10 and 40 steps, computed once"""
    out = {}
    for name, (ny, nx, ih, iw) in TRAJ.items():
        S, args = V.probe(ny, nx, ih, iw, seed=21, mask="ones")
        Zc0 = (V.surface(ny // 2, nx // 2, 5, amp=0.05)).astype(np.float32)
        states, st = {}, (Zc0, None, None, 0)
        for n in (1, 2, 10, 40):
            st = V.optimize(S, st[0], n - st[3], alpha=10.0, m=st[1], v=st[2], step=st[3])
            states[n] = st
        out[name] = (S, args, Zc0, states)
    return out


@pytest.mark.parametrize("name", sorted(TRAJ))
def test_trajectory_is_the_oracles_bit_for_bit(gpu_ctx, trajectories, name):
    import torch
    S, args, Zc0, states = trajectories[name]
    with refinement.VariationalRefinement(ctx=gpu_ctx, **args) as vr:
        runs = {}
        for n in (1, 2, 10, 40):
            Zc, st, Z = vr.optimize_coarse(Zc0, n, alpha=10.0)
            wZc, wm, wv, wstep = states[n]
            assert same(Zc, wZc), (name, n, np.abs(Zc - wZc).max())
            assert same(st.m, wm) and same(st.v, wv) and st.step == wstep == n
            assert same(Z, V.resize(S, wZc) * S.mask)
            runs[n] = (Zc, st, Z)
            # the trace: before the first step, after steps 1, 11, 21, 31, after the last
            steps = sorted({0, n} | {i + 1 for i in range(0, n, 10)})
            assert [int(r[0]) for r in vr.losses] == steps
        assert not same(runs[40][0], runs[10][0]) and np.abs(runs[40][0] - Zc0).max() > 1e-3
        # the first and the last row against the oracle's fp64 sums
        for row, Zc in ((vr.losses[0], Zc0), (vr.losses[-1], states[40][0])):
            d, s = V.loss(S, V.resize(S, Zc))
            assert abs(row[1] - d) <= gamma(S.Xb.size) * d and abs(row[2] - s) <= gamma(S.Xb.size) * s
            assert abs(row[3] - (row[1] + 10.0 * row[2])) <= 4 * EPS64 * row[3]
        # 4 x 10 continued through the state
        Zc, st = Zc0, None
        for _ in range(4):
            Zc, st, Z = vr.optimize_coarse(Zc, 10, alpha=10.0, state=st)
        assert same(Zc, runs[40][0]) and same(st.m, runs[40][1].m) and same(st.v, runs[40][1].v) and st.step == 40 and same(Z, runs[40][2])
        # again: the same bits; another report_every: the same Zc; device tensors in: the same bits, device tensors out
        again = vr.optimize_coarse(Zc0, 40, alpha=10.0)
        assert same(again[0], runs[40][0]) and same(again[1].v, runs[40][1].v)
        for every in (1, 7, 0):
            other = vr.optimize_coarse(Zc0, 40, alpha=10.0, report_every=every)
            assert same(other[0], runs[40][0]) and same(other[1].m, runs[40][1].m)
            assert len(vr.losses) == (2 if every == 0 else len(sorted({0, 40} | {i + 1 for i in range(0, 40, every)})))
        d_Zc0 = torch.from_numpy(Zc0).to(torch.device("cuda", gpu_ctx.device_id))
        keep = d_Zc0.clone()
        dZc, dst, dZ = vr.optimize_coarse(d_Zc0, 40, alpha=10.0)
        assert dZc.is_cuda and dst.m.is_cuda and dZ.is_cuda and torch.equal(d_Zc0, keep)
        assert same(dZc.cpu().numpy(), runs[40][0]) and same(dst.v.cpu().numpy(), runs[40][1].v) and same(dZ.cpu().numpy(), runs[40][2])
    # device tensors for the whole set-up: the same bits
    dev = torch.device("cuda", gpu_ctx.device_id)
    dargs = {k: (torch.from_numpy(np.ascontiguousarray(v)).to(dev) if k in ("I0", "I1", "XX", "YY", "mask") else v) for k, v in args.items()}
    with refinement.VariationalRefinement(ctx=gpu_ctx, **dargs) as vr2:
        assert same(vr2.optimize_coarse(Zc0, 10, alpha=10.0)[0], runs[10][0])


# ---------------------------------------------------------------------------------------------------------------- end to end
def test_end_to_end_scene_on_the_device(gpu_ctx):
    """the scene of tests/test_vref.py: the same assertion on the masked RMS error, and the oracle's surface bit for bit"""
    S, args = V.e2e_scene(TV.e2e_setup(), TS.IH, TS.IW)
    c0, N = V.E2E["c0"], V.E2E["N"]
    zero = np.zeros((N, N), np.float32)
    with refinement.VariationalRefinement(ctx=gpu_ctx, **args) as vr:
        Z = vr.optimize(zero, max_iters=V.E2E["iters"], alpha=V.E2E["alpha"])
        losses = vr.losses
    start, end = V.masked_rms(zero, c0, S.mask), V.masked_rms(Z, c0, S.mask)
    print(f"masked rms {start:.4f} -> {end:.4f}; data loss {losses[0][1]:.3g} -> {losses[-1][1]:.3g}")
    assert end < 0.5 * start and Z[S.mask != 0].mean() > 0.5 * c0
    assert losses[-1][1] < losses[0][1] and int(losses[-1][0]) == V.E2E["iters"]
    wZc = V.optimize(S, np.zeros((N // 2, N // 2), np.float32), V.E2E["iters"], alpha=V.E2E["alpha"])[0]
    assert same(Z, V.resize(S, wZc) * S.mask)


NX, NY = 32, 24


def test_refine_surface_on_a_work_directory(gpu_ctx, oracle, tmp_path):
    """setup_grid's dict straight into refine_surface: the shape, float32, NaN exactly where the mask is 0, and the convention
    -Zi / baseline in, -Z * baseline out against the class used by hand"""
    rng = np.random.default_rng(321)
    h, w = 60, 120
    Rpl, Tpl = gridding.sea_plane_RT(TS.PLANE)
    gx = rng.uniform(-13.0, 5.0, (h, w)); gy = rng.uniform(-37.0, -23.0, (h, w))
    hz = 0.2 * np.sin(gx * 0.8) + 0.1 * np.cos(gy * 0.6)
    aligned = np.stack([gx, gy, -hz]).reshape(3, -1) / TS.BASELINE
    p3d = np.ascontiguousarray((Rpl.T @ (aligned - Tpl)).T.reshape(h, w, 3))
    picture = np.clip(V.texture(TS.IH, TS.IW, 9), 0, 255).astype(np.uint8)
    wd = tmp_path / "000000_wd"
    TS.write_workdir(str(wd), picture=picture, mesh_bytes=oracle.encode_xyzc(np.ones((h, w), np.uint8), p3d, TS.PLANE))
    res = gridding.setup_grid(wd, TS.PLANE, TS.BASELINE, area_center=np.array([-4.0, -30.0]), area_size_x=16.0, area_size_y=16.0 * (NY - 1) / (NX - 1),
                              Nx=NX, Ny=NY, ctx=gpu_ctx)
    yy, xx = np.mgrid[0:NY, 0:NX]
    mask = ((xx - 15.5) ** 2 / 200.0 + (yy - 11.5) ** 2 / 100.0 < 1).astype(np.float32)
    Zi = (0.05 * np.sin(xx * 0.3) * np.cos(yy * 0.2)).astype(np.float32)
    Zi[mask == 0] = np.nan
    other = np.clip(V.texture(TS.IH, TS.IW, 10), 0, 255).astype(np.float32)
    out = refinement.refine_surface(Zi, mask, picture, other, res, ctx=gpu_ctx, max_iters=7)
    assert out.shape == (NY, NX) and out.dtype == np.float32
    assert np.array_equal(np.isnan(out), mask == 0) and 0 < (mask == 0).sum() < mask.size
    assert not np.array_equal(out[mask != 0], Zi[mask != 0])
    Rp2c = res["Rpl"].T
    with refinement.VariationalRefinement(picture, other, Rp2c, -Rp2c @ res["Tpl"], res["P0cam"], res["P1cam"], res["XX"], res["YY"], TS.BASELINE,
                                          mask, ctx=gpu_ctx) as vr:
        zin = np.where(mask != 0, -Zi.astype(np.float64) / TS.BASELINE, 0.0).astype(np.float32)
        z = vr.optimize(zin, max_iters=7)
        with pytest.raises(ValueError):
            vr.optimize(Zi)                                    # NaN outside the mask: the class refuses it
    assert np.array_equal(out[mask != 0], (-z.astype(np.float64) * TS.BASELINE).astype(np.float32)[mask != 0])


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_through_the_c_abi(gpu_ctx):
    import torch
    lib, ctx = gpu_ctx._lib, gpu_ctx
    dev = torch.device("cuda", ctx.device_id)
    S, args = V.probe(6, 8, 8, 8, seed=1)
    f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)  # noqa: E731
    xb, yb, mask, I0, I1 = f32(S.Xb), f32(S.Yb), f32(S.mask), f32(S.I0), f32(S.I1)
    dp = C.POINTER(C.c_double)
    mats = [np.ascontiguousarray(args[k], np.float64) for k in ("Rp2c", "Tp2c", "P0cam", "P1cam")]
    kernels = np.ascontiguousarray(np.stack(refinement.derivative_of_gaussian_win(7, 0.8)).astype(np.float32))
    torch.cuda.synchronize(dev)

    def create(ny=6, nx=8, ih0=8, iw0=8, ih1=8, iw1=8, xbp=None, i1p=None, ker=None, R=None, out=True):
        h = C.c_void_p()
        m = [a.ctypes.data_as(dp) for a in mats]
        if R is not None:
            m[0] = R.ctypes.data_as(dp) if isinstance(R, np.ndarray) else None
        rc = lib.wass_vref_create(ctx._h, ny, nx, xb.data_ptr() if xbp is None else xbp, yb.data_ptr(), mask.data_ptr(), *m, I0.data_ptr(), ih0, iw0,
                                  I1.data_ptr() if i1p is None else i1p, ih1, iw1, kernels.ctypes.data if ker is None else ker, C.byref(h) if out else None)
        return rc, h

    def message():
        return lib.wass_last_error(ctx._h).decode()

    for kw, word in ((dict(ny=1), "grid"), (dict(nx=1), "grid"), (dict(ny=0, nx=0), "grid"), (dict(ih0=1), "picture"), (dict(iw1=1), "picture"),
                     (dict(xbp=0), "null"), (dict(i1p=0), "null"), (dict(ker=0), "null"), (dict(out=False), "null"),
                     (dict(R=np.full(9, np.nan)), "finite")):
        rc, h = create(**kw)
        assert rc == -1 and not h.value and word in message(), (kw, message())
    bad_mask = mask.clone(); bad_mask[2, 3] = float("inf")
    torch.cuda.synchronize(dev)
    h = C.c_void_p()
    rc = lib.wass_vref_create(ctx._h, 6, 8, xb.data_ptr(), yb.data_ptr(), bad_mask.data_ptr(), *[a.ctypes.data_as(dp) for a in mats], I0.data_ptr(), 8, 8,
                              I1.data_ptr(), 8, 8, kernels.ctypes.data, C.byref(h))
    assert rc == -1 and not h.value and "finite" in message()
    rc, h = create()
    assert rc == 0 and h.value
    try:
        Z = f32(np.zeros((6, 8))); Zbad = Z.clone(); Zbad[5, 7] = float("nan")
        Zc = f32(np.zeros((3, 4))); Zcbad = Zc.clone(); Zcbad[0, 0] = float("-inf")
        m, v = torch.zeros_like(Zc), torch.zeros_like(Zc)
        o = [torch.empty((6, 8), dtype=torch.float32, device=dev) for _ in range(3)]
        uv = torch.empty((4, 6, 8), dtype=torch.float32, device=dev)
        gc = torch.empty((3, 4), dtype=torch.float32, device=dev)
        torch.cuda.synchronize(dev)
        a, b, st, n = C.c_double(), C.c_double(), C.c_int64(0), C.c_int(0)
        P = lambda t: t.data_ptr()  # noqa: E731
        assert lib.wass_vref_sample(h, P(Zbad), P(o[0]), P(o[1]), P(uv)) == -1 and "finite" in message()
        assert lib.wass_vref_sample(h, P(Z), None, P(o[1]), P(uv)) == -1 and "null" in message()
        assert lib.wass_vref_zgrad(h, P(Zbad), P(o[0]), P(o[1])) == -1 and lib.wass_vref_zgrad(h, None, P(o[0]), P(o[1])) == -1
        assert lib.wass_vref_loss(h, P(Zbad), C.byref(a), C.byref(b)) == -1 and lib.wass_vref_loss(h, P(Z), None, C.byref(b)) == -1
        assert lib.wass_vref_gradient(h, P(Zcbad), 10.0, P(gc), None) == -1 and lib.wass_vref_gradient(h, P(Zc), 10.0, None, None) == -1
        assert lib.wass_vref_gradient(h, P(Zc), float("nan"), P(gc), None) == -1
        assert lib.wass_vref_adjoint(h, P(Zbad), P(Z), P(Z), 10.0, P(gc), None) == -1 and lib.wass_vref_adjoint(h, P(Z), P(Z), None, 10.0, P(gc), None) == -1
        opt = lambda zc, mm, it, stp=st: lib.wass_vref_optimize(h, zc, mm, P(v), C.byref(stp) if stp is not None else None, it, 10.0, 1e-3, 1e-7, 10,  # noqa: E731
                                                                None, 0, C.byref(n), None)
        assert opt(P(Zc), P(m), -1) == -1 and "iters" in message()
        assert opt(P(Zcbad), P(m), 1) == -1 and "finite" in message()
        assert opt(None, P(m), 1) == -1 and opt(P(Zc), None, 1) == -1 and opt(P(Zc), P(m), 1, None) == -1
        assert opt(P(Zc), P(m), 1, C.c_int64(-3)) == -1
        assert st.value == 0 and float(Zc.abs().max()) == 0.0 and float(m.abs().max()) == 0.0      # nothing was touched
        # and the handle still works: no step is a no-op, one step moves
        assert opt(P(Zc), P(m), 0) == 0 and st.value == 0 and float(Zc.abs().max()) == 0.0
        assert lib.wass_vref_sample(h, P(Z), P(o[0]), P(o[1]), P(uv)) == 0
        assert same(o[0].cpu().numpy(), V.sample(S, np.zeros((6, 8), np.float32))[0])
        assert opt(P(Zc), P(m), 1) == 0 and st.value == 1 and float(Zc.abs().max()) > 0
    finally:
        lib.wass_vref_destroy(h)
    with pytest.raises(ValueError):
        refinement.VariationalRefinement(ctx=ctx, **dict(args, mask=np.ones((6, 7))))
    with refinement.VariationalRefinement(ctx=ctx, **args) as vr:
        for call in (lambda: vr.sample_images(np.zeros((6, 7), np.float32)), lambda: vr.compute_loss(np.full((6, 8), np.nan, np.float32)),
                     lambda: vr.energy_gradient(np.zeros((6, 8), np.float32)), lambda: vr.optimize(np.full((6, 8), np.inf, np.float32)),
                     lambda: vr.optimize_coarse(np.zeros((3, 4), np.float32), -1), lambda: vr.optimize(Zbad)):
            with pytest.raises(ValueError):
                call()
