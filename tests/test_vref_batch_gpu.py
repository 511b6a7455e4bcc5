"""The batched variational refinement on the GPU (wass_amd/csrc/vref.hip: the frame from blockIdx.z; refinement.SequenceRefiner,
refine_sequence; gridding.grid_sequence(refine=...)).  The oracle is the single path, which tests/test_vref_gpu.py pins to numpy:
frame i of a batch must be the single run of frame i bit for bit, so every comparison is np.array_equal."""
import ctypes as C
import os

import numpy as np
import pytest

import grid_seq_oracle as GS
import test_grid_setup as TS
import test_vref as TV
import vref_batch_probes as P
import vref_oracle as V
from wass_amd import gridding, refinement

pytestmark = pytest.mark.gpu


def same(a, b, nan=False):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=nan)


def host(t):
    return t.cpu().numpy()


def single_runs(ctx, F, frames, iters, alpha=10.0, report_every=10):
    """per frame: (Zc, m, v, Z, losses) of VariationalRefinement.optimize_coarse on a handle of its own"""
    out = {}
    for f in frames:
        with refinement.VariationalRefinement(ctx=ctx, **F.single(f)) as vr:
            Zc, st, Z = vr.optimize_coarse(F.Zc0[f], iters, alpha=alpha, report_every=report_every)
            out[f] = (Zc, st.m, st.v, Z, vr.losses.copy())
    return out


def batch_run(sr, F, frames, iters, alpha=10.0, report_every=10):
    """the same frames in one load: per position (Zc, m, v, Z, losses)"""
    idx = list(frames)
    sr.load(np.zeros((len(idx),) + F.shape, np.float32), F.I0[idx], F.I1[idx], F.mask[idx])
    sr.set_state(F.Zc0[idx])
    sr.optimize(iters, alpha=alpha, report_every=report_every)
    Zc, m, v, step = sr.get_state()
    assert step == iters
    _, Z = sr.result(with_plane=True)
    Zc, m, v, Z = host(Zc), host(m), host(v), host(Z)
    return [(Zc[k], m[k], v[k], Z[k], sr.losses[k]) for k in range(len(idx))]


def assert_equal_runs(got, want, what):
    for name, g, w in zip(("Zc", "m", "v", "Z", "losses"), got, want):
        assert same(g, w), (what, name)


# ---------------------------------------------------------------------------------------------------------------- edge shapes
EDGE_GRIDS = ((2, 2), (3, 5), (13, 9), (16, 64), (17, 65), (65, 67), (130, 34))


@pytest.mark.parametrize("k", range(len(EDGE_GRIDS)))
def test_edge_shapes_equal_the_singles(gpu_ctx, k):
    """3 frames (masks ones, checkerboard, zeros), 10 steps from a stated coarse field; camera 0 sees 5 x 7 pixels, camera 1 64 x 48"""
    ny, nx = EDGE_GRIDS[k]
    F = P.Frames(ny, nx, 3, seed=40 + k)
    want = single_runs(gpu_ctx, F, range(3), 10)
    with refinement.SequenceRefiner(F.gridsetup, F.pics, 3, gpu_ctx) as sr:
        got = batch_run(sr, F, range(3), 10)
    for f in range(3):
        assert_equal_runs(got[f], want[f], (ny, nx, f))
        assert [int(r[0]) for r in got[f][4]] == [0, 1, 10]
    assert not same(got[0][0], F.Zc0[0]) if min(ny, nx) > 2 else True
    assert same(got[2][3], np.zeros((ny, nx), np.float32))                   # the all-zero mask


# ---------------------------------------------------------------------------------------------------------------- trajectories
TRAJ = {"13x9": (13, 9), "65x67": (65, 67)}


@pytest.fixture(scope="module")
def trajectories(gpu_ctx):
    """per scene: 5 distinct frames, their single runs of 40 steps, and the numpy oracle's 40 steps of frame 0; computed once"""
    out = {}
    for name, (ny, nx) in TRAJ.items():
        F = P.Frames(ny, nx, 5, seed=7)
        oracle = V.optimize(F.scene(0), F.Zc0[0], 40, alpha=10.0)
        out[name] = (F, single_runs(gpu_ctx, F, range(5), 40), oracle)
    return out


@pytest.mark.parametrize("name", sorted(TRAJ))
def test_trajectories_equal_the_singles(gpu_ctx, trajectories, name):
    F, want, oracle = trajectories[name]
    with refinement.SequenceRefiner(F.gridsetup, F.pics, 8, gpu_ctx) as sr:                  # 5 frames in a handle of 8
        got = batch_run(sr, F, range(5), 40)
        for f in range(5):
            assert_equal_runs(got[f], want[f], (name, f))
            assert [int(r[0]) for r in got[f][4]] == [0, 1, 11, 21, 31, 40]
        # the two device paths cannot be wrong together: frame 0 against numpy
        assert same(got[0][0], oracle[0]) and same(got[0][1], oracle[1]) and same(got[0][2], oracle[2])
        assert same(got[0][3], V.resize(F.scene(0), oracle[0]) * F.scene(0).mask)
        assert np.abs(got[0][0] - F.Zc0[0]).max() > 1e-3
        # 4 x 10 continued through get_state / set_state equal the 40
        sr.load(np.zeros((5,) + F.shape, np.float32), F.I0, F.I1, F.mask)
        sr.set_state(F.Zc0)
        for r in range(4):
            sr.optimize(10)
            Zc, m, v, step = sr.get_state()
            assert step == 10 * (r + 1)
            sr.load(np.ones((5,) + F.shape, np.float32), F.I0, F.I1, F.mask)                 # a load in between resets everything
            assert sr.get_state()[3] == 0 and float(sr.get_state()[1].abs().max()) == 0.0
            sr.set_state(Zc, m, v, step)
        for f in range(5):
            assert same(host(Zc)[f], want[f][0]) and same(host(m)[f], want[f][1]) and same(host(v)[f], want[f][2])
        # another report_every: the same Zc, the single path's trace lengths
        for every in (1, 7, 0):
            sr.set_state(F.Zc0)
            sr.optimize(40, report_every=every)
            Zc = host(sr.get_state()[0])
            rows = 2 if every == 0 else len(sorted({0, 40} | {i + 1 for i in range(0, 40, every)}))
            for f in range(5):
                assert same(Zc[f], want[f][0]) and len(sr.losses[f]) == rows
                assert same(sr.losses[f][[0, -1]], want[f][4][[0, -1]])


# ---------------------------------------------------------------------------------------------------------------- no leakage
def test_frames_do_not_leak_into_each_other(gpu_ctx, trajectories):
    F, _, _ = trajectories["65x67"]
    want = single_runs(gpu_ctx, F, range(5), 10)
    with refinement.SequenceRefiner(F.gridsetup, F.pics, 5, gpu_ctx) as sr:
        fwd = batch_run(sr, F, range(5), 10)
        rev = batch_run(sr, F, range(4, -1, -1), 10)
        for f in range(5):
            assert_equal_runs(fwd[f], want[f], ("forward", f))
            assert_equal_runs(rev[4 - f], want[f], ("reversed", f))
    # a handle of 4 loaded with 4, then 1, then 3 frames: each load's own singles; stale planes and state are not seen
    with refinement.SequenceRefiner(F.gridsetup, F.pics, 4, gpu_ctx) as sr:
        for frames in ((0, 1, 2, 3), (4,), (3, 0, 4)):
            got = batch_run(sr, F, frames, 10)
            assert len(got) == len(frames) == len(sr.losses)
            for k, f in enumerate(frames):
                assert_equal_runs(got[k], want[f], (frames, f))
        with pytest.raises(ValueError):
            sr.load(np.zeros((5,) + F.shape, np.float32), F.I0, F.I1, F.mask)                # 5 frames into a handle of 4
    # an all-zero mask in the middle: that frame comes back all NaN, its neighbours are what they are alone
    F2 = P.Frames(65, 67, 3, seed=7, masks=("ones", "zeros", "checkerboard"))
    Zi, _ = F2.surfaces()
    Zi = np.nan_to_num(Zi, nan=0.0)
    with refinement.SequenceRefiner(F2.gridsetup, F2.pics, 3, gpu_ctx) as sr:
        out = host(sr.refine(Zi, F2.I0, F2.I1, refinement.RefineOptions(max_iters=10), mask=F2.mask))
        _, m, v, _ = sr.get_state()
        assert float(m[1].abs().max()) == 0.0 and float(v[1].abs().max()) == 0.0
    assert np.isnan(out[1]).all()
    for f in (0, 2):
        alone = refinement.refine_surface(Zi[f], F2.mask[f], F2.I0[f], F2.I1[f], F2.gridsetup, ctx=gpu_ctx, max_iters=10)
        assert same(out[f], alone, nan=True) and np.isfinite(out[f]).any()


# ---------------------------------------------------------------------------------------------------------------- ingest, down-sampling, finish
@pytest.mark.parametrize("shape", [(24, 32), (13, 9), (65, 67)])
def test_refine_sequence_equals_refine_surface(gpu_ctx, shape, tmp_path):
    import torch
    F = P.Frames(*shape, 5, seed=11, baseline=2.5)
    Zi, mask = F.surfaces()
    assert np.isnan(Zi).any() and all(0 < m.sum() < m.size for m in mask)
    dev = torch.device("cuda", gpu_ctx.device_id)
    for iters in (0, 7):                                                     # 0: ingest, down-sampling and finish alone
        want = np.stack([refinement.refine_surface(Zi[f], mask[f], F.I0[f], F.I1[f], F.gridsetup, ctx=gpu_ctx, max_iters=iters) for f in range(5)])
        assert same(np.isnan(want), mask == 0)
        if iters:
            assert not same(want[0][mask[0] != 0], Zi[0][mask[0] != 0])
        for batch in (1, 2, 5):
            o = refinement.RefineOptions(max_iters=iters, batch=batch)
            got, losses = refinement.refine_sequence(Zi, F.I0, F.I1, F.gridsetup, options=o, ctx=gpu_ctx)       # mask: where Zi is not NaN
            assert got.dtype == np.float32 and same(got, want, nan=True), (shape, iters, batch)
            assert len(losses) == 5 and all(int(t[-1][0]) == iters for t in losses)
        o = refinement.RefineOptions(max_iters=iters, batch=2)
        # the caller's masks, per frame; a memmap in, a caller's array filled in place; device tensors in and out
        got, _ = refinement.refine_sequence(Zi, F.I0, F.I1, F.gridsetup, mask=mask, options=o, ctx=gpu_ctx)
        assert same(got, want, nan=True)
        mm = np.memmap(tmp_path / f"zi{iters}.bin", np.float32, "w+", shape=Zi.shape)
        mm[:] = Zi
        out = np.zeros(Zi.shape, np.float32)
        got, _ = refinement.refine_sequence(mm, F.I0, F.I1, F.gridsetup, options=o, ctx=gpu_ctx, out=out)
        assert got is out and same(out, want, nan=True)
        d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
        d_out = torch.zeros(Zi.shape, dtype=torch.float32, device=dev)
        got, _ = refinement.refine_sequence(d(Zi), d(F.I0), d(F.I1), F.gridsetup, options=o, ctx=gpu_ctx, out=d_out)
        assert got is d_out and same(host(d_out), want, nan=True)
    # uint8 pictures
    I0, I1 = np.round(F.I0).astype(np.uint8), np.round(F.I1).astype(np.uint8)
    got, _ = refinement.refine_sequence(Zi[:2], I0[:2], I1[:2], F.gridsetup, options=refinement.RefineOptions(max_iters=3, batch=2), ctx=gpu_ctx)
    for f in range(2):
        assert same(got[f], refinement.refine_surface(Zi[f], mask[f], I0[f], I1[f], F.gridsetup, ctx=gpu_ctx, max_iters=3), nan=True)


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_refusals(gpu_ctx):
    import torch
    F = P.Frames(13, 9, 4, seed=3)
    Zi, mask = F.surfaces()
    bad = Zi.copy()
    iy, ix = np.argwhere(mask[2] != 0)[5]
    bad[2, iy, ix] = np.inf
    for batch in (4, 2, 1):                                                  # frame 2 wherever it falls in its sub-batch
        with pytest.raises(ValueError, match="frame 2"):
            refinement.refine_sequence(bad, F.I0, F.I1, F.gridsetup, options=refinement.RefineOptions(max_iters=1, batch=batch), ctx=gpu_ctx)
    outside = Zi.copy()
    outside[2][mask[2] == 0] = np.inf                                        # outside the caller's mask nothing is looked at
    refinement.refine_sequence(outside, F.I0, F.I1, F.gridsetup, mask=mask, options=refinement.RefineOptions(max_iters=1), ctx=gpu_ctx)
    # through the C ABI
    lib, dev = gpu_ctx._lib, torch.device("cuda", gpu_ctx.device_id)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)          # noqa: E731
    d_Zi, d_I0, d_I1, d_bad = d(np.nan_to_num(Zi)), d(F.I0), d(F.I1), d(bad)
    d_Zc = torch.zeros((4,) + F.coarse, dtype=torch.float32, device=dev)
    d_out = torch.empty((4,) + F.shape, dtype=torch.float32, device=dev)
    torch.cuda.synchronize(dev)
    st, rows = C.c_int64(0), C.c_int(0)
    message = lambda: lib.wass_last_error(gpu_ctx._h).decode()               # noqa: E731
    with refinement.SequenceRefiner(F.gridsetup, F.pics, 3, gpu_ctx) as sr:
        h = sr._h
        load = lambda n, zi=d_Zi.data_ptr(), i0=d_I0.data_ptr(), i1=d_I1.data_ptr(): lib.wass_vref_batch_load(h, n, zi, None, i0, i1, 2.0)  # noqa: E731
        opt = lambda it: lib.wass_vref_batch_optimize(h, it, 10.0, 1e-3, 1e-7, 10, None, 0, C.byref(rows))                                 # noqa: E731
        assert opt(1) == -1 and "loaded" in message()                        # nothing is loaded yet
        assert lib.wass_vref_batch_result(h, d_out.data_ptr(), None) == -1
        assert load(0) == -1 and load(4) == -1 and "4 frames" in message() and load(-2) == -1
        assert load(2, zi=None) == -1 and "null" in message() and load(2, i0=None) == -1 and load(2, i1=None) == -1
        assert lib.wass_vref_batch_load(h, 2, d_Zi.data_ptr(), None, d_I0.data_ptr(), d_I1.data_ptr(), 0.0) == -1
        assert load(3, zi=d_bad.data_ptr()) == -1 and "frame 2" in message()
        assert opt(1) == -1                                                  # the refused load left nothing loaded
        assert load(3) == 0
        assert opt(-1) == -1 and "iters" in message()
        assert lib.wass_vref_batch_set_state(h, None, d_Zc.data_ptr(), d_Zc.data_ptr(), 0) == -1
        assert lib.wass_vref_batch_set_state(h, d_Zc.data_ptr(), d_Zc.data_ptr(), d_Zc.data_ptr(), -1) == -1
        assert lib.wass_vref_batch_get_state(h, d_Zc.data_ptr(), d_Zc.data_ptr(), d_Zc.data_ptr(), None) == -1
        assert lib.wass_vref_batch_result(h, None, None) == -1
        assert lib.wass_vref_optimize(h, d_Zc.data_ptr(), d_Zc.data_ptr(), d_Zc.data_ptr(), C.byref(st), 1, 10.0, 1e-3, 1e-7, 10, None, 0, C.byref(rows),
                                      None) == -1 and "batch" in message()   # a batch handle is none for the single entries
        # the context and the handle still work
        assert opt(2) == 0 and lib.wass_vref_batch_result(h, d_out.data_ptr(), None) == 0
    want = refinement.refine_surface(np.nan_to_num(Zi[1]), np.ones(F.shape), F.I0[1], F.I1[1], F.gridsetup, ctx=gpu_ctx, max_iters=2)
    assert same(host(d_out)[1], want, nan=True)
    with refinement.VariationalRefinement(ctx=gpu_ctx, **F.single(0)) as vr:
        assert lib.wass_vref_batch_load(vr._h, 1, d_Zi.data_ptr(), None, d_I0.data_ptr(), d_I1.data_ptr(), 2.0) == -1


# ---------------------------------------------------------------------------------------------------------------- grid_sequence
NX, NY = 32, 24


def _frames_on_disk(tmp_path, oracle, n):
    """n frame directories the way tests/test_vref_gpu.py writes its one: the rig's files, a mesh_cam.xyzC from the oracle's encoder
    and two textured PNGs, all distinct"""
    rng = np.random.default_rng(77)
    h, w = 60, 120
    Rpl, Tpl = gridding.sea_plane_RT(TS.PLANE)
    dirs, views = [], []
    for i in range(n):
        gx = rng.uniform(-13.0, 5.0, (h, w)); gy = rng.uniform(-37.0, -23.0, (h, w))
        hz = 0.2 * np.sin(gx * 0.8 + 0.4 * i) + 0.1 * np.cos(gy * 0.6 - 0.3 * i)
        aligned = np.stack([gx, gy, -hz]).reshape(3, -1) / TS.BASELINE
        p3d = np.ascontiguousarray((Rpl.T @ (aligned - Tpl)).T.reshape(h, w, 3))
        pics = [np.clip(V.texture(TS.IH, TS.IW, 20 + 2 * i + c), 0, 255).astype(np.uint8) for c in (0, 1)]
        wd = tmp_path / ("%06d_wd" % (2 * i + 3))
        TS.write_workdir(str(wd), picture=pics[0], mesh_bytes=oracle.encode_xyzc(np.ones((h, w), np.uint8), p3d, TS.PLANE))
        TS._write_png(os.path.join(str(wd), "undistorted", "00000001.png"), pics[1])
        dirs.append(str(wd)); views.append(pics)
    return dirs, views


def test_grid_sequence_refines_every_frame(gpu_ctx, oracle, tmp_path):
    n = 5
    dirs, views = _frames_on_disk(tmp_path, oracle, n)
    setup = gridding.setup_grid(dirs[0], TS.PLANE, TS.BASELINE, area_center=np.array([-4.0, -30.0]), area_size_x=16.0,
                                area_size_y=16.0 * (NY - 1) / (NX - 1), Nx=NX, Ny=NY, ctx=gpu_ctx)
    um = np.ones((NY, NX), np.uint8); um[:, :3] = 0; um[20:, 27:] = 0
    opts = {"Nfreqs": 12, "MAX_ITERS": 60}
    args = dict(baseline=TS.BASELINE, xmin=setup["xmin"], xmax=setup["xmax"], ymin=setup["ymin"], ymax=setup["ymax"], width=NX, height=NY)
    # the existing single chain: solve, filter, refine_surface, statistics
    plain, refined = [], []
    for d, (p0, p1) in zip(dirs, views):
        mesh = gridding.upload_camera_mesh(gpu_ctx, gridding.load_camera_mesh(os.path.join(d, "mesh_cam.xyzC")))
        g = mesh.grid_dct(TS.PLANE, **args, cell="median", dct_options=opts, user_mask=um)[0]
        mesh.close()
        zi = GS.median_blur(g, 3, um)
        plain.append(zi)
        refined.append(refinement.refine_surface(zi, ~np.isnan(zi), p0, p1, setup, ctx=gpu_ctx, max_iters=7))
    plain, refined = np.stack(plain), np.stack(refined)
    common = dict(mf=3, user_mask=um * 255, alg_options=opts, batch=5, ctx=gpu_ctx)
    for fzm in (False, True):
        want = GS.sequence_stats(refined, force_zero_mean=fzm)
        cube = GS.zero_mean(want["z_mm"], want["mean_perpoint_mm"]) if fzm else want["z_mm"]
        for rb in (1, 2, 5):
            res = gridding.grid_sequence(dirs, setup, force_zero_mean=fzm, refine=refinement.RefineOptions(max_iters=7, batch=rb), **common)
            assert same(res.Z, cube, nan=True), (fzm, rb)
            assert np.array_equal(res.mean_perpoint_mm, want["mean_perpoint_mm"], equal_nan=True)
            assert res.zmin == want["zmin"] and np.array_equal(res.frame_min, want["frame_min"]) and np.array_equal(res.frame_max, want["frame_max"])
            assert len(res.refine_losses) == n and all(int(t[0][0]) == 0 and int(t[1][0]) == 7 and len(t[0]) == 4 for t in res.refine_losses)
    # refine=None: what the sequence gave before, and nothing about the refinement is reported
    res = gridding.grid_sequence(dirs, setup, refine=refinement.RefineOptions(max_iters=7, batch=2), **common)
    none = gridding.grid_sequence(dirs, setup, refine=None, **common)
    before = gridding.grid_sequence(dirs, setup, **common)
    assert same(none.Z, before.Z, nan=True) and same(none.Z, GS.sequence_stats(plain)["z_mm"], nan=True) and none.refine_losses is None
    assert same(np.isnan(res.Z), np.isnan(none.Z)) and same(np.isnan(res.Z), np.broadcast_to(um == 0, res.Z.shape).copy())
    inside = ~np.isnan(res.Z)
    assert not np.array_equal(res.Z[inside], none.Z[inside]) and all(not np.array_equal(res.Z[f][inside[f]], none.Z[f][inside[f]]) for f in range(n))


# ---------------------------------------------------------------------------------------------------------------- end to end
E2E_HEIGHTS = (0.1, 0.08, 0.06)      # vref_oracle.E2E's plane and two lower ones: Adam moves at most about lr = 1e-3 a step, 0.12 in 120


def test_end_to_end_scene_three_planes_in_one_batch(gpu_ctx):
    """the scene of tests/test_vref.py as three frames, each looking at its own true plane: the single test's assertion on the
    masked RMS error per frame, and the oracle's surface bit for bit"""
    gs = TV.e2e_setup()
    N, iters, alpha = V.E2E["N"], V.E2E["iters"], V.E2E["alpha"]
    S0, args = V.e2e_scene(gs, TS.IH, TS.IW)
    I0 = np.stack([V.render_plane(args["Rp2c"], args["Tp2c"], gs["P0cam"], TS.IH, TS.IW, c0, V.E2E["waves"]).astype(np.float32) for c0 in E2E_HEIGHTS])
    I1 = np.stack([V.render_plane(args["Rp2c"], args["Tp2c"], gs["P1cam"], TS.IH, TS.IW, c0, V.E2E["waves"]).astype(np.float32) for c0 in E2E_HEIGHTS])
    assert same(I0[0], args["I0"]) and same(I1[0], args["I1"])
    mask = V.e2e_mask((N, N))
    zero = np.zeros((N, N), np.float32)
    with refinement.SequenceRefiner(gs, ((TS.IH, TS.IW), (TS.IH, TS.IW)), 3, gpu_ctx) as sr:
        sr.load(np.zeros((3, N, N), np.float32), I0, I1, np.stack([mask] * 3))
        sr.set_state(np.zeros((3, N // 2, N // 2), np.float32))
        sr.optimize(iters, alpha=alpha)
        _, Z = sr.result(with_plane=True)
        Z, losses = host(Z), sr.losses
    for f, c0 in enumerate(E2E_HEIGHTS):
        start, end = V.masked_rms(zero, c0, mask), V.masked_rms(Z[f], c0, mask)
        print(f"plane {c0}: masked rms {start:.4f} -> {end:.4f}; data loss {losses[f][0][1]:.3g} -> {losses[f][-1][1]:.3g}")
        assert end < 0.5 * start and Z[f][mask != 0].mean() > 0.5 * c0
        assert losses[f][-1][1] < losses[f][0][1] and int(losses[f][-1][0]) == iters
        S = V.scene(**dict(args, I0=I0[f], I1=I1[f]))
        wZc = V.optimize(S, np.zeros((N // 2, N // 2), np.float32), iters, alpha=alpha)[0]
        assert same(Z[f], V.resize(S, wZc) * S.mask)
