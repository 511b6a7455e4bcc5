"""Grid set-up on the GPU: wass_quantiles_f64_dev and wass_mesh_aligned_z_quantiles against tests/grid_setup_oracle.py, bit for bit
(sizes at the launch shape's edges, value sets in which each pass of the selection decides, NaN, empty input, validity patterns),
and setup_grid end to end on a synthetic work directory, into grid_sequence and radiance, from the dict and from config.mat."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import grid_bin_oracle as B
import grid_setup_oracle as G
import test_grid_setup as TS
import wass_amd
from wass_amd import gridding
from wass_amd.stereo import quantiles_launch_shape

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QS = (0.0, 0.02, 0.5, 0.98, 1.0)


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _dev(ctx, a):
    import torch
    d = torch.from_numpy(np.ascontiguousarray(a, np.float64)).to(torch.device("cuda", ctx.device_id))
    torch.cuda.synchronize()
    return d


def _check(ctx, a, qs=QS, together=True, by_value=False):
    """every q alone and all of them in one call against the oracle: the same bits (NaN equal to NaN)"""
    d = _dev(ctx, a)
    want = G.quantile(a, list(qs))
    calls = [([q], want[i:i + 1]) for i, q in enumerate(qs)] + ([(list(qs), want)] if together else [])
    for q, w in calls:
        got = ctx.quantiles_dev(d, q)
        if by_value:
            assert np.array_equal(got, w, equal_nan=True), (q, got, w)
        else:
            nan = np.isnan(w)
            assert np.array_equal(np.isnan(got), nan) and np.array_equal(_bits(got)[~nan], _bits(w)[~nan]), (len(a), q, got, w)
    return want


def _sizes():
    per_block, per_launch = quantiles_launch_shape()
    return [1, 2, 3, 255, 256, 257, per_block - 1, per_block, per_block + 1, per_launch - 1, per_launch, per_launch + 1, 100_003]


def test_launch_shape_is_what_the_sizes_below_assume():
    per_block, per_launch = quantiles_launch_shape()
    assert 256 <= per_block < per_launch <= 1 << 23 and per_launch % per_block == 0


@pytest.mark.parametrize("k", range(13))
def test_quantiles_at_every_size_edge(gpu_ctx, k):
    n = _sizes()[k]
    a = np.random.default_rng(n).normal(0.1, 0.7, n)
    _check(gpu_ctx, a)


# ---- value sets in which one pass decides.  Each asserts on the host first that the selection with that pass left out gives
# another answer (grid_setup_oracle.select), so the set can fail.
def _decides(a, q, p):
    full, skipped = G.select(a, q), G.select(a, q, skip=p)
    assert np.array_equal(_bits(full), _bits(G.quantile(a, q)))
    assert not np.array_equal(_bits(full), _bits(skipped)), f"pass {p} does not decide on this set"


def _from_bits(base, shift, count, rng, repeat=3):
    """count values whose bit patterns differ from base's only in the digit at `shift`, each up to `repeat` times, shuffled"""
    u = np.float64(base).view(np.uint64) + (np.arange(1, count + 1, dtype=np.uint64) << np.uint64(shift))
    return rng.permutation(np.repeat(u, rng.integers(1, repeat + 1, count))).view(np.float64)


@pytest.mark.parametrize("p", range(6))
def test_each_digit_pass_decides(gpu_ctx, p):
    rng = np.random.default_rng(40 + p)
    if p == 0:                                               # the top digit: the sign and ten bits of the exponent
        a = rng.permutation(np.concatenate([2.0 ** (2 * np.arange(-40, 41)), -(2.0 ** (2 * np.arange(-12, 30)))]))
    else:
        a = _from_bits(1.0, G.SHIFTS[p], min(700, (1 << G.NBITS[p]) - 2), rng)
        if p == 5:
            assert (np.diff(np.unique(_bits(a))) == 1).all()                  # neighbours one ulp apart: only the lowest bits differ
    for q in (0.3, 0.5, 0.98):
        _decides(a, q, p)
    _check(gpu_ctx, a, qs=(0.0, 0.3, 0.5, 0.98, 1.0))
    _check(gpu_ctx, -a, qs=(0.0, 0.3, 0.5, 0.98, 1.0))                        # the same digits under the flipped keys


def test_sign_only_denormals_and_infinities(gpu_ctx):
    rng = np.random.default_rng(7)
    a = rng.permutation(np.concatenate([np.full(30, 0.75), np.full(21, -0.75)]))   # values that differ in the sign only
    _decides(a, 0.5, 0)
    _check(gpu_ctx, a)
    den = rng.permutation(np.concatenate([(np.arange(1, 400, dtype=np.uint64) * np.uint64(7)).view(np.float64),
                                          -(np.arange(1, 300, dtype=np.uint64) * np.uint64(5)).view(np.float64)]))
    assert (np.abs(den) < 2.3e-308).all() and (den != 0).all()
    _decides(den, 0.9, 4)
    _decides(den, 0.5, 5)
    _check(gpu_ctx, den)
    inf = rng.normal(size=101)
    inf[[3, 50]] = np.inf; inf[[4, 77, 78]] = -np.inf
    _decides(inf, 0.5, 0)
    want = _check(gpu_ctx, inf)                                               # q = 0 and 1 hit inf - inf in numpy's lerp: NaN
    assert np.isnan(want[[0, 4]]).all() and np.isfinite(want[1:4]).any()
    zeros = rng.permutation(np.concatenate([np.full(20, -0.0), np.full(20, 0.0), [-1.0, 1.0]]))
    _check(gpu_ctx, zeros, by_value=True)                                      # numpy leaves the order of the two zeros open


def test_ties_and_the_next_value_pass(gpu_ctx):
    rng = np.random.default_rng(11)
    # half of the array equals the answer (sorted positions 250 .. 749): lo and hi both lie in the run of ties with a weight
    # strictly between 0 and 1, so taking the next larger key for a[hi] would change the answer; at 0.7495 lo is the last tie
    a = rng.permutation(np.concatenate([np.full(500, 0.125), rng.uniform(-1, 0.125, 250), rng.uniform(0.126, 1, 251)]))
    tie_qs = (0.2503, 0.4003, 0.5007, 0.6502, 0.7489)
    lo, hi, gamma = G.indexes(a.size, tie_qs)
    assert (lo >= 250).all() and (hi <= 749).all() and (hi == lo + 1).all() and ((gamma > 0.05) & (gamma < 0.95)).all()
    assert (G.quantile(a, tie_qs) == 0.125).all()
    for q in tie_qs:
        _decides(a, q, "tie")
    _check(gpu_ctx, a, qs=tie_qs)
    lo, hi, gamma = G.indexes(a.size, 0.7495)
    assert (lo[0], hi[0]) == (749, 750) and 0 < gamma[0] < 1
    _decides(a, 0.7495, "next")
    _check(gpu_ctx, a, qs=(0.02, 0.25, 0.5, 0.7495, 0.98))
    # the last of the ties is a[lo]: a[hi] is the next value up
    b = np.concatenate([np.full(6, 2.0), [3.0, 5.0, 9.0, 17.0, 33.0]])
    lo, hi, gamma = G.indexes(b.size, 0.55)
    assert (lo[0], hi[0]) == (5, 6) and 0 < gamma[0] < 1
    _decides(b, 0.55, "next")
    _check(gpu_ctx, rng.permutation(b), qs=(0.45, 0.5, 0.55, 0.62, 0.95))
    # a[hi] is the array's maximum
    lo, hi, _ = G.indexes(b.size, 0.95)
    assert (lo[0], hi[0]) == (9, 10)
    _decides(b, 0.95, "next")
    # sorted, reversed and shuffled copies: identical bits
    c = rng.normal(size=5000)
    outs = [gpu_ctx.quantiles_dev(_dev(gpu_ctx, v), list(QS)) for v in (np.sort(c), np.sort(c)[::-1].copy(), rng.permutation(c))]
    assert np.array_equal(_bits(outs[0]), _bits(outs[1])) and np.array_equal(_bits(outs[0]), _bits(outs[2]))
    assert np.array_equal(_bits(outs[0]), _bits(G.quantile(c, list(QS))))


def test_nan_empty_and_argument_errors(gpu_ctx):
    import torch
    a = np.random.default_rng(5).normal(size=3000)
    for pos, val in ((1234, np.nan), (0, -np.nan), (2999, np.nan)):
        b = a.copy(); b[pos] = val
        assert np.isnan(gpu_ctx.quantiles_dev(_dev(gpu_ctx, b), list(QS))).all()
    assert np.isnan(gpu_ctx.quantiles_dev(_dev(gpu_ctx, np.array([np.nan])), [0.5])).all()
    empty = torch.empty(0, dtype=torch.float64, device=torch.device("cuda", gpu_ctx.device_id))
    assert np.isnan(gpu_ctx.quantiles_dev(empty, list(QS))).all()            # n = 0: NaN, and the call succeeds (no exception)
    dp = C.POINTER(C.c_double)
    q, out = np.array([0.5] * 9), np.zeros(9)
    call = lambda qq, nq: gpu_ctx._lib.wass_quantiles_f64_dev(gpu_ctx._h, None, 0, qq.ctypes.data_as(dp), nq, out.ctypes.data_as(dp))  # noqa: E731
    assert call(q, 8) == 0 and np.isnan(out[:8]).all()
    assert call(q, 9) == -1 and call(q, 0) == -1
    assert call(np.array([1.5]), 1) == -1 and call(np.array([np.nan]), 1) == -1 and call(np.array([-1e-9]), 1) == -1
    with pytest.raises(ValueError):
        gpu_ctx.quantiles_dev(empty.to(torch.float32), [0.5])


# ---- the mesh entry
PATTERNS = ("none", "one", "all", "first", "last", "checkerboard", "row")


def _pattern(name, h, w):
    v = np.zeros((h, w), np.uint8)
    if name == "one":
        v[h // 2, w // 2] = 1
    elif name == "all":
        v[:] = 1
    elif name == "first":
        v[0, 0] = 1
    elif name == "last":
        v[-1, -1] = 1
    elif name == "checkerboard":
        v[(np.add.outer(np.arange(h), np.arange(w)) % 2) == 0] = 1
    elif name == "row":
        v[h // 2] = 1
    return v


@pytest.mark.parametrize("h,w", [(1, 1), (1, 257), (5, 513)])
def test_mesh_aligned_z_quantiles(gpu_ctx, h, w):
    rng = np.random.default_rng(h * w)
    tilted, Tt = G.sea_plane_RT(TS.PLANE)
    p3d = np.stack([rng.uniform(-30, 30, (h, w)), rng.uniform(-5, 3, (h, w)), rng.uniform(10, 40, (h, w))], axis=-1)
    for fill in (np.nan, 1e300):
        for name in PATTERNS:
            valid = _pattern(name, h, w)
            pts = p3d.copy()
            pts[valid == 0] = fill                           # what an invalid point holds must not leak into the result
            mesh = gpu_ctx.mesh_upload(valid, pts)
            for R, T in ((np.eye(3), np.array([0.0, 0.0, -11.0])), (tilted, Tt.ravel())):
                for baseline in (1.0, 2.5):
                    got, n = mesh.aligned_z_quantiles(R, T, baseline, list(QS))
                    z = G.aligned_z(pts[valid != 0], R, T, baseline)
                    want = G.quantile(z, list(QS))
                    assert n == int(valid.sum()) == z.size, (name, n)
                    if z.size == 0:
                        assert np.isnan(got).all()
                    else:
                        assert np.isfinite(want).all() and np.array_equal(_bits(got), _bits(want)), (name, fill, baseline, got, want)
            mesh.close()
    # a NaN in a valid point is a NaN among the values
    valid = np.ones((h, w), np.uint8)
    pts = p3d.copy(); pts[-1, -1, 1] = np.nan
    mesh = gpu_ctx.mesh_upload(valid, pts)
    got, n = mesh.aligned_z_quantiles(tilted, Tt, 2.5, [0.02, 0.98])
    assert n == h * w and np.isnan(got).all()
    mesh.close()


def test_repeat_calls_and_two_contexts_give_the_same_bits(gpu_ctx):
    rng = np.random.default_rng(99)
    h, w = 37, 301
    p3d = np.stack([rng.uniform(-30, 30, (h, w)), rng.uniform(-5, 3, (h, w)), rng.uniform(10, 40, (h, w))], axis=-1)
    valid = (rng.random((h, w)) < 0.8).astype(np.uint8)
    R, T = G.sea_plane_RT(TS.PLANE)
    a = rng.normal(size=70_001)
    outs = []
    with wass_amd.Context(0) as other:
        for ctx in (gpu_ctx, other, gpu_ctx):
            mesh = ctx.mesh_upload(valid, p3d)
            outs.append(np.concatenate([mesh.aligned_z_quantiles(R, T, 2.5, list(QS))[0], ctx.quantiles_dev(_dev(ctx, a), list(QS)),
                                        mesh.aligned_z_quantiles(R, T, 2.5, [0.98, 0.02])[0]]))
            mesh.close()
    assert np.array_equal(_bits(outs[0]), _bits(outs[1])) and np.array_equal(_bits(outs[0]), _bits(outs[2]))
    assert np.array_equal(_bits(outs[0][:5]), _bits(G.quantile(G.aligned_z(p3d[valid != 0], R, T, 2.5), list(QS))))


# ---- end to end
NX, NY = 64, 48
AREA = dict(area_center=np.array([-4.0, -30.0]), area_size_x=16.0, area_size_y=16.0 * (NY - 1) / (NX - 1), Nx=NX, Ny=NY)


@pytest.fixture(scope="module")
def workdir(tmp_path_factory, oracle):
    """A sequence directory with one frame: a plane plus a sinusoid, 20 000 points, a 320 x 240 picture that is a ramp in x."""
    root = tmp_path_factory.mktemp("gridsetup")
    rng = np.random.default_rng(321)
    h, w = 100, 200
    Rpl, Tpl = G.sea_plane_RT(TS.PLANE)
    gx = rng.uniform(-13.0, 5.0, (h, w)); gy = rng.uniform(-37.0, -23.0, (h, w))       # grid frame, metres
    hz = 0.2 * np.sin(gx * 0.8) + 0.1 * np.cos(gy * 0.6)
    aligned = np.stack([gx, gy, -hz]).reshape(3, -1) / TS.BASELINE
    p3d = np.ascontiguousarray((Rpl.T @ (aligned - Tpl)).T.reshape(h, w, 3))
    picture = np.broadcast_to(np.minimum(np.arange(TS.IW), 255).astype(np.uint8), (TS.IH, TS.IW)).copy()
    wd = root / "000000_wd"
    TS.write_workdir(str(wd), picture=picture, mesh_bytes=oracle.encode_xyzc(np.ones((h, w), np.uint8), p3d, TS.PLANE))
    np.savetxt(root / "planes.txt", np.vstack([TS.PLANE, [np.nan] * 4, TS.PLANE]))
    return root, wd, picture


def test_setup_grid_end_to_end(gpu_ctx, oracle, workdir, tmp_path):
    """grid_sequence's surface is held to the DCT tests' bound (test_grid_dct_gpu.assert_matches: rms inside the footprint within
    1 % of the data's spread, data loss within 2 %, the same step count) against a solution that owes nothing to the GPU: the
    cloud binned by tests/grid_bin_oracle.py with the set-up's extent, solved by tests/dct_oracle.py in float32 from the seeded
    start value.  The equality with the single-frame GPU path is kept beside it."""
    import dct_oracle as D
    from test_grid_dct_gpu import assert_matches
    import scipy.io
    from wass_amd import postproc
    root, wd, picture = workdir
    plane = gridding.mean_plane(root / "planes.txt")
    assert np.array_equal(plane, TS.PLANE)
    res = gridding.setup_grid(wd, plane, TS.BASELINE, **AREA, fps=10.0, timestring="t0", ctx=gpu_ctx, outdir=tmp_path)
    assert set(res) == set(gridding.CONFIG_MAT_KEYS) | {"cam0_rectified", "coverage"}
    # zmin / zmax from the oracle's quantiles of the cloud as the file holds it
    pts = gridding.load_camera_mesh(wd / "mesh_cam.xyzC")
    Rpl, Tpl = G.sea_plane_RT(plane)
    z02, z98 = G.quantile(G.aligned_z(pts.T, Rpl, Tpl, TS.BASELINE), [0.02, 0.98])
    assert (res["zmin"], res["zmax"]) == G.zrange(z02, z98) and 0.3 < res["zmax"] < 0.5
    f = TS.rig_files()
    want = gridding.setup_algebra(f["K0"], f["K1"], f["R"], f["T"], f["P0cam"], f["P1cam"], plane, TS.BASELINE, **AREA, Iw=TS.IW, Ih=TS.IH,
                                  z_q02=z02, z_q98=z98, fps=10.0, timestring="t0")
    for k in gridding.CONFIG_MAT_KEYS:
        assert np.array_equal(np.asarray(res[k]), np.asarray(want[k])), k
    # the rectified picture and the coverage
    assert res["cam0_rectified"].shape == (NY, NX) and res["cam0_rectified"].dtype == np.uint8
    assert np.array_equal(res["cam0_rectified"], oracle.warp_perspective(picture, res["Hcam0toTexture"], NX, NY))
    assert res["cam0_rectified"].max() > res["cam0_rectified"].min()
    ax, ay, az = B.align(pts.T, Rpl, Tpl, TS.BASELINE)
    cell, ok = B.bin(ax, ay, B.GridSpec(res["xmin"], res["xmax"], res["ymin"], res["ymax"], NX, NY))
    filled = int((B.counts(cell, ok, NX, NY) > 0).sum())
    assert res["coverage"] == filled / (NX * NY) and 0.5 < res["coverage"] < 1.0
    # the files
    back = scipy.io.loadmat(str(tmp_path / "config.mat"))
    assert set(k for k in back if not k.startswith("__")) == set(gridding.CONFIG_MAT_KEYS)
    from PIL import Image
    with Image.open(tmp_path / "cam0_rectified.png") as im:
        assert np.array_equal(np.asarray(im), res["cam0_rectified"])
    # into grid_sequence, from the dict and from the file
    opts = {"Nfreqs": 24, "MAX_ITERS": 120}
    seq = gridding.grid_sequence([str(wd)], res, alg_options=opts, ctx=gpu_ctx)
    seq2 = gridding.grid_sequence([str(wd)], str(tmp_path / "config.mat"), alg_options=opts, ctx=gpu_ctx)
    assert seq.Z.shape == (1, NY, NX) and np.array_equal(seq.Z, seq2.Z, equal_nan=True) and np.array_equal(seq.time, [0.0])
    mesh = gridding.upload_camera_mesh(gpu_ctx, pts)
    single = mesh.grid_dct(plane, TS.BASELINE, res["xmin"], res["xmax"], res["ymin"], res["ymax"], NX, NY, cell="median", dct_options=opts)[0]
    mesh.close()
    assert np.array_equal(seq.Z[0], single * np.float32(1000)) and np.isfinite(seq.Z).all()
    cells = B.cells_median(cell, ok, az, NX, NY).astype(np.float32)
    want, _, steps, _, _ = D.interpolate(cells, D.splitmix_x0(0, opts["Nfreqs"]), opts, dtype=np.float32)
    info = seq.dct_info[0]
    print("surface against the oracle: rms %.3g of std %.3g; steps %d / %d" % (
        np.sqrt(np.nanmean((seq.Z[0] / np.float32(1000) - want)[~np.isnan(cells)].astype(np.float64) ** 2)), np.nanstd(cells), info["steps"], steps))
    assert_matches(seq.Z[0] / np.float32(1000), want, cells, info["data_loss"], info["steps"], steps)
    assert 0.1 < np.nanstd(cells) < 0.25                                         # metres: the sinusoids are there
    # into radiance: the picture is the ramp I(x) = x, so a cell reads its own pixel column.  Bound, in grey levels: 0.5 for the
    # sampler's rounding to uint8, 1/64 for its 1/32-pixel positions, 0.05 for Lanczos4 not reproducing a ramp exactly
    # (its quantised 8-tap weights sum to one; their first moment is within a few hundredths of the offset).
    for setup in (res, back):
        rad = postproc.radiance(picture[None], seq.Z, setup["XX"], setup["YY"], setup["P0plane"], ctx=gpu_ctx)
        pcam = postproc.radiance_pcam(setup["P0plane"], TS.IW, TS.IH)
        z = (seq.Z[0] * np.float32(1e-3)).astype(np.float64)
        g = np.stack([setup["XX"], setup["YY"], z, np.ones_like(z)])
        pix = np.einsum("ij,jyx->iyx", pcam, g)
        px, py = pix[0] / pix[2], pix[1] / pix[2]
        assert px.min() > 8 and px.max() < 247 and py.min() > 8 and py.max() < TS.IH - 8
        assert np.abs(rad[0].astype(np.float64) * 255.0 - px).max() <= 0.5 + 1.0 / 64 + 0.05


def test_command_line_setup(workdir, tmp_path):
    import scipy.io
    root, wd, _ = workdir
    cfg = tmp_path / "gridconfig.txt"
    cfg.write_text("[Area]\narea_center_x=-4.0\narea_center_y=-30.0\narea_size_x=16\narea_size_y=%r\nNx=%d\nNy=%d\n" % (AREA["area_size_y"], NX, NY))
    p = subprocess.run([sys.executable, "-m", "wass_amd.gridding", str(root), str(tmp_path), "--action", "setup", "--gridconfig", str(cfg),
                        "-b", "2.5", "-f", "10", "-t", "t0", "-n", "1"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    back = scipy.io.loadmat(str(tmp_path / "config.mat"))
    assert back["XX"].shape == (NY, NX) and float(back["CAM_BASELINE"].squeeze()) == 2.5 and float(back["fps"].squeeze()) == 10.0
    assert float(back["zmax"].squeeze()) == -float(back["zmin"].squeeze()) > 0.3
    assert (tmp_path / "cam0_rectified.png").exists()
