"""The prepare stage on the GPU: k_remap_cubic, k_warp_linear, k_undistort (rectify.hip) and the two CLAHE kernels (clahe.hip) on the
probes of tests/prepare_probes.py, bit for bit against the C oracle, which tests/test_prepare_edges.py ties to the direct restatement
of tests/prepare_direct.py and to hand answers.  Nothing of the reference is read here.

What is exact: everything, array_equal; a failure names the probe and the first differing pixel.  Every source is a window of a larger
array (a row stride above the width) and every destination a window of a guarded parent (tests/guarded.py), on the host entries and on
the device entries alike: a read with the wrong stride or a write outside ow x oh shows.

What each test can see, and the mistake it would catch:
  undistort, calibrated K   camera matrices whose inverse has ir[8] != 1, with 0, 4, 5, 8 and 12 coefficients, one row per stripe (5000 x 5)
                            and several (90 x 70): the refusal "camera matrix with skew is not supported" of an ordinary calibration;
                            prepare_pol goes through the same tables;
  table cache               A, B, A, C, A, B over (K, w, h), A and B sharing K: a hit that compares K alone, an entry evicted while in use;
  horizons                  W == 0, |W| = 2^-30, W < 0, bw0 = 64 and 204, whole and with an ROI that starts inside a block: 32 / W at
                            W == 0, a missing clamp, wrap for saturate, the block's origin taken from the ROI instead of the picture;
  windows                   every partial 4 x 4 and 2 x 2 window at four fractions on sources from 1 x 1, destinations 63 / 64 / 65 wide and
                            3 / 4 / 5 tall around the 64 x 4 thread block, ROIs at odd offsets;
  lattices, ties, extremes  all 1024 phases; exact ties of map * 32; coordinates beyond int16 and beyond int32;
  wrap                      the undistortion's plain cast to int16 where the other two saturate;
  CLAHE                     tiles_x != tiles_y, hand-worked residuals, ties of the table, clip 1 and 0, pictures smaller than the grid,
                            grids of different size one after the other in one table buffer.
test_every_mistake_misses_the_gpu: each switch of prepare_direct misses the GPU's result by the count that the oracle alone gives
(half of what the switch misses the oracle by, at least 1).  Every test prints its figures before it asserts."""
import ctypes as C

import numpy as np
import pytest

import prepare_direct as D
import prepare_pol_oracle as PP
import prepare_probes as PR
from guarded import Guarded, host

pytestmark = pytest.mark.gpu


def _same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, what
    bad = np.argwhere(got != want)
    print(f"{what}: {len(bad)} of {want.size} pixels differ")
    if len(bad):
        y, x = bad[0]
        pytest.fail(f"{what}: {len(bad)} of {want.size} pixels differ, the first at (x {x}, y {y}): {got[y, x]} for {want[y, x]}")


def _ptr(a):
    return a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data


def _row_stride(a):
    return a.stride(0) if hasattr(a, "data_ptr") else a.strides[0]


def _doubles(v):
    v = np.asarray(v, float).ravel()
    return (C.c_double * max(len(v), 1))(*v)


def _run(ctx, p, dev, roi=None):
    """One probe through the C entry of its kind (the device entry if `dev`): the source a strided window, the destination a window of a
    guarded parent; the guards are checked."""
    lib, h = ctx._lib, ctx._h
    g = Guarded(dev)
    src = g.input(np.asarray(p["src"])[None])[0]
    sh, sw = p["src"].shape
    assert _row_stride(src) > sw
    kind = p["kind"]
    if kind in ("remap", "warp"):
        dh, dw = p["my"].shape if kind == "remap" else (p["dh"], p["dw"])
        out = g.out((roi[3], roi[2]) if roi is not None else (dh, dw), np.uint8, dense=True)
        r = (C.c_int * 4)(*roi) if roi is not None else None
    else:
        out = g.out((sh, sw), np.uint8, dense=True)
    keep = []
    if dev:
        import torch
        keep = [torch.from_numpy(np.array(p[k])).cuda() for k in ("mx", "my") if k in p]
        torch.cuda.synchronize()                        # the library runs on a stream of its own
    maps = [_ptr(m) for m in keep] if dev else [p[k].ctypes.data for k in ("mx", "my") if k in p]
    if kind == "remap":
        rc = (lib.wass_remap_cubic_dev if dev else lib.wass_remap_cubic)(h, _ptr(src), sw, sh, _row_stride(src), maps[0], maps[1], dw, dh, r, _ptr(out))
    elif kind == "warp":
        rc = (lib.wass_warp_perspective_dev if dev else lib.wass_warp_perspective)(h, _ptr(src), sw, sh, _row_stride(src), _doubles(p["H"]), dw, dh, r, _ptr(out))
    elif kind == "undistort":
        rc = (lib.wass_undistort_dev if dev else lib.wass_undistort)(h, _ptr(src), sw, sh, _row_stride(src), _doubles(p["K"]), _doubles(p["dist"]),
                                                                     len(p["dist"]), _ptr(out))
    else:
        rc = (lib.wass_clahe_dev if dev else lib.wass_clahe)(h, _ptr(src), sw, sh, _row_stride(src), p["clip"], p["tiles_x"], p["tiles_y"], _ptr(out))
    ctx._check(rc)
    ctx.synchronize()
    g.check(f"{p['name']}, {'device' if dev else 'host'} entry")
    return host(out).copy()


_GPU = {}


def _gpu(ctx, p):
    """the whole destination through the host entry, computed once per probe"""
    if p["name"] not in _GPU:
        _GPU[p["name"]] = _run(ctx, p, False)
    return _GPU[p["name"]]


def _both_entries(ctx, oracle, p, roi=None):
    want = PR.oracle_answer(oracle, p)
    _same(_gpu(ctx, p), want, f"{p['name']}, host entry")
    _same(_run(ctx, p, True), want, f"{p['name']}, device entry")
    if roi is not None:
        for dev in (False, True):
            _same(_run(ctx, p, dev, roi), PR.crop(want, roi), f"{p['name']}, roi {roi}, {'device' if dev else 'host'} entry")


# ---- undistortion ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("camera", list(PR.CAMERAS))
def test_undistort_calibrated_cameras(gpu_ctx, oracle, camera):
    K, w, h = PR.CAMERAS[camera]
    print(f"{camera}: {w} x {h}, ir[8] - 1 = {PR.ir8(K) - 1.0:.3e}, {min(max(1, 4096 // w), h)} rows per stripe")
    for n in PR.DISTS:
        p = PR.probes()[f"undistort_{camera}_{n}"]
        _both_entries(gpu_ctx, oracle, p)
        _same(gpu_ctx.undistort(p["src"], K, p["dist"]), PR.oracle_answer(oracle, p), f"{p['name']}, Context.undistort")
    none = PR.probes()[f"undistort_{camera}_0"]
    assert np.array_equal(_gpu(gpu_ctx, none), _run(gpu_ctx, dict(none, dist=[0.0] * 4), False))                 # no coefficients: four zeros
    assert np.array_equal(_gpu(gpu_ctx, none), none["src"])                                                      # and the identity


def test_undistort_strong_distortion_and_wrap(gpu_ctx, oracle):
    _both_entries(gpu_ctx, oracle, PR.probes()["undistort_round_strong"])
    p = PR.probes()["wrap"]
    _both_entries(gpu_ctx, oracle, p)
    got = _gpu(gpu_ctx, p)
    sat = D.undistort(p["src"], p["K"], p["dist"], saturate_undistort=True)
    print(f"wrap: {int((got != sat).sum())} pixels are not what a saturating cast gives, all non-zero: {bool(np.all(got[got != sat] != 0))}")
    assert (got != sat).sum() >= 32 and np.all(got[got != sat] != 0)


def test_prepare_pol_takes_a_calibrated_camera(gpu_ctx):
    from wass_amd import prepare as W
    for camera in ("short", "diag1234"):
        K, w, h = PR.CAMERAS[camera]
        assert PR.ir8(K) != 1.0
        mosaic = PP.random_mosaic(h, w, 5)
        dist = np.array(PR.DISTS[5])
        want = PP.prepare(mosaic, K, dist)
        got = W.polarimetric_prepare(mosaic, K, dist, outputs=("stokes", "channels"), ctx=gpu_ctx)
        for field in ("S", "channels", "image"):
            g = np.asarray(getattr(got, field))
            bad = int((~((g == want[field]) | ((g != g) & (want[field] != want[field])))).sum())
            print(f"{camera}: {field} differs in {bad} of {g.size}")
            assert bad == 0


def test_table_cache_hit_after_eviction(gpu_ctx, oracle):
    """Two entries, replaced in turn: A, B, A, C, A, B.  A and B share K and differ in size (a hit must compare both), C evicts one of them,
    and the calls after it meet one entry that stayed and one that has to be rebuilt."""
    dist = PR.DISTS[5]
    pictures, answers = {}, {}
    for key in set(PR.CACHE_SEQUENCE):
        cam, w, h = key
        pictures[key] = PR.picture(w, h, 9)
        answers[key] = oracle.undistort(pictures[key], PR.CAMERAS[cam][0], dist)
    assert len(answers) == 3
    for k, key in enumerate(PR.CACHE_SEQUENCE):
        _same(gpu_ctx.undistort(pictures[key], PR.CAMERAS[key[0]][0], dist), answers[key], f"call {k}: {key}")


# ---- warps --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["horizon_zero", "horizon_tiny", "horizon_204", "tie_64", "tie_204", "lattice_warp"])
def test_warps(gpu_ctx, oracle, name):
    p = PR.probes()[name]
    _both_entries(gpu_ctx, oracle, p, p["roi"])
    _same(gpu_ctx.warp_perspective(p["src"], p["H"], p["dw"], p["dh"], roi=p["roi"]), PR.crop(PR.oracle_answer(oracle, p), p["roi"]), f"{name}, Context.warp_perspective")


@pytest.mark.parametrize("sw,sh", PR.SIZES)
def test_border_windows_linear(gpu_ctx, oracle, sw, sh):
    cases = [p for p in PR.of_kind("warp") if p["name"].startswith(f"border_warp_{sw}x{sh}_")]
    assert len(cases) == 16
    for k, p in enumerate(cases):
        want = PR.oracle_answer(oracle, p)
        _same(_run(gpu_ctx, p, k % 2 == 1), want, p["name"])
        assert (want[0] == 0).all() and (want[:, -1] == 0).all() and want.any()          # wholly outside along the rim, not everywhere


# ---- maps ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sw,sh", PR.SIZES)
def test_border_windows_cubic(gpu_ctx, oracle, sw, sh):
    p = PR.probes()[f"border_map_{sw}x{sh}"]
    x, y, w, h = p["roi"]
    assert x % 2 == 1 and y % 2 == 1
    _both_entries(gpu_ctx, oracle, p, p["roi"])
    want = PR.oracle_answer(oracle, p)
    assert (want[0] == 0).all() and (want[:, -1] == 0).all() and want.any()


@pytest.mark.parametrize("name", ["lattice_map", "ties_map", "extreme_map"])
def test_maps(gpu_ctx, oracle, name):
    p = PR.probes()[name]
    _both_entries(gpu_ctx, oracle, p, p["roi"])
    _same(gpu_ctx.remap_cubic(p["src"], p["mx"], p["my"]), PR.oracle_answer(oracle, p), f"{name}, Context.remap_cubic")


@pytest.mark.parametrize("dh", [3, 4, 5])
@pytest.mark.parametrize("dw", [63, 64, 65])
def test_destinations_around_the_thread_block(gpu_ctx, oracle, dw, dh):
    """64 x 4 threads per block: one block exactly, one column or row short, one over."""
    lat = PR.probes()["lattice_map"]
    p = dict(lat, name=f"lattice_map_{dw}x{dh}", mx=np.ascontiguousarray(lat["mx"][7:7 + dh, 31:31 + dw]), my=np.ascontiguousarray(lat["my"][7:7 + dh, 31:31 + dw]), roi=None)
    want = PR.crop(PR.oracle_answer(oracle, lat), (31, 7, dw, dh))                        # the remap knows nothing of its neighbours
    for dev in (False, True):
        _same(_run(gpu_ctx, p, dev), want, f"{p['name']}, {'device' if dev else 'host'} entry")
    q = dict(PR.probes()["lattice_warp"], name=f"lattice_warp_{dw}x{dh}", dw=dw, dh=dh, roi=None)
    want = oracle.warp_perspective(q["src"], q["H"], dw, dh)
    for dev in (False, True):
        _same(_run(gpu_ctx, q, dev), want, f"{q['name']}, {'device' if dev else 'host'} entry")
    roi = (1, 1, dw - 2, dh - 2)
    _same(_run(gpu_ctx, q, True, roi), PR.crop(want, roi), f"{q['name']}, roi {roi}")


# ---- CLAHE ----------------------------------------------------------------------------------------------------------------------------------------
def test_clahe_probes(gpu_ctx, oracle):
    cases = PR.of_kind("clahe")
    grids = {(p["tiles_x"], p["tiles_y"]) for p in cases}
    print(f"{len(cases)} probes, {len(grids)} grids, {sum(tx != ty for tx, ty in grids)} of them not square")
    for p in cases:
        _both_entries(gpu_ctx, oracle, p)


def test_clahe_grids_of_different_size_in_turn(gpu_ctx, oracle):
    """the table buffer is kept between calls: 300 tiles, 21, 300 again, 21 the other way round, 1"""
    for k, name in enumerate(("grid_150x2", "grid_3x7", "grid_150x2", "grid_7x3", "area510", "grid_2x150", "grid_7x3")):
        p = PR.probes()[name]
        _same(_run(gpu_ctx, p, k % 2 == 0), PR.oracle_answer(oracle, p), f"call {k}: {name}")


def test_clahe_hand_answers(gpu_ctx):
    for p, levels, r in PR.hand_cases():
        want = PR.hand_answer(levels, r, p["src"].size)
        expect = np.zeros_like(p["src"])
        for v, o in want.items():
            expect[p["src"] == v] = o
        _same(_gpu(gpu_ctx, p), expect, f"{p['name']} (residual {r})")


# ---- every mistake misses the GPU --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("switch", D.SWITCHES)
def test_every_mistake_misses_the_gpu(gpu_ctx, oracle, switch):
    for name in PR.SWITCH_PROBES[switch]:
        p = PR.probes()[name]
        bound, found = PR.switch_bound(oracle, switch, name)
        got = _gpu(gpu_ctx, p)
        miss = int((PR.run_direct(p, **{switch: True}) != got).sum())
        right = int((PR.run_direct(p) != got).sum())
        print(f"{switch} on {name}: the variant misses the GPU in {miss} pixels (the oracle in {found}; bound {bound}); the restatement without it in {right}")
        assert miss >= bound
        assert right == 0
