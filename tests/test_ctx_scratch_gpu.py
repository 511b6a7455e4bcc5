"""The scratch the operators carve out of the context's buffers (csrc/scratch.h: measure, ensure, carve), where it can go wrong
and the oracles' tests do not look: pointers carved before ensure() moved the buffer, or carved for another size.  Every operator
runs a small problem, one whose scratch crosses the 1 MiB step of ensure() (the buffer is reallocated) and the small one again,
all on one context: the third result equals the first bit for bit, and the second equals the same call on a fresh context.
Then: a context that has filled a dozen buffers gives all of their memory back when it is destroyed."""
import ctypes as C
import functools

import numpy as np
import pytest

import autocal_oracle as AO
import epipolar_oracle as EO
import match_oracle as M
import prepare_pol_oracle as PP
import wass_amd
from wass_amd import autocalibrate as AC
from wass_amd import epipolar as EP
from wass_amd import match
from wass_amd import prepare as W
from wass_amd.stereo import grid_setup

pytestmark = pytest.mark.gpu

MIB = 1 << 20
SMALL, LARGE = 0, 1


def _flat(v):
    """the arrays and scalars of a result, in a fixed order"""
    if v is None:
        return [np.zeros(0)]
    if isinstance(v, np.ndarray):
        return [v]
    if isinstance(v, dict):
        return [x for k in sorted(v) for x in _flat(v[k])]
    if isinstance(v, (list, tuple)):
        return [x for e in v for x in _flat(e)]
    if hasattr(v, "__dataclass_fields__"):
        return [x for k in v.__dataclass_fields__ for x in _flat(getattr(v, k))]
    return [np.asarray(v)]


def _assert_same_bits(got, want, what):
    g, w = _flat(got), _flat(want)
    assert len(g) == len(w) and len(g) > 0, what
    for k, (a, b) in enumerate(zip(g, w)):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), f"{what}: part {k} of the result differs"


def _grow_shrink_grow(run, what):
    with wass_amd.Context(0) as ctx:
        first, second, third = run(ctx, SMALL), run(ctx, LARGE), run(ctx, SMALL)
    with wass_amd.Context(0) as fresh:
        alone = run(fresh, LARGE)
    _assert_same_bits(third, first, f"{what}: the small problem after the large one")
    _assert_same_bits(second, alone, f"{what}: the large problem after the small one")


# ----------------------------------------------------------------------------------------------------------------------- match
@functools.lru_cache(maxsize=None)
def _match_inputs(size):
    """pairs of feature sets for gt_match_batch (6 candidates; 64 problems of 192) and one problem for the host form of the payoff
    (6 candidates; 400, a matrix of 1.28 MB in the staging buffer)"""
    n, k, pairs = (3, 2, 1) if size == SMALL else (64, 3, 64)
    feats = []
    for seed in range(pairs):
        fa, fb, da, db, _ = M.scene(100 + seed, n=n)
        feats.append((match.Features(fa[:, :2], fa[:, 2], fa[:, 3], da), match.Features(fb[:, :2], fb[:, 2], fb[:, 3], db)))
    m = 3 if size == SMALL else 200
    fa, fb, _, _, _ = M.scene(7, n=m)
    i = np.arange(m, dtype=np.int32)
    cand = np.concatenate([np.stack([i, i], 1), np.stack([i, (i + 1) % m], 1)])
    return feats, k, fa, fb, cand


def _iidyn_host(ctx, A, max_iters):
    """wass_match_iidyn, the host form of the dynamics from the uniform start (match.iidyn takes the device form)"""
    n = A.shape[0]
    x, group = np.zeros(n), np.zeros(n, np.uint8)
    steps, size, err = C.c_int(), C.c_int(), C.c_double()
    ctx._check(ctx._lib.wass_match_iidyn(ctx._h, A.ctypes.data, n, x.ctypes.data, 1, C.c_double(1e-20), max_iters, C.c_double(0.7), C.byref(steps),
                                         C.byref(err), group.ctypes.data, C.byref(size)))
    return x, np.flatnonzero(group), steps.value, err.value


def _match(ctx, size):
    """the candidates' host form and the round (gt_match_batch), the payoff's host form, both forms of the dynamics"""
    feats, k, fa, fb, cand = _match_inputs(size)
    res = match.gt_match_batch(feats, k=k, max_rounds=1, max_iters=200, ctx=ctx)
    A = match.payoff_matrix(fa, fb, cand, ctx=ctx)
    dyn, host = match.iidyn(A, max_iters=50, ctx=ctx), _iidyn_host(ctx, A, 50)
    _assert_same_bits(host, (dyn.x, dyn.group, dyn.steps, dyn.err), "the host form of the dynamics against the device form")
    return [(r.matches, r.rounds) for r in res], A, dyn


def test_match_grow_shrink_grow():
    feats, k, _, _, cand = _match_inputs(LARGE)
    batch, nmax = len(feats), len(feats[0][0]) * k
    own = match.scratch_bytes(batch, nmax) - batch * (nmax * nmax * 8 + nmax * 8 + nmax + 2 * nmax * 4)
    assert own > MIB and cand.shape[0] ** 2 * 8 > MIB                            # the context's layout and the staging both grow
    _grow_shrink_grow(_match, "match")


# -------------------------------------------------------------------------------------------------------------------- epipolar
EPI_ROUNDS = (16, 2000)


def _epipolar(ctx, size):
    _, x0, x1, _, t = EO.select_scene(8)
    return EP.find_essential_batch([(x0, x1)], t, rounds=EPI_ROUNDS[size], ctx=ctx)


def test_epipolar_grow_shrink_grow():
    assert EP.scratch_bytes(1, EPI_ROUNDS[SMALL]) < MIB < EP.scratch_bytes(1, EPI_ROUNDS[LARGE])
    _grow_shrink_grow(_epipolar, "find_essential_batch")


# --------------------------------------------------------------------------------------------------------------------- autocal
AC_POINTS = (8, 4096)


@functools.lru_cache(maxsize=None)
def _ba_scene(n):
    cams, pts, obs, _, _, _ = AO.ba_scene(n, 7, noise=0.2, rot_deg=0.5, t_off=0.01)
    return cams, pts, obs


def _autocal(ctx, size):
    cams, pts, obs = _ba_scene(AC_POINTS[size])
    return AC.ba_step(cams, pts, obs, 1e-3, ctx=ctx)


def test_autocal_grow_shrink_grow():
    assert AC.wass_ac_scratch_bytes(AC_POINTS[SMALL]) < MIB < AC.wass_ac_scratch_bytes(AC_POINTS[LARGE])
    _grow_shrink_grow(_autocal, "ba_step")


# ------------------------------------------------------------------------------------------------------------------------ grid
GRID_SIDE = (16, 192)                           # 192 x 192 cells of 42 bytes: 1.5 MB


@functools.lru_cache(maxsize=None)
def _cloud():
    """300 points over the unit-scale 16 x 16 grid, a few outside it and a few invalid, 32 to a row"""
    rng = np.random.default_rng(11)
    p = np.stack([rng.uniform(-1.0, 16.0, 320), rng.uniform(-1.0, 16.0, 320), rng.integers(-4096, 4097, 320) / 1024.0], axis=1)
    v = (np.arange(320) % 16 != 5).astype(np.uint8)
    return v.reshape(10, 32), p.reshape(10, 32, 3)


def _grid(ctx, size, cell):
    side = GRID_SIDE[size]
    gs = grid_setup(np.eye(3), np.zeros(3), 1.0, 0.0, 15.0, 0.0, 15.0, side, side)
    with ctx.mesh_upload(*_cloud()) as mesh:
        return mesh.grid_idw(gs=gs, cell=cell)


@pytest.mark.parametrize("cell", ["mean", "median"])
def test_grid_bin_grow_shrink_grow(cell):
    assert GRID_SIDE[SMALL] ** 2 * 42 < MIB < GRID_SIDE[LARGE] ** 2 * 42
    _grow_shrink_grow(lambda ctx, size: _grid(ctx, size, cell), f"grid_bin, {cell}")


# ------------------------------------------------------------------------------------------------------------------------- DCT
DCT_SHAPE = ((1, 16, 4), (4, 192, 16))          # frames, side, Nfreqs: the padded maps of four 192 x 192 frames alone take 1.2 MB


@functools.lru_cache(maxsize=None)
def _cell_maps(size):
    n, side, _ = DCT_SHAPE[size]
    rng = np.random.default_rng(13)
    y, x = np.mgrid[0:side, 0:side] / side
    zz = np.stack([np.sin(3 * x + f) * np.cos(2 * y) + 0.01 * rng.normal(size=(side, side)) for f in range(n)]).astype(np.float32)
    zz[rng.random(zz.shape) < 0.4] = np.nan
    return zz


def _dct(ctx, size):
    grid, coeffs, info, status = ctx.grid_dct_batch(_cell_maps(size), {"Nfreqs": DCT_SHAPE[size][2], "MAX_ITERS": 60}, seed=3)
    return grid, coeffs, info, status


def test_dct_grow_shrink_grow():
    n, side, _ = DCT_SHAPE[LARGE]
    assert 2 * DCT_SHAPE[SMALL][1] ** 2 * 4 < MIB < n * 2 * side * side * 4
    _grow_shrink_grow(_dct, "grid_dct_batch")


# --------------------------------------------------------------------------------------------------------------------- prepare
@functools.lru_cache(maxsize=None)
def _mosaic(side):
    return PP.random_mosaic(side, side, 5), PP.camera(side, side)


@pytest.mark.parametrize("outputs,large", [(W.PREP_OUTPUTS, 256), ((), 1040)], ids=["every output", "image alone"])
def test_prepare_grow_shrink_grow(outputs, large):
    """the staged results take 27 bytes per pixel with every output and 1 with the picture alone"""
    per = 27 if outputs else 1
    assert 16 * 16 * per < MIB < large * large * per

    def run(ctx, size):
        mosaic, K = _mosaic((16, large)[size])
        return W.polarimetric_prepare(mosaic, K, PP.DIST["calibdir"], outputs=outputs, ctx=ctx)

    _grow_shrink_grow(run, "polarimetric_prepare")


# --------------------------------------------------------------------------------------------------------------------- no leak
def test_a_destroyed_context_gives_its_buffers_back():
    """Six times: a context, the match, grid and DCT calls above at both sizes (a dozen buffers filled, most of them twice), destroy.
    The free device memory after cycles 2 to 6 is one number; the first cycle also fills the caches of the HIP runtime and of torch.
    Measured on commit e849e9c, whose wass_ctx_destroy frees through a hand-kept list: no spread either."""
    import torch
    free = []
    for _ in range(6):
        with wass_amd.Context(0) as ctx:
            for size in (SMALL, LARGE):
                _match(ctx, size)
                _grid(ctx, size, "mean")
                _grid(ctx, size, "median")
                _dct(ctx, size)
        torch.cuda.synchronize()
        free.append(torch.cuda.mem_get_info()[0])
    print("free bytes after each destroy:", free)
    assert len(set(free[1:])) == 1, free
