"""DCT surface interpolation on the GPU (grid_dct.hip) at the shapes its launch plan makes awkward: every k_dct_resid<NFT>
instance, more than one pass over the f-tiles (Nf > 160), ragged and tiny grids, one and eight column chunks.  The case table and
what it reaches are in tests/dct_oracle.py (SHAPE_CASES, plan) and asserted in tests/test_grid_dct.py; the references are the
numpy oracle (evaluate, interpolate, rprop_steps) and the closed form of a one-cell grid (probe_expected)."""
import numpy as np
import pytest

import dct_oracle as D
import wass_amd
from test_grid_dct_gpu import assert_matches, data_loss

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -23
ids = lambda c: "x".join(map(str, c))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def surface(shape, keep=0.6):
    H, W, _ = shape
    return D.holey_surface(H, W, seed=7 * H + W, keep=keep)


def start(shape):
    return np.random.default_rng(shape[2]).random((shape[2], shape[2])).astype(np.float32)


# ---- a. one evaluation of loss and gradient at every case of the table against the fp64 oracle
# The three norm-wise criteria are those of test_eval_matches_fp64_oracle (tests/test_grid_dct_gpu.py), derived there.
# Per 16 x 16 tile of the gradient: norm(g_tile - gr_tile) <= 2e-5 * norm(gr) / sqrt(ntiles) * TILE_MARGIN, so that one wrong tile
# cannot hide in the norm of the others.  TILE_MARGIN is 8 x the worst such ratio of the oracle's own fp32 gradient (_grad_fp32,
# blocked BLAS sums) on these same inputs, measured on the CPU over the whole table: 0.103, at (330, 322, 321); the next ones are
# 0.051 at (176, 176, 176) and 0.040 at (113, 120, 113), and 0.002 ... 0.034 elsewhere.  The factor 8 allows a k-ordered fma
# chain to lose more than a blocked sum (0.75 ... 1.5e-7 * sum |a b| for K <= 1024).  The norm-wise error of _grad_fp32 on the
# same inputs is 4.8e-8 ... 5.5e-7 of the gradient's norm, 36 x inside the 2e-5.
TILE_MARGIN = 8 * 0.103


@pytest.mark.parametrize("shape", D.SHAPE_CASES, ids=ids)
def test_eval_matches_fp64_oracle_at_every_shape(gpu_ctx, shape):
    H, W, nf = shape
    zz = surface(shape)
    x = D.eval_point(nf, seed=nf + H)
    g, dl, rl = gpu_ctx.grid_dct_eval(zz, x, alpha=8e-7)
    gr, dlr, rlr = D.evaluate(zz, x, 8e-7, np.float64)
    te, nt = D.tile_errors(g, gr)
    lim = 2e-5 * np.linalg.norm(gr) / np.sqrt(nt) * TILE_MARGIN
    print(f"{shape}: gradient {np.linalg.norm(g - gr) / np.linalg.norm(gr):.3e} of its norm, worst tile {te.max() / lim:.3f} of its "
          f"bound, data loss {abs(dl - dlr) / dlr:.3e}, |x|_1 {abs(rl - rlr) / max(rlr, 1e-300):.3e}")
    assert g.shape == (nf, nf) and np.isfinite(g).all()
    assert np.linalg.norm(g - gr) <= 2e-5 * np.linalg.norm(gr)
    assert abs(dl - dlr) <= 1e-5 * dlr
    assert abs(rl - rlr) <= 1e-6 * rlr
    assert (te <= lim).all(), f"tiles {np.argwhere(te > lim).tolist()} off by up to {te.max() / lim:.2f} x the bound"


# ---- b. near-exact probes: one data cell, at most one coefficient, alpha = 0
# Every contraction then has a single non-zero term and the kernels' fma chains reduce to the f32 products of probe_expected.
# Bound (derived, not measured): the device's fp64 cosine may round to a neighbouring f32 for the two basis entries of an element
# (1 ulp each), the products round once each: 4 * 2^-23 relative on every element, 1e-37 absolute for exact zeros.  z = 0.37 and
# c = 0.5 keep |Irec| < |z|, so the subtraction amplifies nothing.  The data loss is one f32 difference squared in fp64: 1e-6.
PROBE_SHAPES = [(50, 37, 33), (90, 131, 80), (176, 176, 176), (330, 322, 321), (24, 2300, 20)]


def probe_cells(H, W, nf):
    """Corners, the cells around the first tile boundary, the first and last column of every column chunk, and in the first chunk
    a column of the last tile each wave owns (tile t of a chunk goes to wave t % 4)."""
    p = D.plan(H, W, nf)
    cells = [(0, 0), (H - 1, W - 1), (15, 16), (16, 15)]
    for ch in range(p["nchunk"]):
        first, last = ch * p["tpc"] * 16, min((ch + 1) * p["tpc"] * 16, W) - 1
        cells += [((7 * ch + 3) % H, first), ((11 * ch + H // 2) % H, last)]
    tiles = p["tpc"] if p["nchunk"] > 1 else p["last"]
    for w in range(min(4, tiles)):
        t = w + 4 * ((tiles - 1 - w) // 4)
        cells.append(((5 * w + 17) % H, min(t * 16 + 5 + w, W - 1)))
    assert all(0 <= y < H and 0 <= x < W for y, x in cells)
    return list(dict.fromkeys(cells))


def probe_coefs(nf):
    """x = 0, then the one coefficient in the corners and around the first tile boundary; above 160 frequencies also around the
    boundary between two passes of k_dct_resid and at the last coefficient of each pass."""
    coefs = [None, (0, 0), (nf - 1, nf - 1), (15, 16), (16, 15)]
    if nf > 160:
        coefs += [(159, 160), (160, 159)] + [(e, e) for e in (min(160 * (k + 1), nf) - 1 for k in range((nf + 159) // 160))]
    return list(dict.fromkeys(coefs))


def describe(H, W, nf, cell, g, want, bad):
    f, gg = (int(v) for v in np.argwhere(bad)[0])
    Ay, Ax = D._basis32(H, nf), D._basis32(W, nf)
    return (f"{int(bad.sum())} elements off, first G[{f}, {gg}] = {g[f, gg]!r}, closed form {want[f, gg]!r}; oracle basis "
            f"Ay[{f}, {cell[0]}] = {Ay[f, cell[0]]!r}, Ax[{gg}, {cell[1]}] = {Ax[gg, cell[1]]!r}")


@pytest.mark.parametrize("shape", PROBE_SHAPES, ids=ids)
def test_single_cell_probes(gpu_ctx, shape):
    H, W, nf = shape
    failures, n = [], 0
    for cell in probe_cells(H, W, nf):
        zz = np.full((H, W), np.nan, np.float32)
        zz[cell] = 0.37
        for coef in probe_coefs(nf):
            x = np.zeros((nf, nf), np.float32)
            if coef is not None:
                x[coef] = 0.5
            g, dl, rl = gpu_ctx.grid_dct_eval(zz, x, alpha=0.0)
            want, wl = D.probe_expected(H, W, nf, cell, 0.37, coef)
            bad = ~(np.abs(g.astype(np.float64) - want) <= 4 * EPS * np.abs(want.astype(np.float64)) + 1e-37)
            n += 1
            if bad.any():
                failures.append(f"cell {cell} coefficient {coef}: " + describe(H, W, nf, cell, g, want, bad))
            if not abs(dl - wl) <= 1e-6 * wl:
                failures.append(f"cell {cell} coefficient {coef}: data loss {dl!r}, closed form {wl!r}")
            if rl != (0.0 if coef is None else 0.5):
                failures.append(f"cell {cell} coefficient {coef}: |x|_1 {rl!r}")
    assert not failures, f"{len(failures)} findings in {n} probes:\n" + "\n".join(failures[:12])


@pytest.mark.parametrize("shape", [(50, 37, 33), (330, 322, 321)], ids=ids)
def test_two_cell_probe_sees_the_padding(gpu_ctx, shape):
    """Two data cells in opposite corners of a ragged grid, x = 0: cs = 2 / 2, and each element of the gradient is the f32 sum of the
    two closed forms (one more rounding: 8 * 2^-23 of the larger term).  A padded cell that counts as data changes cs; a padded
    basis row or column that is not zero adds a term."""
    H, W, nf = shape
    zz = np.full((H, W), np.nan, np.float32)
    zz[0, 0] = zz[H - 1, W - 1] = 0.37
    g, dl, _ = gpu_ctx.grid_dct_eval(zz, np.zeros((nf, nf), np.float32), alpha=0.0)
    a, la = D.probe_expected(H, W, nf, (0, 0), 0.37, count=2)
    b, lb = D.probe_expected(H, W, nf, (H - 1, W - 1), 0.37, count=2)
    want = a.astype(np.float64) + b
    bad = ~(np.abs(g - want) <= 8 * EPS * np.maximum(np.abs(a), np.abs(b)) + 1e-37)
    assert not bad.any(), describe(H, W, nf, (0, 0), g, want, bad)
    assert abs(dl - (la + lb)) <= 1e-6 * (la + lb)


# ---- c. Rprop steps on awkward plans: the criteria of test_rprop_steps_match_oracle
# The 0.1 % of coefficients that may differ is that test's cap.  On the CPU, Rprop with the oracle's fp32 gradient (_grad_fp32)
# against rprop_steps (fp64 gradient) on exactly these inputs gave 100 % bit-equal coefficients at all four shapes and both step
# counts, so the reference itself uses none of the allowance.
@pytest.mark.parametrize("max_iters", [0, 3])
@pytest.mark.parametrize("shape", [(17, 33, 17), (90, 131, 80), (176, 176, 176), (330, 322, 321)], ids=ids)
def test_rprop_steps_match_oracle_on_awkward_plans(gpu_ctx, shape, max_iters):
    nf = shape[2]
    zz, x0 = surface(shape), start(shape)
    opts = {"Nfreqs": nf, "MAX_ITERS": max_iters, "TOLERANCE_CHANGE": 0.0}
    _, coeffs, info = gpu_ctx.grid_dct(zz, opts, x0=x0)
    assert info["steps"] == max_iters + 1 and not info["converged"]
    want, step = D.rprop_steps(zz, x0, opts, max_iters + 1)
    print(f"{shape} MAX_ITERS {max_iters}: {np.mean(coeffs == want):.6f} of the coefficients bit-equal")
    assert np.mean(coeffs == want) >= 0.999
    assert (np.abs(coeffs - want) <= step * (1 + 1e-6)).all()


# ---- d. whole solves on ragged, multi-pass and one-cell-wide grids against the fp32 oracle (assert_matches: the tolerance model
# of tests/test_grid_dct_gpu.py, unchanged)
# The maps keep 95 % of their cells.  With Nf = min(H, W) and 60 % kept there are more coefficients than data, Rprop does not
# settle, and the oracle's own fp32 and fp64 runs (interpolate with either dtype, CPU) end 3.6 ... 5.3 % of the data's std apart
# after 100 steps at (176, 176, 176) and (330, 322, 321): no fp32 solver can be told from a wrong one at 1 % there.  At 95 %
# kept the same two runs differ by 0.06 / 0.22 / 0.10 % of std and 0.01 / 0.75 / 0.33 % in data loss on the first three cases
# below (criteria: 1 % and 2 %), and not at all on the one-cell-wide ones.
@pytest.mark.parametrize("shape,opts", [pytest.param(s, o, id=ids(s)) for s, o in (
    ((50, 37, 33), {"MAX_ITERS": 200}),
    ((176, 176, 176), {"MAX_ITERS": 100, "TOLERANCE_CHANGE": 0.0}),
    ((330, 322, 321), {"MAX_ITERS": 100, "TOLERANCE_CHANGE": 0.0}),
    ((1, 40, 1), {"MAX_ITERS": 100}),
    ((40, 1, 1), {"MAX_ITERS": 100}))])
def test_whole_solve_matches_oracle(gpu_ctx, shape, opts):
    H, W, nf = shape
    zz, x0 = surface(shape, keep=0.95), start(shape)
    opts = {"Nfreqs": nf, **opts}
    grid, coeffs, info = gpu_ctx.grid_dct(zz, opts, x0=x0)
    want, _, steps, _, _ = D.interpolate(zz, x0, opts, dtype=np.float32)
    assert grid.shape == (H, W) and grid.dtype == np.float32 and coeffs.shape == (nf, nf)
    assert np.isfinite(grid).all() and np.isfinite(coeffs).all()
    if opts.get("TOLERANCE_CHANGE") == 0.0:
        assert info["steps"] == steps == opts["MAX_ITERS"] + 1
    assert_matches(grid, want, zz, info["data_loss"], info["steps"], steps)
    assert abs(info["data_loss"] - data_loss(grid, zz)) <= 1e-6 * data_loss(grid, zz) + 1e-12


# ---- e. the stopping rule around the 50-step check window (16 coefficient tiles: k_dct_maxred has something to reduce)
def test_stopping_rule_and_fdelta(gpu_ctx):
    shape = (70, 115, 60)
    nf = shape[2]
    zz, x0 = surface(shape), start(shape)
    co, info = {}, {}
    for mi in (0, 49, 50, 51, 99, 100):
        opts = {"Nfreqs": nf, "MAX_ITERS": mi, "TOLERANCE_CHANGE": 0.0}
        _, co[mi], info[mi] = gpu_ctx.grid_dct(zz, opts, x0=x0)
        assert info[mi]["steps"] == mi + 1 and not info[mi]["converged"], mi
        assert D.interpolate(zz, x0, opts, dtype=np.float32)[2] == mi + 1
    # fdelta is max |dx| of the last checked step (ii = 0, 50, 100); solves are deterministic, so two of them give that step
    assert info[0]["fdelta"] == float(np.max(np.abs(co[0] - x0)))
    assert info[49]["fdelta"] == info[0]["fdelta"]
    assert info[50]["fdelta"] == float(np.max(np.abs(co[50] - co[49]))) > 0
    assert info[51]["fdelta"] == info[50]["fdelta"] == info[99]["fdelta"]
    assert info[100]["fdelta"] == float(np.max(np.abs(co[100] - co[99]))) > 0
    opts = {"Nfreqs": nf, "MAX_ITERS": 100, "TOLERANCE_CHANGE": 1e30}
    _, c1, i1 = gpu_ctx.grid_dct(zz, opts, x0=x0)
    assert i1["steps"] == 1 and i1["converged"] and i1["fdelta"] == info[0]["fdelta"]
    np.testing.assert_array_equal(bits(c1), bits(co[0]))
    assert D.interpolate(zz, x0, opts, dtype=np.float32)[2:4] == (1, True)


# ---- f. entries and state
@pytest.mark.parametrize("shape", [(50, 37, 33), (176, 176, 176)], ids=ids)
def test_device_entry_equals_host_entry(gpu_ctx, shape):
    import torch
    H, W, nf = shape
    zz, x0 = surface(shape), start(shape)
    um = (np.random.default_rng(H).random((H, W)) < 0.8).astype(np.uint8)
    opts = {"Nfreqs": nf, "MAX_ITERS": 60}
    grid, coeffs, info = gpu_ctx.grid_dct(zz, opts, x0=x0, user_mask=um)
    d_zz, d_x0, d_um = (torch.from_numpy(a).cuda() for a in (zz, x0, um))
    d_out = torch.full((H, W), 7.0, dtype=torch.float32, device="cuda")
    d_co = torch.full((nf, nf), 7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    dinfo = gpu_ctx.grid_dct_dev(d_zz, d_out, opts, d_x0=d_x0, d_user_mask=d_um, d_coeffs=d_co)
    torch.cuda.synchronize()
    assert np.array_equal(np.isnan(grid), um == 0)
    np.testing.assert_array_equal(bits(d_out.cpu().numpy()), bits(grid))
    np.testing.assert_array_equal(bits(d_co.cpu().numpy()), bits(coeffs))
    assert dinfo == info
    np.testing.assert_array_equal(bits(d_zz.cpu().numpy()), bits(zz))
    np.testing.assert_array_equal(bits(d_x0.cpu().numpy()), bits(x0))
    # without the optional arguments: the seeded start, no mask, no coefficients
    g2, _, i2 = gpu_ctx.grid_dct(zz, opts, seed=5)
    assert gpu_ctx.grid_dct_dev(d_zz, d_out, opts, seed=5) == i2
    torch.cuda.synchronize()
    np.testing.assert_array_equal(bits(d_out.cpu().numpy()), bits(g2))


def test_seeded_start_is_the_documented_generator(gpu_ctx):
    shape = (50, 37, 33)
    nf = shape[2]
    zz = surface(shape)
    opts = {"Nfreqs": nf, "MAX_ITERS": 20}
    co = {}
    for seed in (0, 1, 2 ** 63 + 12345):
        g_seed, co[seed], i_seed = gpu_ctx.grid_dct(zz, opts, seed=seed)
        g_x0, c_x0, i_x0 = gpu_ctx.grid_dct(zz, opts, x0=D.splitmix_x0(seed, nf))
        np.testing.assert_array_equal(bits(g_seed), bits(g_x0))
        np.testing.assert_array_equal(bits(co[seed]), bits(c_x0))
        assert i_seed == i_x0
    assert not np.array_equal(co[0], co[1])
    # MAX_ITERS = 0 is one step of size LEARNING_RATE from the start value: it can be read back from the coefficients' signs
    _, c0, _ = gpu_ctx.grid_dct(zz, {"Nfreqs": nf, "MAX_ITERS": 0, "TOLERANCE_CHANGE": 0.0, "LEARNING_RATE": 0.25}, seed=1)
    assert (np.abs(np.abs(c0 - D.splitmix_x0(1, nf)) - 0.25) <= 2 * EPS).all()


def test_buffers_reused_across_problem_sizes(gpu_ctx):
    """A large problem, a small one and the large one again on one context: no padding, slab or Rprop state leaks between them."""
    big, small = (330, 322, 321), (17, 33, 17)
    ob = {"Nfreqs": big[2], "MAX_ITERS": 20, "TOLERANCE_CHANGE": 0.0}
    os_ = {"Nfreqs": small[2], "MAX_ITERS": 60, "TOLERANCE_CHANGE": 0.0}
    r1 = gpu_ctx.grid_dct(surface(big), ob, x0=start(big))
    r2 = gpu_ctx.grid_dct(surface(small), os_, x0=start(small))
    e2 = gpu_ctx.grid_dct_eval(surface(small), D.eval_point(small[2], 3))
    r3 = gpu_ctx.grid_dct(surface(big), ob, x0=start(big))
    with wass_amd.Context(0) as fresh:
        f2 = fresh.grid_dct(surface(small), os_, x0=start(small))
        fe = fresh.grid_dct_eval(surface(small), D.eval_point(small[2], 3))
    for a, b in ((r1, r3), (r2, f2)):
        np.testing.assert_array_equal(bits(a[0]), bits(b[0]))
        np.testing.assert_array_equal(bits(a[1]), bits(b[1]))
        assert a[2] == b[2]
    np.testing.assert_array_equal(bits(e2[0]), bits(fe[0]))
    assert e2[1:] == fe[1:]


def test_multi_pass_solve_is_deterministic(gpu_ctx):
    shape = (176, 176, 176)
    opts = {"Nfreqs": shape[2], "MAX_ITERS": 60, "TOLERANCE_CHANGE": 0.0}
    a = gpu_ctx.grid_dct(surface(shape), opts, x0=start(shape))
    b = gpu_ctx.grid_dct(surface(shape), opts, x0=start(shape))
    np.testing.assert_array_equal(bits(a[0]), bits(b[0]))
    np.testing.assert_array_equal(bits(a[1]), bits(b[1]))
    assert a[2] == b[2] and a[2]["steps"] == 61


# ---- g. rejected calls leave the context usable
def test_errors_leave_the_context_usable(gpu_ctx):
    shape = (50, 37, 33)
    zz, x0 = surface(shape), start(shape)
    opts = {"Nfreqs": shape[2], "MAX_ITERS": 30}
    g0, c0, i0 = gpu_ctx.grid_dct(zz, opts, x0=x0)
    for bad in ({"Nfreqs": 38}, {"Nfreqs": 33, "MAX_ITERS": -1}, {"Nfreqs": 33, "LEARNING_RATE": 0.0},
                {"Nfreqs": 33, "LEARNING_RATE": float("nan")}):
        with pytest.raises(wass_amd.WassError) as e:
            gpu_ctx.grid_dct(zz, bad, x0=x0 if bad["Nfreqs"] == 33 else None)
        assert e.value.code == -1, bad
        g1, c1, i1 = gpu_ctx.grid_dct(zz, opts, x0=x0)
        np.testing.assert_array_equal(bits(g0), bits(g1))
        np.testing.assert_array_equal(bits(c0), bits(c1))
        assert i0 == i1
    with pytest.raises(wass_amd.WassError) as e:
        gpu_ctx.grid_dct_eval(zz, np.zeros((38, 38), np.float32))
    assert e.value.code == -1
    g1, _, _ = gpu_ctx.grid_dct(zz, opts, x0=x0)
    np.testing.assert_array_equal(bits(g0), bits(g1))
