"""The mesh stage (wass_amd/csrc/mesh.hip) at its launch edges, on hard component geometry and exactly on its thresholds, through
Context.mesh_upload and the Mesh methods, against the numpy / fp64 references of tests/mesh_oracle.py and the C oracle.

Every comparison is an equality.  The only tolerances are the two tests/test_post_mesh_gpu.py states: refine_plane (fp64 sums in a
tree order, atol 1e-9) does not occur here: the fused calls are compared with the stage-by-stage calls, which run the same
kernels, and both with the C oracle on mesh_oracle.exact_sea, whose sums no order of additions rounds; the triangulation allows
two validity flips from acos and rtol = atol = 1e-12 on the points.

Shapes: wass_mesh_upload accepts every width, height >= 1, so every shape of mesh_oracle.SMALL runs every stage; the kernels'
guards for them (k_gap_hist: 1 <= j < w - 1 and i >= 1; hlink / vlink) were read before the first run.
NaN heights are left out of the percentile: the reference sorts them with a comparison that is not a strict weak order then, and the
result of that is not defined.  What tests/test_mesh_edges.py proves on the CPU -- every probe scene is changed by the wrong variant
named there -- gives these comparisons their power."""
import numpy as np
import pytest

import mesh_oracle as M
import wass_amd

pytestmark = pytest.mark.gpu

ids = lambda c: "x".join(str(v) for v in c) if isinstance(c, tuple) else str(c)
WASS_ERR_INVALID_ARG, WASS_ERR_UNSUPPORTED, WASS_ERR_TOO_FEW_POINTS = -1, -2, -6


def _same(a, b):
    return a == b or (a != a and b != b)


def _up(ctx, valid, z):
    valid, p3d = M.as_mesh(valid, z)
    return ctx.mesh_upload(valid, p3d), valid, p3d


# ---------------------------------------------------------------------------------------------------------------- z-gap percentile
def _both_percentiles(ctx, valid, z, pct, tag):
    """the percentile alone (zgap_percentile) and as the first stage of the chain (remove_outliers) against the reference"""
    m, valid, p3d = _up(ctx, valid, z)
    ref = M.zgap_percentile(valid, p3d[..., 2], pct)
    a = m.zgap_percentile(pct)
    zg, ng, size = m.remove_outliers(pct)
    print(f"{tag} pct={pct}: ref {ref} zgap_percentile {a} remove_outliers {(zg, ng)} component {size}")
    assert _same(a[0], ref[0]) and a[1] == ref[1]
    assert _same(zg, ref[0]) and ng == ref[1]
    return ref, size


@pytest.mark.parametrize("shape", M.SMALL, ids=ids)
def test_zgap_percentile_both_ways_on_every_small_shape(gpu_ctx, shape):
    w, h = shape
    valid, z = M.holes(w, h)
    for pct in M.PCTS:
        ref, _ = _both_percentiles(gpu_ctx, valid, z, pct, f"{w}x{h}")
        if w < 3 or h < 2:
            assert ref[1] == 0 and ref[0] != ref[0]              # no interior column or no second row: (nan, 0)


@pytest.mark.parametrize("name", M.GAP_PROBES + ("consecutive",))
def test_zgap_value_probes(gpu_ctx, name):
    if name == "consecutive":
        valid, z = M.gap_consecutive(65, 9, 300)
    else:
        valid, z = M.gap_pairs(65, 9, M.gap_values(name))
    for pct in M.PCTS:
        _both_percentiles(gpu_ctx, valid, z, pct, name)


def test_zgap_rank_probes(gpu_ctx):
    for n, pct in M.RANK_CASES:
        w, h, valid, z = M.rank_scene(n)
        ref, _ = _both_percentiles(gpu_ctx, valid, z, pct, f"n={n}")
        assert ref == (float(M.rank_index(pct, n) + 1), n)


# ------------------------------------------------------------------------------------------------------------ connected components
def _check_biggest(ctx, oracle, valid, z, zgap, tag):
    m, valid, p3d = _up(ctx, valid, z)
    size = m.keep_biggest_component(zgap)
    got = m.download()[0]
    r_mask, r_size = M.keep_biggest(valid, p3d[..., 2], zgap)
    o_mask, o_size = oracle.keep_biggest_component(valid, p3d, zgap)
    ncomp = len(M.component_order(valid, p3d[..., 2], zgap)[1])
    print(f"{tag} {valid.shape[1]}x{valid.shape[0]} zgap={zgap!r}: {ncomp} components, biggest {size} (reference {r_size}, oracle {o_size})")
    assert size == r_size == o_size
    np.testing.assert_array_equal(got, r_mask)
    np.testing.assert_array_equal(got, o_mask)
    return size


@pytest.mark.parametrize("shape", M.SMALL, ids=ids)
def test_biggest_component_on_every_small_shape(gpu_ctx, oracle, shape):
    w, h = shape
    valid, z = M.holes(w, h, frac=0.3 if w * h > 64 else 0.1)
    for q in (50.0, 90.0):
        zgap = M.zgap_percentile(valid, z, q)[0]
        _check_biggest(gpu_ctx, oracle, valid, z, 1.0 if zgap != zgap else zgap, f"holes q={q}")
    _check_biggest(gpu_ctx, oracle, np.zeros((h, w), np.uint8), z, 1.0, "empty")
    _check_biggest(gpu_ctx, oracle, np.ones((h, w), np.uint8), np.zeros((h, w)), 1.0, "solid")


@pytest.mark.parametrize("shape", M.COMPONENT_SHAPES, ids=ids)
def test_biggest_component_on_built_scenes(gpu_ctx, oracle, shape):
    w, h = shape
    scenes = {}
    v, z, _ = M.snake(w, h); scenes["snake"] = (v, z)
    v, z, _ = M.snake(w, h, transpose=True); scenes["snake_t"] = (v, z)
    v, z, _ = M.spiral(w, h); scenes["spiral"] = (v, z)
    scenes["checkerboard"] = M.checkerboard(w, h)
    v, z, _ = M.stripes(w, h); scenes["stripes"] = (v, z)
    v, z, _, _ = M.twins(w, h); scenes["twins"] = (v, z)
    v, z, _ = M.islands_on_block_starts(w, h); scenes["islands"] = (v, z)
    for name, (v, z) in scenes.items():
        _check_biggest(gpu_ctx, oracle, v, z, 1.0, name)


@pytest.mark.parametrize("shape", [(5, 60), (33, 20), (5, 3400)], ids=ids)
def test_runs_that_wrap_rows_inside_a_wave(gpu_ctx, oracle, shape):
    w, h = shape
    v, z, zgap = M.ramp(w, h)
    assert _check_biggest(gpu_ctx, oracle, v, z, zgap, "ramp") == w
    assert _check_biggest(gpu_ctx, oracle, v, np.zeros((h, w)), 1.0, "solid") == w * h


@pytest.mark.parametrize("col", M.LINK_CELL_COLUMNS)
def test_the_16_link_patterns_component_by_component(gpu_ctx, oracle, col):
    """keep_biggest_component hands out one component; taking it away and asking again hands out the next: all 33 components of the
    16 patterns, in the reference's order, each mask equal.  The probe of the rule that skips a vertical union "the pixel to the
    left already made"."""
    valid, z, ncomp = M.link_cells_at(col)
    labels, order = M.component_order(valid, z, 1.0)
    left = valid.copy()
    for k, (root, size) in enumerate(order):
        m, lv, _ = _up(gpu_ctx, left, z)
        got_size = m.keep_biggest_component(1.0)
        got = m.download()[0]
        assert got_size == size, f"component {k}: size {got_size}, reference {size}"
        np.testing.assert_array_equal(got, (labels == root).astype(np.uint8))
        left = left & ~got
    print(f"cells at column {col}: {len(order)} components (by hand {ncomp}), sizes {[s for _, s in order]}")
    assert len(order) == ncomp == 33 and not left.any()
    m, _, _ = _up(gpu_ctx, left, z)
    assert m.keep_biggest_component(1.0) == 0


@pytest.mark.parametrize("zgap", [1.0, 0.1, 1e-300, 0.0, float("inf")])
@pytest.mark.parametrize("shape", [(65, 9), (256, 4), (129, 64)], ids=ids)
def test_links_exactly_at_the_threshold(gpu_ctx, oracle, shape, zgap):
    w, h = shape
    valid, z, c = M.comb(w, h, zgap if 0 < zgap < np.inf else 1.0)
    size = _check_biggest(gpu_ctx, oracle, valid, z, zgap, "comb")
    print(f"  spine {c['spine']}, teeth one ulp below / at / one ulp above the threshold: {c['pred']} / {c['at']} / {c['succ']}")
    if zgap == 0.0:
        assert size == 1
    elif zgap == np.inf:
        assert size == int(valid.sum())
    else:
        assert size == c["spine"] + c["pred"]


def test_remove_outliers_is_percentile_then_component(gpu_ctx, oracle):
    v1, z1, _ = M.snake(129, 64)
    z1 = z1 + np.random.default_rng(1).normal(0, 1e-3, z1.shape)
    v2, z2 = M.holes(300, 41, frac=0.3)
    v3, z3, _ = M.comb(65, 9, 1.0)
    for tag, v, z, pct in (("snake", v1, z1, 50.0), ("holes", v2, z2, 90.0), ("comb", v3, z3, 99.0), ("comb", v3, z3, 3.0)):
        a, valid, p3d = _up(gpu_ctx, v, z)
        zg, ng = a.zgap_percentile(pct)
        size = a.keep_biggest_component(zg)
        b, _, _ = _up(gpu_ctx, v, z)
        got = b.remove_outliers(pct)
        r_mask, r_size = M.keep_biggest(valid, p3d[..., 2], M.zgap_percentile(valid, p3d[..., 2], pct)[0])
        print(f"{tag} pct={pct}: step by step {(zg, ng, size)}, fused {got}, reference size {r_size}")
        assert got == (zg, ng, size) and size == r_size
        np.testing.assert_array_equal(a.download()[0], b.download()[0])
        np.testing.assert_array_equal(b.download()[0], r_mask)


# ----------------------------------------------------------------------------------------------------------------- RANSAC scoring
def _one_round(ctx, oracle, valid, p3d, uv, thr, tag, want=None):
    m = ctx.mesh_upload(valid, p3d)
    found, plane, best = m.ransac_plane(uv, thr)
    ok, opl, obest, per = oracle.ransac_plane(valid, p3d, uv, thr)
    ref = M.plane_count(valid, p3d, M.plane_of(p3d, uv[0]), thr)
    print(f"{tag} thr={thr}: best {best}, reference {ref}, oracle round count {per[0]}" + (f", by construction {want}" if want is not None else ""))
    assert best == ref == per[0] == obest and found == ok
    assert want is None or best == want
    np.testing.assert_array_equal(plane, opl)
    for reps in (63, 64, 65, 400):                          # the same plane in every slot of the 64-plane groups
        f2, p2, b2 = m.ransac_plane(np.repeat(uv, reps, axis=0), thr)
        assert (f2, b2) == (found, best), reps
        np.testing.assert_array_equal(p2, plane)
    return best


@pytest.mark.parametrize("thr", [1.0, 0.1])
@pytest.mark.parametrize("shape", M.LATTICE_SHAPES, ids=ids)
def test_ransac_counts_on_the_threshold_lattice(gpu_ctx, oracle, shape, thr):
    w, h = shape
    uv = M.lattice_samples(w, h)
    for kind in ("mixed", "pred", "at", "patches"):
        valid, p3d, c, inside = M.lattice(w, h, thr, kind)
        print(f"{w}x{h} {kind}: at thr {c['at']}, one ulp inside {c['pred']}, one ulp outside {c['succ']}, well inside {c['inside']}, well outside {c['outside']}")
        _one_round(gpu_ctx, oracle, valid, p3d, uv, thr, f"{w}x{h} {kind}", inside)
    valid, p3d = M.lattice_far(w, h, thr)
    _one_round(gpu_ctx, oracle, valid, p3d, uv, thr, f"{w}x{h} far")


@pytest.mark.parametrize("shape", M.LATTICE_SHAPES[:4], ids=ids)
def test_ransac_never_counts_a_point_with_a_nan_coordinate(gpu_ctx, oracle, shape):
    """fabs(NaN) < thr is false: the reference never counts the point, also where its patch is decided as a whole by its bounds"""
    w, h = shape
    for thr in (1.0, 0.1):
        for axis in range(3):
            valid, p3d, inside = M.lattice_nan(w, h, thr, axis)
            _one_round(gpu_ctx, oracle, valid, p3d, M.lattice_samples(w, h), thr, f"{w}x{h} NaN in axis {axis}", inside)


def test_ransac_degenerate_triple_and_one_pixel_mesh(gpu_ctx, oracle):
    """two samples on one pixel give the normal 0 / 0: the C oracle counts 0 for the round (every comparison with NaN is false)"""
    valid, p3d, _, _ = M.lattice(65, 9, 1.0, "pred")
    _one_round(gpu_ctx, oracle, valid, p3d, np.array([[0, 0, 0, 0, 5, 5]], np.int32), 1.0, "degenerate", 0)
    valid, p3d = M.as_mesh(np.ones((1, 1), np.uint8), np.zeros((1, 1)))
    _one_round(gpu_ctx, oracle, valid, p3d, np.zeros((1, 6), np.int32), 1.0, "1x1", 0)


def test_ransac_1800_rounds_and_the_refusals(gpu_ctx, oracle):
    w, h = 65, 9
    p3d, plane_true = M.sea(w, h, noise=0.3)
    valid = (np.random.default_rng(5).random((h, w)) > 0.1).astype(np.uint8)
    rng = np.random.default_rng(6)
    seen, rows = set(), []
    while len(rows) < 1801:
        t = tuple(int(x) for x in (rng.integers(0, w), rng.integers(0, h), rng.integers(0, w), rng.integers(0, h), rng.integers(0, w), rng.integers(0, h)))
        if t not in seen:
            seen.add(t); rows.append(t)
    uv = np.array(rows, np.int32)
    m = gpu_ctx.mesh_upload(valid, p3d)
    found, plane, best = m.ransac_plane(uv[:1800], 0.5)
    ok, opl, obest, per = oracle.ransac_plane(valid, p3d, uv[:1800], 0.5)
    print(f"1800 rounds: best {best} (oracle {obest}) of {int(valid.sum())}, found {found}; {int((per >= 0).sum())} rounds had three valid samples")
    assert (found, best) == (ok, obest)
    np.testing.assert_array_equal(plane, opl)
    with pytest.raises(wass_amd.WassError) as e:
        m.ransac_plane(uv, 0.5)
    assert e.value.code == WASS_ERR_UNSUPPORTED
    with pytest.raises(wass_amd.WassError) as e:
        m.fit_plane(uv, 0.5, 1.5)
    assert e.value.code == WASS_ERR_UNSUPPORTED
    for bad in ([w, 0, 1, 1, 2, 2], [0, h, 1, 1, 2, 2], [0, 0, -1, 1, 2, 2], [0, 0, 1, 1, 2, -1]):
        with pytest.raises(wass_amd.WassError) as e:
            m.ransac_plane(np.array([bad], np.int32), 0.5)
        assert e.value.code == WASS_ERR_INVALID_ARG


# ----------------------------------------------------------------------------------------------------------------- crop
@pytest.mark.parametrize("shape", M.SMALL, ids=ids)
def test_crop_plane_exactly_at_the_threshold(gpu_ctx, oracle, shape):
    w, h = shape
    plane = np.array([0.0, 0.0, 1.0, 0.0])
    for thr in (1.0, 0.1):
        vals = np.array([thr, M.pred(thr), M.succ(thr), 0.0, -thr, -M.pred(thr), -M.succ(thr)])
        z = vals[np.arange(h * w) % 7].reshape(h, w)
        valid, p3d = M.as_mesh((np.arange(h * w) % 11 != 5).reshape(h, w), z)
        m = gpu_ctx.mesh_upload(valid, p3d)
        kept = m.crop_plane(plane, thr)
        r_mask, r_kept = M.crop(valid, p3d, plane, thr)
        o_mask, o_kept = oracle.crop_plane(valid, p3d, plane, thr)
        az = np.abs(p3d[..., 2])[valid != 0]
        print(f"crop {w}x{h} thr={thr}: at {int((az == thr).sum())}, one ulp inside {int((az == M.pred(thr)).sum())}, "
              f"one ulp outside {int((az == M.succ(thr)).sum())}; kept {kept} (reference {r_kept}, oracle {o_kept})")
        assert kept == r_kept == o_kept
        np.testing.assert_array_equal(m.download()[0], r_mask)
        np.testing.assert_array_equal(r_mask, o_mask)


@pytest.mark.parametrize("shape", M.LATTICE_SHAPES, ids=ids)
def test_crop_plane_on_the_lattice_scenes(gpu_ctx, oracle, shape):
    w, h = shape
    for thr in (1.0, 0.1):
        scenes = [(k,) + M.lattice(w, h, thr, k)[:2] for k in ("mixed", "pred", "at", "patches")] + [("far",) + M.lattice_far(w, h, thr)]
        scenes += [(f"nan{a}",) + M.lattice_nan(w, h, thr, a)[:2] for a in range(3)]
        for kind, valid, p3d in scenes:
            plane = M.plane_of(p3d, M.lattice_samples(w, h)[0])
            m = gpu_ctx.mesh_upload(valid, p3d)
            kept = m.crop_plane(plane, thr)
            o_mask, o_kept = oracle.crop_plane(valid, p3d, plane, thr)
            print(f"crop {w}x{h} {kind} thr={thr}: kept {kept} (oracle {o_kept})")
            assert kept == o_kept == M.crop(valid, p3d, plane, thr)[1]
            np.testing.assert_array_equal(m.download()[0], o_mask)


# ----------------------------------------------------------------------------------------------------- block counts, scan, pack
@pytest.mark.parametrize("nb", M.BLOCK_COUNTS)
def test_xyzc_and_inlier_selection_over_block_counts_and_validity_patterns(gpu_ctx, oracle, nb):
    w, h = M.block_shape(nb)
    p3d, plane = M.sea(w, h)
    kw = dict(xmin=-2.0, xmax=1.5, ymin=-9999.0, ymax=9999.0, max_distance=float(np.median(np.sqrt((p3d ** 2).sum(-1)))) + 2.0)
    for pattern in M.PATTERNS:
        valid = M.pattern_valid(w, h, pattern)
        m = gpu_ctx.mesh_upload(valid, p3d)
        blob = m.encode_xyzc(plane)
        ref = oracle.encode_xyzc(valid, p3d, plane)
        nsel = []
        for every in (1, 2, 10):
            for central in (False, True):
                got = m.refinement_inliers(every=every, central_third_only=central, **kw)
                want, n_in = M.refinement_inliers(valid, p3d, every, central, **kw)
                np.testing.assert_array_equal(got, want)
                nsel.append(len(want))
        print(f"nb={nb} ({w}x{h}) {pattern}: {int(valid.sum())} valid, {len(blob)} bytes, inliers selected {nsel}")
        assert len(blob) == len(ref) == 148 + 6 * int(valid.sum())
        assert blob == ref
        if pattern == "none":
            assert len(blob) == 148 and blob[:4] == b"\0\0\0\0"


def test_xyzc_with_a_zero_extent_axis(gpu_ctx, oracle):
    """every point shares one x and the plane has a = 0, so the aligned x has no extent and its scale is 65535 / 0: whatever the C
    oracle's bytes say"""
    w, h = 37, 13
    p3d, plane = M.sea(w, h, flat_x=3.0)
    valid = M.pattern_valid(w, h, "random")
    blob = gpu_ctx.mesh_upload(valid, p3d).encode_xyzc(plane)
    ref = oracle.encode_xyzc(valid, p3d, plane)
    print(f"zero extent: scale {np.frombuffer(ref[4:28], np.float64)}, first triples {np.frombuffer(ref[148:166], np.uint16)}")
    assert np.isinf(np.frombuffer(ref[4:12], np.float64)[0])
    assert len(blob) == 148 + 6 * int(valid.sum()) and blob == ref


# ----------------------------------------------------------------------------------------------------------------- fused paths
@pytest.mark.parametrize("shape", [(65, 9), (129, 64), (257, 5)], ids=ids)
def test_fused_calls_equal_the_stages_at_edge_shapes(gpu_ctx, oracle, shape):
    import torch
    w, h = shape
    p3d, _ = M.sea(w, h, noise=0.15)
    valid = (np.random.default_rng(w).random((h, w)) > 0.15).astype(np.uint8)
    p3d[valid == 0] = 0
    uv = wass_amd.ransac_sample(w, h, 400, 12345)
    a = gpu_ctx.mesh_upload(valid, p3d)
    zg, ng = a.zgap_percentile(99.0)
    sz = a.keep_biggest_component(zg)
    found, pl, best = a.ransac_plane(uv, 1.0)
    k1 = a.crop_plane(pl, 1.0)
    pl2, ninl = a.refine_plane()
    k2 = a.crop_plane(pl2, 1.5)
    ref_bytes = a.encode_xyzc(pl2)
    b = gpu_ctx.mesh_upload(valid, p3d)
    assert b.remove_outliers(99.0) == (zg, ng, sz)
    res = b.fit_plane(uv, 1.0, 1.5)
    print(f"{w}x{h}: zgap {zg} of {ng} gaps, component {sz}, RANSAC best {best} found {found}, kept {k1} -> refine {ninl} -> kept {k2}, {len(ref_bytes)} bytes")
    assert found and bool(res.found) and res.ransac_inliers == best
    np.testing.assert_array_equal(np.array(res.ransac_plane[:]), pl)
    assert (res.kept_after_ransac_crop, res.refine_inliers, res.kept_final) == (k1, ninl, k2)
    np.testing.assert_array_equal(np.array(res.plane[:]), pl2)
    np.testing.assert_array_equal(a.download()[0], b.download()[0])
    assert (zg, ng) == oracle.zgap_percentile(valid, p3d, 99.0)
    ok, opl, obest, _ = oracle.ransac_plane(oracle.keep_biggest_component(valid, p3d, zg)[0], p3d, uv, 1.0)
    assert obest == best
    np.testing.assert_array_equal(opl, pl)
    pin = torch.zeros(148 + 6 * w * h, dtype=torch.uint8).pin_memory()
    c = gpu_ctx.mesh_upload(valid, p3d)
    c.finish_frame_async(uv, pin.data_ptr(), pin.numel())
    c.close()
    fr = gpu_ctx.frame_result()
    assert (fr.zgap, fr.n_gaps, fr.component_size) == (zg, ng, sz)
    assert fr.found == res.found and fr.refine_ok == 1 and fr.ransac_inliers == best
    np.testing.assert_array_equal(np.array(fr.plane[:]), pl2)
    assert (fr.kept_after_ransac_crop, fr.refine_inliers, fr.kept_final) == (k1, ninl, k2)
    assert fr.xyzc_bytes == len(ref_bytes) and pin[:fr.xyzc_bytes].numpy().tobytes() == ref_bytes


# ------------------------------------------------------------------------------------ the stage-by-stage calls on the chain's record
# zgap_percentile, ransac_plane, crop_plane and refine_plane run the chain's kernels on the context's device record, with the
# parameters the chain would find there written by the call itself.  What two separate implementations could not get wrong: a
# record nobody initialised, a record an earlier fit left "no plane" in, a record a frame in flight is still being read from.
# Scenes: mesh_oracle.exact_sea (the refined plane equals the C oracle's bit for bit, tests/test_mesh_edges.py shows why) and
# sparse_sea (no plane to find).
RP = M.EXACT_REFINE
FUSED_RP = dict(refine_max_distance=RP["max_distance"], weight_by_distance=RP["weight_by_distance"])


def _raw_refine(ctx, m):
    """wass_mesh_refine_plane through the C ABI -- Mesh.refine_plane drops n_inliers when it raises: (code, message, plane, n_inliers)"""
    import ctypes as C
    rp = wass_amd.RefineParams(-9999.0, 9999.0, -9999.0, 9999.0, RP["max_distance"], int(RP["weight_by_distance"]), 0)
    plane = (C.c_double * 4)(); n = C.c_uint64(12345)
    rc = ctx._lib.wass_mesh_refine_plane(ctx._h, m._h, C.byref(rp), plane, C.byref(n))
    return rc, ctx._lib.wass_last_error(ctx._h).decode() if rc else "", np.array(plane[:]), int(n.value)


def _check_refine(ctx, oracle, valid, p3d):
    m = ctx.mesh_upload(valid, p3d)
    rc, msg, plane, n = _raw_refine(ctx, m)
    opl, on, _ = oracle.refine_plane(valid, p3d, **RP)
    print(f"refine_plane {valid.shape[1]}x{valid.shape[0]}: code {rc} {msg!r}, {n} inliers (oracle {on}), plane {plane} (oracle {opl})")
    assert n == on
    if on < 3:
        assert (rc, msg) == (WASS_ERR_TOO_FEW_POINTS, f"plane refinement has {on} inliers")
    else:
        assert rc == 0
        np.testing.assert_array_equal(plane, opl)
    np.testing.assert_array_equal(m.download()[0], valid)             # its crop stayed off
    return opl if on >= 3 else np.array([0.0, 0.0, 1.0, -20.0])


def _check_crop(ctx, oracle, valid, p3d, plane, thr=0.25):
    m = ctx.mesh_upload(valid, p3d)
    kept = m.crop_plane(plane, thr)
    o_mask, o_kept = oracle.crop_plane(valid, p3d, plane, thr)
    print(f"crop_plane {valid.shape[1]}x{valid.shape[0]}: kept {kept} of {int(valid.sum())} (oracle {o_kept})")
    assert kept == o_kept == M.crop(valid, p3d, plane, thr)[1]
    np.testing.assert_array_equal(m.download()[0], o_mask)


def _check_fit(ctx, oracle, valid, p3d, uv, thr=1.0, maxd=0.25):
    """fit_plane against ransac_plane -> crop -> refine_plane -> crop of the references"""
    m = ctx.mesh_upload(valid, p3d)
    found, rpl, best, _ = oracle.ransac_plane(valid, p3d, uv, thr)
    m1, k1 = M.crop(valid, p3d, rpl, thr) if found else (valid, 0)
    pl2, ninl, _ = oracle.refine_plane(m1, p3d, **RP)
    if found and ninl < 3:
        with pytest.raises(wass_amd.WassError) as e:
            m.fit_plane(uv, thr, maxd, **FUSED_RP)
        assert e.value.code == WASS_ERR_TOO_FEW_POINTS
        return
    res = m.fit_plane(uv, thr, maxd, **FUSED_RP)
    print(f"fit_plane {valid.shape[1]}x{valid.shape[0]}: found {res.found} best {res.ransac_inliers} (oracle {found}, {best}), kept {res.kept_after_ransac_crop}"
          f" -> refine {res.refine_inliers} -> kept {res.kept_final}")
    assert (bool(res.found), res.ransac_inliers) == (found, best)
    np.testing.assert_array_equal(np.array(res.ransac_plane[:]), rpl)
    if not found:
        assert np.isnan(np.array(res.plane[:])).all() and (res.kept_after_ransac_crop, res.refine_inliers, res.kept_final) == (0, 0, 0)
        np.testing.assert_array_equal(m.download()[0], valid)
        return
    m2, k2 = M.crop(m1, p3d, pl2, maxd)
    assert (res.kept_after_ransac_crop, res.refine_inliers, res.kept_final) == (k1, ninl, k2)
    np.testing.assert_array_equal(np.array(res.plane[:]), pl2)
    np.testing.assert_array_equal(m.download()[0], m2)


@pytest.mark.parametrize("first", ["crop_plane", "refine_plane"])
@pytest.mark.parametrize("shape", M.RECORD_SHAPES, ids=ids)
def test_the_first_call_on_a_fresh_context(oracle, shape, first):
    """no percentile, RANSAC or fused call has initialised the record before"""
    valid, p3d = M.exact_sea(*shape)
    plane = oracle.refine_plane(valid, p3d, **RP)[0] if valid.sum() >= 3 else np.array([0.0, 0.0, 1.0, -20.0])
    with wass_amd.Context(0) as ctx:
        if first == "crop_plane":
            _check_crop(ctx, oracle, valid, p3d, plane)
        else:
            _check_refine(ctx, oracle, valid, p3d)


@pytest.mark.parametrize("shape", M.RECORD_SHAPES, ids=ids)
def test_a_record_left_without_a_plane_and_the_other_order(gpu_ctx, oracle, shape):
    """fit_plane on sparse_sea leaves ransac_found = refine_ok = 0 in the record (1 x 1: found, not refined); refine_plane and
    crop_plane on another mesh must read switch words of their own.  Then the other order: the fused call after them."""
    w, h = shape
    uv = M.record_samples(w, h)
    _check_fit(gpu_ctx, oracle, *M.sparse_sea(w, h), uv)
    valid, p3d = M.exact_sea(w, h)
    plane = _check_refine(gpu_ctx, oracle, valid, p3d)
    _check_fit(gpu_ctx, oracle, *M.sparse_sea(w, h), uv)
    _check_crop(gpu_ctx, oracle, valid, p3d, plane)
    _check_fit(gpu_ctx, oracle, valid, p3d, uv)


FRAME_FIELDS = ("n_gaps", "component_size", "found", "refine_ok", "ransac_inliers", "refine_inliers", "kept_after_ransac_crop", "kept_final",
                "n_points", "xyzc_bytes")


@pytest.mark.parametrize("shape", M.RECORD_SHAPES, ids=ids)
def test_stage_by_stage_calls_while_a_frame_is_in_flight(gpu_ctx, oracle, shape):
    """finish_frame_async for mesh A, the four calls on mesh B and the encoder twice (with the plane, without) before A's record is
    read: A's result and bytes are those of A run alone, B's results the references'.  Once: an ordering check."""
    import torch
    w, h = shape
    uv = M.record_samples(w, h)
    va, pa = M.exact_sea(w, h, seed=2)
    vb, pb = M.exact_sea(w, h)
    z_ref = M.zgap_percentile(vb, pb[..., 2], 99.0)
    r_found, r_plane, r_best, _ = oracle.ransac_plane(vb, pb, uv, 0.3)
    p_ref, n_ref, _ = oracle.refine_plane(vb, pb, **RP)
    crop_by = p_ref if n_ref >= 3 else np.array([0.0, 0.0, 1.0, -20.0])
    c_mask, c_kept = oracle.crop_plane(vb, pb, crop_by, 0.25)
    enc_by = crop_by if n_ref >= 3 else TILTED             # (the stand-in plane of 1 x 1 is level: see TILTED)

    def frame(between):
        pin = torch.zeros(148 + 6 * w * h, dtype=torch.uint8).pin_memory()
        a = gpu_ctx.mesh_upload(va, pa)
        a.finish_frame_async(uv, pin.data_ptr(), pin.numel(), **FUSED_RP)
        got = between()
        fr = gpu_ctx.frame_result()
        return fr, pin[:fr.xyzc_bytes].numpy().tobytes(), got

    def four_calls():
        b = gpu_ctx.mesh_upload(vb, pb)
        zg = b.zgap_percentile(99.0)
        rs = b.ransac_plane(uv, 0.3)
        rf = _raw_refine(gpu_ctx, b)
        kept = b.crop_plane(crop_by, 0.25)
        return zg, rs, rf, kept, b.encode_xyzc(enc_by), b.encode_xyzc(None), b.download()[0]

    alone, alone_bytes, _ = frame(lambda: None)
    fr, fr_bytes, (zg, rs, rf, kept, enc, enc_none, mask) = frame(four_calls)
    print(f"{w}x{h}: frame {[getattr(fr, k) for k in FRAME_FIELDS]} zgap {fr.zgap}; between: zgap {zg}, RANSAC {rs[0], rs[2]}, refine {rf[0], rf[3]}, kept {kept}")
    assert [getattr(fr, k) for k in FRAME_FIELDS] == [getattr(alone, k) for k in FRAME_FIELDS] and _same(fr.zgap, alone.zgap)
    np.testing.assert_array_equal(np.array(fr.ransac_plane[:]), np.array(alone.ransac_plane[:]))
    np.testing.assert_array_equal(np.array(fr.plane[:]), np.array(alone.plane[:]))
    assert fr_bytes == alone_bytes and len(fr_bytes) == 148 + 6 * fr.n_points
    assert _same(zg[0], z_ref[0]) and zg[1] == z_ref[1]
    assert (rs[0], rs[2]) == (r_found, r_best)
    np.testing.assert_array_equal(rs[1], r_plane)
    assert rf[3] == n_ref and rf[0] == (0 if n_ref >= 3 else WASS_ERR_TOO_FEW_POINTS)
    if n_ref >= 3:
        np.testing.assert_array_equal(rf[2], p_ref)
    assert kept == c_kept
    np.testing.assert_array_equal(mask, c_mask)
    assert enc == oracle.encode_xyzc(c_mask, pb, enc_by) and enc_none == _identity_xyzc(c_mask, pb)


# The encoder is a stage-by-stage call like the four above: it writes R|T and the crop switch, off, into the record and runs the
# chain's last step (k_crop_limits_counts_dev, k_scan_blocks, k_frame_header, k_xyzc_pack_dev).
# Planes for the encoder are tilted: RT_from_plane divides by a^2 + b^2, and a plane [0, 0, 1, d] makes its R a matrix of NaNs in
# the reference as here, which neither keeps out of its limits the same way (reduce.h: the callers of order_key keep NaN out).
TILTED = np.array([0.6, 0.0, 0.8, -16.0])
FAR_PLANE = np.array([0.6, 0.0, 0.8, -1e6])                # about 1e6 away from every point of exact_sea: a crop by it keeps none


def _identity_xyzc(valid, p3d):
    """oracle.encode_xyzc without a plane (the C oracle takes one; RT_from_plane has no plane that gives the identity: a = b = 0 is 0 / 0).
    With R = I and T = 0 the oracle's R p + T is p itself -- 1 x + 0 y + 0 z + 0 rounds nothing for finite points -- so its limits,
    scales and truncating conversions are these fp64 expressions; 0 * inf (one point, or no extent on an axis) converts to 0."""
    pts = p3d.reshape(-1, 3)[valid.ravel() != 0]
    n = len(pts)
    mn = pts.min(0) if n else np.full(3, np.finfo(np.float64).max)
    mx = pts.max(0) if n else np.full(3, -np.finfo(np.float64).max)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        sc = 65535.0 / (mx - mn)
        q = (pts - mn) * sc
    q = np.where(np.isnan(q), 0.0, q).astype(np.uint16)
    return np.uint32(n).tobytes() + sc.tobytes() + mn.tobytes() + np.eye(3).tobytes() + np.zeros(3).tobytes() + q.tobytes()


def _encode_both(ctx, oracle, valid, p3d, plane, tag):
    """the encoder with a plane and without on a fresh upload, against the references; the valid mask stays as uploaded"""
    m = ctx.mesh_upload(valid, p3d)
    got, got_none = m.encode_xyzc(plane), m.encode_xyzc(None)
    print(f"{tag} {valid.shape[1]}x{valid.shape[0]}: {int(valid.sum())} valid, {len(got)} and {len(got_none)} bytes")
    assert len(got) == len(got_none) == 148 + 6 * int(valid.sum())
    assert got == oracle.encode_xyzc(valid, p3d, plane) and got_none == _identity_xyzc(valid, p3d)
    np.testing.assert_array_equal(m.download()[0], valid)


@pytest.mark.parametrize("shape", M.RECORD_SHAPES, ids=ids)
def test_the_encoder_first_on_a_fresh_context(oracle, shape):
    """no record, no pinned stage: the encoder's own put creates both"""
    valid, p3d = M.exact_sea(*shape)
    with wass_amd.Context(0) as ctx:
        _encode_both(ctx, oracle, valid, p3d, TILTED, "fresh")


@pytest.mark.parametrize("shape", M.RECORD_SHAPES, ids=ids)
def test_the_encoder_after_a_fit_that_left_its_crop_switch_on(gpu_ctx, oracle, shape):
    """fit_plane on exact_sea leaves refine_ok = 1 and its plane in the record (1 x 1: no refinement, refine_ok = 0).  The encoder
    of another mesh with a plane far from its points must switch the crop off itself: a crop that ran would remove every point.
    refine_plane and crop_plane after it write their own switches again."""
    w, h = shape
    _check_fit(gpu_ctx, oracle, *M.exact_sea(w, h), M.record_samples(w, h))
    valid, p3d = M.exact_sea(w, h, seed=3)
    _encode_both(gpu_ctx, oracle, valid, p3d, FAR_PLANE, "after a fit")
    plane = _check_refine(gpu_ctx, oracle, valid, p3d)
    _check_crop(gpu_ctx, oracle, valid, p3d, plane)


@pytest.mark.parametrize("shape", M.RECORD_SHAPES, ids=ids)
def test_the_encoder_after_a_fit_that_found_no_plane(gpu_ctx, oracle, shape):
    w, h = shape
    _check_fit(gpu_ctx, oracle, *M.sparse_sea(w, h), M.record_samples(w, h))
    valid, p3d = M.exact_sea(w, h, seed=3)
    _encode_both(gpu_ctx, oracle, valid, p3d, TILTED, "after 'not found'")


@pytest.mark.parametrize("shape", M.RECORD_SHAPES, ids=ids)
def test_the_encoder_into_a_buffer_of_exactly_its_size(gpu_ctx, oracle, shape):
    """encode_xyzc_to into pinned memory of exactly 148 + 6 n bytes, n < w h, between guard cells: it fits, one byte fewer is refused
    before anything is downloaded, no guard cell changes, and the mesh still encodes afterwards"""
    import torch
    from guarded import GUARD, Guarded, host
    valid, p3d = M.exact_sea(*shape)
    valid.ravel()[0] = 0
    p3d[valid == 0] = 0
    plane = TILTED
    need = 148 + 6 * int(valid.sum())
    assert valid.sum() < valid.size
    ref = oracle.encode_xyzc(valid, p3d, plane)
    g = Guarded(False)
    parent = torch.full((need + 64,), GUARD["u"], dtype=torch.uint8).pin_memory()
    inside = np.zeros(need + 64, bool)
    inside[32:-32] = True
    g.kept.append((parent, host(parent).copy(), inside))
    m = gpu_ctx.mesh_upload(valid, p3d)
    with pytest.raises(wass_amd.WassError) as e:
        m.encode_xyzc_to(plane, parent.data_ptr() + 32, need - 1)
    print(f"{shape}: {need} bytes; one fewer: {e.value}")
    assert e.value.code == WASS_ERR_INVALID_ARG and f"xyzC needs {need} bytes, buffer has {need - 1}" in str(e.value)
    assert (host(parent) == GUARD["u"]).all()                          # refused before the download
    assert m.encode_xyzc_to(plane, parent.data_ptr() + 32, need) == need
    assert host(parent)[32:-32].tobytes() == ref
    g.check("encode_xyzc_to")
    assert m.encode_xyzc(plane) == ref


def test_the_refusals_answer_as_before(gpu_ctx, oracle):
    """What test_ransac_1800_rounds_and_the_refusals, test_ransac_degenerate_triple_and_one_pixel_mesh and the small shapes of the
    percentile test do not already hold: refine_plane's refusal with its inlier count, samples on invalid pixels only, the
    percentile at 1 x 5 and 5 x 1, a bad sample through fit_plane, and the mesh untouched by every refused call."""
    w, h = 65, 9
    full, p3d = M.exact_sea(w, h)
    for n in (0, 1, 2):
        valid = np.zeros((h, w), np.uint8)
        valid.ravel()[np.flatnonzero(full.ravel())[:n]] = 1
        assert int(valid.sum()) == n
        _check_refine(gpu_ctx, oracle, valid, p3d * valid[..., None])
    # every sample on an invalid pixel: no candidate at all
    valid = full.copy()
    valid[0, 0] = valid[0, 1] = valid[1, 0] = 0
    uv = np.array([[0, 0, 1, 0, 0, 1]] * 3, np.int32)
    m = gpu_ctx.mesh_upload(valid, p3d)
    found, plane, best = m.ransac_plane(uv, 1.0)
    ok, opl, obest, _ = oracle.ransac_plane(valid, p3d, uv, 1.0)
    assert (found, best) == (ok, obest) == (False, 0) and (plane == 0).all() and (opl == 0).all()
    for ww, hh in ((1, 5), (5, 1)):
        v1, z1 = M.holes(ww, hh, frac=0.0)
        got = gpu_ctx.mesh_upload(*M.as_mesh(v1, z1)).zgap_percentile(50.0)
        assert got[0] != got[0] and got[1] == 0 and M.zgap_percentile(v1, z1, 50.0)[1] == 0
    # refused before anything is enqueued, by both tiers: the valid plane is as uploaded
    many = np.tile(M.record_samples(w, h), (29, 1))[:1801]
    for bad in (many, np.array([[0, 0, w, 1, 2, 2]], np.int32)):
        code = WASS_ERR_UNSUPPORTED if len(bad) == 1801 else WASS_ERR_INVALID_ARG
        for call in (lambda: m.ransac_plane(bad, 1.0), lambda: m.fit_plane(bad, 1.0, 0.25, **FUSED_RP)):
            with pytest.raises(wass_amd.WassError) as e:
                call()
            assert e.value.code == code
    np.testing.assert_array_equal(m.download()[0], valid)
    res = m.fit_plane(many[:1800], 1.0, 0.25, **FUSED_RP)             # ... and the mesh still fits
    assert res.found and res.kept_final < res.kept_after_ransac_crop


# ----------------------------------------------------------------------------------------------------------------- triangulation
@pytest.mark.parametrize("shape", [(8, 6), (65, 9), (257, 5)], ids=ids)
def test_triangulate_with_rois_on_every_border(gpu_ctx, oracle, shape):
    from wass_amd import synth
    w, h = shape
    rng = np.random.default_rng(w)
    uu, vv = np.meshgrid(np.arange(w), np.arange(h))
    disp = (1.2 + 0.04 * w * (0.2 + 0.5 * vv / h) + 0.3 * np.sin(uu / 3.0)).astype(np.float32)
    disp[rng.random((h, w)) < 0.1] = 0
    right = rng.integers(1, 255, (h, w), dtype=np.uint8)
    rig = synth.rig_geometry(w, h)
    a = 0.01
    Rr = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1.0]])
    rig["R1"] = Rr; rig["R2"] = Rr.T
    og, gg = oracle.make_geom(rig), wass_amd.make_geom(rig)
    for roi_l, roi_r in (((0, 0, w, h), (0, 0, w, h)), ((1, 0, w - 1, h), (0, 0, w - 1, h)), ((0, 0, w - 1, h), (1, 0, w - 1, h))):
        x0, y0, rw, rh = roi_r
        droi = np.ascontiguousarray(disp[y0:y0 + rh, x0:x0 + rw])
        full = np.zeros((h, w), np.float32); full[y0:y0 + rh, x0:x0 + rw] = droi
        n_ref, v_ref, p_ref, g_ref = oracle.triangulate(full, roi_l, roi_r, og, right, None, None, 1.0, None, 1.0)
        mesh, n = gpu_ctx.triangulate(droi, w, h, roi_l, roi_r, gg, right, None, None, 1.0, None, 1.0)
        valid, p3d, gray = mesh.download()
        flips = int((valid != v_ref).sum())
        print(f"{w}x{h} roi_l {roi_l} roi_r {roi_r}: {n} points (oracle {n_ref}), {flips} validity flips")
        assert n_ref > 0 and flips <= 2 and abs(n - n_ref) <= 2
        both = (valid == 1) & (v_ref == 1)
        np.testing.assert_allclose(p3d[both], p_ref[both], rtol=1e-12, atol=1e-12)
        np.testing.assert_array_equal(gray[both], g_ref[both])
        assert (p3d[valid == 0] == 0).all()
