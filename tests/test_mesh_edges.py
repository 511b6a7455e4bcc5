"""The references and scenes of the mesh edge suite (tests/mesh_oracle.py) on the CPU: every numpy reference equals the C oracle on
every scene the GPU tests use, every probe scene is changed by the wrong variant it is there to catch, and the builders have
the properties their docstrings state.  What the GPU tests (tests/test_mesh_edges_gpu.py) compare against is held in place here."""
import numpy as np
import pytest

import mesh_oracle as M

ids = lambda c: "x".join(str(v) for v in c) if isinstance(c, tuple) else str(c)


def _same(a, b):
    return a == b or (a != a and b != b)


def component_scenes(w, h):
    """name -> (valid, z, zgap, variant that must change the result)"""
    out = {}
    for name, tr in (("snake", False), ("snake_t", True)):
        v, z, size = M.snake(w, h, transpose=tr)
        out[name] = (v, z, 1.0, ("link", "le"))
    v, z, _ = M.spiral(w, h)
    out["spiral"] = (v, z, 1.0, ("link", "le"))
    v, z = M.checkerboard(w, h)
    out["checkerboard"] = (v, z, 1.0, ("tie", "raster"))
    v, z, _ = M.stripes(w, h)
    out["stripes"] = (v, z, 1.0, ("tie", "raster"))
    v, z, _, _ = M.twins(w, h)
    out["twins"] = (v, z, 1.0, ("tie", "raster"))
    v, z, _ = M.islands_on_block_starts(w, h)
    out["islands"] = (v, z, 1.0, ("link", "le"))
    return out


def ramp_scenes():
    out = {}
    for w, h in ((5, 60), (33, 20)):
        v, z, zgap = M.ramp(w, h)
        out[f"ramp{w}"] = (v, z, zgap, ("link", "le"))
    return out


# ---------------------------------------------------------------------------------------------------------------- z-gap percentile
@pytest.mark.parametrize("shape", M.SMALL, ids=ids)
def test_zgap_reference_equals_the_c_oracle_on_every_small_shape(oracle, shape):
    w, h = shape
    valid, z = M.holes(w, h)
    valid, p3d = M.as_mesh(valid, z)
    z = p3d[..., 2]
    for pct in M.PCTS:
        ref = M.zgap_percentile(valid, z, pct)
        orc = oracle.zgap_percentile(valid, p3d, pct)
        print(f"{w}x{h} pct={pct}: ref={ref} oracle={orc}")
        assert _same(ref[0], orc[0]) and ref[1] == orc[1]
    if w < 3 or h < 2:
        assert M.zgap_percentile(valid, z, 50.0)[1] == 0 and np.isnan(M.zgap_percentile(valid, z, 50.0)[0])


def test_zgap_reference_on_a_cloud_and_its_column_and_neighbour_variants(oracle):
    valid, z = M.holes(210, 140, frac=0.15)
    valid, p3d = M.as_mesh(valid, z)
    for pct in M.PCTS:
        assert M.zgap_percentile(valid, p3d[..., 2], pct) == oracle.zgap_percentile(valid, p3d, pct)
    valid, z = M.holes(65, 9)
    base = M.zgap_percentile(valid, z, 50.0)
    allc = M.zgap_percentile(valid, z, 50.0, cols="all")
    two = M.zgap_percentile(valid, z, 50.0, above="two")
    print(f"65x9 holes: {base}; cols=all {allc}; above=two {two}")
    assert allc[1] > base[1] and two[1] < base[1] and allc[0] != base[0] and two[0] != base[0]


@pytest.mark.parametrize("name", M.GAP_PROBES + ("consecutive",))
def test_gap_value_probes_have_their_gaps_and_catch_the_two_neighbour_variant(oracle, name):
    """catches above="two": every probe gap is reached through the upper RIGHT neighbour (the consecutive doubles through all three)"""
    if name == "consecutive":
        valid, z = M.gap_consecutive(65, 9, 300)
        want = 1.0 + np.arange(300) * 2.0 ** -52
        bits = np.sort(M.zgaps(valid, z)).view(np.uint64)
        assert (np.diff(bits) == 1).all() and len({int(b) >> 9 for b in bits}) <= 2       # only the last 9-bit digit (and its carry) differ
    else:
        vals = M.gap_values(name)
        valid, z = M.gap_pairs(65, 9, vals)
        want = np.sort(np.array(vals))
    got = np.sort(M.zgaps(valid, z))
    print(f"{name}: {got.size} gaps, min {got[0]!r} max {got[-1]!r}")
    np.testing.assert_array_equal(got, want)
    valid, p3d = M.as_mesh(valid, z)
    for pct in M.PCTS:
        ref = M.zgap_percentile(valid, z, pct)
        assert ref == oracle.zgap_percentile(valid, p3d, pct)
        assert M.zgap_percentile(valid, z, pct, above="two") != ref or (ref[0] != ref[0])
    assert M.zgap_percentile(valid, z, 50.0, above="two")[1] < got.size


def test_rank_probes_land_on_and_just_below_integers_and_catch_the_ceiling(oracle):
    """catches rank="ceil" wherever pct / 100.0 * n is not an integer in fp64; where it is one, floor and ceiling are the same index"""
    below = exact = 0
    for n, pct in M.RANK_CASES:
        x = pct / 100.0 * float(n)
        w, h, valid, z = M.rank_scene(n)
        assert M.zgaps(valid, z).size == n
        ref = M.zgap_percentile(valid, z, pct)
        ceil = M.zgap_percentile(valid, z, pct, rank="ceil")
        valid, p3d = M.as_mesh(valid, z)
        orc = oracle.zgap_percentile(valid, p3d, pct)
        print(f"n={n} pct={pct}: pct/100*n={x!r} floor index {M.rank_index(pct, n)} value {ref[0]} ceil value {ceil[0]} oracle {orc}")
        assert ref == orc and ref[0] == float(M.rank_index(pct, n) + 1)      # the gaps are 1 .. n
        if x == np.floor(x):
            exact += 1
            assert ceil == ref
        else:
            below += int(np.ceil(x) - x < 1e-9)
            assert ceil != ref
    assert (100, 99.0) in M.RANK_CASES and (1000, 98.7) in M.RANK_CASES
    print(f"{exact} exact, {below} just below an integer")
    assert exact >= 2 and below >= 2


# ------------------------------------------------------------------------------------------------------------ connected components
def _check_components(oracle, valid, z, zgap, variant, name):
    valid, p3d = M.as_mesh(valid, z)
    z = np.where(valid != 0, z, 0.0)
    mask, size = M.keep_biggest(valid, z, zgap)
    o_mask, o_size = oracle.keep_biggest_component(valid, p3d, zgap)
    _, order = M.component_order(valid, z, zgap)
    print(f"{name} {valid.shape[1]}x{valid.shape[0]}: {len(order)} components, biggest {size} (oracle {o_size})")
    assert size == o_size
    np.testing.assert_array_equal(mask, o_mask)
    if variant is not None:
        wrong = M.keep_biggest(valid, z, zgap, **{variant[0]: variant[1]})
        assert wrong[1] != size or (wrong[0] != mask).any(), f"{name}: {variant} changes nothing"
    return len(order), size


@pytest.mark.parametrize("shape", M.SMALL + [(210, 140)], ids=ids)
def test_component_reference_equals_the_c_oracle_on_holes(oracle, shape):
    w, h = shape
    valid, z = M.holes(w, h, frac=0.3 if w * h > 64 else 0.1)
    for q in (50.0, 90.0):
        zgap = M.zgap_percentile(valid, z, q)[0]
        _check_components(oracle, valid, z, 1.0 if zgap != zgap else zgap, None, f"holes q={q}")


@pytest.mark.parametrize("shape", M.COMPONENT_SHAPES, ids=ids)
def test_component_scenes_equal_the_c_oracle_and_catch_their_variant(oracle, shape):
    w, h = shape
    for name, (valid, z, zgap, variant) in component_scenes(w, h).items():
        _check_components(oracle, valid, z, zgap, variant, name)


def test_component_builders_have_their_stated_properties(oracle):
    for w, h in M.COMPONENT_SHAPES:
        v, z, size = M.snake(w, h)
        assert M.keep_biggest(v, z, 1.0)[1] == size == ((h + 1) // 2) * w + h // 2
        assert (M.keep_biggest(v, z, 1.0)[0] == (z == 0.0)).all()
        v, z, size = M.spiral(w, h)
        lab, order = M.component_order(v, z, 1.0)
        assert len(order) == 2 and size in (order[0][1], order[1][1])       # the corridor and its wall, one component each
        v, z = M.checkerboard(w, h)
        m, s = M.keep_biggest(v, z, 1.0)
        assert s == 1 and m[1, 0] == 1 and M.keep_biggest(v, z, 1.0, tie="raster")[0][0, 1] == 1
        assert len(M.component_order(v, z, 1.0)[1]) == int(v.sum())
        v, z, L = M.stripes(w, h)
        assert M.keep_biggest(v, z, 1.0)[0][2, 0] == 1 and M.keep_biggest(v, z, 1.0, tie="raster")[0][0, 2] == 1
        v, z, size, (ra, rb) = M.twins(w, h)
        m, s = M.keep_biggest(v, z, 1.0)
        assert s == size and m[rb, 0] == 1 and m[ra].sum() == 0
        for r, c in ((ra, 8), (rb, 0)):
            assert (r * w + c) // 256 != ((r + 1) * w + c + 5) // 256
        v, z, big = M.islands_on_block_starts(w, h)
        m, s = M.keep_biggest(v, z, 1.0)
        assert s == big and not m.ravel()[::8192].any()
    for name, (v, z, zgap, variant) in ramp_scenes().items():
        h, w = v.shape
        n, size = _check_components(oracle, v, z, zgap, variant, name)
        assert n == h and size == w                        # every row a component of its own
        assert abs(z[0, w - 1] - z[1, 0]) < zgap and abs(z[0, 0] - z[1, 0]) == zgap


def test_the_16_link_patterns_give_the_component_counts_computed_by_hand(oracle):
    """catches link="le" (absent links sit at |dz| == zgap wherever the four heights allow it)"""
    assert [M.cell_components(p) for p in range(16)] == [4, 3, 3, 2, 3, 2, 2, 1, 3, 2, 2, 1, 2, 1, 1, 1]
    for p in range(16):
        tl, tr, bl, br = M.cell_heights(p)
        present = [abs(tl - tr) < 1, abs(bl - br) < 1, abs(tl - bl) < 1, abs(tr - br) < 1]
        assert present == [bool(p >> k & 1) for k in range(4)]
    for col in M.LINK_CELL_COLUMNS:
        valid, z, ncomp = M.link_cells_at(col)
        assert ncomp == 33
        n, _ = _check_components(oracle, valid, z, 1.0, None, f"cells@{col}")
        assert n == 33
        # every single component, largest first: what the GPU test peels off one by one
        labels, order = M.component_order(valid, z, 1.0)
        left = valid.copy()
        for root, size in order:
            m, s = oracle.keep_biggest_component(left, M.as_mesh(left, z)[1], 1.0)
            assert s == size
            np.testing.assert_array_equal(m, (labels == root).astype(np.uint8))
            left = left & ~m
        assert not left.any()
        assert len(M.component_order(valid, z, 1.0, link="le")[1]) != 33


@pytest.mark.parametrize("zgap", [1.0, 0.1, 1e-300, 0.0, float("inf")])
def test_comb_counts_its_teeth_at_the_threshold(oracle, zgap):
    """catches link="le": the teeth at |dz| == zgap would join the spine"""
    w, h = 65, 9
    valid, z, c = M.comb(w, h, zgap if 0 < zgap < np.inf else 1.0)
    mask, size = M.keep_biggest(valid, z, zgap)
    print(f"zgap={zgap}: spine {c['spine']}, teeth pred/at/succ {c['pred']}/{c['at']}/{c['succ']}, biggest {size}")
    assert min(c["pred"], c["at"], c["succ"]) >= 10
    if zgap == 0.0:
        assert size == 1 and mask[0, 0] == 1
    elif zgap == np.inf:
        assert size == int(valid.sum())
    else:
        assert size == c["spine"] + c["pred"]
        assert M.keep_biggest(valid, z, zgap, link="le")[1] == c["spine"] + c["pred"] + c["at"]
    o_mask, o_size = oracle.keep_biggest_component(*M.as_mesh(valid, z), zgap)
    assert o_size == size
    np.testing.assert_array_equal(o_mask, mask)


# ----------------------------------------------------------------------------------------------------------------- planes
@pytest.mark.parametrize("thr", [1.0, 0.1])
@pytest.mark.parametrize("shape", M.LATTICE_SHAPES, ids=ids)
def test_lattice_counts_at_and_around_the_threshold(oracle, shape, thr):
    """catches count="le" (kinds mixed and at)"""
    w, h = shape
    uv = M.lattice_samples(w, h)
    for kind in ("mixed", "pred", "at", "patches"):
        valid, p3d, c, inside = M.lattice(w, h, thr, kind)
        plane = M.plane_of(p3d, uv[0])
        assert abs(plane[2]) == 1.0 and plane[0] == 0 and plane[1] == 0 and plane[3] == 0
        n = M.plane_count(valid, p3d, plane, thr)
        ok, opl, obest, per = oracle.ransac_plane(valid, p3d, uv, thr)
        print(f"{w}x{h} thr={thr} {kind}: at {c['at']} pred {c['pred']} succ {c['succ']} inside {c['inside']} outside {c['outside']}"
              f" -> count {n} (oracle {per[0]})")
        assert n == inside == c["inside"] + c["pred"] == per[0] == obest
        np.testing.assert_array_equal(np.abs(plane), np.abs(opl))
        assert c["at"] + c["pred"] + c["succ"] + c["inside"] + c["outside"] == w * h
        if kind in ("mixed", "at"):
            assert M.plane_count(valid, p3d, plane, thr, count="le") == n + c["at"] != n
        if kind == "mixed" and w * h > 12:
            assert min(c["at"], c["pred"], c["succ"]) >= (w * h - 3) // 6 - 1
        if kind == "pred":
            assert n == w * h
        if kind == "at":
            assert n == 3
        m, k = M.crop(valid, p3d, plane, thr)
        om, ok_ = oracle.crop_plane(valid, p3d, plane, thr)
        assert k == ok_ == n
        np.testing.assert_array_equal(m, om)


@pytest.mark.parametrize("shape", M.LATTICE_SHAPES, ids=ids)
def test_far_lattice_and_nan_point_against_the_c_oracle(oracle, shape):
    w, h = shape
    uv = M.lattice_samples(w, h)
    for thr in (1.0, 0.1):
        valid, p3d = M.lattice_far(w, h, thr)
        plane = M.plane_of(p3d, uv[0])
        ok, opl, obest, per = oracle.ransac_plane(valid, p3d, uv, thr)
        n = M.plane_count(valid, p3d, plane, thr)
        np.testing.assert_array_equal(plane, opl)
        # the fp32 pass of a scoring kernel cannot decide within 2^-21 (|a| + |b| + |c|) max|coordinate| of the band edge
        assert 2.0 ** -21 * np.abs(plane[:3]).sum() * np.abs(p3d).max() > thr / 4
        print(f"far {w}x{h} thr={thr}: count {n} of {w * h} (oracle {per[0]})")
        assert n == per[0] and (w * h < 12 or 3 < n < w * h)
        for axis in range(3):
            valid, p3d, inside = M.lattice_nan(w, h, thr, axis)
            if (h // 2, w // 2) in {(0, 0), (0, w - 1), (h - 1, 0)}:
                continue                                   # 2 x 2: the middle pixel is a sample
            plane = M.plane_of(p3d, uv[0])
            ok, opl, obest, per = oracle.ransac_plane(valid, p3d, uv, thr)
            assert M.plane_count(valid, p3d, plane, thr) == inside == per[0] == w * h - 1     # the NaN point is never counted
            assert oracle.crop_plane(valid, p3d, plane, thr)[1] == inside == M.crop(valid, p3d, plane, thr)[1]


def test_a_degenerate_triple_counts_nothing_in_the_c_oracle(oracle):
    """two samples on one pixel: the normal is 0 / 0 = NaN, every comparison is false, the round counts 0"""
    valid, p3d, _, _ = M.lattice(65, 9, 1.0, "pred")
    uv = np.array([[0, 0, 0, 0, 5, 5]], np.int32)
    ok, plane, best, per = oracle.ransac_plane(valid, p3d, uv, 1.0)
    assert per[0] == 0 and best == 0 and not ok and (plane == 0).all()
    assert np.isnan(M.plane_of(p3d, uv[0])).all()
    assert M.plane_count(valid, p3d, M.plane_of(p3d, uv[0]), 1.0) == 0


@pytest.mark.parametrize("shape", M.SMALL, ids=ids)
def test_crop_reference_equals_the_c_oracle(oracle, shape):
    w, h = shape
    for thr in (1.0, 0.1):
        vals = np.array([thr, M.pred(thr), M.succ(thr), 0.0, -thr, -M.pred(thr), -M.succ(thr)])       # the GPU test's input
        valid, p3d = M.as_mesh((np.arange(h * w) % 11 != 5).reshape(h, w), vals[np.arange(h * w) % 7].reshape(h, w))
        plane = np.array([0.0, 0.0, 1.0, 0.0])
        m, k = M.crop(valid, p3d, plane, thr)
        om, ok_ = oracle.crop_plane(valid, p3d, plane, thr)
        print(f"crop {w}x{h} thr={thr}: kept {k} of {w * h}")
        assert k == ok_
        np.testing.assert_array_equal(m, om)
        at = int(((np.abs(p3d[..., 2]) == thr) & (valid != 0)).sum())
        assert M.crop(valid, p3d, plane, thr, count="le")[1] == k + at                  # catches count="le"


def test_block_shapes_and_patterns():
    for nb in M.BLOCK_COUNTS:
        w, h = M.block_shape(nb)
        assert (w * h + 255) // 256 == nb and 256 % w != 0
        assert M.pattern_valid(w, h, "block_first").sum() == nb
        assert M.pattern_valid(w, h, "block_last").ravel()[-1] == 1
        assert M.pattern_valid(w, h, "none").sum() == 0 and M.pattern_valid(w, h, "last").sum() == 1
    assert M.block_shape(1025)[0] * M.block_shape(1025)[1] < 263000


def test_refinement_inlier_reference_is_the_formula_of_the_existing_test():
    rng = np.random.default_rng(3)
    h, w = 40, 77
    p3d = rng.normal(0, 30, (h, w, 3)); p3d[..., 2] += 60
    valid = (rng.random((h, w)) < 0.8).astype(np.uint8)
    kw = dict(xmin=-40.0, xmax=35.0, ymin=-50.0, ymax=45.0, max_distance=75.0)
    for central in (False, True):
        u0, u1, v0, v1 = (w // 4, w * 3 // 4, h // 4, h * 2 // 3) if central else (0, w - 1, 0, h - 1)
        uu, vv = np.meshgrid(np.arange(w), np.arange(h))
        x, y, z = p3d[..., 0], p3d[..., 1], p3d[..., 2]
        ok = (valid != 0) & (uu >= u0) & (uu <= u1) & (vv >= v0) & (vv <= v1) & (x > kw["xmin"]) & (x < kw["xmax"]) & \
             (y > kw["ymin"]) & (y < kw["ymax"]) & (np.sqrt(x * x + y * y + z * z) < kw["max_distance"])
        got, n = M.refinement_inliers(valid, p3d, 10, central, **kw)
        np.testing.assert_array_equal(got, p3d[ok][::10])
        assert n == ok.sum() > 100


# ----------------------------------------------------------------------------------------- the plane stages on a shared device record
@pytest.mark.parametrize("shape", M.RECORD_SHAPES, ids=ids)
def test_exact_sea_refines_to_the_same_bits_in_any_summation_order(oracle, shape):
    """What lets the GPU tests compare refine_plane with the C oracle by equality: with EXACT_REFINE every sum of the refinement is an
    integer multiple of a power of two and the sums of the magnitudes stay below 2^53, so no order of additions rounds anything.  The
    moments of the C oracle's raster loop equal the integer computation exactly."""
    w, h = shape
    valid, p3d = M.exact_sea(w, h)
    n = int(valid.sum())
    assert n & (n - 1) == 0 and w * h // 2 < n <= w * h                       # a power of two
    P = np.rint(p3d[valid != 0] * 8).astype(np.int64)
    assert (P / 8.0 == p3d[valid != 0]).all()
    plane, cnt, mom = oracle.refine_plane(valid, p3d, **M.EXACT_REFINE)
    assert cnt == n
    if n < 3:
        return                                                              # 1 x 1: the refusal with one inlier
    S = P.sum(0)
    Q = P * n - S                                                           # 8 n (p - centroid), integers
    A = Q.T @ Q
    bound = (np.abs(Q).T @ np.abs(Q)).max()
    print(f"{w}x{h}: {n} inliers, largest sum of |terms| 2^{np.log2(float(bound)):.1f} in units of 1 / (8 n)^2, plane {plane}")
    assert bound < 2 ** 53 and np.abs(S).max() < 2 ** 53
    assert mom[0] == n
    np.testing.assert_array_equal(mom[1:4], S / (8.0 * n))
    np.testing.assert_array_equal(mom[4:13], (A / (8.0 * n) ** 2).ravel())
    assert abs(plane[0]) > 0.05 and abs(plane[1]) > 0.05                    # tilted in both directions: no axis drops out of the solve
    # a crop by the refined plane that keeps some points and drops some; the numpy reference equals the C oracle
    m, k = M.crop(valid, p3d, plane, 0.25)
    om, ok_ = oracle.crop_plane(valid, p3d, plane, 0.25)
    assert k == ok_ and n // 4 < k < 3 * n // 4
    np.testing.assert_array_equal(m, om)
    # the default RANSAC band holds every point for the candidate that wins: the refinement behind the fused call's crop sees the same n
    uv = M.record_samples(w, h)
    found, rpl, best, per = oracle.ransac_plane(valid, p3d, uv, 1.0)
    assert found and best == n == M.crop(valid, p3d, rpl, 1.0)[1]
    # ... and a narrow band separates the candidates: the choice among them is a real one
    found, rpl, best, per = oracle.ransac_plane(valid, p3d, uv, 0.3)
    assert found and n // 10 <= best < n and len(set(int(c) for c in per if c > 0)) > 5


@pytest.mark.parametrize("shape", M.RECORD_SHAPES, ids=ids)
def test_sparse_sea_has_no_plane(oracle, shape):
    """the mesh whose fit leaves "no plane found" and "not refined" behind in the record: best < w h / 10 in the oracle.  At 1 x 1 the
    limit is 0: found with nothing valid, and the refinement is what fails."""
    w, h = shape
    valid, p3d = M.sparse_sea(w, h)
    found, plane, best, per = oracle.ransac_plane(valid, p3d, M.record_samples(w, h), 1.0)
    print(f"{w}x{h}: {int(valid.sum())} valid, best {best}, limit {w * h // 10}, found {found}")
    assert (3 <= int(valid.sum()) <= w * h // 20 or w * h == 1 and not valid.any()) and (plane == 0).all()
    assert (best < w * h // 10 and not found) if w * h > 1 else (best == 0 and found)
    assert oracle.refine_plane(valid, p3d, **M.EXACT_REFINE)[1] == int(valid.sum())
