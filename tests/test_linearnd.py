"""The LinearND oracle (tests/linearnd_oracle.py) against scipy, the conditions its scenes must meet before the GPU test may lean
on them, and every probe against the mistake it is there to catch.  No GPU."""
import functools

import numpy as np
import pytest

import linearnd_oracle as L

N = 32                                             # the lattice of the random scenes
CAP = 0.01                                         # share of nodes that may stay uncertified (flags 2 and 3) on a random scene


@functools.lru_cache(maxsize=None)
def oracle_scene(kind):
    x, y, z = L.scene(kind)
    return (x, y, z) + L.interpolate(x, y, z, *L.UNIT, N, N)


@pytest.mark.parametrize("kind", L.SCENES)
def test_walk_and_certificate_against_scipy(kind):
    from scipy.interpolate import LinearNDInterpolator
    from scipy.spatial import Delaunay
    x, y, z, out, flags, tri, info = oracle_scene(kind)
    qx, qy = L.nodes(*L.UNIT, N, N)
    XX, YY = np.meshgrid(qx, qy)
    d = Delaunay(np.c_[x, y])
    ref = LinearNDInterpolator(d, z)(XX, YY)
    simplex = d.find_simplex(np.c_[XX.ravel(), YY.ravel()]).reshape(N, N)
    decided = flags <= 1
    assert np.array_equal(np.isnan(out)[decided], np.isnan(ref)[decided])
    assert not np.isnan(out[flags == 0]).any() and np.isnan(out[flags == 1]).all()
    m = flags == 0
    assert m.sum() > 500
    assert np.array_equal(np.sort(d.simplices[simplex[m]], axis=1), tri[m])          # the same triangle as a set of indices
    err, bound = np.abs(out[m] - ref[m]), L.value_bound(x, y, z, tri[m])
    print(kind, "flags", np.bincount(flags.ravel(), minlength=4), "max |oracle - scipy|", err.max(), "smallest bound", bound.min(),
          "largest err / bound", (err / bound).max(), "walk steps", info["max_steps"])
    assert (err <= bound).all()


@pytest.mark.parametrize("kind", L.SCENES)
def test_scenes_are_almost_everywhere_certified(kind):
    flags = oracle_scene(kind)[4]
    assert (flags >= 2).mean() <= CAP
    assert (flags == 0).sum() > 500 and (flags == 1).sum() > 50                       # both sides of the hull are there


# ---- the probes
def test_probe_duplicates_lower_index_stands():
    """a tie broken by order instead of index: the duplicates carry another z, so letting the other one stand changes values"""
    x, y, z = L.scene("uniform", seed=3, n=300)
    x, y, z = np.r_[x, x[:150]], np.r_[y, y[:150]], np.r_[z, z[:150] + 1.0]
    good = L.interpolate(x, y, z, *L.UNIT, 9, 7)
    bad = L.interpolate(x, y, z, *L.UNIT, 9, 7, mistake="last")
    assert np.array_equal(good[1], bad[1]) and good[3]["n_taken"] == 300
    m = good[1] == 0
    assert m.sum() > 20 and (good[0][m] != bad[0][m]).sum() > 20
    ref = L.interpolate(x[:300], y[:300], z[:300], *L.UNIT, 9, 7)
    assert np.array_equal(good[0], ref[0], equal_nan=True) and np.array_equal(good[2], ref[2])


def test_probe_apex_lies_rings_behind_a_nearer_candidate():
    """an apex search that stops one ring early: on the scene with the hole, with a fine acceleration grid, many triangles have
    on every edge an apex that lies at least two rings farther from the edge's midpoint than another point left of that edge"""
    x, y, z, out, flags, tri, info = oracle_scene("hole")
    G = 200
    cell = lambda v: np.minimum(np.floor(v * G), G - 1).astype(int)
    hard = 0
    for t in np.unique(tri[flags == 0].reshape(-1, 3), axis=0):
        every = True
        for a, b, c in ((0, 1, 2), (1, 2, 0), (2, 0, 1)):
            pa, pb, pc = t[a], t[b], t[c]
            if L.orient(x[pa], y[pa], x[pb], y[pb], x[pc], y[pc])[0] < 0:
                pa, pb = pb, pa
            mx, my = cell(0.5 * (x[pa] + x[pb])), cell(0.5 * (y[pa] + y[pb]))
            ring = np.maximum(np.abs(cell(x) - mx), np.abs(cell(y) - my))
            left = L.orient(x[pa], y[pa], x[pb], y[pb], x, y)[0] > 0
            left[[pa, pb]] = False
            every = every and ring[left].min() + 2 <= ring[pc]
        hard += every
    print("triangles whose apex lies two rings behind a nearer candidate on every edge:", hard)
    assert hard >= 10                              # whichever edge the walk came in by, and not by a single triangle


def test_probe_certificate_must_look_at_both_sides():
    """four cocircular points: the walk ends on the diagonal with the fourth point on the OTHER side of the last edge"""
    x, y, z = np.array([0.0, 1.0, 1.0, 0.0]), np.array([0.0, 0.0, 1.0, 1.0]), np.array([0.0, 1.0, 3.0, 1.0])
    fooled = 0
    for qx, qy in ((0.3, 0.6), (0.6, 0.3), (0.8, 0.7), (0.2, 0.1), (0.45, 0.55), (0.7, 0.8), (0.75, 0.9)):
        status, t, _ = L.walk(x, y, qx, qy)
        assert status == 0
        assert L.certify(x, y, z, t, qx, qy)[0] == 2
        fooled += L.certify(x, y, z, t, qx, qy, mistake="left")[0] == 0
    assert fooled >= 1


def test_probe_area_mask_is_closed():
    """< for <=: the points on the border of the area are most of this cloud's hull"""
    x, y, z = L.scene("uniform", seed=5, n=200)
    x[:40], y[40:80] = np.repeat([0.0, 1.0], 20), np.repeat([0.0, 1.0], 20)
    good = L.interpolate(x, y, z, *L.UNIT, 9, 7)
    bad = L.interpolate(x, y, z, *L.UNIT, 9, 7, mistake="open")
    assert good[3]["n_taken"] == 200 and bad[3]["n_taken"] == 120
    assert (good[1] != bad[1]).sum() >= 10


def test_probe_vertices_are_sorted_before_the_value():
    x, y, z, out, flags, tri, info = oracle_scene("uniform")
    keep = L.taken(x, y, *L.UNIT)
    qx, qy = L.nodes(*L.UNIT, N, N)
    differ = n = 0
    for r in range(0, N, 2):
        for c in range(0, N, 2):
            if flags[r, c] != 0:
                continue
            status, t, _ = L.walk(x[keep], y[keep], qx[c], qy[r])
            f, v = L.certify(x[keep], y[keep], z[keep], t, qx[c], qy[r], mistake="unsorted")
            assert f == 0 and abs(v - out[r, c]) <= L.value_bound(x, y, z, tri[r, c])
            differ += v != out[r, c]
            n += 1
    print("values that change bits with the order of the vertices:", differ, "of", n)
    assert differ >= 10


# ---- exact scenes, on the oracle (the GPU test holds the kernel to the oracle on the same scenes)
def test_square_lattice_is_cocircular_everywhere_inside():
    x, y, z = L.square_lattice(6)
    ext = (-0.75, 5.75, -0.75, 5.75)
    out, flags, tri, info = L.interpolate(x, y, z, *ext, 14, 14)
    qx, qy = L.nodes(*ext, 14, 14)
    XX, YY = np.meshgrid(qx, qy)
    outside = (XX < 0) | (XX > 5) | (YY < 0) | (YY > 5)                               # the closed form of the hull
    assert np.array_equal(flags == 1, outside)
    assert (flags[~outside] == 2).all()
    plane = 2.0 * XX - 3.0 * YY + 1.0
    assert np.abs(out[~outside] - plane[~outside]).max() <= 16 * L.EPS * 25 * 2      # weights of 5 x 5 products, |z| <= 16


def test_too_few_points_and_collinear():
    for n in (0, 1, 2):
        out, flags, _, info = L.interpolate(np.arange(n) * 0.3, np.arange(n) * 0.2, np.ones(n), *L.UNIT, 3, 3)
        assert info["too_few"] and np.isnan(out).all() and (flags == 1).all()
    t = np.arange(1, 8) / 8.0                                                         # dyadic: exactly collinear in fp64
    assert L.interpolate(t, 0.5 * t + 0.125, t, *L.UNIT, 3, 3)[3]["too_few"]


def test_scratch_bytes_need_no_gpu():
    from wass_amd import stereo
    small, big = stereo.linear_scratch_bytes(1000, 32, 32), stereo.linear_scratch_bytes(4_000_000, 1024, 1024)
    assert 0 < small < big < 1 << 30
    assert big >= 4_000_000 * (3 * 8 + 4) + 1024 * 1024 * 9                            # at least the bucketed cloud and the result
    with pytest.raises(ValueError):
        stereo.linear_scratch_bytes(10, 0, 5)
