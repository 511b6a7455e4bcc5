"""The radiance chain without a GPU: the numpy restatements of tests/radiance_oracle.py against what can be had here -- the C oracle's
table builder, scipy's uniform_filter1d, numpy's histogram, a float64 Lanczos resampling -- and the parts of wass_amd.postproc that
need no device (the table the library builds, the VATS rule, scratch arithmetic, argument errors).  OpenCV itself is not
available: the Lanczos4 restatement is unpinned (see the oracle's docstring).  Every test prints its figures before it asserts."""
import numpy as np
import pytest

import radiance_oracle as RO
from wass_amd import postproc as P

F = np.float32


@pytest.mark.parametrize("ksize", [2, 4])
def test_table_builder_equals_the_c_oracle(oracle, ksize):
    got, want = RO.inter_tab(ksize), oracle.inter_tab(ksize)
    print(f"ksize {ksize}: {int((got != want).sum())} of {want.size} entries differ")
    assert np.array_equal(got, want)


def test_lanczos4_table_structure_and_library_table():
    tab = RO.lanczos_tab().astype(np.int64)
    raw = RO.lanczos_tab(fixup=False).astype(np.int64)
    sums = tab.sum(axis=(1, 2))
    fixed = (tab != raw).any(axis=(1, 2))
    print(f"phases that sum to 32768: {int((sums == 32768).sum())} of 1024; fixed-up phases: {int(fixed.sum())}; "
          f"entries changed per fixed phase: {(tab != raw).sum(axis=(1, 2))[fixed].max()}")
    assert (sums == 32768).all()
    assert tab[0, 3, 3] == 32767 and tab[0, 4, 4] == 1 and np.count_nonzero(tab[0]) == 2
    # the fix-up touches one entry, inside OpenCV's window of taps 4 .. 5
    changed = np.argwhere(tab != raw)
    assert ((tab != raw).sum(axis=(1, 2)) <= 1).all() and changed[:, 1:].min() >= 4 and changed[:, 1:].max() <= 5
    # symmetry: phase (fy, fx) transposed is phase (fx, fy), before the fix-up everywhere
    r4 = raw.reshape(32, 32, 8, 8)
    assert np.array_equal(r4.transpose(1, 0, 3, 2), r4)
    t4 = tab.reshape(32, 32, 8, 8)
    off = t4.transpose(1, 0, 3, 2) != t4
    print(f"entries where the transposed table differs: {int(off.sum())} (all in fixed-up entries)")
    assert not (off & ~((t4 != r4) | (t4 != r4).transpose(1, 0, 3, 2))).any()
    lib = P.lanczos4_table()
    print(f"library table against the numpy builder: {int((lib.reshape(1024, 8, 8) != tab).sum())} entries differ")
    assert lib.dtype == np.int16 and np.array_equal(lib.reshape(1024, 8, 8), tab)


def test_remap_properties():
    img = RO.picture(61, 97, 1)
    yy, xx = np.mgrid[0:61, 0:97]
    same = RO.remap_lanczos4(img, xx.astype(F), yy.astype(F))
    print(f"integer maps: {int((same != img).sum())} pixels differ from the source")
    assert np.array_equal(same, img)
    rng = np.random.default_rng(2)
    mx, my = rng.uniform(3, 97 - 5, (40, 50)).astype(F), rng.uniform(3, 61 - 5, (40, 50)).astype(F)
    for level in (0, 1, 77, 255):
        flat = RO.remap_lanczos4(np.full((61, 97), level, np.uint8), mx, my)
        assert (flat == level).all(), level
    # a smooth picture against float64 Lanczos: quantising the position to 1/32 moves it by at most 1/64 per axis, the int16
    # weights and the final rounding cost less than one grey level
    y, x = np.mgrid[0:120, 0:160]
    smooth = np.clip(np.rint(128 + 60 * np.sin(x / 11.0) + 50 * np.cos(y / 13.0)), 0, 255).astype(np.uint8)
    mx, my = rng.uniform(4, 160 - 6, (64, 64)).astype(F), rng.uniform(4, 120 - 6, (64, 64)).astype(F)
    got = RO.remap_lanczos4(smooth, mx, my).astype(np.float64)
    want = RO.lanczos_float(smooth, mx, my).reshape(got.shape)
    gy, gx = np.gradient(smooth.astype(np.float64))
    bound = 1.0 + max(np.abs(gx).max(), np.abs(gy).max()) / 32.0
    err = np.abs(got - np.clip(want, 0, 255)).max()
    print(f"against float64 Lanczos: largest error {err:.3f} grey levels, bound {bound:.3f}")
    assert np.isfinite(want).all() and err <= bound


def test_undefined_map_values_give_zero_and_variants_differ():
    img = RO.picture(61, 97, 3)
    mx, my = RO.lattice_maps(37, 67, 61, 97, 4)
    want = RO.remap_lanczos4(img, mx, my)
    with np.errstate(invalid="ignore"):
        undefined = ~(np.abs(mx) < 2.0 ** 26) | ~(np.abs(my) < 2.0 ** 26)
    print(f"{int(undefined.sum())} undefined cells, all zero: {bool((want[undefined] == 0).all())}")
    assert undefined.sum() == 14 and (want[undefined] == 0).all()
    X, _ = RO.quantise(mx.ravel())
    Y, _ = RO.quantise(my.ravel())
    assert len(set(((Y & 31) * 32 + (X & 31)).tolist())) == 1024
    for name, kw in RO.VARIANTS.items():
        miss = int((RO.remap_lanczos4(img, mx, my, **kw) != want).sum())
        print(f"{name}: differs from the oracle in {miss} of {want.size} cells")
        assert miss >= want.size * RO.VARIANT_MISS[name]


@pytest.mark.parametrize("count,size", RO.BG_PAIRS)
def test_bgimage_oracle_equals_scipy(count, size):
    from scipy.ndimage import uniform_filter1d
    rng = np.random.default_rng(count * 7 + size)
    x = rng.uniform(0, 1, (count, 23)).astype(F)
    x[:, 5] = RO.wide_series(count, 1, size)[:, 0]
    want = uniform_filter1d(x, size=size, axis=0, mode="reflect")
    got = RO.bgimage(x, size)
    print(f"count {count}, size {size}: {int((got != want).sum())} of {want.size} samples differ from scipy")
    assert want.dtype == np.float32 and np.array_equal(got, want)


def test_bgimage_update_order_and_nan():
    from scipy.ndimage import uniform_filter1d
    x = RO.wide_series(400, 64, 9)
    want = uniform_filter1d(x, size=7, axis=0, mode="reflect")
    miss = {u: int((RO.bgimage(x, 7, update=u) != want).sum()) for u in ("diff", "two", "divided")}
    print(f"wide series, size 7: samples that differ from scipy: {miss}")
    assert miss["diff"] == 0 and miss["two"] > 0 and miss["divided"] > 0
    y = np.random.default_rng(1).uniform(0, 1, (50, 3)).astype(F)
    y[20, 1] = np.nan
    with np.errstate(invalid="ignore"):
        want = uniform_filter1d(y, size=5, axis=0, mode="reflect")
    got = RO.bgimage(y, 5)
    print(f"NaN at t = 20: the series is NaN from t = {int(np.flatnonzero(np.isnan(got[:, 1]))[0])} to the end")
    assert np.array_equal(got, want, equal_nan=True) and np.isnan(got[18:, 1]).all() and np.isfinite(got[:18, 1]).all()
    assert np.isfinite(got[:, [0, 2]]).all()


def test_threshold_oracle_counts_equal_numpy():
    I, bg = RO.threshold_frames(33, 65, 5)
    s = RO.isub(I, bg)
    edges = np.histogram_bin_edges(np.array([s.min(), s.max()], F), bins=30)
    s.ravel()[:31] = edges                              # values exactly on the float32 edges
    s.ravel()[31:61] = np.nextafter(edges[1:], F(-1))   # and just below them
    want, e2 = np.histogram(s, bins=30)
    got = RO.counts_by_edges(s, edges)
    print(f"edges dtype {edges.dtype}; counts differ in {int((got != want).sum())} bins")
    assert edges.dtype == np.float32 and np.array_equal(edges, e2) and np.array_equal(got, want)
    flat = np.full((9, 11), F(0.25))
    want, e = np.histogram(flat, bins=30)
    assert np.array_equal(np.histogram_bin_edges(np.array([0.25, 0.25], F), bins=30), e)
    assert np.array_equal(RO.counts_by_edges(flat, e), want)


def test_vats_rule_equals_the_oracle():
    for seed in range(20):
        I, bg = RO.threshold_frames(40, 50, 100 + seed)
        s = RO.isub(I, bg)
        counts, edges = np.histogram(s, bins=30)
        got, want = P.vats_threshold(counts, edges), RO.vats(s)
        assert got.dtype == np.float32 and got == want, (seed, got, want)
    flat = np.full((5, 5), F(0.5))
    counts, edges = np.histogram(flat, bins=30)
    print(f"constant frame: threshold {P.vats_threshold(counts, edges)} (oracle {RO.vats(flat)})")
    assert P.vats_threshold(counts, edges) == RO.vats(flat)


def test_projection_against_one_matrix_product():
    H = W = 1024
    XX, YY = RO.grid(H, W, 0.1)
    Z = RO.heights(1, H, W, 6)[0]
    Pp = RO.pplane(2456, 2058, XX, YY, "crossing")
    Pc = RO.pcam(Pp, 2456, 2058)
    assert np.array_equal(Pc, P.radiance_pcam(Pp, 2456, 2058))
    mx, my = RO.project(Z, XX, YY, Pc)
    rx, ry = RO.project_matmul(Z, XX, YY, Pc)
    # float32(1e-3) is 1e-3 (1 + 4.8e-8) and the product and the quotient each round once: the two heights differ by at most
    # 1.6e-7 |z|, which moves row k by |P[k][2]| times as much; the matrix product may round its sums otherwise (a few 2^-53);
    # both maps are then rounded to float32
    z = np.abs(Z.astype(np.float64) * 1e-3)
    r2 = np.abs(((Pc[2, 0] * XX + Pc[2, 1] * YY) + Pc[2, 2] * z) + Pc[2, 3])
    worst = 0.0
    for m, r, k in ((mx, rx, 0), (my, ry, 1)):
        bound = 1.7e-7 * z * (abs(Pc[k, 2]) + np.abs(m) * abs(Pc[2, 2])) / r2 + 2.0 ** -23 * np.abs(m) + 1e-9
        worst = max(worst, float((np.abs(m.astype(np.float64) - r) / bound).max()))
    qx, _ = RO.quantise(mx.ravel())
    qrx, _ = RO.quantise(rx.ravel())
    qy, _ = RO.quantise(my.ravel())
    qry, _ = RO.quantise(ry.ravel())
    moved = (qx != qrx) | (qy != qry)
    print(f"largest map difference / bound = {worst:.3f}; quantised coordinates differ in {int(moved.sum())} of {moved.size} cells")
    assert worst <= 1.0
    assert moved.sum() <= moved.size // 10000
    img = RO.picture(2058, 2456, 7, noise=10.0)
    sub = np.s_[::8, ::8]
    a = RO.remap_lanczos4(img, mx[sub], my[sub])
    b = RO.remap_lanczos4(img, rx[sub], ry[sub])
    assert np.array_equal(a[~moved.reshape(H, W)[sub]], b[~moved.reshape(H, W)[sub]])


def test_scratch_arithmetic():
    al = lambda v: (v + 255) & ~255
    assert P.radiance_scratch_bytes(100, 64, 96, 200, 300, host=False) == (0, 8)
    b, n = P.radiance_scratch_bytes(3, 64, 96, 200, 300, batch=8)
    assert n == 3 and b == 2 * al(64 * 96 * 8) + al(3 * 200 * 300) + 2 * al(3 * 64 * 96 * 4)
    b, n = P.radiance_scratch_bytes(3000, 1024, 1024, 2058, 2456, batch=1024)
    print(f"radiance, 1024^2 from 2456 x 2058, batch 1024 asked: {n} frames per launch, {b / 2 ** 30:.2f} GiB")
    assert b <= 16 << 30 and n == 1024
    assert P.bgimage_scratch_bytes(3000, 1024, 1024, host=False) == (0, 1024)
    b, r = P.bgimage_scratch_bytes(3000, 1024, 1024)
    print(f"bgimage 3000 x 1024 x 1024 from the host: slabs of {r} rows, {b / 2 ** 30:.2f} GiB")
    assert b <= 16 << 30 and r == ((16 << 30) - 512) // (3000 * 1024 * 8) and b == 2 * al(3000 * r * 1024 * 4)
    assert P.bgimage_scratch_bytes(10, 16, 257, slab_rows=5) == (2 * al(10 * 5 * 257 * 4), 5)
    head = al(7 * 32) + 2 * al(7 * 4) + al(7 * 31 * 4) + al(7 * 30 * 4)
    assert P.radiance_threshold_scratch_bytes(7, 33, 65, host=False) == (head, 7)
    assert P.radiance_threshold_scratch_bytes(7, 33, 65, batch=2) == (head + 2 * al(2 * 33 * 65 * 4) + al(2 * 33 * 65), 2)
    for bad in (lambda: P.radiance_scratch_bytes(0, 4, 4, 8, 8), lambda: P.radiance_scratch_bytes(1, 4, 4, 40000, 8),
                lambda: P.bgimage_scratch_bytes(4, 4, 4, filtersize=0), lambda: P.radiance_threshold_scratch_bytes(1, 0, 4)):
        with pytest.raises(ValueError):
            bad()


def test_argument_errors():
    Z = np.zeros((2, 4, 5), F)
    XX, YY = RO.grid(4, 5)
    img = np.zeros((2, 8, 9), np.uint8)
    with pytest.raises(NotImplementedError):
        P.radiance(img, Z, XX, YY, np.eye(4), upscalefactor=2)
    for call in (lambda: P.radiance(img, Z[0], XX, YY, np.eye(4)), lambda: P.radiance(img, Z, XX[:3], YY, np.eye(4)),
                 lambda: P.radiance(img, Z, XX, YY, np.eye(3)), lambda: P.radiance(img[:1], Z, XX, YY, np.eye(4)),
                 lambda: P.radiance(img, Z, XX, YY, np.eye(4), batch=0), lambda: P.bgimage(Z[0]), lambda: P.bgimage(Z, filtersize=0),
                 lambda: P.radiance_threshold(Z, Z[:1]), lambda: P.radiance_threshold(Z, Z, batch=0),
                 lambda: P.remap_lanczos4(img[0], np.zeros((3, 3), F), np.zeros((3, 4), F)),
                 lambda: P.remap_lanczos4(img, np.zeros((3, 3), F), np.zeros((3, 3), F)), lambda: P.radiance_pcam(np.eye(3), 4, 4)):
        with pytest.raises(ValueError):
            call()
