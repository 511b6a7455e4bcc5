"""Wave-by-wave statistics on the GPU: every map bit for bit against the numpy oracle (tests/wavestats_oracle.py).  The exactness
rests on fp64 add, multiply and divide alone, each rounded on its own; sqrt runs in numpy on both sides."""
import functools

import numpy as np
import pytest

import wavestats_oracle as WO
import wavestats_probes as WP
from wass_amd import postproc as P

pytestmark = pytest.mark.gpu

MAPS = WO.FIELDS + ("n_cross", "n_waves", "sigma", "hs_m0", "skewness", "kurtosis", "h_rms")
WIDTHS, HEIGHTS = (1, 63, 64, 65, 257), (1, 3)
# 8 samples are loaded ahead of the scan: 7, 8, 9 and 15, 16, 17 sit around one and two blocks; 4099 = 512 blocks and a tail of 3
COUNTS = (1, 2, 3, 7, 8, 9, 15, 16, 17, 4099)


def _host(v):
    return v.cpu().numpy() if hasattr(v, "data_ptr") else np.asarray(v)


def assert_same(got, ref, where=""):
    for name in MAPS:
        g = _host(getattr(got, name))
        assert g.dtype == ref[name].dtype and g.shape == ref[name].shape, (name, where)
        if not np.array_equal(g, ref[name], equal_nan=True):
            bad = np.argwhere(~((g == ref[name]) | (np.isnan(g) & np.isnan(ref[name]))))
            r, c = bad[0]
            pytest.fail(f"{where}: {name} differs in {len(bad)} cells, first at {(r, c)}: {g[r, c]!r} for {ref[name][r, c]!r}")
    if ref["hist"] is None:
        assert got.hist is None
    else:
        assert got.hist.dtype == np.uint64 and np.array_equal(got.hist, ref["hist"]), where


def assert_same_bits(a, b):
    for name in MAPS:
        assert np.array_equal(_host(getattr(a, name)), _host(getattr(b, name)), equal_nan=True), name
    assert (a.hist is None and b.hist is None) or np.array_equal(a.hist, b.hist)


@functools.lru_cache(maxsize=None)
def _shape_case(count):
    """the widest cube of `count` frames and its oracle; a narrower case is a corner of both (a cell depends on no other)"""
    z = WP.random_cube(count, max(HEIGHTS), max(WIDTHS), seed=100 + count, noise=0.4)
    z.setflags(write=False)
    kw = dict(dt=0.25, datascale=1e-3, hist_bins=12, hist_width=4e-4)
    return z, kw, WO.wave_stats(z, **kw)


@pytest.mark.parametrize("count", COUNTS)
def test_shapes(gpu_ctx, count):
    z, kw, ref = _shape_case(count)
    for H in HEIGHTS:
        for W in WIDTHS:
            got = P.wave_statistics(np.ascontiguousarray(z[:, :H, :W]), ctx=gpu_ctx, **kw)
            part = {n: (v[..., :H, :W] if n != "hist" else None) for n, v in ref.items()}
            live = ~np.isnan(part["H"])
            q = np.floor(part["H"][live] / kw["hist_width"])
            part["hist"] = np.bincount(np.minimum(q, kw["hist_bins"] - 1).astype(np.int64), minlength=kw["hist_bins"]).astype(np.uint64)
            assert_same(got, part, f"{count} x {H} x {W}")
    if count == 4099:
        assert ref["n_waves"].max() > 300 and ref["hist"][-1] > 0 and (ref["hist"] > 0).sum() >= 6


@pytest.mark.parametrize("name", sorted(WP.probes()))
def test_probe(gpu_ctx, name):
    z, kw = WP.probes()[name]
    for crossing in ("up", "down"):
        assert_same(P.wave_statistics(z, crossing=crossing, ctx=gpu_ctx, **kw), WO.wave_stats(z, crossing=crossing, **kw), f"{name}, {crossing}")


def test_nan_and_infinity_touch_one_cell_each(gpu_ctx):
    z = WP.random_cube(70, 3, 66, seed=7)
    kw = dict(dt=0.5, hist_bins=8, hist_width=0.5)
    clean = P.wave_statistics(z, ctx=gpu_ctx, **kw)
    z2 = z.copy()
    z2[69, 1, 64], z2[0, 1, 63], z2[33, 2, 0] = np.nan, -np.inf, np.inf
    got = P.wave_statistics(z2, ctx=gpu_ctx, **kw)
    assert_same(got, WO.wave_stats(z2, **kw), "invalid cells")
    bad = np.zeros((3, 66), bool)
    bad[1, 64] = bad[1, 63] = bad[2, 0] = True
    for name in MAPS:
        g, c = getattr(got, name), getattr(clean, name)
        assert np.array_equal(g[~bad], c[~bad]), name
        assert (g[bad] == -1).all() if g.dtype == np.int32 else np.isnan(g[bad]).all(), name
    assert got.hist.sum() == got.n_waves[~bad].sum() == clean.hist.sum() - clean.n_waves[bad].sum()


def test_down_is_up_on_the_negated_cube(gpu_ctx):
    z = WP.random_cube(130, 2, 65, seed=8)
    kw = dict(dt=0.5, datascale=2e-3, hist_bins=6, hist_width=1e-3)
    dn = P.wave_statistics(z, crossing="down", ctx=gpu_ctx, **kw)
    up = P.wave_statistics(-z, crossing="up", ctx=gpu_ctx, **kw)
    assert_same(dn, WO.wave_stats(z, crossing="down", **kw), "down")
    swap = {"mean": -up.mean, "m3": -up.m3, "eta_max": -up.eta_min, "eta_min": -up.eta_max, "skewness": -up.skewness}
    for name in MAPS:
        assert np.array_equal(getattr(dn, name), swap.get(name, getattr(up, name)), equal_nan=True), name
    assert np.array_equal(dn.hist, up.hist) and (dn.n_waves >= 2).all()
    assert not np.array_equal(dn.h_13, P.wave_statistics(z, ctx=gpu_ctx, **kw).h_13)


def test_input_forms_give_the_same_bits(gpu_ctx, tmp_path):
    import torch
    z = WP.random_cube(40, 5, 67, seed=9)
    z[11, 2, 3] = np.nan
    kw = dict(dt=0.5, datascale=1e-3, hist_bins=5, hist_width=1e-3)
    base = P.wave_statistics(z, ctx=gpu_ctx, **kw)
    assert_same(base, WO.wave_stats(z, **kw), "contiguous host cube")
    assert P.wave_statistics_scratch_bytes(40, 5, 67, slab_rows=1)[1] == 1
    assert_same_bits(P.wave_statistics(z, ctx=gpu_ctx, slab_rows=1, **kw), base)
    assert_same_bits(P.wave_statistics(z, ctx=gpu_ctx, slab_rows=2, **kw), base)
    assert_same_bits(P.wave_statistics(z, ctx=gpu_ctx, **kw), base)                       # a second run
    big = np.full((80, 7, 70), np.float32(7.0))
    view = big[::2, 1:6, 2:69]
    view[...] = z
    assert view.strides == (2 * 7 * 70 * 4, 70 * 4, 4)
    assert_same_bits(P.wave_statistics(view, ctx=gpu_ctx, **kw), base)
    assert_same_bits(P.wave_statistics(view, ctx=gpu_ctx, slab_rows=1, **kw), base)
    mm = np.memmap(tmp_path / "cube.f32", np.float32, "w+", shape=z.shape)
    mm[...] = z
    mm.flush()
    assert_same_bits(P.wave_statistics(np.memmap(tmp_path / "cube.f32", np.float32, "r", shape=z.shape), ctx=gpu_ctx, **kw), base)
    d = torch.from_numpy(z).cuda()
    on_dev = P.wave_statistics(d, ctx=gpu_ctx, **kw)
    assert all(hasattr(getattr(on_dev, n), "data_ptr") for n in MAPS) and isinstance(on_dev.hist, np.ndarray)
    assert_same_bits(on_dev, base)
    assert_same_bits(P.wave_statistics(d, ctx=gpu_ctx, slab_rows=1, **kw), base)
    assert_same_bits(P.wave_statistics(d, ctx=gpu_ctx, **kw), base)
    dview = torch.from_numpy(big).cuda()[::2, 1:6, 2:69]
    assert_same_bits(P.wave_statistics(dview, ctx=gpu_ctx, slab_rows=2, **kw), base)
    assert on_dev.summary() == base.summary()
    s = base.summary()
    assert s["valid_cells"] == 5 * 67 - 1 and s["n_waves"] == base.n_waves[base.n_waves > 0].sum() == base.hist.sum()
    assert s["h_max"] == np.nanmax(base.h_max) == base.h_max[s["h_max_cell"]] and s["eta_max"] == base.eta_max[s["eta_max_cell"]]
    assert s["median_h_13"] == np.nanmedian(base.h_13) and s["median_hs_m0"] == np.nanmedian(base.hs_m0)


@pytest.mark.parametrize("bins", [1, 2, 512, 513, 3000])
def test_histogram(gpu_ctx, bins):
    """up to 512 bins a block counts in LDS before it adds to the histogram, above that every wave goes straight to memory"""
    z = WP.random_cube(200, 3, 130, seed=13, noise=0.5)
    z[100, 1, 5] = np.nan
    kw = dict(dt=0.5, hist_bins=bins, hist_width=3.0 / bins if bins > 2 else 1.0)
    ref = WO.wave_stats(z, **kw)
    got = P.wave_statistics(z, ctx=gpu_ctx, **kw)
    assert_same(got, ref, f"{bins} bins")
    assert got.hist.sum() == got.n_waves[got.n_waves > 0].sum() > 2000 and got.hist[-1] > 0
    assert bins < 512 or (got.hist > 0).sum() > 300
    assert_same_bits(P.wave_statistics(z, ctx=gpu_ctx, slab_rows=1, **kw), got)


def test_no_histogram_and_no_demean(gpu_ctx):
    z = WP.random_cube(50, 2, 9, seed=10)
    for kw in (dict(dt=1.0), dict(dt=1.0, demean=False), dict(dt=2.0, demean=False, crossing="down", datascale=-1.5)):
        got = P.wave_statistics(z, ctx=gpu_ctx, **kw)
        assert got.hist is None
        assert_same(got, WO.wave_stats(z, **kw), str(kw))


def _sea(count, H, W, dt, seed):
    """millimetres: a narrow band of long-crested components around 0.15 Hz above a level of 300, NaN outside a disc"""
    rng = np.random.default_rng(seed)
    t = np.arange(count)[:, None, None] * dt
    y, x = np.mgrid[0:H, 0:W][:, None]
    z = np.zeros((count, H, W))
    for f in rng.uniform(0.13, 0.17, 12):
        k = (2 * np.pi * f) ** 2 / 9.81
        z += rng.uniform(60.0, 140.0) * np.cos(2 * np.pi * f * t - k * (0.9 * x + 0.4 * y) + rng.uniform(0, 2 * np.pi))
    z += 300.0
    z[:, (y[0] - H / 2 + 0.5) ** 2 + (x[0] - W / 2 + 0.5) ** 2 > (0.48 * min(H, W)) ** 2 + 20] = np.nan
    return z.astype(np.float32)


def test_filtered_sea_into_wave_statistics(gpu_ctx):
    dt, count = 0.5, 600
    z = _sea(count, 10, 14, dt, seed=11)
    mask = np.isnan(z[0])
    assert 10 < mask.sum() < 100 and np.array_equal(np.isnan(z).any(axis=0), mask)
    filt = P.butterworth_filter(z, dt, cutoff=0.05, type="highpass", ctx=gpu_ctx)
    got = P.wave_statistics(filt, dt, datascale=1e-3, ctx=gpu_ctx, hist_bins=20, hist_width=0.1)
    assert np.array_equal(got.n_cross < 0, mask) and np.isnan(got.h_13[mask]).all()
    assert_same(got, WO.wave_stats(filt, dt, datascale=1e-3, hist_bins=20, hist_width=0.1), "filtered sea")
    assert got.hist.sum() == got.n_waves[~mask].sum()
    # The band of h_13 / hs_m0: the oracle's own ratios on the unfiltered sea (it removes the level itself).  The high-pass at a third
    # of the band's frequency leaves the waves as they are but for its transients, which may add or take a wave or move one across
    # the cut of the third: h_13 then changes by at most about one part in n13 = Nw / 3.
    raw = WO.wave_stats(np.where(mask, np.float32(0), z), dt, datascale=1e-3)
    ratio = (raw["h_13"] / raw["hs_m0"])[~mask]
    slack = 1.0 / raw["n_waves"][~mask].min() * 3.0
    lo, hi = ratio.min() * (1 - slack), ratio.max() * (1 + slack)
    print("h_13 / hs_m0 of the oracle on the raw sea:", ratio.min(), ratio.max(), "band", lo, hi)
    assert 0.7 < lo < hi < 1.3                           # a narrow-banded sea: near the Rayleigh value of 1.0
    mine = (got.h_13 / got.hs_m0)[~mask]
    print("on the GPU, filtered:", mine.min(), mine.max())
    assert (mine >= lo).all() and (mine <= hi).all()
    s = got.summary()
    assert s["valid_cells"] == (~mask).sum() and 5.5 < s["median_t_z"] < 7.5 and 0.5 < s["median_hs_m0"] < 3.0
