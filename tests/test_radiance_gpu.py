"""wass_amd.postproc's radiance chain on the GPU against the numpy restatements of tests/radiance_oracle.py (which test_radiance.py
holds to the C oracle's tables, scipy and numpy).  Every comparison is np.array_equal (equal_nan for bgimage): nothing here has a
tolerance.  Discriminating power: on the lattice cases of 37 x 67 and 130 x 257 a window offset of 4, truncation, a table without
the fix-up and exchanged phases must miss the GPU result by the fractions radiance_oracle.VARIANT_MISS states (printed).  Every test
prints its figures before it asserts."""
import os

import numpy as np
import pytest

import radiance_oracle as RO
import wass_amd
from wass_amd import postproc as P

pytestmark = pytest.mark.gpu
F = np.float32


def _torch():
    import torch
    return torch


def _same(got, want, what, equal_nan=False):
    got = got.cpu().numpy() if hasattr(got, "cpu") else np.asarray(got)
    bad = int((~((got == want) | (equal_nan & np.isnan(got) & np.isnan(want)))).sum()) if got.shape == want.shape else -1
    print(f"{what}: {bad} of {want.size} differ")
    assert got.dtype == want.dtype and got.shape == want.shape and bad == 0, what


# ---- remap_lanczos4 with explicit maps -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", [(5, 7), (37, 67), (130, 257)])
def test_remap_lattice(gpu_ctx, h, w):
    img = RO.picture(61, 97, 3)
    mx, my = RO.lattice_maps(h, w, 61, 97, 4)
    want = RO.remap_lanczos4(img, mx, my)
    got = P.remap_lanczos4(img, mx, my, ctx=gpu_ctx)
    X, ok = RO.quantise(mx.ravel())
    Y, _ = RO.quantise(my.ravel())
    print(f"{h} x {w}: {len(set(((Y & 31) * 32 + (X & 31)).tolist()))} phases, {int((want != 0).sum())} cells not zero, "
          f"{int((~ok).sum())} undefined x")
    _same(got, want, f"remap {h} x {w}, host")
    torch = _torch()
    dev = P.remap_lanczos4(torch.from_numpy(img).cuda(), torch.from_numpy(mx).cuda(), torch.from_numpy(my).cuda(), ctx=gpu_ctx)
    assert dev.is_cuda
    _same(dev, want, f"remap {h} x {w}, device")
    if h * w >= 37 * 67:
        for name, kw in RO.VARIANTS.items():
            miss = int((RO.remap_lanczos4(img, mx, my, **kw) != got).sum())
            print(f"{name}: misses the GPU result in {miss} of {got.size} cells (at least {got.size * RO.VARIANT_MISS[name]:.1f} asked)")
            assert miss >= got.size * RO.VARIANT_MISS[name]


def test_remap_windows_at_every_border(gpu_ctx):
    """every partial-window count on both sides of both axes, at every phase of the other axis' corner, and wholly outside"""
    img = RO.picture(61, 97, 8)
    xs = np.array(list(range(-9, 2)) + list(range(97 - 8, 97 + 2)), np.float64) + 3
    ys = np.array(list(range(-9, 2)) + list(range(61 - 8, 61 + 2)), np.float64) + 3
    for frac in (0.0, 1 / 32, 0.5, 31 / 32):
        mx, my = np.meshgrid((xs + frac).astype(F), (ys + frac).astype(F))
        want = RO.remap_lanczos4(img, mx, my)
        assert (want[0] == 0).all() and (want[:, -1] == 0).all()           # window start -9 and size + 1: wholly outside
        _same(P.remap_lanczos4(img, mx, my, ctx=gpu_ctx), want, f"border windows, phase {frac}")


# ---- radiance --------------------------------------------------------------------------------------------------------------------
H, W, IH, IW = 64, 96, 200, 300


@pytest.fixture(scope="module")
def scene():
    XX, YY = RO.grid(H, W)
    Z = RO.heights(8, H, W, 21)
    Z[1, 10:14, 20:30] = np.nan
    Z[5, 0, 0] = np.nan
    imgs = np.stack([RO.picture(IH, IW, 30 + t) for t in range(8)])
    want = {k: RO.radiance(imgs, Z, XX, YY, RO.pplane(IW, IH, XX, YY, k)) for k in ("inside", "crossing", "outside")}
    for v in want.values():
        v.setflags(write=False)
    return XX, YY, Z, imgs, want


@pytest.mark.parametrize("kind", ["inside", "crossing", "outside"])
def test_radiance_projections(gpu_ctx, scene, kind):
    XX, YY, Z, imgs, want = scene
    Pp = RO.pplane(IW, IH, XX, YY, kind)
    w = want[kind]
    zero = float((w == 0).mean())
    print(f"{kind}: {100 * zero:.1f} % of the cells are 0, borders reached: "
          f"{[bool((w[0][s] == 0).all()) for s in (np.s_[0, :], np.s_[-1, :], np.s_[:, 0], np.s_[:, -1])]}")
    if kind == "outside":
        assert zero == 1.0
    if kind == "inside":
        assert (w[0] != 0).mean() > 0.99
    assert (w[1, 10:14, 20:30] == 0).all()
    got = P.radiance(imgs, Z, XX, YY, Pp, ctx=gpu_ctx)
    _same(got, w, f"radiance {kind}, host, batch 8")
    for batch in (1, 2, 3):
        _same(P.radiance(imgs, Z, XX, YY, Pp, ctx=gpu_ctx, batch=batch), w, f"radiance {kind}, batch {batch}")
    singles = np.concatenate([P.radiance(imgs[t:t + 1], Z[t:t + 1], XX, YY, Pp, ctx=gpu_ctx) for t in range(8)])
    _same(singles, w, f"radiance {kind}, single frames")
    for name, kw in RO.VARIANTS.items():
        if kind != "outside":
            miss = int((RO.radiance(imgs[:1], Z[:1], XX, YY, Pp, **kw) != got[:1]).sum())
            print(f"{name}: misses the GPU result in {miss} of {H * W} cells")
            assert miss > 0


def test_radiance_calling_forms(gpu_ctx, scene, tmp_path):
    XX, YY, Z, imgs, want = scene
    Pp, w = RO.pplane(IW, IH, XX, YY, "crossing"), want["crossing"]
    torch = _torch()
    dev = P.radiance(torch.from_numpy(imgs).cuda(), torch.from_numpy(Z).cuda(), XX, YY, Pp, ctx=gpu_ctx, batch=3)
    assert dev.is_cuda
    _same(dev, w, "device tensors")
    _same(P.radiance(imgs, torch.from_numpy(Z).cuda(), XX, YY, Pp, ctx=gpu_ctx), w, "host pictures, device cube")
    mm = np.memmap(tmp_path / "z.bin", np.float32, "w+", shape=Z.shape)
    mm[:] = Z
    _same(P.radiance(imgs, mm, XX, YY, Pp, ctx=gpu_ctx), w, "memmap")
    big = np.full((8, H + 3, W + 5), np.float32(7))
    big[:, 1:1 + H, 2:2 + W] = Z
    _same(P.radiance(imgs, big[:, 1:1 + H, 2:2 + W], XX, YY, Pp, ctx=gpu_ctx, batch=5), w, "strided view")
    _same(P.radiance(iter(list(imgs)), Z, XX, YY, Pp, ctx=gpu_ctx, batch=3), w, "iterable of frames")
    from PIL import Image
    for t in range(3):
        d = tmp_path / ("%06d_wd" % t) / "undistorted"
        os.makedirs(d)
        Image.fromarray(imgs[t]).save(d / "00000001.png")
    _same(P.radiance(P.workspace_images(str(tmp_path), 1, 3), Z[:3], XX, YY, Pp, ctx=gpu_ctx), w[:3], "PNG files of a workspace")
    with pytest.raises(ValueError):
        P.radiance(iter(list(imgs[:5])), Z, XX, YY, Pp, ctx=gpu_ctx)
    # other units: datascale is applied in float32
    _same(P.radiance(imgs[:2], Z[:2] * F(0.5), XX, YY, Pp, datascale=2e-3, ctx=gpu_ctx),
          RO.radiance(imgs[:2], Z[:2] * F(0.5), XX, YY, Pp, datascale=2e-3), "datascale 2e-3")


# ---- bgimage ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,cols", [(3, 70), (16, 257)])
def test_bgimage_pairs(gpu_ctx, rows, cols):
    rng = np.random.default_rng(rows)
    base = rng.uniform(0, 1, (3000, rows, cols)).astype(F)
    base[:, 1, 5::7] = RO.wide_series(3000, len(range(5, cols, 7)), 3)
    for count, size in RO.BG_PAIRS:
        x = base[:count]
        want = RO.bgimage(x, size)
        _same(P.bgimage(x, size, ctx=gpu_ctx), want, f"bgimage {rows} x {cols}, count {count}, size {size}")


def test_bgimage_forms(gpu_ctx):
    rng = np.random.default_rng(5)
    x = rng.uniform(0, 1, (120, 16, 257)).astype(F)
    x[:, 3, :] = RO.wide_series(120, 257, 6)
    x[40, 7, 100] = np.nan
    want = RO.bgimage(x, 64)
    nan_series = np.isnan(want).any(axis=0)
    print(f"NaN series: {int(nan_series.sum())}, NaN from t = {int(np.flatnonzero(np.isnan(want[:, 7, 100]))[0])}")
    assert nan_series.sum() == 1 and np.isnan(want[-1, 7, 100])
    _same(P.bgimage(x, 64, ctx=gpu_ctx), want, "unslabbed", equal_nan=True)
    for slab in (1, 5):
        _same(P.bgimage(x, 64, ctx=gpu_ctx, slab_rows=slab), want, f"slabs of {slab} rows", equal_nan=True)
    big = np.zeros((120, 20, 300), F)
    big[:, 2:18, 30:287] = x
    out = np.zeros((120, 18, 257), F)
    _same(P.bgimage(big[:, 2:18, 30:287], 64, ctx=gpu_ctx, out=out[:, 1:17]), want, "strided view in and out", equal_nan=True)
    torch = _torch()
    d = torch.from_numpy(big).cuda()
    dev = P.bgimage(d[:, 2:18, 30:287], 64, ctx=gpu_ctx)
    assert dev.is_cuda
    _same(dev, want, "device tensor, strided", equal_nan=True)
    _same(P.bgimage(torch.from_numpy(x).cuda(), 64, ctx=gpu_ctx, slab_rows=5), want, "device tensor, slabs of 5", equal_nan=True)
    with pytest.raises(ValueError):
        P.bgimage(d, 5, ctx=gpu_ctx, out=d)


# ---- threshold -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", [(33, 65), (128, 257)])
def test_threshold(gpu_ctx, h, w):
    frames = [RO.threshold_frames(h, w, 40 + t) for t in range(5)]
    I, bg = np.stack([f[0] for f in frames]), np.stack([f[1] for f in frames])
    I[1] *= F(3.0)                                      # frames that differ in range
    I[2] = I[2] * F(0.01) - F(2.0)
    I[3], bg[3] = F(0.75), F(0.125)                     # a constant frame
    s0 = RO.isub(I[0], bg[0])
    # cells exactly at the fixed threshold, and one float32 above it
    m = np.amin(bg[0])
    for k, target in enumerate((F(0.35), np.nextafter(F(0.35), F(1)))):
        cand = (target + (bg[0] - m)).astype(F)
        hit = np.flatnonzero((cand - (bg[0] - m)).ravel() == target)[:20 + k]
        I[0].ravel()[hit[k::2]] = cand.ravel()[hit[k::2]]
    s0 = RO.isub(I[0], bg[0])
    print(f"{h} x {w}: {int((s0 == F(0.35)).sum())} cells exactly at 0.35, {int((s0 == np.nextafter(F(0.35), F(1))).sum())} just above")
    assert (s0 == F(0.35)).sum() >= 5
    want, thr = RO.threshold(I, bg)
    got, gthr = P.radiance_threshold(I, bg, ctx=gpu_ctx, batch=2)
    assert np.array_equal(gthr, thr) and gthr.dtype == np.float32
    _same(got, want, "fixed threshold 0.35, host")
    counts, edges, mins = P.radiance_histogram(I, bg, ctx=gpu_ctx, batch=3)
    for t in range(5):
        c, e = np.histogram(RO.isub(I[t], bg[t]), bins=30)
        print(f"frame {t}: range {e[0]:.6g} .. {e[-1]:.6g}, counts differ in {int((counts[t] != c).sum())} bins, sum {int(counts[t].sum())}")
        assert np.array_equal(edges[t], e) and edges.dtype == e.dtype and np.array_equal(counts[t], c) and mins[t] == np.amin(bg[t])
    wantv, thrv = RO.threshold(I, bg, use_vats=True)
    gotv, gthrv = P.radiance_threshold(I, bg, use_vats=True, ctx=gpu_ctx)
    print(f"VATS thresholds {gthrv} (oracle {thrv})")
    assert np.array_equal(gthrv, thrv)
    _same(gotv, wantv, "VATS, host")
    torch = _torch()
    dI, dbg = torch.from_numpy(I).cuda(), torch.from_numpy(bg).cuda()
    dm, dthr = P.radiance_threshold(dI, dbg, use_vats=True, ctx=gpu_ctx, batch=4)
    assert dm.is_cuda and np.array_equal(dthr, thrv)
    _same(dm, wantv, "VATS, device")
    _same(P.radiance_threshold(dI, dbg, ctx=gpu_ctx)[0], want, "fixed, device")
    # values exactly on the float32 edges of their own histogram
    s = RO.isub(I[4], bg[4])
    e = np.histogram_bin_edges(np.array([s.min(), s.max()], F), bins=30)
    onedge = np.zeros((1, h, w), F) + e[0]
    onedge.ravel()[:31] = e
    onedge.ravel()[31:61] = np.nextafter(e[1:], F(-1))
    onedge.ravel()[61:91] = np.nextafter(e[:-1], F(9))
    zero = np.zeros_like(onedge)
    c, _, _ = P.radiance_histogram(onedge, zero, ctx=gpu_ctx)
    wc, _ = np.histogram(onedge[0], bins=30)
    print(f"values on the edges: counts differ in {int((c[0] != wc).sum())} bins")
    assert np.array_equal(c[0], wc)
    bad = I.copy()
    bad[2, 5, 5] = np.nan
    with pytest.raises(ValueError):
        P.radiance_threshold(bad, bg, use_vats=True, ctx=gpu_ctx)
    _same(P.radiance_threshold(bad, bg, ctx=gpu_ctx)[0], RO.threshold(bad, bg)[0], "a NaN cell with the fixed threshold")
    nbg = bg.copy()
    nbg[1, 0, 0] = np.nan
    with np.errstate(invalid="ignore"):
        _same(P.radiance_threshold(I, nbg, ctx=gpu_ctx)[0], RO.threshold(I, nbg)[0], "a NaN in the background")


# ---- end to end ------------------------------------------------------------------------------------------------------------------
def test_chain(gpu_ctx):
    h, w, n = 48, 80, 40
    XX, YY = RO.grid(h, w)
    Z = RO.heights(n, h, w, 50)
    rng = np.random.default_rng(51)
    imgs = np.stack([np.clip(RO.picture(150, 220, 60, noise=5.0).astype(int) // 2 + (rng.uniform(size=(150, 220)) > 0.98) * 120, 0, 255)
                     .astype(np.uint8) for _ in range(n)])
    Pp = RO.pplane(220, 150, XX, YY, "inside")
    r = RO.radiance(imgs, Z, XX, YY, Pp)
    b = RO.bgimage(r, 15)
    for vats in (False, True):
        wm, wt = RO.threshold(r, b, use_vats=vats)
        torch = _torch()
        gr = P.radiance(torch.from_numpy(imgs).cuda(), torch.from_numpy(Z).cuda(), XX, YY, Pp, ctx=gpu_ctx)
        gb = P.bgimage(gr, 15, ctx=gpu_ctx)
        gm, gt = P.radiance_threshold(gr, gb, use_vats=vats, ctx=gpu_ctx)
        print(f"chain, VATS {vats}: {100 * wm.mean():.2f} % of the cells above the threshold, thresholds {gt[:3]} ...")
        _same(gr, r, "chain: radiance")
        _same(gb, b, "chain: background")
        assert np.array_equal(gt, wt) and 0 < wm.mean() < 0.5
        _same(gm, wm, "chain: mask")
        hm, ht = P.radiance_threshold(P.radiance(imgs, Z, XX, YY, Pp, ctx=gpu_ctx), P.bgimage(r, 15, ctx=gpu_ctx), use_vats=vats, ctx=gpu_ctx)
        assert np.array_equal(ht, wt)
        _same(hm, wm, "chain from the host: mask")
