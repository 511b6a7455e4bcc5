"""The staging that the one-shot cube operators share (csrc/cube.h: the scratch arena, upload_rows / download_rows, the slab and
batch rules), on the smallest shape at which it can go wrong: H = 5 rows of W = 67 cells (one wave and three lanes), 5 frames (the
temporal filter: padlen + 1 with a one-section filter; pyr_up, whose batch of 8 is not the caller's to set: 9), pictures of 9 x 11,
slab_rows = 2 (slabs of 2, 2, 1 rows) and batch = 2 (batches of 2, 2, 1 frames).  The cube is a view that is dense in no axis but
the last: every second frame and an inner window of rows and columns of an array whose other cells hold a guard value, and so is
`out` where the operator takes one (a contiguous window of a guarded vector where it must be contiguous).

Every operator with a host and a device form runs four times, host and device, default and small slab or batch.  All four give the
same bits, no guard cell of an input's or an output's parent changes, and the result is array_equal to the operator's oracle under
tests/; the incident angles keep the bound of their own test files (visibility_oracle.angle_bound)."""
import functools

import numpy as np
import pytest

import filter_oracle as FO
import polarimetric_oracle as PO
import pyramid_oracle as PYO
import radiance_oracle as RO
import visibility_oracle as VO
import wavestats_oracle as WO
from guarded import Guarded, host as _host
from wass_amd import postproc as P

pytestmark = pytest.mark.gpu

H, W, COUNT, IH, IW = 5, 67, 5, 9, 11


# ---- the operators: run(ctx, g, small) -> {name: host array}, oracle() -> the same names (or, for angles, (a64, n) per frame) ----------
@functools.lru_cache(maxsize=None)
def _cube(count=COUNT, seed=5):
    z = (400.0 * np.random.default_rng(seed).standard_normal((count, H, W))).astype(np.float32)
    z.setflags(write=False)
    return z


@functools.lru_cache(maxsize=None)
def _sos():
    sos = P.butter_sos(2, 1.0, "lowpass", 12.0)
    assert sos.shape[0] == 1
    return sos


def run_sosfiltfilt(ctx, g, small):
    x = _cube(P.sos_padlen(_sos()) + 1)
    out = g.out(x.shape, np.float32)
    assert P.sosfiltfilt(_sos(), g.input(x), ctx=ctx, out=out, slab_rows=2 if small else 0) is out
    return {"out": _host(out)}


def oracle_sosfiltfilt():
    return {"out": FO.sosfiltfilt(_sos(), _cube(P.sos_padlen(_sos()) + 1)).astype(np.float32)}


def run_bgimage(ctx, g, small):
    out = g.out(_cube().shape, np.float32)
    assert P.bgimage(g.input(_cube()), 3, ctx=ctx, out=out, slab_rows=2 if small else 0) is out
    return {"out": _host(out)}


def run_zeromean(ctx, g, small):                # its slabs are cut by the scratch cap alone
    out = g.out(_cube().shape, np.float32)
    assert P.zeromean(g.input(_cube()), out=out, ctx=ctx) is out
    return {"out": _host(out)}


def run_clip_cube(ctx, g, small):               # its batch is cut by the scratch cap alone
    out = g.out(_cube().shape, np.float32)
    got, vmin, vmax = P.clip_cube(g.input(_cube()), -250.0, 300.0, out=out, ctx=ctx)
    assert got is out
    return {"out": _host(out), "vmin": np.float32(vmin), "vmax": np.float32(vmax)}


def oracle_clip_cube():
    out, vmin, vmax = PO.clip_cube(_cube(), -250.0, 300.0)
    return {"out": out, "vmin": vmin, "vmax": vmax}


WAVE_KW = dict(dt=0.25, datascale=1e-3, hist_bins=12, hist_width=1e-1)
WAVE_MAPS = WO.FIELDS + ("n_cross",)


def run_wave_statistics(ctx, g, small):
    r = P.wave_statistics(g.input(_cube()), ctx=ctx, slab_rows=2 if small else 0, **WAVE_KW)
    return dict({k: _host(getattr(r, k)) for k in WAVE_MAPS}, hist=r.hist)


def oracle_wave_statistics():
    ref = WO.wave_stats(_cube(), **WAVE_KW)
    assert ref["hist"].sum() > 0
    return {k: ref[k] for k in WAVE_MAPS + ("hist",)}


@functools.lru_cache(maxsize=None)
def _sea():
    XX, YY = VO.make_grid(H, W, 0.25)
    cam = VO.camera(XX, YY, "west", 4.0, 25.0)
    Z = np.stack([VO.make_sea(H, W, 0.25, 11, 1.0, t=0.7 * t) for t in range(COUNT)])
    for a in (cam, Z):                          # (the grid goes to the device through torch.from_numpy, which wants it writable)
        a.setflags(write=False)
    return Z, XX, YY, cam


def run_visibility_map(ctx, g, small):
    Z, XX, YY, cam = _sea()
    om, oa = g.out(Z.shape, np.uint8, dense=True), g.out(Z.shape, np.float32, dense=True)
    m, a, pct = P.visibility_map(g.input(Z), XX, YY, cam, angle_limit=None, ctx=ctx, out_occlusion=om, out_angles=oa, batch=2 if small else 8)
    assert m is om and a is oa
    return {"occlusion": _host(om), "angles": _host(oa), "percent": pct}


def oracle_visibility_map():
    Z, XX, YY, cam = _sea()
    masks, _, pct = VO.visibility(Z, XX, YY, cam[:3, 3], angle_limit=None)
    assert 0 < masks.sum() < masks.size
    return {"occlusion": masks, "percent": pct, "angles": [VO.noise(XX, YY, VO.heights(Z[t]), cam[:3, 3]) for t in range(COUNT)]}


@functools.lru_cache(maxsize=None)
def _radiance_scene():
    XX, YY = RO.grid(H, W)
    imgs = np.stack([RO.picture(IH, IW, 30 + t) for t in range(COUNT)])
    return imgs, RO.heights(COUNT, H, W, 21), XX, YY, RO.pplane(IW, IH, XX, YY, "crossing")


def run_radiance(ctx, g, small):
    imgs, Z, XX, YY, Pp = _radiance_scene()
    out = g.out(Z.shape, np.float32, dense=True)
    assert P.radiance(imgs, g.input(Z), XX, YY, Pp, ctx=ctx, out=out, batch=2 if small else 8) is out
    return {"out": _host(out)}


def oracle_radiance():
    want = RO.radiance(*_radiance_scene())
    assert (want != 0).any()
    return {"out": want}


def run_pyr_up(ctx, g, small):                  # 9 frames: the batch of 8 and a last one of 1
    x = _cube(9)
    out = g.out((9, 2 * H, 2 * W), np.float32)
    assert P.pyr_up(g.input(x), 1, ctx=ctx, out=out) is out
    return {"out": _host(out)}


@functools.lru_cache(maxsize=None)
def _pol_scene():
    Z, XX, YY, cam = _sea()
    cx, cy = XX.mean(), YY.mean()
    shift = np.eye(4)
    shift[0, 3], shift[1, 3] = -cx, -cy
    return (PO.stokes_pictures(COUNT, IH, IW, 11), Z, XX, YY, RO.pplane(IW, IH, XX - cx, YY - cy, "crossing") @ shift, cam, PO.intrinsics(IW, IH))


POL_EXACT = ("S", "occlusion", "dolp", "normals", "rays_cam", "Savg", "Navg", "Zavg", "valid")


def run_polarimetric_setup(ctx, g, small):
    stokes, Z, *rest = _pol_scene()
    r = P.polarimetric_setup(g.input(stokes), g.input(Z), *rest, angle_limit=None, outputs=P.POL_OUTPUTS, ctx=ctx, batch=2 if small else 8)
    return dict({k: _host(getattr(r, k)) for k in POL_EXACT + ("angles",)}, percent=r.occluded_percent)


def oracle_polarimetric_setup():
    stokes, Z, XX, YY, _, cam, _ = _pol_scene()
    want = PO.setup(*_pol_scene(), angle_limit=None)
    assert want["not_up"] == 0 and np.isfinite(want["S"]).any()
    return dict({k: want[k] for k in POL_EXACT}, percent=want["occluded_percent"],
                angles=[VO.noise(XX, YY, want["zf"][t], cam[:3, 3]) for t in range(COUNT)])


@functools.lru_cache(maxsize=None)
def _threshold_frames():
    frames = [RO.threshold_frames(H, W, 40 + t) for t in range(COUNT)]
    return np.stack([f[0] for f in frames]), np.stack([f[1] for f in frames])


def run_radiance_threshold(ctx, g, small):
    I, bg = _threshold_frames()
    mask, thr = P.radiance_threshold(g.input(I), g.input(bg), use_vats=True, ctx=ctx, batch=2 if small else 8)
    return {"mask": _host(mask), "thr": _host(thr)}


def oracle_radiance_threshold():
    mask, thr = RO.threshold(*_threshold_frames(), use_vats=True)
    assert 0 < mask.sum() < mask.size
    return {"mask": mask, "thr": thr}


OPS = {
    "sosfiltfilt": (run_sosfiltfilt, oracle_sosfiltfilt),
    "bgimage": (run_bgimage, lambda: {"out": RO.bgimage(_cube(), 3)}),
    "zeromean": (run_zeromean, lambda: {"out": PO.zeromean(_cube())}),
    "clip_cube": (run_clip_cube, oracle_clip_cube),
    "wave_statistics": (run_wave_statistics, oracle_wave_statistics),
    "visibility_map": (run_visibility_map, oracle_visibility_map),
    "radiance": (run_radiance, oracle_radiance),
    "pyr_up": (run_pyr_up, lambda: {"out": PYO.pyr_up(_cube(9), 1)}),
    "polarimetric_setup": (run_polarimetric_setup, oracle_polarimetric_setup),
    "radiance_threshold": (run_radiance_threshold, oracle_radiance_threshold),
}


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, what
    assert np.array_equal(got, want, equal_nan=got.dtype.kind == "f"), f"{what}: {int((~np.isclose(got, want, rtol=0, atol=0, equal_nan=True)).sum())} values differ"


@pytest.mark.parametrize("name", list(OPS))
def test_staging(gpu_ctx, name):
    run, oracle = OPS[name]
    results = {}
    for dev in (False, True):
        for small in (False, True):
            g = Guarded(dev)
            results[dev, small] = run(gpu_ctx, g, small)
            g.check(f"{name}, {'device' if dev else 'host'}, {'small' if small else 'default'} slab or batch")
    base = results[False, False]
    for (dev, small), r in results.items():
        for k in base:
            _same(r[k], base[k], f"{name}: {k}, {'device' if dev else 'host'} with the {'small' if small else 'default'} slab or batch, against the host's default")
    want = oracle()
    assert set(want) == set(base)
    for k in base:
        if k != "angles":
            _same(base[k], want[k], f"{name}: {k} against the oracle")
            continue
        for t, (a64, n) in enumerate(want[k]):
            nan = np.isnan(a64)
            assert np.array_equal(np.isnan(base[k][t]), nan)
            ratio = np.abs(base[k][t].astype(np.float64) - a64)[~nan] / VO.angle_bound(a64, n)[~nan]
            print(f"{name}: frame {t}: largest angle error / bound = {ratio.max():.4f}")
            assert ratio.max() <= 1.0
