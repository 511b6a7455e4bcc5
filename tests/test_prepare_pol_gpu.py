"""wass_amd.prepare.polarimetric_prepare on the GPU against the staged numpy oracle of tests/prepare_pol_oracle.py (which
test_prepare_pol.py ties to oracle.undistort and to the definitions).  Nothing of the reference is read here.

S0, S1, S2, the four channel pictures, the plain stereo picture, the DOLP index and all ranges are exact: array_equal.  The HDR picture and
the AOLP index hold one transcendental function each: their float32 values before rounding lie within half a float32 ulp plus four times
the oracle's own float32-against-fp64 difference of the oracle evaluated in fp64, and the u8 pictures are equal wherever the fp64 value is
farther than that from a rounding boundary (at most 1 % of the pixels are nearer; there they differ by at most 1).
Every test prints its figures before it asserts."""
import functools

import numpy as np
import pytest

import polarimetric_oracle as PO
import prepare_pol_oracle as PP
import radiance_oracle as RO
import visibility_oracle as VO
from wass_amd import postproc as P
from wass_amd import prepare as W

pytestmark = pytest.mark.gpu

SHAPES = [(2, 2), (3, 5), (64, 48), (70, 50), (131, 67), (258, 10)]                # cols x rows of the mosaic
EVERY = W.PREP_OUTPUTS


@functools.lru_cache(maxsize=None)
def _case(cols, rows, dist, hdr=False, seed=5):
    """a mosaic, its camera and the oracle's results, computed once and not changed by any test"""
    mosaic = PP.random_mosaic(rows, cols, seed)
    K = PP.camera(cols // 2 * 2, rows // 2 * 2)
    want = PP.prepare(mosaic, K, PP.DIST[dist], hdr=hdr)
    for a in [mosaic, K] + [v for v in want.values() if isinstance(v, np.ndarray)]:
        a.setflags(write=False)
    return mosaic, K, PP.DIST[dist], want


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a)).to("cuda:0")


def _ranges(frame):
    return np.array([v for name in W.RANGE_NAMES for v in frame.ranges[name]], np.float32)


def _check_exact(got, want, what):
    for field in ("S", "channels", "dolp"):
        g = np.asarray(getattr(got, field))
        assert g.shape == want[field].shape and g.dtype == want[field].dtype
        bad = int((~((g == want[field]) | ((g != g) & (want[field] != want[field])))).sum())
        print(f"{what}: {field} differs in {bad} of {g.size}")
        assert bad == 0
    r = _ranges(got)
    print(f"{what}: ranges {r} (oracle {want['ranges']})")
    assert np.array_equal(r, want["ranges"], equal_nan=True)


def _check_transcendental(g32, g8, want, key, what):
    o32, o64 = want[key + "_f32"], want[key + "_f64"]
    bound, n = PP.transcendental_bound(o32, o64)
    ok = np.isfinite(o64)
    assert np.array_equal(np.isnan(g32), np.isnan(o64)), f"{what}: NaN pattern"
    err = np.abs(g32.astype(np.float64) - o64)
    worst = float(np.max(err[ok] / bound[ok])) if ok.any() else 0.0
    near = PP.near_boundary(o64, bound)
    ref8 = PP.sat_u8(o64)
    d8 = np.abs(g8.astype(np.int32) - ref8.astype(np.int32))
    print(f"{what}: oracle float32 against fp64 {n:.3e}; largest error / bound = {worst:.4f} (largest error {np.max(err[ok]) if ok.any() else 0:.3e}); "
          f"pixels near a boundary {near.mean() * 100:.3f} %; u8 differences there {int((d8[near] > 0).sum())}, elsewhere {int((d8[~near] > 0).sum())}")
    assert worst <= 1.0
    assert near.mean() <= 0.01
    assert np.all(d8[~near] == 0)
    assert np.all(d8 <= 1)


@pytest.mark.parametrize("dist", ["zero", "calibdir", "barrel", "eight", "pincushion"])     # the last reads outside along every edge
@pytest.mark.parametrize("cols,rows", SHAPES)
def test_exact_outputs(gpu_ctx, cols, rows, dist):
    mosaic, K, d, want = _case(cols, rows, dist)
    got = W.polarimetric_prepare(mosaic, K, d, outputs=EVERY, ctx=gpu_ctx)
    what = f"{cols} x {rows} {dist}"
    assert got.image.shape == (rows // 2 * 2, cols // 2 * 2) and got.image.dtype == np.uint8
    _check_exact(got, want, what)
    print(f"{what}: image differs in {int((got.image != want['image']).sum())}; pixels that read outside: {int((want['S'][0] == 0).sum())}")
    assert np.array_equal(got.image, want["image"])
    assert np.array_equal(got.image_f32, want["image_f32"], equal_nan=True)              # S0 * 127.0f: no transcendental function
    _check_transcendental(got.aolp_f32, got.aolp, want, "aolp", what + " aolp")


@pytest.mark.parametrize("dist", ["zero", "calibdir", "barrel", "eight"])
@pytest.mark.parametrize("cols,rows", [(3, 5), (64, 48), (131, 67)])
def test_hdr(gpu_ctx, cols, rows, dist):
    mosaic, K, d, want = _case(cols, rows, dist, True)
    got = W.polarimetric_prepare(mosaic, K, d, hdr=True, outputs=EVERY, ctx=gpu_ctx)
    what = f"{cols} x {rows} {dist} hdr"
    _check_exact(got, want, what)                                                       # everything else is as without HDR
    _check_transcendental(got.image_f32, got.image, want, "image", what)
    # the plain picture is not the HDR picture: the check can fail
    plain = _case(cols, rows, dist)[3]["image"]
    assert cols < 8 or int((plain != got.image).sum()) > got.image.size // 4


def test_device_entry_equals_host_entry_and_repeats(gpu_ctx):
    import torch
    for cols, rows, dist, hdr in ((131, 67, "calibdir", False), (70, 50, "barrel", True), (3, 5, "eight", False)):
        mosaic, K, d, want = _case(cols, rows, dist, hdr)
        host = W.polarimetric_prepare(mosaic, K, d, hdr=hdr, outputs=EVERY, ctx=gpu_ctx)
        runs = [W.polarimetric_prepare(_dev(mosaic), K, d, hdr=hdr, outputs=EVERY, ctx=gpu_ctx) for _ in range(3)]
        for field in ("image", "S", "dolp", "aolp", "channels", "image_f32", "aolp_f32"):
            h = getattr(host, field)
            for r in runs:
                g = getattr(r, field)
                assert isinstance(g, torch.Tensor) and g.is_cuda
                assert np.array_equal(g.cpu().numpy(), h, equal_nan=h.dtype == np.float32), (field, cols, rows)
        for r in runs:
            assert np.array_equal(_ranges(r), _ranges(host), equal_nan=True)
        # a strided device mosaic (a window of a larger picture) is read in place
        big = torch.zeros((rows + 3, cols + 9), dtype=torch.uint8, device="cuda:0")
        big[1:rows + 1, 4:cols + 4] = _dev(mosaic)
        win = W.polarimetric_prepare(big[1:rows + 1, 4:cols + 4], K, d, hdr=hdr, outputs=("stokes",), ctx=gpu_ctx)
        assert np.array_equal(win.S.cpu().numpy(), host.S, equal_nan=True) and np.array_equal(win.image.cpu().numpy(), host.image)


def test_only_what_was_asked_for(gpu_ctx):
    mosaic, K, d, want = _case(70, 50, "calibdir")
    full = W.polarimetric_prepare(mosaic, K, d, outputs=EVERY, ctx=gpu_ctx)
    fields = {"stokes": "S", "dolp": "dolp", "aolp": "aolp", "channels": "channels", "image_f32": "image_f32", "aolp_f32": "aolp_f32"}
    for asked in ((), ("stokes",), ("dolp",), ("aolp", "channels"), ("aolp_f32",), ("image_f32", "stokes")):
        for src in (mosaic, _dev(mosaic)):
            got = W.polarimetric_prepare(src, K, d, outputs=asked, ctx=gpu_ctx)
            host = lambda a: a if isinstance(a, np.ndarray) else a.cpu().numpy()
            assert np.array_equal(host(got.image), full.image)
            for name, field in fields.items():
                a = getattr(got, field)
                if name in asked:
                    assert np.array_equal(host(a), getattr(full, field), equal_nan=True), (asked, field)
                else:
                    assert a is None, (asked, field)
            r, rf = _ranges(got), _ranges(full)
            assert np.array_equal(r[:6], rf[:6])
            assert np.array_equal(r[6:], rf[6:]) if "dolp" in asked else np.all(np.isnan(r[6:]))


def test_second_camera_after_the_first(gpu_ctx):
    """The per-camera table cache: another K, another size and the first camera again."""
    mosaic, K, d, want = _case(64, 48, "calibdir")
    K2 = np.array(K)
    K2[0, 0] *= 1.07
    K2[0, 2] += 2.75
    K2[1, 2] -= 1.5
    want2 = PP.prepare(mosaic, K2, d)
    assert not np.array_equal(want2["S"], want["S"])
    m3, K3, d3, want3 = _case(70, 50, "eight")
    for k, (mo, Kk, dd, wa) in enumerate(((mosaic, K, d, want), (mosaic, K2, d, want2), (m3, K3, d3, want3), (mosaic, K, d, want), (mosaic, K2, d, want2))):
        got = W.polarimetric_prepare(mo, Kk, dd, outputs=("stokes",), ctx=gpu_ctx)
        assert np.array_equal(got.S, wa["S"], equal_nan=True), f"call {k}"
        assert np.array_equal(got.image, wa["image"]), f"call {k}"
    # the byte picture of the same camera goes through the same tables
    plain = gpu_ctx.undistort(np.ascontiguousarray(mosaic), K2, d)
    assert plain.shape == mosaic.shape


@pytest.mark.parametrize("cols,rows,clip,tiles", [(64, 48, 2.0, 4), (131, 67, 3.5, 5)])
def test_clahe(gpu_ctx, cols, rows, clip, tiles):
    mosaic, K, d, want = _case(cols, rows, "calibdir")
    plain = W.polarimetric_prepare(mosaic, K, d, outputs=("stokes", "image_f32"), ctx=gpu_ctx)
    ref = gpu_ctx.clahe(plain.image, clip, tiles)
    assert int((ref != plain.image).sum()) > plain.image.size // 4
    for src in (mosaic, _dev(mosaic)):
        got = W.polarimetric_prepare(src, K, d, outputs=("stokes", "image_f32"), clahe=(clip, tiles), ctx=gpu_ctx)
        host = lambda a: a if isinstance(a, np.ndarray) else a.cpu().numpy()
        assert np.array_equal(host(got.image), ref)
        assert np.array_equal(host(got.S), plain.S, equal_nan=True) and np.array_equal(host(got.image_f32), plain.image_f32, equal_nan=True)


def test_stokes_pictures_feed_the_polarimetric_setup(gpu_ctx):
    """End to end on the device: frame.S is what remap_linear_f32 and polarimetric_setup take, without conversion."""
    import torch
    mosaic, K, d, want = _case(64, 48, "calibdir")
    frame = W.polarimetric_prepare(_dev(mosaic), K, d, ctx=gpu_ctx)
    Ih, Iw = want["S"].shape[1:]
    assert frame.S.dtype == torch.float32 and tuple(frame.S.shape) == (3, Ih, Iw) and frame.S.is_contiguous()
    mx, my = RO.lattice_maps(9, 11, Ih, Iw, 3)
    for k in range(3):
        got = P.remap_linear_f32(frame.S[k], _dev(mx), _dev(my), ctx=gpu_ctx)
        assert np.array_equal(got.cpu().numpy(), PO.remap_linear_f32(want["S"][k], mx, my), equal_nan=True)
    H = Wg = 8
    XX, YY = VO.make_grid(H, Wg, 0.5)
    cam = VO.camera(XX, YY, "over", 9.0, 0.0)
    Z = VO.make_sea(H, Wg, 0.5, 15, 2.0, t=0.0)[None]
    cx, cy = XX.mean(), YY.mean()
    shift = np.eye(4)
    shift[0, 3], shift[1, 3] = -cx, -cy
    Pplane = RO.pplane(Iw, Ih, XX - cx, YY - cy, "inside") @ shift
    Kc = PO.intrinsics(Iw, Ih)
    res = P.polarimetric_setup(frame.S[None], _dev(Z), XX, YY, Pplane, cam, Kc, outputs=("S", "dolp"), ctx=gpu_ctx)
    ref = PO.setup(want["S"][None], Z, XX, YY, Pplane, cam, Kc)
    assert np.array_equal(res.S.cpu().numpy(), ref["S"], equal_nan=True)
    assert np.array_equal(res.dolp.cpu().numpy(), ref["dolp"], equal_nan=True)
    assert np.array_equal(res.Savg.cpu().numpy(), ref["Savg"], equal_nan=True)
    assert np.isfinite(ref["S"]).sum() > ref["S"].size // 2


def test_files_round_trip(gpu_ctx, tmp_path):
    mosaic, K, d, want = _case(70, 50, "calibdir")
    for src in (mosaic, _dev(mosaic)):
        frame = W.polarimetric_prepare(src, K, d, outputs=("stokes", "channels"), ctx=gpu_ctx)
        out = tmp_path / ("dev" if src is not mosaic else "host")
        written = W.write_polarimetric_outputs(out, "00000000", frame)
        assert len(written) == 8
        for k in range(3):
            back = W.read_tiff_f32(out / f"00000000_S{k}.tiff")
            assert np.array_equal(back.view(np.uint32), want["S"][k].view(np.uint32))


def test_argument_errors(gpu_ctx):
    import ctypes as C
    from wass_amd import _lib
    INVALID = -1
    mosaic, K, d, want = _case(64, 48, "calibdir")
    codes = {}
    for what, kw in (("one row", dict(image=mosaic[:1])), ("one column", dict(image=mosaic[:, :1])), ("three coefficients", dict(dist=d[:3])),
                     ("fourteen coefficients", dict(dist=np.zeros(14))), ("skew", dict(K=K + np.array([[0, 0.5, 0], [0, 0, 0], [0, 0, 0]]))),
                     ("singular K", dict(K=np.zeros((3, 3)))), ("too wide", dict(image=np.zeros((2, 32770), np.uint8)))):
        args = dict(image=mosaic, K=K, dist=d)
        args.update(kw)
        with pytest.raises(_lib.WassError) as e:
            W.polarimetric_prepare(args["image"], args["K"], args["dist"], ctx=gpu_ctx)
        codes[what] = e.value.code
        print(f"{what}: {e.value}")
    und = {}
    for what, kw in (("three coefficients", dict(dist=d[:3])), ("skew", dict(K=K + np.array([[0, 0.5, 0], [0, 0, 0], [0, 0, 0]]))),
                     ("too wide", dict(src=np.zeros((2, 32770), np.uint8)))):
        args = dict(src=mosaic, K=K, dist=d)
        args.update(kw)
        with pytest.raises(_lib.WassError) as e:
            gpu_ctx.undistort(args["src"], args["K"], args["dist"])
        und[what] = e.value.code
    assert codes["one row"] == codes["one column"] == codes["singular K"] == INVALID
    for what, code in und.items():                      # the codes of wass_undistort
        assert codes[what] == code, what
    assert codes["fourteen coefficients"] == codes["three coefficients"]
    # the C entry itself: null pointers, unknown bits, a missing destination
    lib = gpu_ctx._lib
    Kc = (C.c_double * 9)(*K.ravel())
    dc = (C.c_double * 5)(*d)
    img = np.zeros((48, 64), np.uint8)
    p, o = _lib.PolPrepParams(0, 0, 0.0, 0, 0), _lib.PolPrepOut()
    o.image = img.ctypes.data
    call = lambda **kw: lib.wass_prepare_pol(kw.get("ctx", gpu_ctx._h), kw.get("src", mosaic.ctypes.data), 64, 48, kw.get("stride", 64), kw.get("K", Kc),
                                             dc, 5, C.byref(kw.get("p", p)), C.byref(kw.get("o", o)))
    assert call() == 0
    assert call(ctx=None) == INVALID and call(src=None) == INVALID and call(K=None) == INVALID and call(stride=63) == INVALID
    assert call(p=_lib.PolPrepParams(0, 64, 0.0, 0, 0)) == INVALID
    assert call(p=_lib.PolPrepParams(0, 1, 0.0, 0, 0)) == INVALID                      # stokes wanted, no destination
    assert call(p=_lib.PolPrepParams(0, 0, 2.0, -1, 0)) == INVALID
    assert call(o=_lib.PolPrepOut()) == INVALID
    # and the context still works
    got = W.polarimetric_prepare(mosaic, K, d, ctx=gpu_ctx)
    assert np.array_equal(got.S, want["S"], equal_nan=True)
