"""wass_amd.postproc.pyr_up and radiance_upscaled on the GPU against the numpy restatement of tests/pyramid_oracle.py (which
tests/test_pyramid.py holds to the weight matrices and scipy).  Every comparison is np.array_equal, NaN cells equal to NaN cells:
nothing here has a tolerance.  k_pyrup works in blocks of 64 x 4 SOURCE cells (PYR_BX x PYR_BY in pyramid.hip), one lane per source
cell, and stores each pair of destination cells as one vector where the destination is aligned for it: the shapes below sit on
both sides of 64 and 128 columns and of 4 and 8 rows, and the windows start at even and at odd columns.  Every test prints its
figures before it asserts."""
import numpy as np
import pytest

import pyramid_oracle as PO
import radiance_oracle as RO
from wass_amd import postproc as P

pytestmark = pytest.mark.gpu
F = np.float32
DTYPES = [np.float32, np.float64]
# the shapes the issue names, then one either side of every block edge: 63 | 64 | 65 and 127 | 128 | 129 columns, 3 | 4 | 5 and 7 | 8 | 9 rows
SHAPES = [(2, 2), (2, 3), (3, 2), (5, 7), (17, 33), (64, 65), (130, 257), (3, 63), (4, 64), (5, 65), (7, 127), (8, 128), (9, 129)]


def _torch():
    import torch
    return torch


def _host(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def _same(got, want, what):
    got = _host(got)
    bad = int((~((got == want) | (np.isnan(got) & np.isnan(want)))).sum()) if got.shape == want.shape else -1
    print(f"{what}: {bad} of {want.size} differ")
    assert got.dtype == want.dtype and got.shape == want.shape and bad == 0, what


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("h,w", SHAPES)
def test_single_pictures(gpu_ctx, h, w, dtype):
    src = PO.picture(h, w, dtype, seed=1)
    for levels in (1, 2):
        want = PO.pyr_up(src, levels)
        got = P.pyr_up(src, levels, ctx=gpu_ctx)
        assert isinstance(got, np.ndarray)
        _same(got, want, f"{h} x {w} {np.dtype(dtype).name}, {levels} level(s), host")
        dev = P.pyr_up(_torch().from_numpy(src).cuda(), levels, ctx=gpu_ctx)
        assert dev.is_cuda
        _same(dev, want, f"{h} x {w} {np.dtype(dtype).name}, {levels} level(s), device")


@pytest.mark.parametrize("dtype", DTYPES)
def test_cubes_and_batches(gpu_ctx, dtype):
    """1, 3 and 11 frames: frames go 8 at a time, so 11 leaves a ragged launch of 3"""
    h, w = 17, 33
    cube = np.stack([PO.picture(h, w, dtype, seed=10 + t) for t in range(11)])
    assert P.pyr_up_scratch_bytes(11, h, w, 2, dtype)[1] == 8
    for count in (1, 3, 11):
        for levels in (1, 2):
            want = PO.pyr_up(cube[:count], levels)
            _same(P.pyr_up(cube[:count], levels, ctx=gpu_ctx), want, f"{count} frames, {levels} level(s), host")
            _same(P.pyr_up(_torch().from_numpy(cube[:count]).cuda(), levels, ctx=gpu_ctx), want, f"{count} frames, {levels} level(s), device")
    want = PO.pyr_up(cube[:2], 4)
    _same(P.pyr_up(cube[:2], 4, ctx=gpu_ctx), want, "2 frames, 4 levels, host")
    _same(P.pyr_up(_torch().from_numpy(cube[:2]).cuda(), 3, ctx=gpu_ctx), PO.pyr_up(cube[:2], 3), "2 frames, 3 levels, device")


def test_calling_forms_and_repeats(gpu_ctx, tmp_path):
    torch = _torch()
    cube = np.stack([PO.picture(64, 65, F, seed=20 + t) for t in range(3)])
    want = PO.pyr_up(cube, 2)
    mm = np.memmap(tmp_path / "cube.bin", np.float32, "w+", shape=cube.shape)
    mm[:] = cube
    dcube = torch.from_numpy(cube).cuda()
    first = None
    for rep in range(3):
        res = [P.pyr_up(cube, 2, ctx=gpu_ctx), P.pyr_up(mm, 2, ctx=gpu_ctx), _host(P.pyr_up(dcube, 2, ctx=gpu_ctx))]
        first = res[0] if first is None else first
        for name, r in zip(("host", "memmap", "device"), res):
            _same(r, want, f"repeat {rep}, {name}")
            assert r.tobytes() == first.tobytes()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ox", [2, 3])
def test_strided_views(gpu_ctx, dtype, ox):
    """a window cut out of a larger cube, into a window of a larger buffer; ox = 3 puts the pairs of the result on odd columns, where
    the kernel stores cell by cell"""
    torch = _torch()
    n, h, w = 3, 9, 65
    rng = np.random.default_rng(4)
    big = rng.standard_normal((n, h + 5, w + 9)).astype(dtype)
    win = big[:, 2:2 + h, ox + 2:ox + 2 + w]
    for levels in (1, 2):
        want = PO.pyr_up(np.ascontiguousarray(win), levels)
        H2, W2 = h << levels, w << levels
        for side in ("host", "device"):
            buf = np.full((n, H2 + 3, W2 + 8), dtype(-5))     # even strides: only the window's column decides the alignment
            if side == "host":
                o = buf[:, 1:1 + H2, ox:ox + W2]
                assert P.pyr_up(win, levels, ctx=gpu_ctx, out=o) is o
            else:
                dbuf = torch.from_numpy(buf).cuda()
                dbig = torch.from_numpy(big).cuda()
                P.pyr_up(dbig[:, 2:2 + h, ox + 2:ox + 2 + w], levels, ctx=gpu_ctx, out=dbuf[:, 1:1 + H2, ox:ox + W2])
                buf = dbuf.cpu().numpy()
            _same(buf[:, 1:1 + H2, ox:ox + W2], want, f"window at column {ox}, {levels} level(s), {side}")
            frame = np.ones(buf.shape, bool)
            frame[:, 1:1 + H2, ox:ox + W2] = False
            print(f"around the window: {int((buf[frame] != dtype(-5)).sum())} cells touched")
            assert (buf[frame] == dtype(-5)).all()
    # a single picture out of a larger one, into a window
    o = np.zeros((2 * h + 2, 2 * w + 2), dtype)
    P.pyr_up(big[1, 2:2 + h, 3:3 + w], ctx=gpu_ctx, out=o[1:-1, 1:-1])
    _same(o[1:-1, 1:-1], PO.pyr_up(np.ascontiguousarray(big[1, 2:2 + h, 3:3 + w])), "single picture, windows")
    assert (o[0] == 0).all() and (o[-1] == 0).all() and (o[:, 0] == 0).all() and (o[:, -1] == 0).all()


def test_out_over_the_input_is_refused(gpu_ctx):
    torch = _torch()
    buf = np.zeros((16, 10), F)
    with pytest.raises(ValueError):
        P.pyr_up(buf[:4, :5], ctx=gpu_ctx, out=buf[:8])
    d = torch.zeros((16, 10), dtype=torch.float32, device="cuda")
    with pytest.raises(ValueError):
        P.pyr_up(d[:4, :5], ctx=gpu_ctx, out=d[:8])
    with pytest.raises(ValueError):
        P.pyr_up(d[:4, :5], ctx=gpu_ctx, out=np.zeros((8, 10), F))              # the other side
    # the C entry refuses the same pointer on both sides
    assert gpu_ctx._lib.wass_pyrup_f32_dev(gpu_ctx._h, d.data_ptr(), 50, 10, 1, 4, 5, 1, d.data_ptr(), 80, 10) == -1


@pytest.mark.parametrize("dtype", DTYPES)
def test_nan_and_infinity(gpu_ctx, dtype):
    h, w = 17, 66
    cube = np.stack([PO.picture(h, w, dtype, seed=30 + t) for t in range(4)])
    cube[0, 0, 0] = np.nan
    cube[0, 16, 65] = np.nan
    cube[0, 8, 63] = np.inf
    cube[0, 8, 64] = -np.inf                            # next to +inf: their sums are NaN
    cube[0, 3, 20] = -np.inf
    cube[0, 12, 0] = np.inf
    cube[2] = np.nan                                    # a frame of NaN among finite ones
    for levels in (1, 2):
        want = PO.pyr_up(cube, levels)
        print(f"{levels} level(s): frame 0 has {int(np.isnan(want[0]).sum())} NaN and {int(np.isinf(want[0]).sum())} infinite cells")
        assert np.isnan(want[0]).sum() > 20 and np.isinf(want[0]).sum() > 20 and np.isnan(want[2]).all()
        assert np.isfinite(want[1]).all() and np.isfinite(want[3]).all()
        _same(P.pyr_up(cube, levels, ctx=gpu_ctx), want, f"NaN and infinities, {levels} level(s), host")
        _same(P.pyr_up(_torch().from_numpy(cube).cuda(), levels, ctx=gpu_ctx), want, f"NaN and infinities, {levels} level(s), device")


# ---- radiance on the finer grid ----------------------------------------------------------------------------------------------------
def _scene(H, W, Ih, Iw, n, kind, seed):
    XX, YY = RO.grid(H, W)
    Z = RO.heights(n, H, W, seed)
    if H * W > 4:
        Z[0, H // 2, W // 3] = np.nan
        Z[n - 1, :2, :] = np.nan
    imgs = np.stack([RO.picture(Ih, Iw, seed + 1 + t) for t in range(n)])
    return XX, YY, Z, imgs, RO.pplane(Iw, Ih, XX, YY, kind)


@pytest.mark.parametrize("up", [2, 3])
@pytest.mark.parametrize("H,W,Ih,Iw,kind", [(2, 2, 8, 9, "inside"), (9, 13, 40, 56, "crossing"), (9, 13, 8, 9, "inside"), (64, 65, 40, 56, "crossing"),
                                            (64, 65, 40, 56, "outside")])
def test_radiance_upscaled(gpu_ctx, H, W, Ih, Iw, kind, up):
    torch = _torch()
    n = 3
    XX, YY, Z, imgs, Pp = _scene(H, W, Ih, Iw, n, kind, 70 + H)
    want = PO.radiance_upscaled(imgs, Z, XX, YY, Pp, up)
    s = 1 << (up - 1)
    zero = float((want == 0).mean())
    print(f"{H} x {W} from {Ih} x {Iw}, {kind}, upscalefactor {up}: {want.shape}, {100 * zero:.1f} % of the cells are 0")
    assert want.shape == (n, s * H, s * W)
    if kind == "outside":
        assert zero == 1.0
    elif kind == "crossing":
        assert 0.02 < zero < 0.9                         # some cells project outside the picture, most do not
    got = P.radiance_upscaled(imgs, Z, XX, YY, Pp, up, ctx=gpu_ctx)
    assert isinstance(got, np.ndarray)
    _same(got, want, "host, batch 8")
    _same(P.radiance_upscaled(imgs, Z, XX, YY, Pp, up, ctx=gpu_ctx, batch=2), want, "host, batch 2")
    dev = P.radiance_upscaled(torch.from_numpy(imgs).cuda(), torch.from_numpy(Z).cuda(), XX, YY, Pp, up, ctx=gpu_ctx, batch=2)
    assert dev.is_cuda
    _same(dev, want, "device, batch 2")
    _same(P.radiance_upscaled(imgs, torch.from_numpy(Z).cuda(), XX, YY, Pp, upscalefactor=up, ctx=gpu_ctx), want, "host pictures, device cube")
    if kind != "outside" and H * W > 4:
        # the upsampling matters: the radiance of the coarse grid, repeated, is something else
        coarse = np.repeat(np.repeat(RO.radiance(imgs, Z, XX, YY, Pp), s, axis=1), s, axis=2)
        assert (coarse != want).mean() > 0.2


def test_radiance_upscaled_forms(gpu_ctx):
    torch = _torch()
    H, W, n = 9, 13, 5
    XX, YY, Z, imgs, Pp = _scene(H, W, 40, 56, n, "crossing", 90)
    frames = [RO.picture(40, 56, 91), RO.picture(40, 56, 92), RO.picture(8, 9, 93), RO.picture(8, 9, 94), RO.picture(40, 56, 95)]
    want = PO.radiance_upscaled(frames, Z, XX, YY, Pp, 2)
    _same(P.radiance_upscaled(iter(frames), Z, XX, YY, Pp, 2, ctx=gpu_ctx), want, "an iterable whose pictures change size, host")
    _same(P.radiance_upscaled(iter(frames), torch.from_numpy(Z).cuda(), XX, YY, Pp, 2, ctx=gpu_ctx, batch=2), want,
          "an iterable whose pictures change size, device")
    # a strided view of the heights, and out
    big = np.full((n, H + 3, W + 5), F(7))
    big[:, 1:1 + H, 2:2 + W] = Z
    out = np.empty((n, 2 * H, 2 * W), F)
    want = PO.radiance_upscaled(imgs, Z, XX, YY, Pp, 2)
    assert P.radiance_upscaled(imgs, big[:, 1:1 + H, 2:2 + W], XX, YY, Pp, ctx=gpu_ctx, out=out, batch=3) is out
    _same(out, want, "strided view, out")
    _same(P.radiance_upscaled(imgs, Z * F(0.5), XX, YY, Pp, 2, datascale=2e-3, ctx=gpu_ctx),
          PO.radiance_upscaled(imgs, Z * F(0.5), XX, YY, Pp, 2, datascale=2e-3), "datascale 2e-3")
    # upscalefactor 1 is radiance, bit for bit
    plain = P.radiance(imgs, Z, XX, YY, Pp, ctx=gpu_ctx)
    _same(P.radiance_upscaled(imgs, Z, XX, YY, Pp, upscalefactor=1, ctx=gpu_ctx), plain, "upscalefactor 1, host")
    _same(plain, RO.radiance(imgs, Z, XX, YY, Pp), "radiance itself")
    _same(P.radiance_upscaled(torch.from_numpy(imgs).cuda(), torch.from_numpy(Z).cuda(), XX, YY, Pp, upscalefactor=1, ctx=gpu_ctx), plain,
          "upscalefactor 1, device")
    with pytest.raises(ValueError):
        P.radiance_upscaled(imgs, Z, XX, YY, Pp, 2, ctx=gpu_ctx, out=np.empty((n, H, W), F))
    with pytest.raises(ValueError):
        P.radiance_upscaled(iter(frames[:3]), Z, XX, YY, Pp, 2, ctx=gpu_ctx)


# ---- the C entries' argument errors ------------------------------------------------------------------------------------------------
def test_abi_argument_errors(gpu_ctx):
    lib, h = gpu_ctx._lib, gpu_ctx._h
    INVALID = -1                                        # WASS_ERR_INVALID_ARG
    a32, o32 = np.zeros((4, 5), F), np.zeros((16, 20), F)
    a64, o64 = np.zeros((4, 5), np.float64), np.zeros((16, 20), np.float64)
    for fn, a, o in ((lib.wass_pyrup_f32, a32, o32), (lib.wass_pyrup_f64, a64, o64)):
        p, q = a.ctypes.data, o.ctypes.data
        assert fn(h, p, 20, 5, 1, 4, 5, 1, q, 80, 10) == 0
        cases = {"null in": (None, 20, 5, 1, 4, 5, 1, q, 80, 10), "null out": (p, 20, 5, 1, 4, 5, 1, None, 80, 10),
                 "H of 1": (p, 20, 5, 1, 1, 5, 1, q, 80, 10), "W of 1": (p, 20, 5, 1, 4, 1, 1, q, 80, 10),
                 "levels 0": (p, 20, 5, 1, 4, 5, 0, q, 80, 10), "levels 5": (p, 20, 5, 1, 4, 5, 5, q, 80, 10),
                 "input row stride below W": (p, 20, 4, 1, 4, 5, 1, q, 80, 10), "output row stride below 2 W": (p, 20, 5, 1, 4, 5, 1, q, 80, 9),
                 "input frame stride below W": (p, 4, 5, 2, 2, 5, 1, q, 40, 10), "output frames overlap": (p, 10, 5, 2, 2, 5, 1, q, 39, 10),
                 "no frames": (p, 20, 5, 0, 4, 5, 1, q, 80, 10)}
        for name, args in cases.items():
            rc = fn(h, *args)
            print(f"{fn.__name__}, {name}: {rc}")
            assert rc == INVALID, name
    assert lib.wass_pyrup_f32(None, a32.ctypes.data, 20, 5, 1, 4, 5, 1, o32.ctypes.data, 80, 10) == INVALID
    Z, XX, YY = np.zeros((1, 4, 5), F), np.zeros((4, 5)), np.zeros((4, 5))
    img, Pc, out = np.zeros((1, 8, 9), np.uint8), np.ascontiguousarray(np.eye(4)[:3]), np.zeros((1, 8, 10), F)

    def up(**kw):
        a = dict(img=img.ctypes.data, it=72, iy=9, Ih=8, Iw=9, z=Z.ctypes.data, st=20, sy=5, n=1, H=4, W=5, XX=XX.ctypes.data, YY=YY.ctypes.data,
                 P=Pc.ctypes.data, scale=1e-3, batch=0, levels=1, out=out.ctypes.data)
        a.update(kw)
        return lib.wass_radiance_up(h, *a.values())

    assert up() == 0
    for name, kw in {"null heights": dict(z=None), "null grid": dict(YY=None), "null out": dict(out=None), "H of 1": dict(H=1), "W of 1": dict(W=1),
                     "levels 0": dict(levels=0), "levels 5": dict(levels=5), "row stride below W": dict(sy=4), "picture stride below Iw": dict(iy=8)}.items():
        rc = up(**kw)
        print(f"wass_radiance_up, {name}: {rc}")
        assert rc == INVALID, name
