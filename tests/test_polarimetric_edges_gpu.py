"""The polarimetric set-up, clip_cube and zeromean on the GPU at the shapes, strides and values that tests/test_polarimetric_gpu.py
leaves unexecuted: the unrolled blocks of k_zeromean, every stride but the contiguous one, the second launch of clip_cube and its
record across launches, the edges of the ordered-key reduction, pictures with a side of 1 or 2, grids from 2 x 2 up to one ragged
column beyond a block, the iterable form's flush on a change of picture size, and `batch` with a ragged last launch.

Everything is exact against the numpy oracles (array_equal with the NaN pattern equal) but the angles, which keep
visibility_oracle.angle_bound.  The small seas are chosen so that no cell's angle lies within that bound of 85 degrees: the mask with
the rule and occluded_percent are exact too.  A strided call must give the bytes of the contiguous call, must leave every cell
outside its views alone, and must have handed the library the view itself (the library's arguments are recorded): a silent copy
would make these tests vacuous.  Not reached by any GPU test: the host slab path of zeromean (rows < H) and the batch halving of
the plan, which trigger only near the 16 GiB scratch cap (test_scratch_arithmetic has the plan's arithmetic).
Nothing of the reference is read here.  Every test prints its figures before it asserts."""
import functools

import numpy as np
import pytest

import polarimetric_oracle as PO
import radiance_oracle as RO
import visibility_oracle as VO
from test_polarimetric_gpu import AVERAGES, PER_FRAME, _variants
from wass_amd import postproc as P

pytestmark = pytest.mark.gpu

F = np.float32
FLT_MAX = np.finfo(F).max
SENTINEL = F(3e33)                                                               # outside every clip bound used with it


def _diff(a, b):
    return int((~np.isclose(np.asarray(a), np.asarray(b), rtol=0, atol=0, equal_nan=True)).sum())


def _exact(got, want, what):
    """prints the count of differing cells, then: dtype, shape, NaN pattern, values and the sign of every zero"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, what
    print(f"{what}: {_diff(got, want)} of {want.size} cells differ, {int(np.isnan(want).sum()) if want.dtype.kind == 'f' else 0} are NaN")
    if want.dtype.kind == "f":
        assert np.array_equal(np.isnan(got), np.isnan(want)), what + ": NaN pattern"
        assert np.array_equal(got, want, equal_nan=True), what
        assert np.array_equal(np.signbit(got)[~np.isnan(want)], np.signbit(want)[~np.isnan(want)]), what + ": signs"
    else:
        assert np.array_equal(got, want), what


def _host(a):
    return a.cpu().numpy() if hasattr(a, "data_ptr") else np.asarray(a)


class _Spy:
    """stands in for a context's library and records the arguments of every call it forwards"""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        f = getattr(self._lib, name)

        def forward(*args):
            self.calls.append((name, args))
            return f(*args)
        return forward if name.startswith(("wass_polarimetric", "wass_clip_cube", "wass_zeromean")) else f


def _address(a):
    return a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data


def _strides(a, n):
    return tuple(a.stride(k) for k in range(n)) if hasattr(a, "data_ptr") else tuple(s // 4 for s in a.strides[:n])


def _outside_untouched(after, before, inside):
    a, b = _host(after).copy(), _host(before).copy()
    a[inside] = 0
    b[inside] = 0
    return a.tobytes() == b.tobytes()


# ---- zeromean -----------------------------------------------------------------------------------------------------------------------
ZM_COUNTS = (1, 2, 7, 8, 9, 15, 16, 17, 40)                                      # no, one and several unrolled blocks of 8, with and without a tail
ZM_SHAPES = ((1, 1), (3, 5), (5, 257))                                           # 1285 series: five blocks of 256 and 5 lanes of a sixth


@functools.lru_cache(maxsize=None)
def _zm_case(count, H, W):
    x = PO.spread_cube((count, H, W), 100 * count + W)
    if H * W > 1:
        x[count // 2, H - 1, W - 1] = np.nan                                     # the last series is NaN in every frame
    want, backward = PO.zeromean(x), PO.zeromean(x, reverse=True)
    for a in (x, want, backward):
        a.setflags(write=False)
    return x, want, backward


@pytest.mark.parametrize("count", ZM_COUNTS)
def test_zeromean_counts(gpu_ctx, count):
    import torch
    for H, W in ZM_SHAPES:
        x, want, backward = _zm_case(count, H, W)
        what = f"zeromean {count} x {H} x {W}"
        got = P.zeromean(x, ctx=gpu_ctx)
        _exact(got, want, what + " host")
        dx = torch.tensor(x).cuda()
        dgot = P.zeromean(dx, ctx=gpu_ctx)
        assert dgot.is_cuda and dgot.data_ptr() != dx.data_ptr()
        _exact(_host(dgot), want, what + " device")
        assert _host(dx).tobytes() == x.tobytes(), "the input was written"
        assert P.zeromean(dx, out=dx, ctx=gpu_ctx) is dx
        _exact(_host(dx), want, what + " device in place")
        miss = _diff(backward, got)
        print(f"{what}: the sum in reverse frame order misses the GPU result in {miss} of {got.size} cells")
        if count >= 16 and (H, W) == ZM_SHAPES[-1]:
            assert miss > 0


# views of 17 x 5 x 67 in larger arrays with different paddings
VIEW = (17, 5, 67)
IN_BIG, IN_AT = (17, 8, 75), (slice(None), slice(1, 6), slice(3, 70))
OUT_BIG, OUT_AT = (17, 9, 80), (slice(None), slice(2, 7), slice(5, 72))


def _strided_forms(ctx, monkeypatch, x, want, call, entry, out_arg):
    """call(data, out) -> the result cube, which must be `out` where one is given.  The five forms of the strided views; `entry`
    is the library function (its device form has the suffix _dev), whose argument 1 is the input and `out_arg` the output."""
    import torch
    spy = _Spy(ctx._lib)
    monkeypatch.setattr(ctx, "_lib", spy)

    def passed(name, data, out):
        got, args = spy.calls[-1]
        assert got == name
        assert args[1] == _address(data) and tuple(args[2:4]) == _strides(data, 2), "the input went through a copy"
        if out is not None:
            assert args[out_arg] == _address(out) and tuple(args[out_arg + 1:out_arg + 3]) == _strides(out, 2), "the output went through a copy"

    def fresh(shape, at, fill, xp):
        a = np.full(shape, SENTINEL, F)
        if fill is not None:
            a[at] = fill
        return a if xp is np else torch.tensor(a).cuda()

    for xp, name in ((np, entry), (torch, entry + "_dev")):
        side = "host" if xp is np else "device"
        big, obig = fresh(IN_BIG, IN_AT, x, xp), fresh(OUT_BIG, OUT_AT, None, xp)
        before, obefore = _host(big).copy(), _host(obig).copy()
        data, out = big[IN_AT], obig[OUT_AT]
        assert _strides(data, 2) == (8 * 75, 75) and _strides(out, 2) == (9 * 80, 80)
        assert call(data, out) is out
        passed(name, data, out)
        _exact(_host(out), want, f"{entry} {side}, a view into a view")
        assert _host(big).tobytes() == before.tobytes(), "the input's array was written"
        assert _outside_untouched(obig, obefore, OUT_AT), "cells outside the output view were written"
        data = big[IN_AT]
        assert call(data, data) is data                                          # in place on the view
        passed(name, data, data)
        _exact(_host(data), want, f"{entry} {side}, in place on a view")
        assert _outside_untouched(big, before, IN_AT), "cells outside the view were written in place"
    d = torch.full((2 * VIEW[0],) + VIEW[1:], float(SENTINEL), dtype=torch.float32).cuda()
    d[::2] = torch.tensor(x).cuda()
    before = _host(d).copy()
    data = d[::2]
    assert _strides(data, 2) == (2 * VIEW[1] * VIEW[2], VIEW[2])
    got = call(data, None)
    passed(entry + "_dev", data, None)
    _exact(_host(got), want, f"{entry} device, a time stride of 2")
    assert _host(d).tobytes() == before.tobytes()
    assert call(data, data) is data
    passed(entry + "_dev", data, data)
    _exact(_host(data), want, f"{entry} device, in place with a time stride of 2")
    assert np.array_equal(_host(d)[1::2], before[1::2]), "the frames between were written"


def test_zeromean_strided_views(gpu_ctx, monkeypatch):
    x = PO.spread_cube(VIEW, 17)
    x[5, 2, 66] = x[16, 4, 0] = np.nan
    _strided_forms(gpu_ctx, monkeypatch, x, PO.zeromean(x), lambda data, out: P.zeromean(data, out=out, ctx=gpu_ctx), "wass_zeromean", 7)


# ---- clip_cube ----------------------------------------------------------------------------------------------------------------------
def _same_number(got, want):
    return (np.isnan(got) and np.isnan(want)) or got == want


def _clip_both_sides(ctx, x, lo, hi, what):
    """host and device against the oracle: the cube exact, vmin and vmax by == (isnan where the oracle has none)"""
    import torch
    want, vmin, vmax = PO.clip_cube(x, lo, hi)
    for side in ("host", "device"):
        got, gmin, gmax = P.clip_cube(x if side == "host" else torch.tensor(x).cuda(), lo, hi, ctx=ctx)
        assert hasattr(got, "data_ptr") == (side == "device")
        print(f"{what} {side}: range {gmin!r} .. {gmax!r}, oracle {vmin!r} .. {vmax!r}")
        _exact(_host(got), want, f"{what} {side}")
        assert isinstance(gmin, F) and isinstance(gmax, F)
        assert _same_number(gmin, vmin) and _same_number(gmax, vmax), what
    return want, vmin, vmax


def test_clip_cube_second_launch(gpu_ctx):
    """1030 frames: a launch of 1024 and one of 6.  The extremes lie one in each launch, then exchanged: both must be reported,
    which needs the second launch's offsets and the record carried from the first launch to the second."""
    rng = np.random.default_rng(1030)
    x = (rng.standard_normal((1030, 3, 5)) * 40.0).astype(F)
    x[500, 1, 1] = np.nan
    for fmin, fmax in ((1027, 2), (2, 1027)):
        y = x.copy()
        y[fmin, 1, 2], y[fmax, 0, 4] = -5000.0, 7000.0
        _, vmin, vmax = _clip_both_sides(gpu_ctx, y, -6000.0, 8000.0, f"clip 1030 x 3 x 5, minimum in frame {fmin}, maximum in frame {fmax}")
        assert (vmin, vmax) == (F(-5000.0), F(7000.0))
        _, vmin, vmax = _clip_both_sides(gpu_ctx, y, -100.0, 90.5, f"clip 1030 x 3 x 5 to -100 .. 90.5, extremes in frames {fmin} and {fmax}")
        assert (vmin, vmax) == (F(-100.0), F(90.5))


def test_clip_cube_strided_views(gpu_ctx, monkeypatch):
    """the bounds leave the maximum to the data: a sentinel read from outside a view would be reported as the range's end"""
    x = PO.spread_cube(VIEW, 18, pairs=False)
    x[5, 2, 66] = x[16, 4, 0] = np.nan
    want, vmin, vmax = PO.clip_cube(x, -120.5, 1e30)
    assert vmin == F(-120.5) and vmax == np.nanmax(x) and vmax < 1e6
    ranges = []

    def call(data, out):
        got, gmin, gmax = P.clip_cube(data, -120.5, 1e30, out=out, ctx=gpu_ctx)
        ranges.append((gmin, gmax))
        return got

    _strided_forms(gpu_ctx, monkeypatch, x, want, call, "wass_clip_cube", 9)
    print(f"clip of strided views: ranges {sorted(set(ranges))}, oracle {(vmin, vmax)}")
    assert len(ranges) == 6 and all(r == (vmin, vmax) for r in ranges)


def _clip_edge_cases():
    rng = np.random.default_rng(77)
    inf = np.inf
    neg = -np.abs(PO.spread_cube((3, 7, 66), 78, pairs=False)) - F(0.5)
    yield "all negative, nothing clipped", neg, -inf, inf
    yield "all negative, clipped to -50 .. -3", neg, -50.0, -3.0
    yield "all negative, clipped to positive bounds", neg, 2.0, 9.0
    x = (rng.standard_normal((2, 5, 65)) * 10).astype(F)
    x[0, 0, 0], x[1, 4, 64], x[1, 2, 3] = inf, -inf, np.nan
    yield "infinite data, infinite bounds", x, -inf, inf
    yield "infinite data, finite bounds", x, -4.0, 5.5
    yield "only +inf", np.full((1, 2, 3), inf, F), -inf, inf
    yield "only -inf", np.full((1, 2, 3), -inf, F), -inf, inf
    tiny = np.array([1e-45, -1e-45, 3e-45, -4e-45, 1e-40, -1e-40, 1.17549435e-38, -1.17549435e-38, 0.0, np.nan], F)
    yield "subnormals, nothing clipped", np.resize(tiny, (2, 3, 5)), -inf, inf
    yield "subnormals, subnormal bounds", np.resize(tiny, (2, 3, 5)), -3e-45, 1e-44
    big = np.resize(np.concatenate((tiny, np.array([FLT_MAX, -FLT_MAX, 1.0, -1.0], F))), (2, 3, 7))
    yield "subnormals and +-FLT_MAX, nothing clipped", big, -inf, inf
    yield "subnormals and +-FLT_MAX, bounds +-FLT_MAX", big, -float(FLT_MAX), float(FLT_MAX)
    yield "subnormals and +-FLT_MAX, clipped to -1e38 .. 1e-41", big, -1e38, 1e-41
    yield "lo > hi", x, 7.0, -2.5
    yield "lo == hi", x, 2.5, 2.5
    yield "1 x 1 x 1", np.array([[[-3.25]]], F), -10.0, 10.0
    yield "1 x 1 x 1, clipped", np.array([[[-3.25]]], F), 1.0, 10.0
    yield "1 x 1 x 1, NaN", np.array([[[np.nan]]], F), -10.0, 10.0
    lone = np.full((2, 33, 65), np.nan, F)
    lone[1, 32, 64] = -7.5                                                       # lane (0, 0) of the ragged corner block of the last frame
    yield "NaN but the last cell, nothing clipped", lone, -inf, inf
    yield "NaN but the last cell, clipped", lone, -2.0, 3.0
    zeros = np.resize(np.array([0.0, -0.0, np.nan, -0.0, 0.0], F), (2, 5, 67))
    yield "-0.0 and +0.0 are the extremes", zeros, -1.0, 1.0
    mixed = np.resize(np.array([0.0, -0.0, 3.5, -0.0, np.nan, -2.25], F), (2, 5, 67))
    yield "zeros of both signs below a clipped maximum", np.where(mixed < 0, F(-0.0), mixed), -1.0, 0.5


@pytest.mark.parametrize("case", list(_clip_edge_cases()), ids=lambda c: c[0])
def test_clip_cube_edge_values(gpu_ctx, case):
    what, x, lo, hi = case
    want, vmin, vmax = _clip_both_sides(gpu_ctx, x, lo, hi, "clip: " + what)
    finite = want[~np.isnan(want)]
    if lo > hi:
        assert (finite == F(hi)).all() and vmin == vmax == F(hi)
    if finite.size:
        assert vmin == finite.min() and vmax == finite.max()
    else:
        assert np.isnan(vmin) and np.isnan(vmax)


# ---- remap_linear_f32 ---------------------------------------------------------------------------------------------------------------
def _remap_both_sides(ctx, img, mx, my, what):
    import torch
    want = PO.remap_linear_f32(img, mx, my)
    got = P.remap_linear_f32(img, mx, my, ctx=ctx)
    print(f"{what}: {int((want != 0).sum())} of {want.size} cells are not 0")
    _exact(got, want, what + " host")
    dev = P.remap_linear_f32(torch.tensor(img).cuda(), torch.tensor(mx).cuda(), torch.tensor(my).cuda(), ctx=ctx)
    assert dev.is_cuda
    _exact(_host(dev), want, what + " device")
    return got


@pytest.mark.parametrize("sh,sw", [(1, 1), (1, 9), (9, 1), (2, 2)])
def test_remap_linear_f32_thin_pictures(gpu_ctx, sh, sw):
    """a side of 1 or 2: sw - 1 or sh - 1 is 0 or 1, so no or one window takes the interior path of the sampler"""
    img = (np.random.default_rng(10 * sh + sw).standard_normal((sh, sw)) * 3.0 + 1.0).astype(F)
    mx, my = RO.lattice_maps(37, 67, sh, sw, 11 + sw)
    got = _remap_both_sides(gpu_ctx, img, mx, my, f"{sh} x {sw} picture, 37 x 67 maps")
    if (sh, sw) == (2, 2):
        _variants(img, mx, my, got, "2 x 2")


def test_remap_linear_f32_where_the_quantisation_switches(gpu_ctx):
    """A hand-written map on a 5 x 7 picture, every pair of these coordinates: +-2^31 / 32, where the product leaves the int32 range,
    and the floats just inside; +-1023.98 and +-1024 (X = +-32767, +-32768); +-32767, +-32768 and beyond (X >> 5 at and beyond the
    int16 range, where the window's origin saturates); -1/64, -1/32 - eps, -1/32, -1 and -1 - 1/64, negative coordinates whose
    shift and mask must floor; both zeros; the last column and row and the half cell beyond; NaN and +-inf.  The oracle is defined
    for every one of them (quantise gives 0 where the product is not a finite int32), so none is left out."""
    edge = F(2.0 ** 26)
    inside = np.nextafter(edge, F(0))
    vals = np.array([edge, -edge, inside, -inside, 1023.98, -1023.98, 1024.0, -1024.0, 32767.0, -32767.0, 32767.99, 32768.0, -32768.0, -32768.02,
                     -32769.0, 40000.0, -40000.0, -1.0 / 64, np.nextafter(F(-1.0 / 32), F(-1)), -1.0 / 32, -1.0, -1.0 - 1.0 / 64, -0.0, 0.0,
                     0.40625, 1.77, 2.71875, 3.234375, 4.0, 4.5, 6.0, 6.5, 7.0, np.nan, np.inf, -np.inf], F)
    my, mx = (np.ascontiguousarray(a) for a in np.meshgrid(vals, vals, indexing="ij"))
    img = (np.random.default_rng(57).standard_normal((5, 7)) * 3.0 + 1.0).astype(F)
    X, ok = RO.quantise(vals)
    print(f"{int(ok.sum())} of {vals.size} coordinates are defined; X >> 5 from {int((X[ok] >> 5).min())} to {int((X[ok] >> 5).max())}")
    assert not ok[[0, 1, -3, -2, -1]].any() and ok[2:-3].all()
    assert (X[ok] >> 5).min() < -32768 and (X[ok] >> 5).max() > 32767
    q = lambda v: int(RO.quantise(np.array([v], F))[0][0])
    assert q(-1.0 / 64) == 0 and q(vals[18]) == -1 and q(-1.0 - 1.0 / 64) == -32 and (-1 >> 5, -1 & 31) == (-1, 31)      # -0.5 and -32.5 round to even
    assert (q(1023.98), q(-1024.0), q(inside)) == (32767, -32768, 2 ** 31 - 128)
    got = _remap_both_sides(gpu_ctx, img, mx, my, "5 x 7 picture, hand-written map")
    assert int((got != 0).sum()) > 100
    _variants(img, mx, my, got, "hand-written map")


# ---- polarimetric_setup -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _scene(*key):
    """inputs and the oracle's results, computed once and not changed by any test"""
    args = PO.make_scene(*key)
    want = PO.setup(*args)
    pictures = (args[0],) if isinstance(args[0], np.ndarray) else tuple(args[0])
    for a in pictures + args[1:] + tuple(want[k] for k in PER_FRAME + AVERAGES):
        a.setflags(write=False)
    return args, want


def _check_setup(r, want, args, what):
    """every per-frame output and every average of a host result against the oracle, exact but for the angles"""
    XX, YY, cam = args[2], args[3], args[5]
    count, H, W = args[1].shape
    assert want["not_up"] == 0
    near_all = PO.near_85(want, XX, YY, cam)
    print(f"{what}: near_all = {near_all} cells within the bound of 85 degrees, {100.0 * want['occlusion'].mean():.2f} % occluded, "
          f"{100.0 * want['march'].mean():.2f} % by the march")
    assert near_all == 0
    for k in ("S", "dolp", "normals", "rays_cam", "occlusion") + AVERAGES:
        _exact(getattr(r, k), want[k], f"{what}: {k}")
    nan = np.isnan(want["angles"])
    assert r.angles.dtype == F and np.array_equal(np.isnan(r.angles), nan)
    ratio = 0.0
    for t in range(count):
        a64, n = VO.noise(XX, YY, want["zf"][t], cam[:3, 3])
        assert np.array_equal(a64, want["angles"][t], equal_nan=True)
        ok = ~np.isnan(a64)
        ratio = max(ratio, float((np.abs(r.angles[t].astype(np.float64) - a64)[ok] / VO.angle_bound(a64, n)[ok]).max()))
    print(f"{what}: largest angle error / bound = {ratio:.4f}")
    assert ratio <= 1.0
    print(f"{what}: occluded_percent {r.occluded_percent}, oracle {want['occluded_percent']}")
    assert np.array_equal(r.occluded_percent, want["occluded_percent"])


def _bytes(r):
    return {k: _host(getattr(r, k)).tobytes() for k in PER_FRAME + AVERAGES}


def _same_bytes(r, base, what):
    got = _bytes(r)
    bad = [k for k in base if got[k] != base[k]]
    print(f"{what}: outputs that are not byte-identical: {bad}")
    assert not bad, what


@pytest.mark.parametrize("name", list(PO.SMALL))
def test_polarimetric_setup_small_grids(gpu_ctx, name):
    import torch
    args, want = _scene(*PO.SMALL[name])
    stokes, Z = args[:2]
    r = P.polarimetric_setup(*args, outputs=PER_FRAME, ctx=gpu_ctx)
    _check_setup(r, want, args, name)
    nonzero = int((np.nan_to_num(want["S"]) != 0).sum())
    print(f"{name}: {nonzero} of {want['S'].size} samples are neither 0 nor NaN")
    assert nonzero > 0
    off = P.polarimetric_setup(*args, angle_limit=None, outputs=("occlusion",), ctx=gpu_ctx)
    _exact(off.occlusion, want["march"], f"{name}: the march's mask")
    d = P.polarimetric_setup(torch.tensor(stokes).cuda(), torch.tensor(Z).cuda(), *args[2:], outputs=PER_FRAME, ctx=gpu_ctx)
    assert d.S.is_cuda and d.Savg.is_cuda
    _same_bytes(d, _bytes(r), f"{name}: device against host")
    assert np.array_equal(d.occluded_percent, r.occluded_percent)


def test_polarimetric_setup_strided_inputs(gpu_ctx, monkeypatch):
    import torch
    args, want = _scene(*PO.STRIDED)
    stokes, Z = args[:2]
    count, H, W = Z.shape
    Ih, Iw = stokes.shape[2:]
    base_r = P.polarimetric_setup(*args, outputs=PER_FRAME, ctx=gpu_ctx)
    _check_setup(base_r, want, args, "64 x 65 contiguous")
    base = _bytes(base_r)
    spy = _Spy(gpu_ctx._lib)
    monkeypatch.setattr(gpu_ctx, "_lib", spy)
    zbig = np.full((count, H + 5, W + 9), SENTINEL, F)
    zbig[:, 2:2 + H, 4:4 + W] = Z
    pbig = np.full((count, 3, Ih + 5, Iw + 8), SENTINEL, F)
    pbig[:, :, 2:2 + Ih, 3:3 + Iw] = stokes
    big6 = np.full((count, 6, Ih, Iw), SENTINEL, F)
    big6[:, ::2] = stokes
    for xp, entry in ((np, "wass_polarimetric"), (torch, "wass_polarimetric_dev")):
        side = "host" if xp is np else "device"
        put = (lambda a: a) if xp is np else (lambda a: torch.tensor(a).cuda())
        zb, pb, b6 = put(zbig), put(pbig), put(big6)
        cube = zb[:, 2:2 + H, 4:4 + W]
        for what, pics, whole in (("padded rows and columns", pb[:, :, 2:2 + Ih, 3:3 + Iw], pb), ("every other channel", b6[:, ::2], b6)):
            r = P.polarimetric_setup(pics, cube, *args[2:], outputs=PER_FRAME, ctx=gpu_ctx)
            name, a = spy.calls[-1]
            assert name == entry and len([c for c in spy.calls if c[0].startswith("wass_polarimetric")]) >= 1
            # the library was handed the views themselves: their addresses inside the larger arrays, and their strides
            assert a[1] == _address(pics) and tuple(a[2:5]) == _strides(pics, 3), "the pictures went through a copy"
            assert a[7] == _address(cube) and tuple(a[8:10]) == _strides(cube, 2), "the cube went through a copy"
            assert _strides(cube, 2) == ((H + 5) * (W + 9), W + 9) and _strides(pics, 3) != (3 * Ih * Iw, Ih * Iw, Iw)
            if xp is np:
                assert np.shares_memory(pics, whole) and np.shares_memory(cube, zb) and not pics.flags.c_contiguous
            _same_bytes(r, base, f"64 x 65 {side}, {what}")
            assert np.array_equal(r.occluded_percent, base_r.occluded_percent)
        assert _host(zb).tobytes() == zbig.tobytes() and _host(pb).tobytes() == pbig.tobytes() and _host(b6).tobytes() == big6.tobytes()


def test_polarimetric_setup_iterable_changes_picture_size(gpu_ctx):
    """frames 0 and 1 from 240 x 320 pictures, frames 2 to 4 from 120 x 200 ones, batch 8: the change of size forces a flush of two
    frames, whose sums the accumulators carry (unfinished, total_frames = 0) into the call of the other three"""
    import torch
    args, want = _scene(*PO.CHANGING)
    stokes, Z = args[:2]
    assert [f.shape[1:] for f in stokes] == list(PO.FIVE_SIZES)
    triples = lambda: ((f[0], f[1], f[2]) for f in stokes)
    r = P.polarimetric_setup(triples(), *args[1:], outputs=PER_FRAME, ctx=gpu_ctx, batch=8)
    _check_setup(r, want, args, "two picture sizes, batch 8")
    base = _bytes(r)
    _same_bytes(P.polarimetric_setup(triples(), *args[1:], outputs=PER_FRAME, ctx=gpu_ctx, batch=1), base, "two picture sizes, batch 1")
    _same_bytes(P.polarimetric_setup(triples(), *args[1:], outputs=PER_FRAME, ctx=gpu_ctx, batch=2), base, "two picture sizes, batch 2")
    dev = P.polarimetric_setup(((torch.tensor(f[k]).cuda() for k in range(3)) for f in stokes), torch.tensor(Z).cuda(), *args[2:],
                               outputs=PER_FRAME, ctx=gpu_ctx, batch=8)
    assert dev.S.is_cuda
    _same_bytes(dev, base, "two picture sizes, device")
    # total_frames with the per-frame outputs asked for: only Zavg changes
    nine = P.polarimetric_setup(triples(), *args[1:], outputs=PER_FRAME, total_frames=9, ctx=gpu_ctx, batch=8)
    want9 = PO.setup(*args, total_frames=9)
    total = np.zeros(Z.shape[1:])
    for zf in want["zf"]:
        total = total + zf.astype(np.float64)
    assert np.array_equal(want9["Zavg"], total / 9.0, equal_nan=True)
    _exact(nine.Zavg, want9["Zavg"], "total_frames = 9: Zavg")
    changed = [k for k, b in _bytes(nine).items() if b != base[k]]
    print(f"total_frames = 9 changes {changed}")
    assert changed == ["Zavg"]
    # what the comparison can see: the first two frames projected as if their pictures were 120 x 200
    wrong = PO.setup([PO.stokes_pictures(5, 120, 200, PO.CHANGING[3])[t] for t in range(5)], *args[1:])
    miss = _diff(wrong["S"][:2], r.S[:2])
    print(f"pictures of one size throughout miss S of frames 0 and 1 in {miss} of {r.S[:2].size} values")
    assert miss > 0


def test_polarimetric_setup_ragged_last_launch(gpu_ctx):
    """count 5 with batch 2: launches of 2, 2 and 1 frames inside one call; the bytes of batch 5"""
    import torch
    args, want = _scene(*PO.RAGGED)
    stokes, Z = args[:2]
    outs = ("normals", "rays_cam", "dolp")
    for side, a in (("host", args), ("device", (torch.tensor(stokes).cuda(), torch.tensor(Z).cuda()) + args[2:])):
        one = P.polarimetric_setup(*a, outputs=outs, ctx=gpu_ctx, batch=5)
        for b in (2, 3):
            two = P.polarimetric_setup(*a, outputs=outs, ctx=gpu_ctx, batch=b)
            bad = [k for k in outs + AVERAGES if _host(getattr(one, k)).tobytes() != _host(getattr(two, k)).tobytes()]
            print(f"count 5, {side}: batch {b} against batch 5: outputs that are not byte-identical: {bad}")
            assert not bad
            assert two.S is None and two.occlusion is None and two.angles is None
            assert np.array_equal(one.occluded_percent, two.occluded_percent)
        for k in outs + AVERAGES:
            _exact(_host(getattr(one, k)), want[k], f"count 5, {side}, batch 5: {k}")
        assert np.array_equal(one.occluded_percent, want["occluded_percent"])
