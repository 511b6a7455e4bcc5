"""filter.hip on the GPU against tests/filter_oracle.py, bit for bit: every k_sos_forward<NS> / k_sos_backward<NS, DEMEAN> instance, the
paths of sos_run (prologue, blocks of FILT_U = 8 with and without a prefetch, scalar tail) by count and padlen, explicit padlen
through the C ABI in the host and the device form, the edges of the series index, strided views, NaN and the probes of
tests/filter_probes.py.  The kernel's contract is scipy's order of operations in fp64 without contraction, the padding rounded in
float32, the mean summed frame by frame: so the float32 result is the fp64 oracle's, rounded, and every comparison here is
np.array_equal(got, oracle64.astype(float32), equal_nan=True).  No tolerance anywhere in this file.
tests/test_filter_edges.py shows on the CPU that this equality tells a re-associated update, a contracted product, a padding built
in fp64 and a pairwise mean at every section count."""
import functools

import numpy as np
import pytest

import filter_oracle as FO
import filter_probes as FP
from wass_amd import postproc as P

pytestmark = pytest.mark.gpu

RM = pytest.mark.parametrize("rm", [False, True], ids=["DEMEAN0", "DEMEAN1"])


@functools.lru_cache(maxsize=None)
def _sos(order, band):
    bt, fc = FP.BANDS[band]
    sos = P.butter_sos(order, fc, bt, FP.FS)
    sos.setflags(write=False)
    return sos


def _want(sos, cube, rm=False, padlen=None):
    return FP.rounded(FO.sosfiltfilt(sos, cube, remove_mean=rm, padlen=padlen))


def _same(got, want, what):
    assert got.dtype == np.float32 and got.shape == want.shape, what
    eq = (got == want) | (np.isnan(got) & np.isnan(want))
    if not eq.all():
        i = tuple(int(v) for v in np.argwhere(~eq)[0])
        print(f"{what}: {int((~eq).sum())} of {eq.size} elements differ, the first at {i}: got {got[i]!r}, oracle {want[i]!r}")
    assert np.array_equal(got, want, equal_nan=True), what


def _abi(ctx, sos, cube, padlen, rm=False, dev=False, slab_rows=0):
    """wass_sosfiltfilt / wass_sosfiltfilt_dev with an explicit padlen; (return code, output), the output buffer filled with -7 before"""
    sos = np.ascontiguousarray(sos, np.float64)
    zi = np.ascontiguousarray(P.sosfilt_zi(sos))
    count, H, W = cube.shape
    assert cube.dtype == np.float32 and cube.flags.c_contiguous
    tail = (sos.ctypes.data, sos.shape[0], zi.ctypes.data, int(padlen), int(rm), int(slab_rows))
    if dev:
        import torch
        d = torch.from_numpy(cube).to(f"cuda:{ctx.device_id}")
        o = torch.full((count, H, W), -7.0, dtype=torch.float32, device=d.device)
        torch.cuda.synchronize(d.device)
        rc = ctx._lib.wass_sosfiltfilt_dev(ctx._h, d.data_ptr(), H * W, W, count, H, W, *tail, o.data_ptr(), H * W, W)
        ctx.synchronize()
        return rc, o.cpu().numpy()
    o = np.full((count, H, W), np.float32(-7.0))
    rc = ctx._lib.wass_sosfiltfilt(ctx._h, cube.ctypes.data, H * W, W, count, H, W, *tail, o.ctypes.data, H * W, W)
    return rc, o


# ---- every instance ------------------------------------------------------------------------------------------------------------------
@RM
@pytest.mark.parametrize("band", list(FP.BANDS))
@pytest.mark.parametrize("order", FP.ORDERS, ids=[f"order{o}-NS{(o + 1) // 2}" for o in FP.ORDERS])
def test_every_instance(gpu_ctx, order, band, rm):
    """k_sos_forward<NS>, k_sos_backward<NS, DEMEAN> (and k_sos_demean) for NS = 1 .. 6 at an odd and an even order each, on
    series_cube(padlen + 9, 3, 70) and on every probe of that order."""
    sos = _sos(order, band)
    assert sos.shape[0] == (order + 1) // 2
    for name in FP.PROBES:
        cube = FP.probe(name, order)
        assert cube.shape[0] == P.sos_padlen(sos) + 9
        _same(P.sosfiltfilt(sos, cube, remove_mean=rm, ctx=gpu_ctx), _want(sos, cube, rm), f"order {order} {band} remove_mean {rm}, {name}")


# ---- the blocks of sos_run -------------------------------------------------------------------------------------------------------------
# (order, count): the three runs of a pass have n = padlen, count, padlen.  Order 1 (padlen 6: tail only) with the middle run from
# 7 (tail only) over 8, 9, 15 (one block, no prefetch, tails of 0, 1, 7), 16, 17, 23 (two blocks, one prefetch) to 24, 25, 33; order 2
# (padlen 9: one block and a tail of 1), order 7 (padlen 24: three exact blocks, no tail), order 12 (padlen 39: four blocks and 7).
BLOCKS = [(1, c) for c in (7, 8, 9, 15, 16, 17, 23, 24, 25, 33)] + [(2, c) for c in (10, 16, 17)] + [(7, c) for c in (25, 32, 40)] \
    + [(12, c) for c in (40, 48, 49)]


@RM
@pytest.mark.parametrize("order,count", BLOCKS, ids=[f"order{o}-count{c}" for o, c in BLOCKS])
def test_blocks_of_sos_run(gpu_ctx, order, count, rm):
    for band in FP.BANDS:
        sos = _sos(order, band)
        assert count > P.sos_padlen(sos)
        cube = FO.series_cube(count, 3, 70, seed=count + order, offset=40.0)
        _same(P.sosfiltfilt(sos, cube, remove_mean=rm, ctx=gpu_ctx), _want(sos, cube, rm), f"order {order} {band} count {count} remove_mean {rm}")


# ---- explicit padlen through the C ABI -------------------------------------------------------------------------------------------------
PADLENS = [(order, count, p) for order in (8, 1) for count in (17, 40) for p in sorted({0, 1, 7, 8, 9, 16, count - 1})]


@pytest.mark.parametrize("dev", [False, True], ids=["host", "dev"])
@pytest.mark.parametrize("order,count,padlen", PADLENS, ids=[f"order{o}-count{c}-padlen{p}" for o, c, p in PADLENS])
def test_explicit_padlen(gpu_ctx, order, count, padlen, dev):
    """Any 0 <= padlen < count, as scipy takes it: padlen 0 starts from zi times the first sample and extends nothing, count - 1
    reads every sample but the edge one into the padding."""
    cube = FO.series_cube(count, 3, 70, seed=count + padlen, offset=40.0)
    for band in FP.BANDS:
        sos = _sos(order, band)
        for rm in (False, True):
            rc, got = _abi(gpu_ctx, sos, cube, padlen, rm, dev)
            assert rc == 0
            _same(got, _want(sos, cube, rm, padlen), f"order {order} {band} count {count} padlen {padlen} remove_mean {rm} dev {dev}")


@pytest.mark.parametrize("dev", [False, True], ids=["host", "dev"])
@pytest.mark.parametrize("count", [1, 2])
def test_padlen_0_on_the_shortest_series(gpu_ctx, count, dev):
    cube = FO.series_cube(count, 3, 70, seed=count, offset=40.0)
    for order in (1, 8, 12):
        for band in FP.BANDS:
            sos = _sos(order, band)
            for rm in (False, True):
                rc, got = _abi(gpu_ctx, sos, cube, 0, rm, dev)
                assert rc == 0
                _same(got, _want(sos, cube, rm, 0), f"order {order} {band} count {count} padlen 0 remove_mean {rm} dev {dev}")


@pytest.mark.parametrize("dev", [False, True], ids=["host", "dev"])
def test_refused_padlen_leaves_the_output_alone(gpu_ctx, dev):
    cube = FO.series_cube(17, 3, 70, seed=3)
    for order in (8, 1):
        sos = _sos(order, "lp1.0")
        for padlen in (17, 18, -1):
            rc, got = _abi(gpu_ctx, sos, cube, padlen, False, dev)
            assert rc != 0, (order, padlen)
            assert (got == np.float32(-7.0)).all(), (order, padlen)
    rc, got = _abi(gpu_ctx, _sos(1, "lp1.0"), cube, 16, False, dev)            # the context still works
    assert rc == 0
    _same(got, _want(_sos(1, "lp1.0"), cube, False, 16), "after the refusals")


# ---- the series index ----------------------------------------------------------------------------------------------------------------
GRIDS = [(1, 1, 0), (1, 255, 0), (1, 256, 0), (1, 257, 0), (255, 1, 0), (3, 171, 0), (2, 300, 1)]


@pytest.mark.parametrize("H,W,slab_rows", GRIDS, ids=[f"{h}x{w}" + ("-slab1" if s else "") for h, w, s in GRIDS])
def test_series_index_edges(gpu_ctx, H, W, slab_rows):
    """One series, one short of a block of 256 threads, a block, a block and one, a column of rows, 513 series, and slabs of one
    row of 300 (a slab ends inside its second block)."""
    import torch
    order = 5
    cube = FO.series_cube(P.sos_padlen(_sos(order, "lp1.0")) + 9, H, W, seed=H + W, offset=40.0)
    for band in FP.BANDS:
        sos = _sos(order, band)
        for rm in (False, True):
            want = _want(sos, cube, rm)
            what = f"{H} x {W} slab_rows {slab_rows} {band} remove_mean {rm}"
            _same(P.sosfiltfilt(sos, cube, remove_mean=rm, ctx=gpu_ctx, slab_rows=slab_rows), want, what + " host")
            d = torch.from_numpy(cube).to(f"cuda:{gpu_ctx.device_id}")
            _same(P.sosfiltfilt(sos, d, remove_mean=rm, ctx=gpu_ctx, slab_rows=slab_rows).cpu().numpy(), want, what + " dev")


@pytest.mark.parametrize("order", [1, 12], ids=["NS1", "NS6"])
def test_strided_view_in_place(gpu_ctx, order):
    """A strided device view filtered onto itself: the result in the view, the cells around it untouched."""
    import torch
    sos = _sos(order, "hp0.05")
    count = P.sos_padlen(sos) + 9
    cube = FO.series_cube(count, 5, 37, seed=order, offset=40.0)
    for rm in (False, True):
        big = np.full((count, 8, 45), np.float32(7.0))
        big[:, 2:7, 4:41] = cube
        d = torch.from_numpy(big).to(f"cuda:{gpu_ctx.device_id}")
        dv = d[:, 2:7, 4:41]
        assert not dv.is_contiguous()
        assert P.sosfiltfilt(sos, dv, remove_mean=rm, ctx=gpu_ctx, out=dv) is dv
        back = d.cpu().numpy()
        _same(np.ascontiguousarray(back[:, 2:7, 4:41]), _want(sos, cube, rm), f"order {order} in place, remove_mean {rm}")
        back[:, 2:7, 4:41] = 7.0
        assert (back == 7.0).all()
        # a strided host view in, a strided host view out
        hout = np.full((count, 8, 45), np.float32(7.0))
        P.sosfiltfilt(sos, big[:, 2:7, 4:41], remove_mean=rm, ctx=gpu_ctx, out=hout[:, 2:7, 4:41])
        _same(np.ascontiguousarray(hout[:, 2:7, 4:41]), _want(sos, cube, rm), f"order {order} host views, remove_mean {rm}")
        hout[:, 2:7, 4:41] = 7.0
        assert (hout == 7.0).all()


def test_batch_forms_at_six_sections(gpu_ctx):
    """Slabs of every height, repeats, host and device: the bits of the single call, NS = 6 with the mean removed."""
    import torch
    sos = _sos(12, "hp0.05")
    cube = FO.series_cube(48, 7, 300, seed=12, offset=900.0, drift=0.3)
    want = _want(sos, cube, True)
    one = P.sosfiltfilt(sos, cube, remove_mean=True, ctx=gpu_ctx)
    _same(one, want, "one slab")
    d = torch.from_numpy(cube).to(f"cuda:{gpu_ctx.device_id}")
    for rows in (1, 2, 3, 6, 7, 100):
        assert P.sosfiltfilt_scratch_bytes(48, 7, 300, 39, slab_rows=rows)[1] == min(rows, 7)
        assert P.sosfiltfilt(sos, cube, remove_mean=True, ctx=gpu_ctx, slab_rows=rows).tobytes() == one.tobytes()
        assert P.sosfiltfilt(sos, d, remove_mean=True, ctx=gpu_ctx, slab_rows=rows).cpu().numpy().tobytes() == one.tobytes()
    for _ in range(2):
        assert P.sosfiltfilt(sos, cube, remove_mean=True, ctx=gpu_ctx).tobytes() == one.tobytes()


# ---- NaN -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [1, 12], ids=["NS1", "NS6"])
def test_nan_at_the_samples_the_padding_reads(gpu_ctx, order):
    """NaN at t = 0 and count - 1 (every padded sample is 2 x[edge] - x[k]), at t = padlen and count - 1 - padlen (the far ends of
    the two extensions): each makes its series NaN throughout and touches no other."""
    sos = _sos(order, "lp1.0")
    pad = P.sos_padlen(sos)
    count = 2 * pad + 9
    clean = FO.series_cube(count, 3, 70, seed=order, offset=40.0)
    cube = clean.copy()
    spots = [(0, 0, 0), (pad, 1, 5), (count - 1 - pad, 1, 64), (count - 1, 2, 69)]
    for t, r, c in spots:
        cube[t, r, c] = np.nan
    bad = np.isnan(cube).any(axis=0)
    assert bad.sum() == 4
    for rm in (False, True):
        got = P.sosfiltfilt(sos, cube, remove_mean=rm, ctx=gpu_ctx)
        _same(got, _want(sos, cube, rm), f"order {order} NaN, remove_mean {rm}")
        assert np.isnan(got[:, bad]).all()
        base = P.sosfiltfilt(sos, clean, remove_mean=rm, ctx=gpu_ctx)
        assert got[:, ~bad].tobytes() == base[:, ~bad].tobytes()
