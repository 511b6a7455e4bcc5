"""The disparity clean-up kernels (csrc/post.hip, csrc/post_opt.hip) on the probes of tests/cleanup_probes.py, against the direct-form
restatement tests/cleanup_oracle.py (held in place on the CPU by tests/test_cleanup_edges.py).  Every comparison is bit for bit: the
stage is integer or float32 in a fixed order of operations, nothing has a tolerance."""
import numpy as np
import pytest

import cleanup_oracle as R
import cleanup_probes as P
import wass_amd
from wass_amd import default_sgm_params

pytestmark = pytest.mark.gpu

ids = lambda c: "x".join(str(v) for v in c) if isinstance(c, tuple) else str(c)
ND, MD = P.NUMDISP, P.MINDISP


def _params(off=0, md=MD, scale=1.0):
    p = default_sgm_params(ND, min_disp=md, disp_offset=off)
    p.dense_scale = scale
    return p


def _both_paths(ctx, monkeypatch, d, p, nd, ne, med, ref, what):
    """once through the fused tile kernel (where the setting fits), once one kernel per step"""
    monkeypatch.delenv("WASS_CLEAN_CHAIN", raising=False)
    np.testing.assert_array_equal(ctx.disparity_postprocess(d, p, nd, ne, med), ref, err_msg=f"fused {what}")
    monkeypatch.setenv("WASS_CLEAN_CHAIN", "0")
    np.testing.assert_array_equal(ctx.disparity_postprocess(d, p, nd, ne, med), ref, err_msg=f"stepwise {what}")
    monkeypatch.delenv("WASS_CLEAN_CHAIN", raising=False)


# ---------------------------------------------------------------------------------------------------------------- chain
@pytest.mark.parametrize("shape", P.SHAPES, ids=ids)
def test_chain_on_random_holes_at_every_shape_and_setting(gpu_ctx, monkeypatch, shape):
    w, h = shape
    p = _params()
    for frac in P.HOLE_FRACTIONS:
        d = P.random_holes(w, h, frac)
        for nd, ne, med in P.STEPS:
            ref = R.chain(d, MD, ND, 0, 1.0, nd, ne, med)
            _both_paths(gpu_ctx, monkeypatch, d, p, nd, ne, med, ref, f"{w}x{h} holes {frac} {(nd, ne, med)}")


@pytest.mark.parametrize("steps", P.STEPS, ids=ids)
@pytest.mark.parametrize("shape", P.LATTICE_SHAPES, ids=ids)
def test_chain_on_the_seam_lattice_and_its_inverse(gpu_ctx, monkeypatch, shape, steps):
    w, h = shape
    nd, ne, med = steps
    p = _params()
    for name, d in (("lattice", P.seam_lattice(w, h, steps)), ("inverse", P.seam_lattice_inverse(w, h))):
        ref = R.chain(d, MD, ND, 0, 1.0, nd, ne, med)
        _both_paths(gpu_ctx, monkeypatch, d, p, nd, ne, med, ref, f"{name} {w}x{h} {steps}")


def test_chain_last_fused_and_first_stepwise_setting_on_one_map(gpu_ctx):
    """(9, 9, 5) needs 62 752 B of LDS and is fused, (10, 9, 5) needs 65 664 B and is not: the same map through both sides of
    the switch"""
    assert R.chain_lds_bytes(9, 9, 5) == 62752 <= 64 * 1024 < R.chain_lds_bytes(10, 9, 5) == 65664
    w, h = 257, 97
    p = _params()
    for d in (P.random_holes(w, h, 0.50, seed=1), P.seam_lattice(w, h, (9, 9, 5))):
        for st in ((9, 9, 5), (10, 9, 5)):
            np.testing.assert_array_equal(gpu_ctx.disparity_postprocess(d, p, *st), R.chain(d, MD, ND, 0, 1.0, *st), err_msg=str(st))


@pytest.mark.parametrize("shape", [(65, 33), (129, 65), (257, 97)], ids=ids)
def test_chain_values_that_are_no_multiples_of_a_sixteenth(gpu_ctx, monkeypatch, shape):
    """DENSE_SCALE 0.73 with the output as large as the map: still the fused kernel, and the order of the dilation's eight additions
    shows in the last bit"""
    w, h = shape
    p = _params(scale=0.73)
    for frac in (0.20, 0.50):
        d = P.random_holes(w, h, frac)
        for nd, ne, med in ((1, 2, 0), (1, 2, 3), (3, 3, 5)):
            ref = R.chain(d, MD, ND, 0, 1.0 / 0.73, nd, ne, med)
            monkeypatch.delenv("WASS_CLEAN_CHAIN", raising=False)
            np.testing.assert_array_equal(gpu_ctx.disparity_postprocess_ex(d, p, w, h, nd, ne, med), ref)
            monkeypatch.setenv("WASS_CLEAN_CHAIN", "0")
            np.testing.assert_array_equal(gpu_ctx.disparity_postprocess_ex(d, p, w, h, nd, ne, med), ref)
            monkeypatch.delenv("WASS_CLEAN_CHAIN", raising=False)


def test_chain_offsets_and_minimum_disparities(gpu_ctx, monkeypatch):
    w, h = 129, 65
    d = P.random_holes(w, h, 0.20)
    for off in P.OFFSETS:
        for md in P.MIN_DISPS:
            ref = R.chain(d, md, ND, max(off, 0), 1.0, 1, 2, 3)
            _both_paths(gpu_ctx, monkeypatch, d, _params(off, md), 1, 2, 3, ref, f"offset {off} min_disp {md}")


def test_chain_device_entry_gives_the_same_bits(gpu_ctx):
    import torch
    for w, h in ((65, 33), (257, 97)):
        d = P.seam_lattice(w, h, (1, 2, 3))
        out = gpu_ctx.disparity_postprocess_dev(torch.from_numpy(d).cuda(), _params(), 1, 2, 3)
        gpu_ctx.synchronize()
        np.testing.assert_array_equal(out.cpu().numpy(), R.chain(d, MD, ND, 0, 1.0, 1, 2, 3))


# ---------------------------------------------------------------------------------------------------------------- median
@pytest.mark.parametrize("ks", [3, 5])
def test_median_on_maps_smaller_than_the_window_with_ties_and_zeros(gpu_ctx, monkeypatch, ks):
    for name, d in P.median_maps().items():
        for nd, ne in ((0, 0), (1, 0)):
            ref = R.chain(d, MD, ND, 0, 1.0, nd, ne, ks)
            _both_paths(gpu_ctx, monkeypatch, d, _params(), nd, ne, ks, ref, f"{name} median {ks}")


# ---------------------------------------------------------------------------------------------------------------- components
def _biggest(ctx, f, thr):
    import torch
    h, w = f.shape
    t = torch.from_numpy(np.ascontiguousarray(f, np.float32).copy()).cuda()
    rc = ctx._lib.wass_biggest_component_by_gradient_dev(ctx._h, t.data_ptr(), w, h, int(thr))
    assert rc == 0
    ctx.synchronize()
    mask = np.empty((h, w), np.uint8)
    assert ctx._lib.wass_large_gradient_mask(ctx._h, w, h, mask.ctypes.data) == 0
    return t.cpu().numpy(), mask


@pytest.mark.parametrize("shape", P.COMPONENT_SHAPES, ids=ids)
def test_biggest_component_on_every_component_map(gpu_ctx, shape):
    w, h = shape
    for name, make in P.COMPONENT_MAPS.items():
        f = make(w, h)
        ref, area, lg = R.biggest_component(f, P.COMPONENT_THR)
        got, mask = _biggest(gpu_ctx, f, P.COMPONENT_THR)
        np.testing.assert_array_equal(got, ref, err_msg=f"{name} {w}x{h}")
        np.testing.assert_array_equal(mask, lg, err_msg=f"{name} {w}x{h} mask")
        if name in P.HARD_MAPS:                                  # deep parent chains, many unions at once: the same bits again
            again, _ = _biggest(gpu_ctx, f, P.COMPONENT_THR)
            np.testing.assert_array_equal(again, got, err_msg=f"{name} {w}x{h} second run")


def test_sobel_threshold_and_border_probes(gpu_ctx):
    ramp = P.sobel_ramp()
    cases = [(ramp, 100), (ramp, 575), (ramp, 576)]
    for s in (3.0, 2.5):
        f = P.sobel_step(s)
        cases += [(f, int(16 * s * s)), (f, int(16 * s * s) - 1)]
    for f, thr in cases:
        ref, _, lg = R.biggest_component(f, thr)
        got, mask = _biggest(gpu_ctx, f, thr)
        np.testing.assert_array_equal(mask, lg, err_msg=f"mask at {thr}")
        np.testing.assert_array_equal(got, ref, err_msg=f"map at {thr}")
    assert (R.biggest_component(ramp, 100)[0] != 0).sum() == ramp.shape[0]


# ---------------------------------------------------------------------------------------------------------------- speckles
def _speckles(ctx, img, nv, ms, mdiff):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(img, np.int16).copy()).cuda()
    ctx.filter_speckles_dev(t, nv, ms, mdiff)
    ctx.synchronize()
    return t.cpu().numpy()


def test_speckle_probes(gpu_ctx):
    for name, (img, nv, ms, mdiff) in P.speckle_probes().items():
        ref = R.filter_speckles(img, nv, ms, mdiff)
        for run in (1, 2):
            np.testing.assert_array_equal(_speckles(gpu_ctx, img, nv, ms, mdiff), ref, err_msg=f"{name} run {run}")
    img, nv, ms, mdiff = P.speckle_probes()["extremes"]
    np.testing.assert_array_equal(_speckles(gpu_ctx, img, nv, 11, mdiff), R.filter_speckles(img, nv, 11, mdiff))


@pytest.mark.parametrize("shape", P.COMPONENT_SHAPES[:5], ids=ids)
def test_speckles_on_the_component_maps(gpu_ctx, shape):
    w, h = shape
    for name, make in P.COMPONENT_MAPS.items():
        img = P.as_int16(make(w, h))
        ref = R.filter_speckles(img, 0, 7, 0)
        for run in (1, 2):
            np.testing.assert_array_equal(_speckles(gpu_ctx, img, 0, 7, 0), ref, err_msg=f"{name} {w}x{h} run {run}")


def test_speckles_on_the_hard_maps_at_the_largest_size(gpu_ctx):
    """1024 x 256: the flood fill of the reference is slow there, and a map of one value has a simpler one -- the regions are its
    4-connected components"""
    from scipy import ndimage
    w, h = P.COMPONENT_SHAPES[5]
    for name in P.HARD_MAPS:
        img = P.as_int16(P.COMPONENT_MAPS[name](w, h))
        lab, n = ndimage.label(img != 0, R.FOUR)
        small = np.bincount(lab.ravel(), minlength=n + 1) <= 7
        small[0] = False
        ref = np.where(small[lab], 0, img).astype(np.int16)
        for run in (1, 2):
            np.testing.assert_array_equal(_speckles(gpu_ctx, img, 0, 7, 0), ref, err_msg=f"{name} run {run}")


def test_speckle_entry_checks_its_arguments(gpu_ctx):
    import torch
    t = torch.zeros((4, 4), dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    lib, h = gpu_ctx._lib, gpu_ctx._h
    assert lib.wass_filter_speckles_dev(h, None, 4, 4, 0, 1, 1) != 0
    assert lib.wass_filter_speckles_dev(h, t.data_ptr(), 0, 4, 0, 1, 1) != 0
    assert lib.wass_filter_speckles_dev(h, t.data_ptr(), 4, 4, 0, -1, 1) != 0
    assert lib.wass_filter_speckles_dev(h, t.data_ptr(), 4, 4, 0, 1, -1) != 0
    assert lib.wass_filter_speckles_dev(h, t.data_ptr(), 4, 4, 40000, 1, 1) != 0
    with pytest.raises(ValueError):
        gpu_ctx.filter_speckles_dev(t.to(torch.int32), 0, 1, 1)


# ---------------------------------------------------------------------------------------------------------------- resizers
def test_cubic_u8_resize_to_an_explicit_size_from_a_strided_source(gpu_ctx):
    import torch
    for sw, sh, dw, dh in P.resize_cases():
        src = P.picture(sw, sh)
        stride = 128 if (sw, sh) == (97, 61) else sw
        buf = np.full((sh, stride), 7, np.uint8)
        buf[:, :sw] = src
        t = torch.from_numpy(buf).cuda()
        out = torch.full((dh, dw), 99, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()                              # the fill runs on torch's stream, the resize on the context's
        rc = gpu_ctx._lib.wass_resize_cubic_u8_dev(gpu_ctx._h, t.data_ptr(), sw, sh, stride, out.data_ptr(), dw, dh)
        assert rc == 0
        gpu_ctx.synchronize()
        np.testing.assert_array_equal(out.cpu().numpy(), R.resize_cubic_u8(src, dw, dh, sw / dw, sh / dh), err_msg=str((sw, sh, dw, dh)))
    assert gpu_ctx._lib.wass_resize_cubic_u8_dev(gpu_ctx._h, t.data_ptr(), sw, sh, sw - 1, out.data_ptr(), dw, dh) != 0


def test_float_resizers_through_the_clean_up(gpu_ctx):
    """dilate, erode, median and the component threshold all 0: what is left is where(erode(nearest) == 0, 0, cubic)"""
    for ws, hs, scale, ow, oh in P.float_resize_cases():
        d = P.random_holes(ws, hs, 0.05)
        got = gpu_ctx.disparity_postprocess_ex(d, _params(scale=scale), ow, oh, 0, 0, 0, 0)
        a = R.convert(d, MD, ND, 0, 1.0 / scale)
        if (ow, oh) == (ws, hs):
            ref = R.mask_step(a, a)
        else:
            ref = np.where(R.erode(R.resize_f32(a, ow, oh, False)) == 0, np.float32(0), R.resize_f32(a, ow, oh, True))
        np.testing.assert_array_equal(got, ref, err_msg=str((ws, hs, scale, ow, oh)))


# ---------------------------------------------------------------------------------------------------------------- masks
def test_burned_area_mask_at_every_size_and_tail(gpu_ctx):
    import torch
    for n in P.MASK_SIZES:
        b = P.mask_bytes(n)
        t = torch.from_numpy(b).cuda()
        m = torch.full((n + 8,), 77, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()                              # the fill runs on torch's stream, the mask on the context's
        gpu_ctx.burned_area_mask_dev(t, m[:n])
        gpu_ctx.synchronize()
        got = m.cpu().numpy()
        np.testing.assert_array_equal(got[:n], (b <= 254).astype(np.uint8), err_msg=str(n))
        assert (got[n:] == 77).all(), f"n = {n}: written past the end"
    big = torch.zeros(64, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    with pytest.raises(wass_amd.WassError):
        gpu_ctx.burned_area_mask_dev(big[1:33], big[32:64])        # a misaligned picture is refused
    with pytest.raises(wass_amd.WassError):
        gpu_ctx.burned_area_mask_dev(big[0:32], big[33:64])        # and a misaligned mask


def test_camera_mask_with_either_input_missing(gpu_ctx):
    import torch
    lib, h = gpu_ctx._lib, gpu_ctx._h
    for n in (1, 5, 1023, 4100):
        img, fm = P.mask_bytes(n), P.file_mask_bytes(n)
        ti, tf = torch.from_numpy(img).cuda(), torch.from_numpy(fm).cuda()
        for use_img, use_file in ((True, False), (False, True), (True, True)):
            m = torch.full((n + 8,), 77, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            rc = lib.wass_camera_mask_dev(h, ti.data_ptr() if use_img else None, tf.data_ptr() if use_file else None, n, m.data_ptr())
            assert rc == 0
            gpu_ctx.synchronize()
            ref = np.ones(n, np.uint8)
            if use_file:
                ref = (fm != 0).astype(np.uint8)
            if use_img:
                ref = np.where(img > 254, 0, ref).astype(np.uint8)
            got = m.cpu().numpy()
            np.testing.assert_array_equal(got[:n], ref, err_msg=str((n, use_img, use_file)))
            assert (got[n:] == 77).all()
