"""GPU parity of the SGM stage on scenes that carry information (sgm_scenes.py), for every NP and both path modes.

As test_sgm_gpu.test_stage_parity: debug mode on, C, S, the raw map and the final map bit for bit against the CPU oracle, then the
production-mode map against the debug-mode one -- but on volumes that are not saturated and maps that are mostly valid, with a
winner on every lane, slot and 128-disparity boundary, all sub-pixel fractions, exact ties, uniqueness rejections from far lanes and
both outcomes of the left-right check.  tests/test_sgm_scenes.py holds every case here to those conditions on the oracle alone.
All calls go through the C ABI.
"""
import numpy as np
import pytest

import wass_amd
from wass_amd import default_sgm_params

import sgm_scenes as sc

pytestmark = pytest.mark.gpu


def _parity(gpu_ctx, oracle, c):
    right, left, p, disp, st, Co, So, rawo = sc.run_oracle(oracle, c)
    h, w = right.shape
    gpu_ctx.set_debug(True)
    try:
        got = gpu_ctx.sgm_disparity(right, left, p)
        Cg, Sg, rawg = gpu_ctx.sgm_debug_fetch(w, h, p)
    finally:
        gpu_ctx.set_debug(False)
    assert not st.overflow
    assert Cg.shape == Co.shape
    np.testing.assert_array_equal(Cg, Co, err_msg="cost volume C")
    np.testing.assert_array_equal(Sg, So, err_msg="aggregated volume S")
    np.testing.assert_array_equal(rawg, rawo, err_msg="raw disparity (WTA/uniqueness/subpixel/LR)")
    np.testing.assert_array_equal(got, disp[:, c.D:c.D + w], err_msg="median + crop")
    # production mode (S never written) must give the same map
    np.testing.assert_array_equal(gpu_ctx.sgm_disparity(right, left, p), got)


def _ids(cases):
    return [c.id for c in cases]


@pytest.mark.parametrize("c", sc.selection_cases(), ids=_ids(sc.selection_cases()))
def test_selection_at_every_boundary(gpu_ctx, oracle, c):
    """terrace, left-right check off: every index of sgm_scenes.targets wins in valid pixels -- the winner's neighbours come from the
    lane before and the lane after, from the other half of the wave, from the next 128-disparity slot, or do not exist."""
    _parity(gpu_ctx, oracle, c)


@pytest.mark.parametrize("c", sc.subpixel_cases(), ids=_ids(sc.subpixel_cases()))
def test_subpixel_fractions(gpu_ctx, oracle, c):
    """smooth_terrace: all sixteen fractions of the sub-pixel division, on the same winners."""
    _parity(gpu_ctx, oracle, c)


@pytest.mark.parametrize("c", sc.periodic_cases(), ids=_ids(sc.periodic_cases()))
def test_ties_and_uniqueness(gpu_ctx, oracle, c):
    """periodic: exact ties (to the lower d), rejections by a d lanes away, and S * (100 - uniq) == 100 minS exactly."""
    _parity(gpu_ctx, oracle, c)


@pytest.mark.parametrize("c", sc.lrcheck_cases(), ids=_ids(sc.lrcheck_cases()))
def test_left_right_check(gpu_ctx, oracle, c):
    """terrace with the check on: the stairs' occlusions make it reject over half of the map and keep over a tenth."""
    _parity(gpu_ctx, oracle, c)


@pytest.mark.parametrize("c", sc.steady_cases(), ids=_ids(sc.steady_cases()))
def test_steady_state_schedule_on_unsaturated_volumes(gpu_ctx, oracle, c):
    """Half chains of two or more full checkpoint segments (the heights of test_sgm_gpu.CASES and _FUSED5_CASES) over smooth_terrace."""
    _parity(gpu_ctx, oracle, c)


@pytest.mark.parametrize("NP", range(1, 9))
def test_constant_pair_every_np(gpu_ctx, oracle, NP):
    """A black pair: S is flat over all D slots, beside padded ones (D is no multiple of 128), and d = 0 wins exactly where the oracle
    says so.  A grey pair (test_sgm_gpu.test_constant_images at D = 16) adds the step against the zero padding."""
    D = 128 * NP - 48
    for grey in (0, 77):
        img = np.full((12, D + 40), grey, np.uint8)
        R, L = sc.pad(img, img, D)
        for ndirs in (5, 8):
            p = default_sgm_params(D, ndirs=ndirs)
            gpu_ctx.set_debug(True)
            try:
                got = gpu_ctx.sgm_disparity(img, img, p)
                _, Sg, rawg = gpu_ctx.sgm_debug_fetch(img.shape[1], img.shape[0], p, want=("S", "raw"))
            finally:
                gpu_ctx.set_debug(False)
            disp, st, Co, So, rawo = oracle.sgbm_compute(R, L, sc.oracle_params(oracle, p), dump=True)
            assert not st.overflow
            if grey == 0:
                # the tie is real: S is flat over d in every pixel -- zero, where index 0 takes it, but for the last columns, whose
                # windows hold the pre-filter's border value: a tie above zero, which the uniqueness test rejects
                assert (So.max(-1) == So.min(-1)).all()
                np.testing.assert_array_equal(rawo[:, D + 1:] == 16, So.max(-1) == 0)
                assert 0 < (So.max(-1) > 0).sum() <= 7 * 12
            np.testing.assert_array_equal(Sg, So)
            np.testing.assert_array_equal(rawg, rawo)
            np.testing.assert_array_equal(got, disp[:, D:D + img.shape[1]])
            assert set(np.unique(rawg)) == {0, 16}                                       # invalid, or index 0 (min_disp = 1)


@pytest.mark.parametrize("uniq", [99, 100, 101, 150])
def test_uniq_ratio_up_to_100_and_refused_above(gpu_ctx, oracle, uniq):
    """The selection kernels form S * (100 - uniq) as an unsigned 24-bit product, which is the reference's product only for a factor
    that is not negative.  Measured before the refusal existed (periodic, D = 160): at uniq_ratio 101 and at 150 alike the library
    accepted 19 pixels with 8 paths and 24 with 5 where the reference accepts none (at 99 and 100 the maps were equal, 743 and 503
    valid pixels with 8 paths).  The entry points refuse such a ratio; up to 100 the map equals the oracle's."""
    c = sc.Case("periodic", "periodic", 160, 20, 8, 3, 1, uniq, sc.LR_OFF, 0)
    if uniq <= 100:
        _parity(gpu_ctx, oracle, c)
        return
    right, left = sc.make(c)
    with pytest.raises(wass_amd.WassError) as e:
        gpu_ctx.sgm_disparity(right, left, sc.sgm_params(c))
    assert e.value.code == -1 and "uniq" in str(e.value).lower()
    import torch
    with pytest.raises(wass_amd.WassError) as e:                  # and the device-pointer entry point
        gpu_ctx.sgm_disparity_dev(torch.from_numpy(right).cuda(), torch.from_numpy(left).cuda(), sc.sgm_params(c))
    assert e.value.code == -1
