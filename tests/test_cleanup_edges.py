"""The references and probes of the clean-up edge suite on the CPU.  Three things are held in place here, so that what
tests/test_cleanup_edges_gpu.py compares the kernels with can be trusted:
  * the C oracle (oracle/wass_oracle.c, oracle/a9_oracle.c) equals the direct-form restatement (tests/cleanup_oracle.py) bit for bit
    on every probe -- two texts by different routes;
  * every wrong variant of the restatement (the mistakes a kernel could make) differs from the right answer on the probes named
    for it, so the probes can tell them apart -- the counts are printed;
  * the probes have the properties they are built for (component counts, ties, cells on both sides of every tile seam).
The C oracle has no median: the restatement's is compared with scipy.ndimage.median_filter instead."""
import ctypes as C

import numpy as np
import pytest
from scipy import ndimage

import cleanup_oracle as R
import cleanup_probes as P

ids = lambda c: "x".join(str(v) for v in c) if isinstance(c, tuple) else str(c)
ND, MD = P.NUMDISP, P.MINDISP


def _differs(name, probe, right, wrong):
    n = int((np.asarray(right) != np.asarray(wrong)).sum())
    print(f"variant {name:>18} on {probe}: {n} cells differ")
    assert n > 0, f"{name} cannot be told from the right answer on {probe}"
    return n


# ---------------------------------------------------------------------------------------------------------------- the chain
def test_lds_sizes_of_the_last_fused_and_the_first_stepwise_setting():
    """two float32 buffers of (64 + hl + hr) x (32 + 2 hv) cells against 64 KiB"""
    assert R.chain_halo(9, 9, 5) == (12, 30, 21) and R.chain_lds_bytes(9, 9, 5) == 106 * 74 * 8 == 62752 <= 64 * 1024
    assert R.chain_halo(10, 9, 5) == (12, 32, 22) and R.chain_lds_bytes(10, 9, 5) == 108 * 76 * 8 == 65664 > 64 * 1024
    for st in P.STEPS[:-1]:
        assert R.chain_lds_bytes(*st) <= 64 * 1024


@pytest.mark.parametrize("shape", P.SHAPES, ids=ids)
def test_single_steps_equal_the_c_oracle(oracle, shape):
    w, h = shape
    for frac in P.HOLE_FRACTIONS:
        d = P.random_holes(w, h, frac)
        for md in P.MIN_DISPS:
            for off in (0, 3):
                for scale in (1.0, 1.0 / 0.73):
                    np.testing.assert_array_equal(R.convert(d, md, ND, off, scale), oracle.clean_and_convert(d, md, ND, off, scale))
        a = R.convert(d, MD, ND, 0, 1.0 / 0.73)
        for _ in range(3):
            np.testing.assert_array_equal(R.dilate(a), oracle.dilate_zero(a))
            np.testing.assert_array_equal(R.erode(a), oracle.erode_zero(a))
            a = R.dilate(a)


@pytest.mark.parametrize("shape", P.SHAPES, ids=ids)
def test_chain_equals_the_c_oracle_and_its_tiled_form(oracle, shape):
    w, h = shape
    n = 0
    for frac in P.HOLE_FRACTIONS:
        d = P.random_holes(w, h, frac)
        for nd, ne, med in P.STEPS:
            ref = R.chain(d, MD, ND, 0, 1.0, nd, ne, 0)
            np.testing.assert_array_equal(ref, oracle.disparity_postprocess(d, MD, ND, 0, nd, ne))
            np.testing.assert_array_equal(ref, oracle.disparity_postprocess_ex(d, MD, ND, w, h, 0, 1.0, nd, ne))
            if frac == 0.20 and nd < 9:
                np.testing.assert_array_equal(R.chain(d, MD, ND, 0, 1.0, nd, ne, med, tile=P.TILE), R.chain(d, MD, ND, 0, 1.0, nd, ne, med))
            n += 1
    d = P.random_holes(w, h, 0.20)
    for off in P.OFFSETS:
        for md in P.MIN_DISPS:
            np.testing.assert_array_equal(R.chain(d, md, ND, max(off, 0), 1.0, 1, 2, 0), oracle.disparity_postprocess(d, md, ND, max(off, 0), 1, 2))
    np.testing.assert_array_equal(R.chain(d, MD, ND, 0, 1.0 / 0.73, 1, 2, 0), oracle.disparity_postprocess_ex(d, MD, ND, w, h, 0, 0.73, 1, 2))
    print(f"{w}x{h}: {n} chain cases")


@pytest.mark.parametrize("shape", P.LATTICE_SHAPES, ids=ids)
def test_seam_lattice_equals_the_c_oracle_and_has_cells_of_both_kinds_on_every_seam(oracle, shape):
    """Inside every 5-cell band around every tile seam the lattice's result has zero and non-zero cells.  Up to three dilations this
    holds without the picture's own border (the band is cut by what the border zeroes: ne + 1 + med/2 + 1 cells), because the
    lattice grows its holes by what the dilations close; nine dilations close everything, and the zeros are the border's.  The
    inverse lattice is thin by construction: whatever the dilations make of it is narrower than 2 (ne + 1) + 1 unless
    nd > ne + 1, so its result is asserted to be all zero except at (3, 0, 5), where the bands must hold non-zero cells."""
    w, h = shape
    for st in P.STEPS:
        nd, ne, med = st
        d = P.seam_lattice(w, h, st)
        ref = R.chain(d, MD, ND, 0, 1.0, nd, ne, 0)
        np.testing.assert_array_equal(ref, oracle.disparity_postprocess(d, MD, ND, 0, nd, ne))
        ref = R.chain(d, MD, ND, 0, 1.0, nd, ne, med)
        cut = ne + 2 + (med // 2 if med >= 3 else 0) if nd <= 3 else 0
        strip = ne + 1 + 2 * (med // 2 if med >= 3 else 0)        # what the picture's border zeroes, and the median's reach into it
        for X in P.seams(w, P.TILE[0]):
            if X - 2 >= w - strip:                              # the last tile is one column wide: its seam can lie in that strip,
                continue                                        # where nothing can be non-zero
            c = cut if X + 2 < w - cut else 0
            band = ref[c:h - c, X - 2:X + 3]
            assert band.size and (band == 0).any() and (band != 0).any(), (st, "x", X)
        for Y in P.seams(h, P.TILE[1]):
            if Y - 2 >= h - strip:
                continue
            c = cut if Y + 2 < h - cut else 0
            band = ref[Y - 2:Y + 3, c:w - c]
            assert band.size and (band == 0).any() and (band != 0).any(), (st, "y", Y)
        inv = P.seam_lattice_inverse(w, h)
        ri = R.chain(inv, MD, ND, 0, 1.0, nd, ne, 0)
        np.testing.assert_array_equal(ri, oracle.disparity_postprocess(inv, MD, ND, 0, nd, ne))
        ri = R.chain(inv, MD, ND, 0, 1.0, nd, ne, med)
        if st == (3, 0, 5):
            for X in P.seams(w, P.TILE[0]):
                if X - 2 < w - strip:
                    assert (ri[:, X - 2:X + 3] != 0).any() and (ri[:, X - 2:X + 3] == 0).any()
        else:
            assert not ri.any(), st
        # what the dilations alone make of the inverse is not trivial: some cells are filled, most are not
        if nd:
            a = R.convert(inv, MD, ND)
            b = R.dilate(a)
            assert 0 < int(((b != 0) & (a == 0)).sum()) < a.size // 4


@pytest.mark.parametrize("shape", P.LATTICE_SHAPES, ids=ids)
def test_a_halo_one_cell_short_shows_on_the_seam_lattice(shape):
    """Each of the three halo widths in turn one cell short, and the median clamped to the tile: asserted for every setting of up to
    three dilations (the lattice's halo-edge holes are made for the setting), printed for the two of nine and ten."""
    w, h = shape
    for st in P.STEPS:
        nd, ne, med = st
        d = P.seam_lattice(w, h, st)
        ref = R.chain(d, MD, ND, 0, 1.0, nd, ne, med)
        np.testing.assert_array_equal(R.chain(d, MD, ND, 0, 1.0, nd, ne, med, tile=P.TILE), ref)
        hl, hr, hv = R.chain_halo(*st)
        for side, halo in (("left", (hl - 1, hr, hv)), ("right", (hl, hr - 1, hv)), ("rows", (hl, hr, hv - 1))):
            got = R.chain(d, MD, ND, 0, 1.0, nd, ne, med, tile=P.TILE, halo=halo)
            n = int((got != ref).sum())
            print(f"variant halo short {side:>5} on lattice {w}x{h} {st}: {n} cells differ")
            assert n > 0 or nd > 3, (st, side)
        if med:
            got = R.chain(d, MD, ND, 0, 1.0, nd, ne, med, tile=P.TILE, variant="median_tile_clamp")
            _differs("median_tile_clamp", f"lattice {w}x{h} {st}", ref, got)


def test_wrong_chain_steps_show_on_their_probes():
    for w, h in P.LATTICE_SHAPES:
        inv = R.convert(P.seam_lattice_inverse(w, h), MD, ND)
        r20 = R.convert(P.random_holes(w, h, 0.20), MD, ND)
        r50 = R.convert(P.random_holes(w, h, 0.50), MD, ND)
        for name, a in (("inverse lattice", inv), ("20 % holes", r20), ("50 % holes", r50)):
            _differs("centre_k", f"{name} {w}x{h}", R.dilate(a), R.dilate(a, "centre_k"))
            if a is not r20:                                    # a hole with exactly one valid neighbour: not among 20 % holes
                _differs("ge1", f"{name} {w}x{h}", R.dilate(a), R.dilate(a, "ge1"))
        lat = P.seam_lattice(w, h)
        a = R.convert(lat, MD, ND)
        _differs("four", f"lattice {w}x{h}", R.erode(a), R.erode(a, "four"))
        _differs("four", f"50 % holes {w}x{h}", R.erode(r50), R.erode(r50, "four"))
        for st in ((0, 0, 0), (1, 2, 3)):
            d = P.seam_lattice(w, h, st)
            _differs("skip", f"lattice {w}x{h} {st}", R.chain(d, MD, ND, 0, 1.0, *st), R.chain(d, MD, ND, 0, 1.0, *st, variant="skip"))
        # values that are no multiples of 1/16: the order of the eight additions shows
        d = P.random_holes(w, h, 0.20)
        _differs("sorted", f"20 % holes {w}x{h} at DENSE_SCALE 0.73", R.chain(d, MD, ND, 0, 1 / 0.73, 1, 2, 0),
                 R.chain(d, MD, ND, 0, 1 / 0.73, 1, 2, 0, variant="sorted"))
        # ... and at scale 1 it cannot: every value is a multiple of 1/16 below 2^11, every partial sum exact
        np.testing.assert_array_equal(R.chain(d, MD, ND, 0, 1.0, 1, 2, 0), R.chain(d, MD, ND, 0, 1.0, 1, 2, 0, variant="sorted"))


def test_median_is_the_middle_value_with_a_replicated_border():
    for name, d in P.median_maps().items():
        a = R.convert(d, MD, ND)
        for ks in (3, 5):
            np.testing.assert_array_equal(R.median(a, ks), ndimage.median_filter(a, size=ks, mode="nearest"), err_msg=f"{name} {ks}")
    ties = R.convert(P.median_maps()["ties"], MD, ND)
    assert len(np.unique(ties)) == 3
    z = R.chain(P.median_maps()["zeros"], MD, ND, 0, 1.0, 0, 0, 3)
    assert 0.1 < (z == 0).mean() < 0.9


# ---------------------------------------------------------------------------------------------------------------- components
@pytest.mark.parametrize("shape", P.COMPONENT_SHAPES, ids=ids)
def test_component_maps_are_what_they_say_and_equal_the_c_oracle(oracle, shape):
    w, h = shape
    for name, make in P.COMPONENT_MAPS.items():
        f = make(w, h)
        ref, area, lg = R.biggest_component(f, P.COMPONENT_THR)
        assert not lg.any()
        lab, areas = R.label_components(f != 0)
        ncomp, big = P.component_expect(name, w, h)
        assert len(areas) - 1 == ncomp, (name, len(areas) - 1)
        if big is None:
            big = int((f != 0).sum())
        assert area == big, (name, area, big)
        got, oarea = oracle.biggest_component_by_gradient(f, P.COMPONENT_THR)
        np.testing.assert_array_equal(ref, got, err_msg=name)
        assert oarea == area
        print(f"{name} {w}x{h}: {ncomp} components, kept {area}")
    # the tie maps really tie, and the first in raster order is kept although the other starts further left
    f = P.comp_two_equal(w, h)
    lab, areas = R.label_components(f != 0)
    assert areas[1] == areas[2] and np.argwhere(lab == 1)[0][1] > np.argwhere(lab == 2)[0][1]
    assert (R.biggest_component(f, P.COMPONENT_THR)[0] != 0).sum() == areas[1] and R.biggest_component(f, P.COMPONENT_THR)[0][1, w - 4] != 0
    f = P.comp_row_end(w, h)
    assert list(R.label_components(f != 0)[1]) == [0, 1, 1]


def test_wrong_component_rules_show_on_their_probes():
    T = P.COMPONENT_THR
    for w, h in P.COMPONENT_SHAPES[:5]:
        for name in ("diagonal", "antidiagonal", "checkerboard"):
            f = P.COMPONENT_MAPS[name](w, h)
            _differs("four-connected", f"{name} {w}x{h}", R.biggest_component(f, T)[0], R.biggest_component(f, T, "four")[0])
        for name in ("two_equal", "row_end"):
            f = P.COMPONENT_MAPS[name](w, h)
            _differs("tie_last", f"{name} {w}x{h}", R.biggest_component(f, T)[0], R.biggest_component(f, T, "tie_last")[0])
        f = P.comp_row_end(w, h)
        _differs("row_wrap", f"row_end {w}x{h}", R.biggest_component(f, T)[0], R.biggest_component(f, T, "row_wrap")[0])


def test_sobel_probes(oracle):
    ramp = P.sobel_ramp()
    h, w = ramp.shape
    keep = lambda f, thr, v=None: R.biggest_component(f, thr, v)[0]
    for thr in (100, 575, 576):
        np.testing.assert_array_equal(keep(ramp, thr), oracle.biggest_component_by_gradient(ramp, thr)[0])
    # interior: gx = 8 * 3, 576; columns 0 and w-1: reflect-101 makes c - a zero, so they survive and tie; the first wins
    assert (keep(ramp, 100) != 0).sum() == h and (keep(ramp, 100)[:, 0] != 0).all()
    assert (keep(ramp, 576) != 0).all() and (keep(ramp, 575) != 0).sum() == h
    _differs("replicate", "ramp 3x+5", R.large_gradient(ramp, 100), R.large_gradient(ramp, 100, "replicate"))
    _differs("ge", "ramp 3x+5 at 576", R.large_gradient(ramp, 576), R.large_gradient(ramp, 576, "ge"))
    for s in (3.0, 2.5):
        f = P.sobel_step(s)
        thr = int(16 * s * s)
        assert thr == 16 * s * s
        assert not R.large_gradient(f, thr).any() and R.large_gradient(f, thr - 1).sum() == 2 * f.shape[0]
        _differs("ge", f"step {s} at 16 s^2", R.large_gradient(f, thr), R.large_gradient(f, thr, "ge"))
        for t in (thr, thr - 1):
            np.testing.assert_array_equal(keep(f, t), oracle.biggest_component_by_gradient(f, t)[0])


# ---------------------------------------------------------------------------------------------------------------- speckles
def test_speckle_probes_equal_the_c_oracle_and_catch_their_variants(oracle):
    pr = P.speckle_probes()
    for name, (img, nv, ms, mdiff) in pr.items():
        ref = R.filter_speckles(img, nv, ms, mdiff)
        np.testing.assert_array_equal(ref, oracle.filter_speckles(img, nv, ms, mdiff), err_msg=name)
    img, nv, ms, mdiff = pr["exact_size"]
    ref = R.filter_speckles(img, nv, ms, mdiff)
    assert (ref[2:5, 2:6] == nv).all() and (ref[7:10, 2:6] == 160).all()              # 12 go, 13 stay
    _differs("lt", "exact_size", ref, R.filter_speckles(img, nv, ms, mdiff, "lt"))
    c16, c15 = R.filter_speckles(*pr["chain16"]), R.filter_speckles(*pr["chain15"])
    assert (c16 == pr["chain16"][0]).all() and (c15 == -16).all()                       # one region of 9 > 8 stays; nine of 1 go
    img, nv, ms, mdiff = pr["diagonal"]
    ref = R.filter_speckles(img, nv, ms, mdiff)
    assert (ref == nv).all()
    _differs("eight", "diagonal", ref, R.filter_speckles(img, nv, ms, mdiff, "eight"))
    img, nv, ms, mdiff = pr["split"]
    assert (R.filter_speckles(img, nv, ms, mdiff) == nv).all()                          # two halves of 35 <= 40; joined they would be 70
    for name in ("extremes", "extremes_big"):
        img, nv, ms, mdiff = pr[name]
        ref = R.filter_speckles(img, nv, ms, mdiff)
        assert (ref == nv).all()
    img, nv, ms, mdiff = pr["extremes"]
    e13 = R.filter_speckles(img, nv, 11, mdiff)
    assert (e13 == img).all()
    _differs("wrap16", "extremes", R.filter_speckles(img, nv, 12, mdiff), R.filter_speckles(img, nv, 12, mdiff, "wrap16"))


@pytest.mark.parametrize("shape", P.COMPONENT_SHAPES[:5], ids=ids)
def test_component_maps_as_speckle_pictures_equal_the_c_oracle(oracle, shape):
    w, h = shape
    for name, make in P.COMPONENT_MAPS.items():
        img = P.as_int16(make(w, h))
        ref = R.filter_speckles(img, 0, 7, 0)
        np.testing.assert_array_equal(ref, oracle.filter_speckles(img, 0, 7, 0), err_msg=name)
    f = P.as_int16(P.comp_row_end(w, h))
    assert (R.filter_speckles(f, 0, 1, 0) == 0).all() and (R.filter_speckles(f, 0, 0, 0) == f).all()


# ---------------------------------------------------------------------------------------------------------------- resizers
def _orc_resize_u8(oracle, src, dw, dh):
    src = np.ascontiguousarray(src, np.uint8)
    sh, sw = src.shape
    out = np.empty((dh, dw), np.uint8)
    oracle.lib().orc_resize_cubic_u8(src.ctypes.data_as(C.POINTER(C.c_uint8)), sw, sh, out.ctypes.data_as(C.POINTER(C.c_uint8)), dw, dh,
                                     C.c_double(sw / dw), C.c_double(sh / dh))
    return out


def test_resizers_equal_the_c_oracle(oracle):
    n = 0
    for sw, sh, dw, dh in P.resize_cases():
        src = P.picture(sw, sh)
        np.testing.assert_array_equal(R.resize_cubic_u8(src, dw, dh, sw / dw, sh / dh), _orc_resize_u8(oracle, src, dw, dh), err_msg=str((sw, sh, dw, dh)))
        f = (src.astype(np.float32) / np.float32(7.0)).astype(np.float32)
        for cubic in (False, True):
            np.testing.assert_array_equal(R.resize_f32(f, dw, dh, cubic), oracle.resize_f32(f, dw, dh, cubic), err_msg=str((sw, sh, dw, dh, cubic)))
        n += 1
    for sw, sh in P.RESIZE_SOURCES:
        src = P.picture(sw, sh)
        for fx, fy in P.RESIZE_FACTORS:
            dw, dh = oracle.resize_dsize(sw, sh, fx, fy)
            if dw > 0 and dh > 0:
                np.testing.assert_array_equal(R.resize_cubic_u8(src, dw, dh, 1.0 / fx, 1.0 / fy), oracle.resize_cubic_u8(src, fx, fy))
                n += 1
    print(f"{n} resize cases")
    src = P.picture(97, 61)
    for dw, dh in ((133, 84), (194, 61), (513, 33)):
        _differs("no_right_clamp", f"97x61 -> {dw}x{dh}", R.resize_cubic_u8(src, dw, dh, 97 / dw, 61 / dh),
                 R.resize_cubic_u8(src, dw, dh, 97 / dw, 61 / dh, "no_right_clamp"))


def test_postprocess_ex_with_a_resize_equals_the_c_oracle(oracle):
    for ws, hs, scale, ow, oh in P.float_resize_cases():
        d = P.random_holes(ws, hs, 0.05)
        ref = R.postprocess_ex(d, MD, ND, 0, scale, 0, 0, 0, ow, oh)
        np.testing.assert_array_equal(ref, oracle.disparity_postprocess_ex(d, MD, ND, ow, oh, 0, scale, 0, 0), err_msg=str((ws, hs, scale)))
        if (ws, hs) == (97, 61):
            assert 0.2 < (ref != 0).mean() < 1.0
            ref = R.postprocess_ex(d, MD, ND, 0, scale, 1, 2, 0, ow, oh, cc_threshold=30)
            np.testing.assert_array_equal(ref, oracle.disparity_postprocess_ex(d, MD, ND, ow, oh, 0, scale, 1, 2, 30))


# ---------------------------------------------------------------------------------------------------------------- masks
def test_mask_bytes_cover_the_three_values_at_every_position():
    for n in P.MASK_SIZES:
        b = P.mask_bytes(n)
        assert b.shape == (n,)
    b = P.mask_bytes(4100)
    for v in (253, 254, 255):
        assert {int(i) % 4 for i in np.flatnonzero(b == v)} == {0, 1, 2, 3}
    assert set(np.unique(P.file_mask_bytes(64))) == {0, 1, 255}
