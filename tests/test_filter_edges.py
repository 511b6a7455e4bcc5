"""The temporal filter's oracle and probes, without a GPU: tests/filter_oracle.py with an explicit padlen against
scipy.signal.sosfiltfilt bit for bit, the default padlen of every order, and the discriminating power of tests/filter_probes.py:
each known mistake (filter_oracle.VARIANTS) must miss the float32-rounded oracle on at least one cell of at least one probe at
every section count, or the equality that tests/test_filter_edges_gpu.py asserts would let it through.  The shares are printed."""
import functools

import numpy as np
import pytest

import filter_oracle as FO
import filter_probes as FP
from wass_amd import postproc as P

PADLENS = (0, 1, 7, 8, 9, None)


def _sos(order, band):
    bt, fc = FP.BANDS[band]
    return P.butter_sos(order, fc, bt, FP.FS)


def test_default_padlen_of_every_order():
    want = (6, 9, 12, 15, 18, 21, 24, 27, 30, 33, 36, 39)
    for order in range(1, 13):
        for band in FP.BANDS:
            sos = _sos(order, band)
            assert sos.shape == ((order + 1) // 2, 6)
            assert P.sos_padlen(sos) == FO.padlen(sos) == want[order - 1]
            assert FP.probe("levels", order).shape[0] == want[order - 1] + 9


@pytest.mark.parametrize("order", range(1, 13))
def test_oracle_with_padlen_against_scipy(order):
    """The same sections, the same float32 cube and the same steady state through scipy: the same bits at every padlen, in fp64
    already and so in float32.

    The steady state is scipy's own (zi=) because the oracle's and the package's closed form is not scipy's bit for bit and cannot
    be: scipy.signal.sosfilt_zi solves a 2 x 2 system with LAPACK, whose last bits depend on the BLAS build (of 120 designs,
    orders 1 to 12, the closed form gives scipy's bits in 33, an elimination with partial pivoting written out by hand in 96).
    With the closed form the float32 results differ from scipy's wherever the output is fp64 noise (order 2, high-pass 0.05 Hz,
    padlen 0: the last frames are 1e-11 with either sign); the two steady states are held to each other within the conditioning
    of that system, here for every order and in test_filters.py::test_padlen_and_zi against the recorded values."""
    signal = pytest.importorskip("scipy.signal")
    x = FO.series_cube(48, 2, 9, seed=order, offset=40.0)
    for band in FP.BANDS:
        sos = _sos(order, band)
        zi = signal.sosfilt_zi(sos)
        cond = np.max((1 + np.abs(sos[:, 4]) + np.abs(sos[:, 5])) / np.abs(1 + sos[:, 4] + sos[:, 5]))
        assert np.array_equal(P.sosfilt_zi(sos), FO.sosfilt_zi(sos))
        assert np.max(np.abs(FO.sosfilt_zi(sos) - zi)) <= 16 * cond * 2.0 ** -52 * np.max(np.abs(zi))
        for p in PADLENS:
            got = FO.sosfiltfilt(sos, x, padlen=p, zi=zi)
            ref = signal.sosfiltfilt(sos, x, axis=0, padlen=p)
            own = FO.sosfiltfilt(sos, x, padlen=p)
            assert got.dtype == ref.dtype == np.float64 and got.shape == ref.shape == x.shape
            print(f"order {order} {band} padlen {p}: with scipy's zi equal in fp64 in {100 * np.mean(got == ref):.2f} % of the elements; with the "
                  f"closed form in {100 * np.mean(own == ref):.2f} %, in float32 in {100 * np.mean(own.astype(np.float32) == ref.astype(np.float32)):.2f} %")
            assert np.array_equal(got, ref), (band, p)
            assert np.array_equal(got.astype(np.float32), ref.astype(np.float32)), (band, p)
        assert np.array_equal(FO.sosfiltfilt(sos, x), FO.sosfiltfilt(sos, x, padlen=FO.padlen(sos)))


def test_padlen_argument():
    sos = _sos(8, "lp1.0")
    x = FO.series_cube(40, 2, 3, seed=2)
    for bad in (40, 41, -1):
        with pytest.raises(ValueError):
            FO.sosfiltfilt(sos, x, padlen=bad)
    assert FO.sosfiltfilt(sos, x, padlen=39).shape == x.shape
    # padlen 0: no extension, the forward pass starts from zi times the first sample
    one = FO.sosfiltfilt(sos, x[:1], padlen=0)
    zi = FO.sosfilt_zi(sos).reshape(4, 2, 1, 1)
    fwd = FO._sosfilt(sos.copy(), x[:1].astype(np.float64), zi * x[:1].astype(np.float64))
    assert np.array_equal(one, FO._sosfilt(sos.copy(), fwd.copy(), zi * fwd))
    o64, n = FO.noise(sos, x, padlen=5)
    assert np.array_equal(o64, FO.sosfiltfilt(sos, x, padlen=5)) and 0 < n < 1e-9


def test_probes_are_what_they_say():
    tiny = float(np.finfo(np.float32).tiny)
    for order in (1, 12):
        lv = FP.probe("levels", order)
        assert lv.dtype == np.float32 and (lv == lv[:1]).all() and np.unique(lv[0]).size == FP.H * FP.W
        rp = FP.probe("levels_plus_ripple", order)
        assert 0 < np.max(np.abs(rp - lv)) < 1.0
        wd = FP.probe("wide", order)
        assert wd.shape[1:] == FP.WIDE_HW and (wd > 1e6).any() and (wd < -1e6).any() and (np.abs(wd) < 1e-2).any()
        sub = FP.probe("subnormal", order)
        assert (np.abs(sub) < tiny).all() and (sub > 0).any() and (sub < 0).any()
        inf = FP.probe("infinite", order)
        assert np.isposinf(inf).sum() == 1 and np.isneginf(inf).sum() == 1 and np.isinf(inf).any(axis=0).sum() == 2
        for band in FP.BANDS:
            sos = _sos(order, band)
            # the subnormal probe: padding and result are subnormal float32 numbers, most of them not zero, so that a kernel that
            # flushes float32 subnormals (in the padding or in the cast) returns other bits
            edge = FO.padlen(sos)
            pad = 2 * sub[:1] - sub[edge:0:-1]
            assert pad.dtype == np.float32 and (np.abs(pad) < 2 * tiny).all() and (pad != 0).mean() > 0.8
            out = FP.rounded(FO.sosfiltfilt(sos, sub))
            assert (np.abs(out) < 4 * tiny).all() and (out != 0).mean() > 0.5
            # the infinite probe: the two series are not finite from the first frame to the last, the others are untouched
            o = FP.rounded(FO.sosfiltfilt(sos, inf))
            clean = FP.rounded(FO.sosfiltfilt(sos, FO.series_cube(inf.shape[0], FP.H, FP.W, seed=100 + order)))
            bad = np.isinf(inf).any(axis=0)
            assert not np.isfinite(o[:, bad]).any() and np.array_equal(o[:, ~bad], clean[:, ~bad])


@functools.lru_cache(maxsize=None)
def _misses(order, band, name, variant):
    """(cells of the probe where the variant's float32 result is not the oracle's, cells)"""
    sos, x = _sos(order, band), FP.probe(name, order)
    rm = variant == "mean summed pairwise"
    ref = FP.rounded(FO.sosfiltfilt(sos, x, remove_mean=rm))
    got = FP.rounded(FO.sosfiltfilt(sos, x, remove_mean=rm, **FO.VARIANTS[variant]))
    return int((~((got == ref) | (np.isnan(got) & np.isnan(ref)))).sum()), ref.size


def _report(order, variant):
    hits = {}
    for band in FP.BANDS:
        for name in FP.PROBES:
            m, n = _misses(order, band, name, variant)
            if m:
                hits[f"{name} {band}"] = (m, n)
    print(f"order {order} (NS = {(order + 1) // 2}), {variant}: " + (", ".join(f"{k} {m} of {n}" for k, (m, n) in hits.items()) or "not told"))
    return hits


@pytest.mark.parametrize("ns", range(1, 7))
def test_every_variant_is_told_at_every_section_count(ns):
    """Per section count (orders 2 ns - 1 and 2 ns, low- and high-pass): each mistake changes at least one float32 output of at
    least one probe.  Beyond that, per ORDER: the contracted product and the fp64 padding are told at every order, the pairwise
    mean too; the re-associated update at every even order (levels through the high-pass) and at the odd orders from 3 on by the
    wide probe.  At order 1 the one section is of first order, its z1 is always 0 and (b1 x - a1 y) + 0 == b1 x + (0 - a1 y): there
    is no difference to tell."""
    told = {v: {} for v in FO.VARIANTS}
    for order in (2 * ns - 1, 2 * ns):
        for v in FO.VARIANTS:
            told[v][order] = _report(order, v)
    for v in FO.VARIANTS:
        assert any(told[v].values()), f"{v} is not told at NS = {ns}"
    for order in (2 * ns - 1, 2 * ns):
        assert any(k.startswith("levels hp") for k in told["contracted"][order])
        assert any(k.startswith("series") for k in told["padding in fp64"][order])
        assert told["mean summed pairwise"][order]
        if order % 2 == 0:
            assert any(k.startswith("levels hp") for k in told["reassociated"][order])
        elif order > 1:
            assert any(k.startswith("wide") for k in told["reassociated"][order])
        else:
            assert not told["reassociated"][order]


def test_variants_are_switched_off_by_default():
    sos, x = _sos(5, "hp0.05"), FP.probe("series", 5)
    base = FO.sosfiltfilt(sos, x, remove_mean=True)
    assert np.array_equal(base, FO.sosfiltfilt(sos, x, remove_mean=True, update="scipy", first="scipy", pad="input", mean="frames"))
    assert set(FO.VARIANTS) == {"reassociated", "contracted", "padding in fp64", "mean summed pairwise"}
    # the approximate fma rounds once where the plain expression rounds twice
    a, b, c = np.float64(1 + 2.0 ** -30), np.float64(1 - 2.0 ** -30), np.float64(-1.0)
    assert a * b + c == 0.0 and FO._fma(a, b, c) == -2.0 ** -60
