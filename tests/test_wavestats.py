"""Wave-by-wave statistics without a GPU: the numpy oracle (tests/wavestats_oracle.py) checked by independent means, the argument
errors and the scratch formula of the library, and every hand-built probe (tests/wavestats_probes.py) against the mistake it is
there to catch: a deliberately broken model must differ from the specification on it."""
import ctypes as C

import numpy as np
import pytest

import wavestats_oracle as WO
import wavestats_probes as WP
from wass_amd import postproc as P

EPS = np.finfo(np.float64).eps


def test_field_names_agree():
    assert WO.FIELDS == P.WAVE_FIELDS


# ---- the oracle, by independent means ------------------------------------------------------------------------------------------
def test_oracle_crossings_against_the_sign_pattern():
    z = WP.random_cube(300, 2, 5, seed=1)
    z[17, 0, 0] = z[40, 1, 3] = 0.0                      # exact zeros count as positive
    ds, dt = 0.5, 0.25
    for crossing, sign in (("up", 1.0), ("down", -1.0)):
        ref = WO.wave_stats(z, dt, datascale=ds, crossing=crossing, demean=False)
        for r in range(2):
            for c in range(5):
                e = sign * (z[:, r, c].astype(np.float64) * ds)
                neg = e < 0
                at = np.nonzero(neg[:-1] & ~neg[1:])[0]
                assert ref["n_cross"][r, c] == len(at) and ref["n_waves"][r, c] == len(at) - 1
                tau = at + e[at] / (e[at] - e[at + 1])
                assert np.array_equal(ref["T"][:len(at) - 1, r, c], np.diff(tau) * dt)
                heights = np.array([e[a + 1:b + 1].max() - e[a + 1:b + 1].min() for a, b in zip(at[:-1], at[1:])])
                assert np.array_equal(ref["H"][:len(at) - 1, r, c], heights)
                assert np.isnan(ref["H"][len(at) - 1:, r, c]).all()
                third = np.sort(heights)[::-1][:(len(heights) + 2) // 3]
                assert ref["h_13"][r, c] == pytest.approx(third.mean(), rel=64 * EPS)
                assert ref["h_max"][r, c] == heights.max()
                assert ref["t_hmax"][r, c] == (np.diff(tau) * dt)[np.argmax(heights)]
                assert ref["t_z"][r, c] == pytest.approx(np.diff(tau).mean() * dt, rel=1e-12)


def test_oracle_on_a_sampled_sinusoid():
    """z = A sin(w t): every period is P and every height 2 A, up to the sampling.  The crossing of the chord between two samples
    lies where |f| <= max|f''| dt^2 / 8 <= A w^2 dt^2 / 8, and |f'| >= A w cos(w dt) within a step of the true crossing, so a crossing is
    off by at most w dt^2 / (8 cos(w dt)) and a period by twice that; the float32 rounding of the two samples, A 2^-24 each, moves
    the chord's root by at most 2 A 2^-24 / (A w cos(w dt)) more.  The sample nearest a crest is within dt / 2 of it, so a
    height lies between 2 A cos(w dt / 2) and 2 A, give or take the same rounding."""
    A, period, dt, count = 1.25, 7.3, 0.5, 600
    w = 2 * np.pi / period
    t = np.arange(count) * dt
    z = (A * np.sin(w * t + 0.4)).astype(np.float32).reshape(count, 1, 1)
    ref = WO.wave_stats(z, dt, demean=False)
    nw = int(ref["n_waves"][0, 0])
    assert nw == int((t[-1] - (period - 0.4 / w)) // period)        # the first up-crossing is at period - 0.4 / w
    bound = 2 * (w * dt * dt / (8 * np.cos(w * dt)) + 2 * 2.0 ** -24 / (w * np.cos(w * dt)))
    T, Hk = ref["T"][:nw, 0, 0], ref["H"][:nw, 0, 0]
    print("largest period error", np.abs(T - period).max(), "bound", bound)
    assert np.abs(T - period).max() <= bound
    lo, hi = 2 * A * np.cos(w * dt / 2) - 4 * A * 2.0 ** -24, 2 * A * (1 + 2.0 ** -23)
    assert (Hk >= lo).all() and (Hk <= hi).all()
    for name in ("t_z", "t_13", "t_hmax"):
        assert abs(ref[name][0, 0] - period) <= bound
    for name in ("h_13", "h_mean", "h_max", "h_rms"):
        assert lo <= ref[name][0, 0] <= hi
    assert ref["hs_m0"][0, 0] == pytest.approx(4 * A / np.sqrt(2), rel=0.02)      # a few periods short of whole ones


def test_oracle_moments_against_numpy_and_scipy():
    from scipy import stats
    z = WP.random_cube(500, 2, 3, seed=2)
    ds = 1e-3
    ref = WO.wave_stats(z, 1.0, datascale=ds)
    count = z.shape[0]
    for r in range(2):
        for c in range(3):
            x = z[:, r, c].astype(np.float64)
            e = (x - x.mean()) * ds
            tol = 8 * count * EPS                        # a sum of count terms, a few roundings each
            assert ref["mean"][r, c] == pytest.approx(x.mean() * ds, rel=tol, abs=tol * np.abs(x).mean() * ds)
            for k, name in ((2, "m2"), (3, "m3"), (4, "m4")):
                assert ref[name][r, c] == pytest.approx(np.mean(e ** k), abs=tol * np.mean(np.abs(e) ** k))
            sig = np.sqrt(np.mean(e ** 2))
            assert ref["skewness"][r, c] == pytest.approx(stats.skew(e), abs=4 * tol * np.mean(np.abs(e) ** 3) / sig ** 3)
            assert ref["kurtosis"][r, c] == pytest.approx(stats.kurtosis(e, fisher=False), rel=8 * tol)
            assert ref["eta_max"][r, c] == pytest.approx(e.max(), abs=tol * np.abs(e).max())
            assert ref["eta_min"][r, c] == pytest.approx(e.min(), abs=tol * np.abs(e).max())
            assert ref["hs_m0"][r, c] == pytest.approx(4 * sig, rel=tol)


def test_oracle_invalid_cells_and_down_crossings():
    z = WP.random_cube(64, 2, 4, seed=3)
    ref0 = WO.wave_stats(z, 0.5, hist_bins=8, hist_width=0.4)
    z2 = z.copy()
    z2[5, 0, 1], z2[63, 1, 2] = np.nan, np.inf
    ref = WO.wave_stats(z2, 0.5, hist_bins=8, hist_width=0.4)
    bad = np.zeros((2, 4), bool)
    bad[0, 1] = bad[1, 2] = True
    for name in WO.FIELDS + ("sigma", "hs_m0", "skewness", "kurtosis", "h_rms"):
        assert np.isnan(ref[name][bad]).all() and np.array_equal(ref[name][~bad], ref0[name][~bad])
    assert (ref["n_cross"][bad] == -1).all() and (ref["n_waves"][bad] == -1).all()
    assert ref["hist"].sum() == ref["n_waves"][~bad].sum() and ref0["hist"].sum() == ref0["n_waves"].sum()
    dn, up = WO.wave_stats(z, 0.5, crossing="down"), WO.wave_stats(-z, 0.5)
    for name in WO.FIELDS:
        want = {"mean": -up["mean"], "m3": -up["m3"], "eta_max": -up["eta_min"], "eta_min": -up["eta_max"]}.get(name, up[name])
        assert np.array_equal(dn[name], want, equal_nan=True), name
    assert np.array_equal(dn["n_cross"], up["n_cross"])


# ---- the library without a GPU --------------------------------------------------------------------------------------------------
def test_argument_errors():
    z = np.zeros((8, 2, 2), np.float32)
    for kw in (dict(dt=0.0), dict(dt=-1.0), dict(dt=np.inf), dict(dt=np.nan), dict(dt=1.0, datascale=np.inf), dict(dt=1.0, datascale=np.nan),
               dict(dt=1.0, crossing="both"), dict(dt=1.0, hist_bins=4), dict(dt=1.0, hist_bins=4, hist_width=-1.0), dict(dt=1.0, hist_bins=-1),
               dict(dt=1.0, slab_rows=-1)):
        with pytest.raises(ValueError):
            P.wave_statistics(z, **kw)
        with pytest.raises(ValueError):
            P.wave_statistics_scratch_bytes(8, 2, 2, **kw)
    with pytest.raises(ValueError):
        P.wave_statistics(np.zeros((8, 2), np.float32), 1.0)
    with pytest.raises(ValueError):
        P.wave_statistics(np.zeros((0, 2, 2), np.float32), 1.0)
    with pytest.raises(ValueError):
        P.wave_statistics_scratch_bytes(0, 2, 2)


def test_scratch_entry_rejects_bad_arguments():
    from wass_amd import _lib
    lib = _lib.load()
    b, r = C.c_size_t(), C.c_int()
    good = dict(count=8, H=2, W=2, dt=1.0, datascale=1.0, crossing=0, hist_bins=0, hist_width=0.0, slab_rows=0, host=1)
    assert lib.wass_wavestats_scratch_bytes(*good.values(), C.byref(b), C.byref(r)) == 0
    for bad in (dict(count=0), dict(H=0), dict(W=0), dict(dt=0.0), dict(dt=-1.0), dict(dt=float("inf")), dict(dt=float("nan")),
                dict(datascale=float("inf")), dict(datascale=float("nan")), dict(crossing=2), dict(crossing=-1), dict(hist_bins=4),
                dict(hist_bins=4, hist_width=-1.0), dict(hist_bins=-1), dict(slab_rows=-1)):
        args = dict(good, **bad)
        assert lib.wass_wavestats_scratch_bytes(*args.values(), C.byref(b), C.byref(r)) == -1, bad
    assert lib.wass_wavestats_scratch_bytes(*good.values(), None, C.byref(r)) == -1


def _align(v):
    return (v + 255) // 256 * 256


def _scratch(count, rows, W, host, bins):
    total = _align(2 * (count // 2) * rows * W * 8)
    if host:
        total += _align(count * rows * W * 4) + _align(13 * rows * W * 8) + _align(rows * W * 4) + _align(bins * 8)
    return max(total, 256)


@pytest.mark.parametrize("host", [True, False])
def test_scratch_formula(host):
    for count, H, W, bins, slab in ((1, 1, 1, 0, 0), (2, 3, 5, 0, 0), (9, 3, 65, 16, 0), (4099, 3, 257, 0, 2), (1000, 1024, 1024, 64, 0),
                                    (1000, 1024, 1024, 0, 100)):
        got, rows = P.wave_statistics_scratch_bytes(count, H, W, hist_bins=bins, hist_width=1.0, slab_rows=slab, host=host)
        per_row = (2 * (count // 2) * 8 + ((count * 4 + 13 * 8 + 4) if host else 0)) * W
        most = H if per_row == 0 else min(H, ((16 << 30) - 2048 - (_align(bins * 8) if host else 0)) // per_row)
        assert rows == (min(most, slab) if slab else most)
        assert got == _scratch(count, rows, W, host, bins) and got <= 16 << 30
    # a cube whose single row does not fit
    with pytest.raises(ValueError):
        P.wave_statistics_scratch_bytes(2 ** 30, 1, 1024, host=host)


def test_scratch_at_the_flagship_size_needs_slabs_from_the_host_only():
    assert P.wave_statistics_scratch_bytes(1000, 1024, 1024, host=False) == (1000 * 1024 * 1024 * 8, 1024)
    total, rows = P.wave_statistics_scratch_bytes(1000, 1024, 1024, host=True)
    assert rows == 1024 and total < 16 << 30


# ---- every probe against the mistake it is there to catch -----------------------------------------------------------------------
CATCHES = {
    "strict_zero": ["zero_touch", "zeros_waves"],
    "span_off": ["nw1", "nw7", "nw4_demean"],
    "pairwise": ["big_small"],
    "fma_eta": ["random"],
    "fma_tau": ["early_crossings"],
    "fma_moment": ["random"],
    "n13_floor": ["nw1", "nw2", "nw4", "nw7"],
    "tie_later": ["tie_cut", "quantised"],
    "sorted_sum": ["sum_order"],
    "tz_mean": ["random"],
}


def _differs(a, b):
    return any(not np.array_equal(a[n], b[n], equal_nan=True) for n in WO.FIELDS + ("n_cross",))


@pytest.fixture(scope="module")
def probes():
    return WP.probes()


def test_every_mistake_has_a_probe():
    assert sorted(CATCHES) == sorted(WO.BROKEN)


@pytest.mark.parametrize("mistake", sorted(CATCHES))
def test_probe_catches(probes, mistake):
    for name in CATCHES[mistake]:
        z, kw = probes[name]
        assert _differs(WO.wave_stats(z, **kw), WO.wave_stats(z, broken=[mistake], **kw)), f"{name} does not tell {mistake} from the specification"


def test_probes_hold_what_they_are_named_for(probes):
    nw = {name: WO.wave_stats(z, **kw)["n_waves"][0, 0] for name, (z, kw) in probes.items() if z.shape[2] == 2}
    assert nw["all_positive"] == 0 and nw["one_step"] == 0 and nw["one_crossing"] == 0 and nw["zeros"] == 0 and nw["constant"] == 0
    one = WO.wave_stats(*probes["one_crossing"][:1], **probes["one_crossing"][1])
    assert one["n_cross"][0, 0] == 1 and np.isnan(one["h_13"][0, 0]) and np.isnan(one["t_z"][0, 0])
    for k in (1, 2, 3, 4, 7):
        assert nw[f"nw{k}"] == k
    for count in (8, 9, 16, 17):                         # as many crossings as a series can hold
        ref = WO.wave_stats(probes[f"alternating{count}"][0], **probes[f"alternating{count}"][1])
        assert ref["n_cross"][0, 0] == count // 2 and ref["n_cross"][0, 1] == (count - 1) // 2
        assert np.array_equal(ref["H"][:count // 2 - 1, 0, 0], np.full(count // 2 - 1, 2.0))
    assert WO.wave_stats(*probes["zero_touch"][:1], **probes["zero_touch"][1])["n_cross"][0, 0] == 1
    assert WO.wave_stats(*probes["zero_ramp"][:1], **probes["zero_ramp"][1])["n_cross"][0, 0] == 1
    tie = WO.wave_stats(*probes["tie_cut"][:1], **probes["tie_cut"][1])
    assert np.array_equal(tie["H"][:4, 0, 0], [3, 5, 3, 3]) and tie["h_13"][0, 0] == 4.0
    assert tie["t_13"][0, 0] == (tie["T"][0, 0, 0] + tie["T"][1, 0, 0]) / 2 != (tie["T"][1, 0, 0] + tie["T"][3, 0, 0]) / 2
    twice = WO.wave_stats(*probes["hmax_twice"][:1], **probes["hmax_twice"][1])
    assert np.array_equal(twice["H"][:4, 0, 0], [2, 5, 3, 5]) and twice["t_hmax"][0, 0] == twice["T"][1, 0, 0] != twice["T"][3, 0, 0]
    order = WO.wave_stats(*probes["sum_order"][:1], **probes["sum_order"][1])
    assert order["h_13"][0, 0] == (2.0 ** 53 + 2.0) / 3.0 and (2.0 ** 53 + 1.0) + 1.0 == 2.0 ** 53
    const = WO.wave_stats(*probes["constant"][:1], **probes["constant"][1])
    assert const["m2"][0, 0] == 0.0 and np.isnan(const["skewness"][0, 0]) and np.isnan(const["kurtosis"][0, 0])
    for name in ("subnormal", "huge"):
        z = probes[name][0]
        ref = WO.wave_stats(z, **probes[name][1])
        assert ref["n_waves"][0, 0] == 3 and np.isfinite(ref["m4"]).all() and (ref["m4"] > 0).all()
    assert 0 < np.abs(probes["subnormal"][0]).max() < np.finfo(np.float32).tiny
    quant = WO.wave_stats(probes["quantised"][0], **probes["quantised"][1])
    Hq = quant["H"][:, 0, :]
    ties = [np.sum(Hq[:, c] == np.sort(Hq[:quant["n_waves"][0, c], c])[::-1][(quant["n_waves"][0, c] + 2) // 3 - 1]) for c in range(Hq.shape[1])]
    assert max(ties) >= 2                                # several waves exactly at the cut
