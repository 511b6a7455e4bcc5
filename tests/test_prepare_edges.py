"""The prepare stage without a GPU: tests/prepare_direct.py (a direct-form numpy restatement of the three resamplers of rectify.hip and of
CLAHE, written from the notes and sharing no code with the oracle) is held bit-equal to oracle/rectify_oracle.c and oracle/clahe_oracle.c
on every probe of tests/prepare_probes.py, and every probe is shown to be one.  tests/test_prepare_edges_gpu.py runs the same probes
through the kernels.

What is exact: everything.  Tables, coordinates, windows, tap sums, histograms, look-up tables and blends are integer arithmetic or IEEE
arithmetic with one rounding per operation; every comparison is array_equal.

What each probe can see, and the mistake it would catch (each figure is printed, then asserted as a lower bound):
  calibrated K    at least three camera matrices whose inverse has ir[8] != 1 (a calibration gives one in about seven) and one with
                  ir[8] == 1: an undistortion that takes only "round" matrices; the two forms of the tables (_x and _x * (1 / _w)) are
                  compared directly, since no picture can tell them apart;
  horizons        W == 0 exactly (40 and 5 pixels), within 2^-30 of 0 (40 pixels beyond the int32 clamp, 40 / 39 beyond int16), W < 0;
                  a block 204 columns wide: 32 / W taken at W == 0, a missing clamp, wrap for saturate, one block per row;
  windows         every partial window on each side of each axis at four fractions, sources from 1 x 1: a fast path taken one tap too
                  early, a border tap that is not 0;
  lattices        all 1024 phases at wholly-inside windows: phase x / y exchanged, a table without the sum fix-up; exact ties:
                  truncation (or half-up) instead of nearest-even;
  wrap            5185 coordinates beyond int16, 160 wrap back inside, 32 of them non-zero where a saturating cast gives 0;
  CLAHE           7 x 3 against 3 x 7 and 150 x 2 grids: the grid transposed; hand answers for the residuals 0, 1, 3, 85, 128, 129, 255:
                  the residual's step dropped; area 510: half-up for half-even in the table; clip forced to 1, clip 0, a picture smaller
                  than the grid.
Each switch of prepare_direct must miss the oracle on the probes built for it (test_every_mistake_is_seen)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import prepare_direct as D  # noqa: E402
import prepare_pol_oracle as PP  # noqa: E402
import prepare_probes as PR  # noqa: E402


def _same(got, want, what):
    bad = np.argwhere(got != want)
    if len(bad):
        y, x = bad[0]
        pytest.fail(f"{what}: {len(bad)} of {want.size} pixels differ, the first at (x {x}, y {y}): {got[y, x]} for {want[y, x]}")


# ---- the restatement against the oracle ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ksize", [2, 4])
def test_tables(oracle, ksize):
    want = oracle.inter_tab(ksize)
    assert np.array_equal(D.weight_table(ksize), want)
    assert np.all(want.sum(axis=(1, 2)) == 32768)
    plain = D.weight_table(ksize, no_fixup=True)
    moved = int((plain != want).any(axis=(1, 2)).sum())
    print(f"{ksize} x {ksize}: the fix-up changes {moved} of 1024 entries")
    assert moved >= (1 if ksize == 2 else 512)
    if ksize == 2:                                       # NOTES/oracle_and_pins.md: the zero-phase entry becomes {32767, 0, 0, 1}
        assert want[0].ravel().tolist() == [32767, 0, 0, 1] and plain[0].ravel().tolist() == [32767, 0, 0, 0]


@pytest.mark.parametrize("kind", ["remap", "warp", "undistort", "clahe"])
def test_direct_equals_oracle(oracle, kind):
    cases = PR.of_kind(kind)
    assert len(cases) >= 10
    for p in cases:
        want = PR.oracle_answer(oracle, p)
        _same(PR.run_direct(p), want, p["name"])
    print(f"{kind}: {len(cases)} probes, {sum(PR.oracle_answer(oracle, p).size for p in cases)} pixels, all equal")


# ---- calibrated K --------------------------------------------------------------------------------------------------------------------------
def test_calibrated_cameras(oracle):
    off = [name for name, (K, w, h) in PR.CAMERAS.items() if PR.ir8(K) != 1.0]
    on = [name for name in PR.CAMERAS if name not in off]
    frac = PR.refused_fraction()
    print(f"ir[8] != 1: {off}; ir[8] == 1: {on}; of 20000 matrices with fx, fy in [500, 5000): {frac * 100:.2f} % have ir[8] != 1")
    assert len(off) >= 3 and "diag1234" in off and len(on) >= 1
    assert frac >= 0.10
    assert any(w > 4096 for K, w, h in PR.CAMERAS.values()) and any(1 < 4096 // w < h for K, w, h in PR.CAMERAS.values())   # one row per stripe; several stripes of several rows
    for name, (K, w, h) in PR.CAMERAS.items():
        xs, ys = D.undistort_tables(K, w, h)
        xs0, ys0 = D.undistort_tables(K, w, h, divide=False)
        ulp = max(float(np.max(np.abs(xs - xs0) / np.spacing(np.abs(xs0)))), float(np.max(np.abs(ys - ys0) / np.spacing(np.abs(ys0)))))
        moved = 0
        for n, dist in PR.DISTS.items():
            a, b = D.undistort_coords(K, dist, w, h), D.undistort_coords(K, dist, w, h, divide=False)
            moved += int((a[0] != b[0]).sum() + (a[1] != b[1]).sum())
        print(f"{name}: ir[8] - 1 = {PR.ir8(K) - 1.0:.3e}; _x * (1 / _w) against _x: at most {ulp:.2f} ulp; (iu, iv) differ in {moved} places over {len(PR.DISTS)} models")
        # 1 / ir[8] is 1 or one of its two neighbours, at most 2^-52 away: the product moves by less than 2 ulp before it is rounded
        assert ulp <= 2.0
        if name in on:
            assert ulp == 0.0
    # the staged oracle of the polarimetric preparation carries the same tables
    itab = oracle.inter_tab(2)
    for name in ("diag1234", "f3783", "short", "round"):
        K, w, h = PR.CAMERAS[name]
        p = PR.probes()[f"undistort_{name}_5"]
        iu, iv = PP.undistort_map(w, h, K, p["dist"])
        du, dv = D.undistort_coords(K, p["dist"], w, h)
        assert np.array_equal(iu, du) and np.array_equal(iv, dv)
        _same(PP.remap_fixed_u8(p["src"], iu, iv, itab), PR.oracle_answer(oracle, p), f"prepare_pol_oracle {name}")


def test_undistort_probes_move_pixels(oracle):
    """without coefficients the map is the identity whatever ir[8] is; with them the short camera's picture moves"""
    for cam in PR.CAMERAS:
        p = PR.probes()[f"undistort_{cam}_0"]
        assert np.array_equal(PR.oracle_answer(oracle, p), p["src"]), cam
    for n in (4, 5, 8, 12):
        p = PR.probes()[f"undistort_short_{n}"]
        moved = int((PR.oracle_answer(oracle, p) != p["src"]).sum())
        print(f"short, {n} coefficients: {moved} of {p['src'].size} pixels change")
        assert moved > p["src"].size // 2
    p = PR.probes()["undistort_f3366_5"]
    assert int((PR.oracle_answer(oracle, p) != p["src"]).sum()) > p["src"].size // 2


# ---- horizons ------------------------------------------------------------------------------------------------------------------------------
HORIZON_FIGURES = {"horizon_zero": dict(bw0=64, zero=40, negative=1240, clamp=0, x16=0, y16=0, lit=0.45),
                   "horizon_tiny": dict(bw0=64, zero=0, negative=1240, clamp=40, x16=40, y16=39, lit=0.0),
                   "horizon_204": dict(bw0=204, zero=5, negative=855, clamp=0, x16=0, y16=0, lit=0.25)}


@pytest.mark.parametrize("name", list(HORIZON_FIGURES))
def test_horizon_figures(oracle, name):
    p, want = PR.probes()[name], HORIZON_FIGURES[name]
    nx, ny, W = D.warp_terms(p["H"], p["dw"], p["dh"])
    X, Y = D.warp_coords(p["H"], p["dw"], p["dh"])
    live = W != 0
    with np.errstate(all="ignore"):
        s = 32.0 / np.where(live, W, 1.0)
        clamp = int((live & ((np.abs(nx * s) > 2147483647.0) | (np.abs(ny * s) > 2147483647.0))).sum())
    got = dict(bw0=D.block_width(p["dw"], p["dh"]), zero=int((~live).sum()), negative=int((W < 0).sum()), clamp=clamp,
               x16=int((np.abs(X >> 5) > 32767).sum()), y16=int((np.abs(Y >> 5) > 32767).sum()), lit=float((PR.oracle_answer(oracle, p) != 0).mean()))
    print(f"{name}: {got}")
    assert got["bw0"] == want["bw0"]
    for k in ("zero", "negative", "clamp", "x16", "y16", "lit"):
        assert got[k] >= want[k], k
    if name == "horizon_tiny":
        assert got["zero"] == 0
    x, y, w, h = p["roi"]
    cols = np.nonzero((np.abs(W) == np.abs(W).min()).any(axis=0))[0]
    assert x % got["bw0"] != 0 and x <= cols.min() and cols.max() < x + w            # the ROI starts inside a block and holds the horizon


def test_block_widths():
    seen = set()
    for p in PR.of_kind("warp"):
        bw0 = D.block_width(p["dw"], p["dh"])
        assert bw0 in (64, 204, p["dw"])
        if bw0 < p["dw"]:
            seen.add(bw0)                                # dw > bw0: the row spans at least two blocks
    assert seen == {64, 204}


# ---- windows and phases -----------------------------------------------------------------------------------------------------------------------
def _inside_counts(start, taps, n):
    """how many of the window's taps start .. start + taps - 1 lie in 0 .. n - 1"""
    return np.clip(np.minimum(start + taps, n) - np.maximum(start, 0), 0, taps)


def test_border_maps_hold_every_window():
    sizes = set()
    for p in PR.probes().values():
        if not p["name"].startswith("border_map_"):
            continue
        sh, sw = p["src"].shape
        sizes.add((sw, sh))
        X, Y = D.remap_coords(p["mx"], p["my"])
        assert np.max(np.abs(p["mx"])) * 32 < 2 ** 31
        for q, n in ((X, sw), (Y, sh)):
            start = (q >> 5) - 1
            for frac in (0, 1, 16, 31):
                at = start[(q & 31) == frac]
                counts = _inside_counts(at, 4, n)
                # from both sides: wholly outside and every partial count; and somewhere as many taps as fit
                for side in (at < 0, at + 4 > n):
                    assert set(np.unique(counts[side]).tolist()) >= set(range(0, min(3, n) + 1)), (p["name"], frac)
                assert set(np.unique(counts).tolist()) == set(range(0, min(4, n) + 1))
    assert {s for pair in sizes for s in pair} == {1, 2, 3, 4, 5, 9}


def test_border_warps_hold_every_window():
    seen = {}
    for p in PR.probes().values():
        if not p["name"].startswith("border_warp_"):
            continue
        sh, sw = p["src"].shape
        X, Y = D.warp_coords(p["H"], p["dw"], p["dh"])
        key = (sw, sh, int(X[0, 0] & 31), int(Y[0, 0] & 31))
        assert np.all((X & 31) == key[2]) and np.all((Y & 31) == key[3])
        seen[key] = True
        for q, n in ((X, sw), (Y, sh)):
            counts = _inside_counts(q >> 5, 2, n)
            assert set(np.unique(counts)) == set(range(0, min(2, n) + 1))
            assert (q >> 5).min() <= -2 and (q >> 5).max() >= n               # wholly outside on both sides
    assert len(seen) == len(PR.SIZES) * 16 and {k[2] for k in seen} == {0, 1, 16, 31} == {k[3] for k in seen}


def test_lattices_hold_every_phase():
    for name, ksize in (("lattice_map", 4), ("ties_map", 4), ("lattice_warp", 2)):
        p = PR.probes()[name]
        sh, sw = p["src"].shape
        if p["kind"] == "remap":
            X, Y = D.remap_coords(p["mx"], p["my"])
            ties = int((((p["mx"].astype(np.float64) * 32) % 1 == 0.5) & ((p["my"].astype(np.float64) * 32) % 1 == 0.5)).sum())
        else:
            X, Y = D.warp_coords(p["H"], p["dw"], p["dh"])
            ties = 0
        phases = len(np.unique((Y & 31) * 32 + (X & 31)))
        o = ksize // 2 - 1
        inside = ((X >> 5) - o >= 0) & ((X >> 5) - o + ksize <= sw) & ((Y >> 5) - o >= 0) & ((Y >> 5) - o + ksize <= sh)
        windows = len(np.unique((Y >> 5) * 4096 + (X >> 5)))
        print(f"{name}: {phases} phases, {windows} windows, all inside: {bool(inside.all())}, exact ties in both axes: {ties}")
        assert inside.all() and windows >= 12
        assert phases == (1024 if name != "ties_map" else 256)           # a tie rounds to the even neighbour: 16 phases per axis
        if name == "ties_map":
            assert ties == X.size
        if p["roi"] is not None:
            x, y, w, h = p["roi"]
            assert x % 2 == 1 and y % 2 == 1


def test_extreme_map_figures(oracle):
    p = PR.probes()["extreme_map"]
    want = PR.oracle_answer(oracle, p)
    X, Y = D.remap_coords(p["mx"], p["my"])
    beyond = (np.abs(X >> 5) > 32767) | (np.abs(Y >> 5) > 32767)
    back = beyond & (D.wrap16(X >> 5) >= 0) & (D.wrap16(X >> 5) < PR.SRC_W) & (D.wrap16(Y >> 5) >= 0) & (D.wrap16(Y >> 5) < PR.SRC_H)
    big = (np.abs(p["mx"].astype(np.float64)) * 32 >= 2.0 ** 31) | (np.abs(p["my"].astype(np.float64)) * 32 >= 2.0 ** 31)
    print(f"extreme_map: {int(beyond.sum())} pixels beyond int16, {int(back.sum())} would wrap back inside, {int(big.sum())} beyond int32")
    assert back.sum() >= 900 and big.sum() == 4
    assert np.all(want[beyond] == 0) and (want[~beyond] != 0).mean() > 0.9


def test_wrap_figures(oracle):
    p = PR.probes()["wrap"]
    h, w = p["src"].shape
    want = PR.oracle_answer(oracle, p)
    iu, iv = D.undistort_coords(p["K"], p["dist"], w, h)
    u, v = iu >> 5, iv >> 5
    beyond = np.abs(u) > 32768
    wu, wv = D.wrap16(u), D.wrap16(v)
    back = beyond & (wu >= -1) & (wu < w)                  # in x; of the five rows only the principal point's is read inside in y as well
    lit = back & (want != 0)
    assert np.all(((wv >= -1) & (wv < h))[lit])
    sat = D.undistort(p["src"], p["K"], p["dist"], saturate_undistort=True)
    print(f"wrap: |u| > 32768 on {int(beyond.sum())} pixels, {int(back.sum())} wrap back inside, non-zero in {int(lit.sum())} (rows {np.unique(np.nonzero(lit)[0])}); "
          f"a saturating cast gives 0 in {int((sat[lit] == 0).sum())} of them")
    assert beyond.sum() >= 5185 and back.sum() >= 160 and lit.sum() >= 32
    assert np.all(np.nonzero(lit)[0] == 2) and np.all(sat[lit] == 0)


# ---- CLAHE ---------------------------------------------------------------------------------------------------------------------------------------
def test_clahe_hand_answers(oracle):
    for p, levels, r in PR.hand_cases():
        want = PR.hand_answer(levels, r, p["src"].size)
        assert D.clahe_geometry(p["src"].shape[1], p["src"].shape[0], 1, 1, p["clip"])[2] == 1
        expect = np.zeros_like(p["src"])
        for v, o in want.items():
            expect[p["src"] == v] = o
        print(f"{p['name']}: area {p['src'].size}, residual {r}: {want}")
        _same(PR.oracle_answer(oracle, p), expect, p["name"] + " (oracle)")
        _same(PR.run_direct(p), expect, p["name"] + " (direct)")
    # worked by hand, residual 3 at level 100 on 20 x 13: one count left at 100, a batch of 1 in each of the bins 0 .. 100, and of the
    # residual's bins 0, 85, 170 two lie at or below 100: 1 + 101 + 2 = 104, and 104 * 255 / 260 = 102
    assert PR.hand_answer((100,), 3, 260) == {100: 102}
    assert PR.hand_answer((100,), 0, 257) == {100: 101}             # 102 * 255 / 257 = 101.2


def test_clahe_probe_figures(oracle):
    P = PR.probes()
    a, b = PR.oracle_answer(oracle, P["grid_7x3"]), PR.oracle_answer(oracle, P["grid_3x7"])
    diff = int((a != b).sum())
    print(f"7 x 3 against 3 x 7 on 70 x 50: {diff} of {a.size} pixels differ")
    assert diff >= a.size // 2
    for name in ("area510", "area510_2x2"):
        p = P[name]
        assert D.clahe_geometry(p["src"].shape[1], p["src"].shape[0], p["tiles_x"], p["tiles_y"], 0.0)[:2] == (30, 17)
        luts = D.clahe_luts(p["src"], p["clip"], p["tiles_x"], p["tiles_y"])
        up = D.clahe_luts(p["src"], p["clip"], p["tiles_x"], p["tiles_y"], lut_half_up=True)
        print(f"{name}: {int((luts != up).sum())} of {luts.size} table entries are ties that half-up rounds the other way")
        assert (luts != up).sum() >= luts.size // 8
    for name, clip in (("tiny_clip", 1), ("tiny_noclip", 0), ("grid_150x2", 1), ("tiny_tiles", 1), ("area510_clip", 7)):
        p = P[name]
        assert D.clahe_geometry(p["src"].shape[1], p["src"].shape[0], p["tiles_x"], p["tiles_y"], p["clip"])[2] == clip, name
    for name in ("narrow_5x40", "flat_2x31", "one_pixel", "grid_2x150"):
        p = P[name]
        h, w = p["src"].shape
        assert w < p["tiles_x"] or h < p["tiles_y"]
    assert D.clahe_geometry(70, 50, 2, 150, 40.0) == (36, 1, 5)      # 70 is a multiple of 2 and is extended all the same: 72 / 2


def test_oracle_clahe_takes_a_rectangular_grid(oracle):
    img = PR.texture(70, 50)
    assert np.array_equal(oracle.clahe(img, 2.0, 5), oracle.clahe(img, 2.0, 5, 5))
    assert not np.array_equal(oracle.clahe(img, 2.0, 7, 3), oracle.clahe(img, 2.0, 3, 7))


# ---- every mistake is seen ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("switch", D.SWITCHES)
def test_every_mistake_is_seen(oracle, switch):
    """The count a right result must keep from the mistaken variant: half of what the mistake misses the oracle by, at least 1."""
    for name in PR.SWITCH_PROBES[switch]:
        bound, found = PR.switch_bound(oracle, switch, name)
        print(f"{switch} on {name}: misses the oracle in {found} of {PR.oracle_answer(oracle, PR.probes()[name]).size} pixels; bound {bound}")
        assert found >= 1 and found >= bound
    # without any switch the restatement is the oracle: test_direct_equals_oracle
