"""The synthetic-plane probes of tests/kaze_probes.py without a GPU: every hand-made expectation is held to the oracle
(tests/kaze_oracle.py), and every probe group is shown to be changed by the mistake it is there to catch, as tests/test_kaze.py does
for the pictures.  tests/test_kaze_edges_gpu.py runs the same probes on the device."""
from fractions import Fraction

import numpy as np
import pytest

import kaze_oracle as KO
import kaze_probes as KP

F = np.float32


def lv_of(esigma):
    return [dict(esigma=F(e)) for e in esigma]


def angle_diff(a, b):
    d = np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))
    return np.minimum(d, 2 * np.pi - d)


# ------------------------------------------------------------------------------------------------------------------- by hand
def test_extrema_probes_are_what_the_oracle_finds():
    cases = KP.isolated_peaks() + KP.threshold_probes() + KP.border_probes()
    assert len(cases) == 18 + 2 + 6
    for name, vol, thr, es, cand, vals in cases:
        got, gv = KO.extrema(vol, lv_of(es), thr)
        assert np.array_equal(got, cand) and np.array_equal(gv, vals), name
    assert sum(len(c[4]) for c in KP.isolated_peaks()) == 2 * 2 * 20 + 2 * 2
    vol, cand = KP.tie_probes()
    assert np.array_equal(KO.extrema(vol, lv_of(np.zeros(3)))[0], cand)
    vol[2, 3, KP.TIE_X(27) + 1] = KP.below(0.01)             # without its NaN the last peak is found as well
    assert KO.extrema(vol, lv_of(np.zeros(3)))[0].tolist() == [[1, 4, KP.TIE_X(26)], [1, 4, KP.TIE_X(27)]]
    # what the border rule keeps, written out: -0.5 rounds to -0 and stays, w - 0.5 = 69.5 rounds to 70 and goes
    keep = {(float(c[3][0]), c[0][-1]): sorted(set(c[4][:, 2].tolist()) - {35}) for c in KP.border_probes()}
    assert keep[(1.5, "0")] == [4, 6, 8, 62, 64] and keep[(1.5, "1")] == [5, 7, 61, 63]                  # 65 + 4.5 = 69.5 -> 70
    assert keep[(0.5, "0")] == [2, 4, 6, 8, 62, 64, 66] and keep[(0.5, "1")] == [1, 3, 5, 7, 61, 63, 65, 67]      # 68 + 1.5 -> 70, 1 - 1.5 -> -0
    assert keep[(2.5, "0")] == [8] and keep[(2.5, "1")] == [7, 61]                                         # 8 - 7.5 -> 0, 7 - 7.5 -> -0, 62 + 7.5 -> 70
    ldet, planted = KP.cap_probe()
    assert np.array_equal(KO.extrema(ldet, KO.levels(2, 2))[0], planted) and len(planted) == 20


def exact_solution(nb):
    """the refinement of a 3 x 3 x 3 neighbourhood in rationals: (dx, dy, ds), or None where the Hessian is singular"""
    f = lambda dl, dy, dx: Fraction(float(nb[1 + dl, 1 + dy, 1 + dx]))
    v = f(0, 0, 0)
    g = [(f(0, 0, 1) - f(0, 0, -1)) / 2, (f(0, 1, 0) - f(0, -1, 0)) / 2, (f(1, 0, 0) - f(-1, 0, 0)) / 2]
    dxy = (f(0, 1, 1) + f(0, -1, -1) - f(0, -1, 1) - f(0, 1, -1)) / 4
    dxs = (f(1, 0, 1) + f(-1, 0, -1) - f(1, 0, -1) - f(-1, 0, 1)) / 4
    dys = (f(1, 1, 0) + f(-1, -1, 0) - f(1, -1, 0) - f(-1, 1, 0)) / 4
    A = [[f(0, 0, 1) + f(0, 0, -1) - 2 * v, dxy, dxs], [dxy, f(0, 1, 0) + f(0, -1, 0) - 2 * v, dys], [dxs, dys, f(1, 0, 0) + f(-1, 0, 0) - 2 * v]]
    det = lambda m: (m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1]) - m[0][1] * (m[1][0] * m[2][2] - m[1][2] * m[2][0])
                     + m[0][2] * (m[1][0] * m[2][1] - m[1][1] * m[2][0]))
    d = det(A)
    if d == 0:
        return None
    return [det([[(-g[r] if c == k else A[r][c]) for c in range(3)] for r in range(3)]) / d for k in range(3)]      # Cramer


def test_refine_probes_are_what_the_oracle_and_exact_arithmetic_give():
    vol, cand, exp, case = KP.refine_probes()
    ref = KO.refine(vol, cand)
    hand = ~np.isnan(exp[:, 0])
    assert np.array_equal(ref[hand], exp[hand]) and set(case.tolist()) == set(range(len(KP.REFINE_CASES)))
    kept = {c: bool(ref[case == c][0, 4]) for c in set(case.tolist())}
    for c, (name, nb, e) in enumerate(KP.REFINE_CASES):
        if not np.isfinite(nb[:2]).all() or not np.isfinite(nb[2, 1]).all() or not np.isfinite(nb[2, :, 1]).all():
            assert not kept[c], name
            continue
        sol = exact_solution(nb)
        if sol is None:
            assert not kept[c] and "zero pivot" in name, name
            continue
        i = int(np.flatnonzero(case == c)[0])
        assert kept[c] == all(abs(s) <= 1 for s in sol), name
        if kept[c]:
            d = ref[i, :3].astype(np.float64) - [cand[i, 2], cand[i, 1], 0]
            assert np.abs(d - [float(s) for s in sol]).max() < 8e-6, name             # half a float32 step at x = 128
            if e is not None and "6 on" not in name:
                assert [Fraction(float(t)) for t in e[:3]] == sol, name              # dyadic cases: the hand value is the exact one
    assert sum(kept.values()) == 13 and len(kept) == 22


def test_raw_keys_are_not_keys_of_the_extremum_search():
    keys, rows = KP.raw_keys()
    h, w, n = KP.H9, KP.W9, 3
    for k, r in zip(keys.tolist(), rows):
        x, y, lev = int(np.fmod(k, w)), int(np.fmod(int(k / w) if abs(k) < 2 ** 50 else k // w, h)), k // (w * h)
        good = 1 <= k % w <= w - 2 and 1 <= (k // w) % h <= h - 2 and 1 <= lev <= n - 2 and k >= 0
        assert good == (r is None), k
        if r is not None:
            assert (x, y) == r, k                                  # C's truncating % and /
    assert sum(r is None for r in rows) == 3


def test_orientation_khot_probes_by_hand():
    for p in KP.orientation_khot():
        a32 = KO.orientation(p["kp"], p["Lx"], p["Ly"])
        a64 = KO.orientation(p["kp"], p["Lx"], p["Ly"], np.float64)
        for got32, got64, e in zip(a32, a64, p["expect"]):
            if e == 0.0:
                assert got32 == 0 and got64 == 0 and not np.signbit(got32), p["name"]
            else:
                assert angle_diff(got32, e) < 1e-6 and angle_diff(got64, e) < 1e-7, p["name"]
    names = [p["name"] for p in KP.orientation_khot()]
    assert len(names) == len(set(names)) == 1 + 3 * 5 + 3 + 4 + 1 + 1


def test_orientation_edge_and_size_probes_read_what_they_say():
    Lx, Ly = KP.dense_planes()
    t = KP.orientation_edge_table()
    s = (t[:, 2] / F(2) + F(0.5)).astype(np.int64)
    ii = np.array([p[0] for p in KP.LATTICE])
    jj = np.array([p[1] for p in KP.LATTICE])
    outside = [int(((np.trunc(r[0] + (ii * k).astype(F) + F(0.5)) < 0) | (np.trunc(r[0] + (ii * k).astype(F) + F(0.5)) >= KP.WK)
                    | (np.trunc(r[1] + (jj * k).astype(F) + F(0.5)) < 0) | (np.trunc(r[1] + (jj * k).astype(F) + F(0.5)) >= KP.HK)).sum())
               for r, k in zip(t, s)]
    print("samples outside the picture, of 109:", outside)
    # (int)(-1 + 0.5) is 0: at s = 1 a corner keeps the samples with i >= -1 and j >= -1, 46 of 109; at s = 6 those with i, j >= 0, 33
    assert outside[:4] == [63, 70, 70, 76] and outside[8:12] == [76] * 4 and min(outside[:16]) >= 34
    v = F(0.3) + F(-1) + F(0.5)
    assert -1 < v < 0 and int(v) == 0 and np.floor(v) == -1                      # the sample at x + i s = -0.7
    v = F(5.3) + F(-6) + F(0.5)
    assert -1 < v < 0
    z = KP.orientation_size_table()
    assert (z[:, 2] / F(2) + F(0.5)).astype(np.int64).tolist() == [0, 1, 1, 2, 1, 4, 3] * 2
    # size 0: all 109 samples are the keypoint's own pixel, the angle is that pixel's gradient direction
    a = KO.orientation(z[:1], Lx, Ly, np.float64)[0]
    assert angle_diff(a, np.arctan2(float(Ly[1, 34, 30]), float(Lx[1, 34, 30])) % (2 * np.pi)) < 1e-7


def test_descriptor_probes_by_hand():
    zero = np.zeros((KP.NLEV, KP.HK, KP.WK), F)
    d = KO.descriptors(KP.descriptor_edge_table(), zero, zero)
    assert d.shape == (8, 64) and np.isnan(d).all()                             # 0 / 0, as the reference computes it
    for which in (0, 1):
        Lx, Ly, table = KP.descriptor_onehot(which)
        d = KO.descriptors(table, Lx, Ly)
        assert np.isfinite(d).all() and np.abs(np.linalg.norm(d.astype(np.float64), axis=1) - 1).max() < 1e-6
        # angle 0, scale 2: the hot pixel, 10 to the right and 20 above, is sample (k, l) = (5, -10) and no other (every fraction is 0):
        # k is in the subregions i = -2 .. 6 and 3 .. 11 (sub / 4 = 2, 3), l in j = -12 .. -4 only (sub % 4 = 0): subregions 8 and 12
        on = np.flatnonzero(d[0] != 0)
        assert set((on // 4).tolist()) == {8, 12}, on
        on = on[on // 4 == 8]
        # Lx alone: rrx = ry = 0 and rry = rx > 0, so dx, |dx| vanish and dy = |dy|; Ly alone the other way round
        assert (on % 4).tolist() == ([1, 3] if which == 0 else [0, 2]) and d[0, on[0]] == d[0, on[1]] > 0
    D = KP.descriptor_batch_table()
    assert D.shape == (65, 5) and (D[:, 2] / 2 + 0.5).astype(int).min() == 0 and (D[:, 2] / 2 + 0.5).astype(int).max() == 7


def test_stage_probes_by_hand():
    assert [len(t) for t in KP.tap_sets()] == [1, 3, 5, 9, 11, 13, 15, 7]
    a = np.arange(12, dtype=F).reshape(3, 4)
    assert np.array_equal(KO.gauss(a, np.array([1], F)), a)
    # the taps run first to last over x - r .. x + r: taps (1, 0, 0) read the left neighbour, replicated at the border
    assert np.array_equal(KO.gauss(a, np.array([1, 0, 0], F))[1:, 1:], a[:-1, :-1])
    h, w = 7, 129
    z = np.zeros((h, w), F)
    assert KO.contrast_of(z, z)[:3] == (F(0.03), F(0), 0) and KO.contrast_of(z, z)[3].sum() == 0
    one = z.copy()
    one[3, 77] = 0.25
    k, hmax, n, hist = KO.contrast_of(one, z)
    assert hmax == F(0.25) and n == 1 and hist[299] == 1 and hist.sum() == 1
    ring = z.copy()
    ring[0, :], ring[-1, :], ring[:, 0], ring[:, -1] = 1, 2, 3, 4
    assert KO.contrast_of(ring, ring)[1:3] == (F(0), 0)
    lx = KP.bin_edge_plane(h, w)
    k, hmax, n, hist = KO.contrast_of(lx, z)
    assert hmax == 1 and n == 300 and hist.sum() == 300 and hist.max() <= 2 and hist[299] >= 1
    with np.errstate(all="ignore"):
        fl = KO.flow_g2(np.array([[0, 1, 1e-20]], F), np.array([[0, 0, 0]], F), 1e-23)
    assert np.isnan(fl[0, 0]) and fl[0, 1] == 0 and fl[0, 2] == 0 and F(1e-23) * F(1e-23) == 0 and 0 < F(1e-22) * F(1e-22) < np.finfo(F).tiny


def test_small_pictures_on_the_oracle():
    counts = {}
    for w, h, no, ns in KP.SMALL_PICTURES:
        d = KP.small_oracle(w, h, no, ns)
        assert KP.small_picture(w, h).shape == (h, w) and np.isfinite(d["ss"]["Ldet"]).all(), (w, h)
        counts[(w, h)] = len(d["kp"])
    print(counts)
    assert counts == {(70, 6): 0, (6, 70): 0, (6, 6): 0, (23, 23): 0, (23, 130): 3}


# -------------------------------------------------------------------------------------------------------------------- mistakes
MISTAKES = ["one loose neighbour", "border rounding", "pivoting", "offset bound", "orientation", "orientation edges", "orientation sizes",
            "descriptor support", "descriptor border"]


@pytest.mark.parametrize("mistake", MISTAKES)
def test_probes_are_changed_by_the_mistake_they_catch(mistake):
    if mistake == "one loose neighbour":
        vol, cand = KP.tie_probes()
        for p, nb in enumerate(KP.NEIGHBOURS):
            got = KO.extrema(vol, lv_of(np.zeros(3)), loose=nb)[0].tolist()
            # a >= at that neighbour alone lets that one peak through, and of the others only the tied neighbour of the peak whose tie
            # lies the other way, which then looks back at its peak with >=
            centres = [c for c in got if c[1] == 4 and (c[2] - 2) % 4 == 0]
            assert centres == sorted(cand.tolist() + [[1, 4, KP.TIE_X(p)]]) and len(got) - len(centres) <= 1, nb
    elif mistake == "border rounding":
        for rounding in ("away", "trunc"):
            changed = [not np.array_equal(KO.extrema(vol, lv_of(es), thr, rounding=rounding)[0], cand) for _, vol, thr, es, cand, _ in KP.border_probes()]
            assert any(changed), rounding
        # 1 - 1.5 = -0.5: half to even keeps it (-0), half away from zero drops it; truncation keeps 68 + 1.5 = 69.5 (69), half to even drops it
    elif mistake == "pivoting":
        vol, cand, exp, case = KP.refine_probes()
        good = KO.refine(vol, cand)
        names = [c[0] for c in KP.REFINE_CASES]
        none, last = KO.refine(vol, cand, pivot="none"), KO.refine(vol, cand, pivot="last")
        hit = lambda bad: {names[c] for c in set(case[(bad != good).any(axis=1)].tolist())}
        assert {n for n in names if "pivots on row" in n} <= hit(none)
        assert hit(last) == {n for n in names if "tie" in n} and len(hit(last)) == 2
    elif mistake == "offset bound":
        vol, cand, exp, case = KP.refine_probes()
        good, bad = KO.refine(vol, cand), KO.refine(vol, cand, bound="lt")
        names = [c[0] for c in KP.REFINE_CASES]
        assert {names[c] for c in set(case[(bad != good).any(axis=1)].tolist())} == {n for n in names if "exactly is kept" in n}
    elif mistake == "orientation":
        seen = set()
        for p in KP.orientation_khot():
            if p["mistake"] is None:
                continue
            good, bad = KO.orientation(p["kp"], p["Lx"], p["Ly"]), KO.orientation(p["kp"], p["Lx"], p["Ly"], **p["mistake"])
            assert angle_diff(good, bad).max() >= 0.05, p["name"]
            seen |= set(p["mistake"])
        assert seen == {"drop", "transpose", "no_wrap", "no_high", "zero_in", "last_equal", "level0"}
    elif mistake == "orientation edges":
        Lx, Ly = KP.dense_planes()
        t = KP.orientation_edge_table()
        good = KO.orientation(t, Lx, Ly)
        for m in ("floor", "clamp"):
            moved = angle_diff(good, KO.orientation(t, Lx, Ly, **{m: True}))
            print(f"{m}: {int((moved >= 0.05).sum())} of {len(t)} angles move by 0.05 rad or more")
            assert moved.max() >= 0.05, m
        assert (angle_diff(good, KO.orientation(t, Lx, Ly, floor=True))[16:] >= 0.05).any()      # the -0.7 samples themselves
    elif mistake == "orientation sizes":
        Lx, Ly = KP.dense_planes()
        t = KP.orientation_size_table()
        good = KO.orientation(t, Lx, Ly)
        assert angle_diff(good, KO.orientation(t, Lx, Ly, size_floor=True)).max() >= 0.05
        assert good[1] == good[2] and angle_diff(good[[0, 1, 3, 5]], good[[1, 3, 4, 6]]).min() >= 0.05   # each step of s reads other pixels
        assert angle_diff(good[:7], good[7:]).min() >= 0.05                                       # and so does the level
    elif mistake == "descriptor support":
        for m in ("swap_sub", "swap_kl", "rotate_sign", "swap_rr"):
            changed = False
            for which in (0, 1):
                Lx, Ly, table = KP.descriptor_onehot(which)
                good = KO.descriptors(table, Lx, Ly)
                bad = KO.descriptors(table, Lx, Ly, **({m: True} if m != "rotate_sign" else {m: -1.0}))
                changed |= not np.array_equal(good != 0, bad != 0)
            assert changed, m
    else:
        Lx, Ly = KP.dense_planes()
        t = KP.descriptor_edge_table()
        good, d64 = KO.descriptors(t, Lx, Ly), KO.descriptors(t, Lx, Ly, np.float64)
        tol = 0.5 * float(np.spacing(F(1))) + 4.0 * np.abs(good.astype(np.float64) - d64).max()
        moved = np.abs(KO.descriptors(t, Lx, Ly, zero_outside=True).astype(np.float64) - good).max(axis=1)
        print(f"zero_outside: every keypoint moves by {moved.min():.3g} or more; the tolerance is {tol:.3g}")
        assert (moved > 100 * tol).all()
        # Taking the fraction after the clamp cannot show in any result: an index is clamped only where both indices of that axis land
        # on the same border pixel, and the weights of an axis sum to 1 whatever the fraction is.  The variant moves roundings only.
        moved = np.abs(KO.descriptors(t, Lx, Ly, frac_after_clamp=True).astype(np.float64) - good).max()
        print(f"frac_after_clamp: the largest change is {moved:.3g}")
        assert moved < 1e-5


def test_admissible_angles_of_fragile_keypoints():
    """what tests/test_kaze_gpu.py and tests/test_kaze_edges_gpu.py compare a fragile keypoint's angle with"""
    Lx, Ly = KP.dense_planes()
    t = np.concatenate([KP.orientation_edge_table(), KP.orientation_size_table()])
    a, frag, adm = KO.orientation(t, Lx, Ly, flags=True, admissible=True)
    a2, frag2 = KO.orientation(t, Lx, Ly, flags=True)
    assert np.array_equal(a, a2) and np.array_equal(frag, frag2) and np.array_equal(a, KO.orientation(t, Lx, Ly))
    for q in range(len(t)):
        assert (len(adm[q]) > 0) == frag[q]
        if frag[q]:
            assert angle_diff(adm[q], a[q]).min() == 0                          # the oracle's own choice is one of them
    # the two-window tie: both windows' angles are admissible, and nothing else
    p = [p for p in KP.orientation_khot() if p["mistake"] == dict(last_equal=True)][0]
    a, frag, adm = KO.orientation(p["kp"], p["Lx"], p["Ly"], flags=True, admissible=True)
    assert frag[0] and sorted(set(np.round(adm[0].astype(np.float64), 5).tolist())) == [round(np.pi / 2, 5), round(np.pi, 5)]
    # a sample of angle exactly 0: counted in or out of the wrap-around windows
    p = [p for p in KP.orientation_khot() if p["mistake"] == dict(zero_in=True)][0]
    a, frag, adm = KO.orientation(p["kp"], p["Lx"], p["Ly"], flags=True, admissible=True)
    assert frag[0] and angle_diff(adm[0], a[0]).min() == 0 and len(set(adm[0].tolist())) >= 2
