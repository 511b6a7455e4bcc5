"""Synthetic planes for the KAZE kernels (csrc/kaze.hip): probes whose answer is known by hand.  Plain numpy, no GPU.
tests/test_kaze_edges.py holds every probe to its hand-made expectation on the oracle (tests/kaze_oracle.py) and shows which
mistake each one catches; tests/test_kaze_edges_gpu.py runs them on the device.  Sizes are width x height; the stencil kernels and
the extremum search launch 64 x 4 tiles, so 130 x 9 is three tiles across with ragged last tiles in both directions."""
import functools
import math

import numpy as np

import kaze_oracle as KO

F = np.float32
W9, H9 = 130, 9           # 2 x 2 levels admit it (reach 5)
W24, H24 = 70, 24         # 4 x 4 levels admit it (reach 22)
WK = HK = 64              # the per-keypoint probes

below = lambda v: np.nextafter(F(v), F(-np.inf))
above = lambda v: np.nextafter(F(v), F(np.inf))


def sigmas(n, e=0.0):
    """a level table of n levels that all have the same esigma (0: the border rule is out of the way)"""
    return [dict(esigma=F(e), sigma_size=1, octave=0, sublevel=i) for i in range(n)]


# ------------------------------------------------------------------------------------------------------------------- extrema
def _plant(shape, peaks):
    vol = np.zeros(shape, F)
    for i, (l, y, x) in enumerate(peaks):
        vol[l, y, x] = F(0.01) + F(0.001) * F(i)
    return vol


def _expect(vol, peaks):
    c = np.array(sorted(peaks), np.int64).reshape(-1, 3)
    return c, vol[c[:, 0], c[:, 1], c[:, 2]]


def isolated_peaks():
    """cases (name, volume, threshold, esigma per level, expected candidates, expected values): one peak at every x of {1, 63, 64,
    127, 128 = w - 2} and y of {1, 3, 4, 7 = h - 2}, at level 1 and at level nlev - 2, with 4 and with 16 levels.  Neighbouring
    places go into different volumes.  The last case plants peaks where none may be found."""
    out = []
    for nlev in (4, 16):
        for lev in (1, nlev - 2):
            for xs in ((1, 63, 127), (64, 128)):
                for ys in ((1, 3, 7), (4,)):
                    peaks = [(lev, y, x) for y in ys for x in xs]
                    vol = _plant((nlev, H9, W9), peaks)
                    out.append((f"{nlev} levels, level {lev}, x {xs}, y {ys}", vol, 1e-4, np.zeros(nlev, F)) + _expect(vol, peaks))
        bad = [(0, 4, 20), (nlev - 1, 4, 30), (1, 0, 40), (1, H9 - 1, 50), (1, 4, 0), (1, 4, W9 - 1), (nlev - 2, 0, 0), (nlev - 2, H9 - 1, W9 - 1)]
        good = [(1, 4, 64), (nlev - 2, 1, 100)]
        vol = _plant((nlev, H9, W9), bad + good)
        out.append((f"{nlev} levels, peaks outside the searched range", vol, 1e-4, np.zeros(nlev, F)) + _expect(vol, good))
    return out


NEIGHBOURS = [(dl, dy, dx) for dl in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dl, dy, dx) != (0, 0, 0)]
TIE_X = lambda p: 2 + 4 * p


def tie_probes():
    """(volume of 3 x 9 x 130, expected candidates): 28 peaks of 0.01 at level 1, row 4, x = 2 + 4 p, every neighbour one float32 below.
    Peak p < 26 has neighbour NEIGHBOURS[p] equal to it; peak 26 has none; peak 27 has one neighbour NaN.  Only peak 26 is found."""
    v = F(0.01)
    vol = np.zeros((3, H9, W9), F)
    for p in range(28):
        x = TIE_X(p)
        vol[0:3, 3:6, x - 1:x + 2] = below(v)
        vol[1, 4, x] = v
        if p < 26:
            dl, dy, dx = NEIGHBOURS[p]
            vol[1 + dl, 4 + dy, x + dx] = v
        elif p == 27:
            vol[2, 3, x + 1] = np.nan
    return vol, np.array([[1, 4, TIE_X(26)]], np.int64)


def threshold_probes():
    """cases as isolated_peaks(): values at the threshold, one float32 above it, at float32(1e-5) and one below, with the threshold at
    1e-4 and at 1e-6.  A candidate is strictly above the threshold and at least 1e-5."""
    out = []
    for thr, found in ((1e-4, [False, True, False, False]), (1e-6, [False, False, True, False])):
        vals = [F(thr), above(thr), F(1e-5), below(1e-5)]
        vol = np.zeros((3, H9, W9), F)
        places = [(1, 4, 10 + 30 * i) for i in range(4)]
        for (l, y, x), v in zip(places, vals):
            vol[l, y, x] = v
        keep = [p for p, f in zip(places, found) if f]
        out.append((f"threshold {thr:g}", vol, thr, np.zeros(3, F)) + _expect(vol, keep))
    return out


def _rint_even(v):
    """half to even of an exact multiple of 0.5, in integers: Python's round() does that"""
    assert float(v) * 2 == int(float(v) * 2)
    return round(float(v))


def border_probes():
    """cases as isolated_peaks(): esigma 1.5, 0.5 and 2.5 (reach 4.5, 1.5, 7.5: every x -+ r ends in .5), peaks at every x of 1 .. 8 and
    w - 9 .. w - 2 on a row the rule keeps, and at every y of the same on a column it keeps; even and odd places in two volumes.  Found
    are those with rint(x - r) >= 0 and rint(x + r) < w, half to even (-0.5 goes to -0, which is not below 0)."""
    out = []
    w, h = W24, H24
    for e in (1.5, 0.5, 2.5):
        r = 3 * e
        for par in (0, 1):
            xs = [x for x in list(range(1, 9)) + list(range(w - 9, w - 1)) if x % 2 == par]
            ys = [y for y in list(range(1, 9)) + list(range(h - 9, h - 1)) if y % 2 == par]
            peaks = [(1, 11, x) for x in xs] + [(1, y, 35) for y in ys]
            vol = _plant((3, h, w), peaks)
            keep = [(l, y, x) for (l, y, x) in peaks if _rint_even(x - r) >= 0 and _rint_even(x + r) < w and _rint_even(y - r) >= 0 and _rint_even(y + r) < h]
            assert 0 < len(keep) <= len(peaks)
            out.append((f"esigma {e}, places of parity {par}", vol, 1e-4, np.full(3, e, F)) + _expect(vol, keep))
    return out


def cap_probe():
    """(Ldet of 4 x 64 x 64 for a pyramid of 2 x 2 levels, the 20 planted candidates): all inside that pyramid's border rule"""
    peaks = [(1 + (i % 2), 12 + 8 * (i // 5), 10 + 10 * (i % 5)) for i in range(20)]
    return _plant((4, HK, WK), peaks), np.array(sorted(peaks), np.int64)


# ---------------------------------------------------------------------------------------------------------------- refinement
def hood(v, xp, xm, yp, ym, sp, sm, cxy=0, uxp=0, uyp=0, fill=0, **cells):
    """a 3 x 3 x 3 neighbourhood [level, y, x]: the centre, its six face neighbours, C[y+1][x+1] (Dxy = cxy / 4), U[y][x+1] (Dxs = uxp / 4),
    U[y+1][x] (Dys = uyp / 4), everything else `fill`; cells: further (dl, dy, dx) -> value"""
    a = np.full((3, 3, 3), fill, F)
    a[1, 1, 1], a[1, 1, 2], a[1, 1, 0], a[1, 2, 1], a[1, 0, 1], a[2, 1, 1], a[0, 1, 1] = v, xp, xm, yp, ym, sp, sm
    if fill == 0:
        a[1, 2, 2], a[2, 1, 2], a[2, 2, 1] = cxy, uxp, uyp
    for key, val in cells.items():
        dl, dy, dx = (int(t) - 1 for t in key[1:])
        a[1 + dl, 1 + dy, 1 + dx] = val
    return a


E23 = F(2.0 ** -23)
SIXTH = F(1) / F(6)
# name, neighbourhood, (dx, dy, ds, response, kept) by hand.  The Hessian is [[Dxx, Dxy, Dxs], [Dxy, Dyy, Dys], [Dxs, Dys, Dss]] with
# Dxx = xp + xm - 2 v, Dx = (xp - xm) / 2 and so on; it is solved for minus the gradient.
REFINE_CASES = [
    ("a symmetric peak of 8 over 4", hood(8, 4, 4, 4, 4, 4, 4), (0, 0, 0, 8, 1)),
    ("6 on one side: -6 dx = -1", hood(8, 6, 4, 4, 4, 4, 4), (SIXTH, 0, 0, 8, 1)),
    ("6 on the other side", hood(8, 4, 6, 4, 4, 4, 4), (-SIXTH, 0, 0, 8, 1)),
    ("flat: zero pivot at k = 0, the response is still written", hood(1, 1, 1, 1, 1, 1, 1, fill=1), (0, 0, 0, 1, 0)),
    ("column 0 pivots on row 1: Dxx = 0, Dxy = 4", hood(8, 9, 7, 4, 4, 4, 4, cxy=16), (-0.5, -0.25, 0, 8, 1)),
    ("column 0 pivots on row 2: Dxx = Dxy = 0, Dxs = 4", hood(8, 9, 7, 4, 4, 4, 4, uxp=16), (-0.5, 0, -0.25, 8, 1)),
    ("column 1 pivots on row 2: Dyy = 0, Dys = 4", hood(8, 4, 4, 9, 7, 4, 4, uyp=16), (0, -0.5, -0.25, 8, 1)),
    ("zero pivot at k = 0 with the rest alive", hood(8, 8, 8, 4, 4, 4, 4), (0, 0, 0, 8, 0)),
    ("zero pivot at k = 1", hood(8, 4, 4, 8, 8, 4, 4), (0, 0, 0, 8, 0)),
    ("zero pivot at k = 2", hood(8, 4, 4, 4, 4, 8, 8), (0, 0, 0, 8, 0)),
    ("dx = 1 exactly is kept", hood(0, 0.5, -1.5, -1, -1, -1, -1), (1, 0, 0, 0, 1)),
    ("dx = -1 exactly is kept", hood(0, -1.5, 0.5, -1, -1, -1, -1), (-1, 0, 0, 0, 1)),
    ("dy = 1 exactly is kept", hood(0, -1, -1, 0.5, -1.5, -1, -1), (0, 1, 0, 0, 1)),
    ("ds = 1 exactly is kept", hood(0, -1, -1, -1, -1, 0.5, -1.5), (0, 0, 1, 0, 1)),
    ("dx one float32 above 1 is refused", hood(0, F(0.5) + E23, F(-1.5) - E23, -1, -1, -1, -1), (0, 0, 0, 0, 0)),
    ("dy one float32 above 1 is refused", hood(0, -1, -1, F(0.5) + E23, F(-1.5) - E23, -1, -1), (0, 0, 0, 0, 0)),
    ("ds one float32 above 1 is refused", hood(0, -1, -1, -1, -1, F(0.5) + E23, F(-1.5) - E23), (0, 0, 0, 0, 0)),
    ("a NaN where Dxy reads", hood(8, 4, 4, 4, 4, 4, 4, cxy=np.nan), (0, 0, 0, 8, 0)),
    ("an Inf on one side", hood(8, np.inf, 4, 4, 4, 4, 4), (0, 0, 0, 8, 0)),
    ("a NaN in a corner of the level above, which nothing reads", hood(8, 4, 4, 4, 4, 4, 4, c222=np.nan), (0, 0, 0, 8, 1)),
    # equal pivots, found by search over small integers: the other row gives other bits (tests/test_kaze_edges.py asserts that)
    ("column 0: rows 0 and 1 tie (Dxx = -2, Dxy = 2)", hood(0, 0, -2, 2, 2, -2, 0, cxy=8, uxp=4, uyp=0), None),
    ("column 1: rows 1 and 2 tie (-3 and 3 after the first elimination)", hood(0, 0, -4, -3, 0, 1, 0, cxy=0, uxp=-8, uyp=12), None),
]
REFINE_SLOTS = 129        # 43 across at a pitch of 3, three rows of them: 130 x 9 is full


def refine_probes():
    """(volume 3 x 9 x 130, candidates 129 x 3 in a shuffled order, expected n x 5 with NaN where only the oracle says): the cases,
    repeated, one per 3 x 3 block"""
    vol = np.zeros((3, H9, W9), F)
    order = np.random.default_rng(3).permutation(REFINE_SLOTS)
    cand, exp, case = [], [], []
    for slot in order.tolist():
        c = slot % len(REFINE_CASES)
        x, y = 1 + 3 * (slot % 43), 1 + 3 * (slot // 43)
        vol[:, y - 1:y + 2, x - 1:x + 2] = REFINE_CASES[c][1]
        cand.append((1, y, x))
        e = REFINE_CASES[c][2]
        exp.append([np.nan] * 5 if e is None else ([F(x) + F(e[0]), F(y) + F(e[1]), e[2], e[3], e[4]] if e[4] else [x, y, 0, e[3], 0]))
        case.append(c)
    return vol, np.array(cand, np.int64), np.array(exp, F), np.array(case)


def raw_keys(nlev=3, h=H9, w=W9):
    """(keys, rows by hand or None for a good key): keys k_kaze_extrema cannot give, mixed among good ones.  The kernel takes
    x = key % w, y = (key / w) % h, level = key / (w h) with C's truncating division, refuses what is not an interior pixel of levels
    1 .. nlev - 2 before it reads anything, and writes (x, y, 0, 0, 0)."""
    key = lambda l, y, x: (l * h + y) * w + x
    out = [(key(1, 4, 1 + 3 * 5), None), (key(1, 4, 0), (0, 4)), (key(1, 4, w - 1), (w - 1, 4)), (key(1, 0, 7), (7, 0)), (key(1, 1, 1), None),
           (key(1, h - 1, 7), (7, h - 1)), (key(0, 4, 4), (4, 4)), (key(nlev - 1, 4, 4), (4, 4)), (key(nlev, 1, 1), (1, 1)), (key(1, 7, 127), None),
           (key(1000, 4, 4), (4, 4)), (-1, (-1, 0)), (-(w * h) - w - 2, (-2, -1)), (2 ** 40 + 5, ((2 ** 40 + 5) % w, ((2 ** 40 + 5) // w) % h))]
    return np.array([k for k, _ in out], np.int64), [r for _, r in out]


# --------------------------------------------------------------------------------------------------------------- orientation
LATTICE = [(i, j) for i in range(-6, 7) for j in range(-6, 7) if i * i + j * j < 36]       # sample q of the kernel: i outer, j inner
NLEV = 4                   # the pyramid of the per-keypoint probes: 64 x 64, 2 x 2 levels


def _unit(theta):
    return F(math.cos(theta)), F(math.sin(theta))


def _khot(s, hot, level=1, name="", expect=None):
    """one keypoint whose planes are zero but for the samples `hot`: [((i, j), (gx, gy)), ...] at lattice points (i, j) s"""
    i0, j0 = hot[0][0]
    kx, ky = int(np.clip(40 - i0 * s, 0, WK - 1)), int(np.clip(24 - j0 * s, 0, HK - 1))       # the first hot pixel is off the diagonal
    Lx, Ly = np.zeros((NLEV, HK, WK), F), np.zeros((NLEV, HK, WK), F)
    for (i, j), (gx, gy) in hot:
        x, y = kx + i * s, ky + j * s
        assert 0 <= x < WK and 0 <= y < HK and (i, j) in LATTICE
        Lx[level, y, x], Ly[level, y, x] = gx, gy
    return dict(name=name, Lx=Lx, Ly=Ly, kp=np.array([[kx, ky, 2 * s, level]], F), expect=expect)


def _sum_angle(hot):
    """the angle of the weighted sum of the hot samples, in fp64"""
    sx = sum(float(KO.GAUSS25[abs(i), abs(j)]) * float(gx) for (i, j), (gx, gy) in hot)
    sy = sum(float(KO.GAUSS25[abs(i), abs(j)]) * float(gy) for (i, j), (gx, gy) in hot)
    return math.atan2(sy, sx) % (2 * math.pi)


@functools.lru_cache(maxsize=None)
def orientation_khot():
    """list of probes (name, Lx, Ly, kp, expect: the angle by hand, a list, or None); each names the mistake it is there for in `mistake`"""
    out = []

    def add(p, mistake):
        p["mistake"] = mistake
        out.append(p)
    z = _khot(1, [((0, 0), (F(0), F(0)))], name="all-zero planes", expect=[0.0])
    add(z, None)
    for s in (1, 4, 11):
        for q in (0, 63, 64, 108):
            add(_khot(s, [(LATTICE[q], _unit(1.0))], name=f"s = {s}: sample {q} alone", expect=[1.0]), dict(drop=q))
        add(_khot(s, [((5, 2), _unit(2.0))], name=f"s = {s}: hot at (5, 2) s only", expect=[2.0]), dict(transpose=True))
    for name, hot, mistake in (
            ("both samples in window 0 only", [((1, 0), _unit(0.1)), ((0, 1), _unit(1.0))], None),
            ("both samples in window 41 only, across 2 pi", [((1, 0), _unit(6.2)), ((0, 1), _unit(0.88))], dict(no_wrap=True))):
        add(_khot(4, hot, name=name, expect=[_sum_angle(hot)]), mistake)
    half = tuple(F(0.5) * t for t in _unit(3.0))
    hot = [((1, 0), _unit(6.28)), ((0, 1), half)]
    add(_khot(4, hot, name="a sample just below 2 pi beats a weaker one at 3", expect=[_sum_angle(hot[:1])]), dict(no_high=True))
    for zero in (F(0.0), F(-0.0)):
        sign = "-" if np.signbit(zero) else "+"
        add(_khot(4, [((1, 0), (F(1), zero))], name=f"one sample of angle exactly 0 (ry = {sign}0) is in no window", expect=[0.0]), None)
        hot = [((1, 0), (F(4), zero)), ((0, 1), _unit(0.5))]
        add(_khot(4, hot, name=f"a sample of angle exactly 0 (ry = {sign}0) beside one at 0.5", expect=[_sum_angle(hot[1:])]), dict(zero_in=True))
    hot = [((1, 2), (F(0), F(1))), ((2, 1), (F(-1), F(0)))]
    add(_khot(4, hot, name="two samples of equal weight, pi / 2 and pi: the first of equal windows", expect=[math.pi / 2]), dict(last_equal=True))
    p = _khot(4, [((1, 0), _unit(1.0))], level=0, name="the same keypoint at level 0 and at the last level", expect=[1.0, 2.0])
    x, y = int(p["kp"][0, 0]) + 4, int(p["kp"][0, 1])
    p["Lx"][NLEV - 1, y, x], p["Ly"][NLEV - 1, y, x] = _unit(2.0)
    p["kp"] = np.array([[p["kp"][0, 0], p["kp"][0, 1], 8, 0], [p["kp"][0, 0], p["kp"][0, 1], 8, NLEV - 1]], F)
    add(p, dict(level0=True))
    return out


@functools.lru_cache(maxsize=None)
def dense_planes():
    rng = np.random.default_rng(17)
    return rng.standard_normal((NLEV, HK, WK)).astype(F), rng.standard_normal((NLEV, HK, WK)).astype(F)


EDGE_POSITIONS = [(0, 0), (WK - 1, 0), (0, HK - 1), (WK - 1, HK - 1), (31.5, 0), (31.5, HK - 1), (0, 31.5), (WK - 1, 31.5)]


def orientation_edge_table():
    """keypoints on the corners and in the middle of the sides, and two whose column x + i s is -0.7 at i = -1 ((int)(-0.2) is 0, inside:
    a floor would put it outside); s = 1 and 6; on the dense planes"""
    rows = [(x, y, 2 * s, lev) for s in (1, 6) for lev, (x, y) in zip([0, 1, 2, 3] * 2, EDGE_POSITIONS)]
    rows += [(0.3, 20, 2, 1), (5.3, 41, 12, 2), (20, 0.3, 2, 3), (41, 5.3, 12, 0)]
    return np.array(rows, F)


SIZES = [F(0), F(1), below(1), F(3), below(3), F(7), below(7)]


def orientation_size_table():
    """size 0 (s = 0: every sample is the keypoint's own pixel), and sizes on both sides of the steps of (int)(size / 2 + 0.5): 1, 3 and
    7 give s = 1, 2 and 4; one float32 below 3 and 7 gives 1 and 3, but one below 1 gives 1 again: 0.49999997 + 0.5 is a tie in float32
    and rounds to 1"""
    return np.array([(30.4, 33.7, size, lev) for lev in (1, 2) for size in SIZES], F)


# ---------------------------------------------------------------------------------------------------------------- descriptors
HOT_X, HOT_Y = 42, 12      # 10 to the right of and 20 above the keypoint at (32, 32): a sample of scale 2 and of scale 5 at angle 0
DESC_ANGLES = [F(0), F(np.pi / 2), F(6.28)]


def descriptor_onehot(which):
    """(Lx, Ly, table): one pixel of Lx (which = 0) or of Ly (1) is 1, at level 1; keypoints at (32, 32), scale 2 and 5, three angles"""
    Lx, Ly = np.zeros((NLEV, HK, WK), F), np.zeros((NLEV, HK, WK), F)
    (Lx, Ly)[which][1, HOT_Y, HOT_X] = 1
    table = np.array([(32, 32, 2 * s, 1, a) for s in (2, 5) for a in DESC_ANGLES], F)
    return Lx, Ly, table


def descriptor_edge_table():
    """corners and sides at scale 6: most of the 24 x 24 pattern of 6-pixel steps is clamped"""
    ang = [0.3, 1.1, 2.0, 2.9, 3.7, 4.6, 5.4, 6.1]
    return np.array([(x, y, 12, lev, a) for lev, (x, y), a in zip([0, 1, 2, 3] * 2, EDGE_POSITIONS, ang)], F)


def descriptor_batch_table(n=65):
    rng = np.random.default_rng(23)
    return np.column_stack([rng.uniform(0, WK - 1, n), rng.uniform(0, HK - 1, n), rng.uniform(0, 14, n), rng.integers(0, NLEV, n),
                            rng.uniform(0, 2 * np.pi, n)]).astype(F)


# -------------------------------------------------------------------------------------------------------------- stage entries
STAGE_SHAPES = [(3, 3), (3, 70), (70, 3), (65, 4), (64, 5), (129, 7)]        # width x height
TAP_SIGMAS = [0.6, 0.9, 1.0, 1.6, 2.0, 2.3, 2.6]                            # 1, 3, 5, 9, 11, 13, 15 taps


def tap_sets():
    sets = [KO.gaussian_taps(s) for s in TAP_SIGMAS]
    assert [len(t) for t in sets] == [1, 3, 5, 9, 11, 13, 15]
    sets.append(np.random.default_rng(5).uniform(-1, 1, 7).astype(F))         # no symmetry: the order of the taps shows
    return sets


def plane(w, h, seed=0):
    return np.random.default_rng(1000 * w + h + seed).standard_normal((h, w)).astype(F)


def bin_edge_plane(h, w):
    """moduli b / 300 for b = 1 .. 300 in the interior of an h x w plane, zero elsewhere: 300 x (m / hmax) sits on or beside an integer"""
    lx = np.zeros((h, w), F)
    v = (np.arange(1, 301, dtype=np.float64) / 300).astype(F)
    inner = np.zeros((h - 2) * (w - 2), F)
    inner[:300] = v
    lx[1:-1, 1:-1] = inner.reshape(h - 2, w - 2)
    return lx


# ------------------------------------------------------------------------------------------------------------ small pictures
SMALL_PICTURES = [(70, 6, 2, 2), (6, 70, 2, 2), (6, 6, 2, 2), (23, 23, 4, 4), (23, 130, 4, 4)]      # width, height, octaves, sublevels
STRIP_SEED = 1


@functools.lru_cache(maxsize=None)
def small_picture(w, h):
    import kaze_pictures as P
    return P.blobs(w, h, 300 + STRIP_SEED + w + h, n=max(4, (w * h) // 100))


@functools.lru_cache(maxsize=None)
def small_oracle(w, h, no, ns):
    return KO.detect(small_picture(w, h), no, ns)
