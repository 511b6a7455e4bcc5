"""Stereo pairs that leave the SGM stage something to decide, the cases built on them, and a numpy restatement of the selection.

synth.make_pair ramps the true disparity by 0.6 D over the picture's height: at the small heights the large-D cases of
test_sgm_gpu.py use, no disparity matches a cost window and S is one constant (NOTES/traps.md).  The scenes here vary the disparity
over the COLUMNS instead, as a staircase through the indices a selection kernel can get wrong (targets), so that a picture of twenty
rows carries every one of them:

  terrace         integer-hash texture, right(x) = left(x - d(x)), independent noise per camera
  smooth_terrace  the same staircase plus make_pair's two small sines, through synth._tex: sub-pixel disparities
  periodic        the terrace over a texture (and left-camera noise) of period P in x: the costs at d and d + P are exactly equal,
                  but for one grey level on a seventh of the left pixels, which makes the two NEARLY equal in most places

Conventions are those of test_sgm_gpu.py: (right, left) pictures, a disparity INDEX d stands for the disparity d + min_disp, and the
oracle sees the pictures padded by D columns (pad).  Data generation and test arithmetic only.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

from wass_amd import synth

INVALID_COST = 0x7FFF
LR_OFF = 4000                                                   # a disp12_max_diff no pair of disparities exceeds: the check never fires
STEP = 12                                                       # columns per stair
# a 13 x 13 window that straddles two stairs matches at neither disparity; at make_pair's full contrast that costs enough to saturate
# the sum of eight paths in over a tenth of the pixels (the pre-filter clips the gradient, so the share falls only well below 0.6)
SMOOTH_CONTRAST = 0.3


# --------------------------------------------------------------------------- inputs
def nslots(D: int) -> int:
    """V: disparities per lane, 2 * NP."""
    return 2 * ((D + 127) // 128)


def targets(D: int):
    """The disparity indices a case must make win: both ends, the slots on either side of a lane boundary (V), of d = 64
    and of every 128-slot boundary, and the last slots of the last lane."""
    V = nslots(D)
    t = [0, 1, 2, V - 1, V, V + 1, 2 * V - 1, 2 * V, 63, 64, 65, D // 2, D - V - 1, D - V, D - 3, D - 2, D - 1]
    for k in range(D // 128 + 2):
        t += [128 * k - 1, 128 * k, 128 * k + 1]
    return sorted({int(d) for d in t if 0 <= d < D})


def staircase(D: int, min_disp: int):
    """(starts, disparities, width): stair k holds the disparity targets(D)[k] + min_disp from column starts[k] on, STEP columns or
    more wide, and starts no earlier than disparity + 2, so that its match lies inside the left picture."""
    starts, disps, pos = [], [], 0
    for t in targets(D):
        s = max(pos, t + min_disp + 2)
        starts.append(s); disps.append(t + min_disp)
        pos = s + STEP
    return np.array(starts), np.array(disps), pos


def stair_disparity(D: int, min_disp: int):
    """d(x) of the staircase as an int64 row, and the picture's width."""
    starts, disps, w = staircase(D, min_disp)
    k = np.searchsorted(starts, np.arange(w), side="right") - 1
    return disps[np.maximum(k, 0)].astype(np.int64), w


def _u32(a):
    return (np.asarray(a, np.int64) & 0xFFFFFFFF).astype(np.uint64)


def hash_tex(x, y, amp: int = 60):
    """Integer-hash texture of two-pixel blocks, `amp` grey levels, at integer coordinates of either sign."""
    m = np.uint64(0xFFFFFFFF)
    v = ((_u32(np.asarray(x) >> 1) * np.uint64(73856093)) & m) ^ ((_u32(np.asarray(y) >> 1) * np.uint64(19349663)) & m)
    v ^= v >> np.uint64(13); v = (v * np.uint64(0x5BD1E995)) & m; v ^= v >> np.uint64(15)
    return 90 + (v % np.uint64(amp)).astype(np.int64)


def _noise(seed: int, cam: int, y, x):
    """synth._hash_noise at coordinate arrays (x may be any non-negative column): integer noise in [-3, 3]."""
    h, w = int(np.max(y)) + 1, int(np.max(x)) + 1
    return synth._hash_noise(seed, cam, h, w)[y, x]


def _u8(a):
    return np.ascontiguousarray(np.clip(np.rint(a), 1, 254).astype(np.uint8))


def terrace(D: int, h: int, min_disp: int = 1, seed: int = 0, period: int = 0):
    """(right, left) u8: right(x) = left(x - d(x)) over hash_tex, d the staircase, noise of +-3 grey levels per camera.  period > 0:
    the left picture, noise included, has that period in x (the `periodic` scene)."""
    d, w = stair_disparity(D, min_disp)
    x = np.arange(w, dtype=np.int64)[None, :]; y = np.arange(h, dtype=np.int64)[:, None]
    yy = np.broadcast_to(y, (h, w))
    wrap = (lambda c: np.mod(c, period)) if period else (lambda c: c)
    sd = seed + 977 * D + min_disp
    left = hash_tex(wrap(x), y) + _noise(sd, 0, yy, np.broadcast_to(wrap(x), (h, w)))
    right = hash_tex(wrap(x - d[None, :]), y) + _noise(sd, 1, yy, np.broadcast_to(x, (h, w)))
    return _u8(right), _u8(left)


def periodic_period(D: int) -> int:
    return 100 if D >= 1024 else 37


def periodic(D: int, h: int, min_disp: int = 1, seed: int = 0):
    """The terrace over a left picture of period P in x, one grey level added to a seventh of its pixels without that period.  Where
    no such pixel weighs on them S[d] and S[d + P] are exactly equal: ties, which go to the lower d, and uniqueness rejections by a
    d that lies lanes away.  Elsewhere they differ by a few per cent of the minimum, spread over the thresholds of the uniqueness test,
    so that some pixels meet S[d] * (100 - uniq) == minS * 100 exactly (the exactly periodic picture leaves that to one pixel in
    thousands)."""
    right, left = terrace(D, h, min_disp, seed, period=periodic_period(D))
    bump = synth._hash_noise(seed + 31 * D, 2, h, left.shape[1]) == 3
    return right, _u8(left.astype(np.int64) + bump)


def smooth_terrace(D: int, h: int, min_disp: int = 1, seed: int = 0):
    """The staircase plus make_pair's two sines (0.4 px over x, 0.2 px over y), sampled through make_pair's analytic texture."""
    d, w = stair_disparity(D, min_disp)
    params = synth.texture_params(seed + D)
    x = np.arange(w, dtype=np.float64)[None, :]; y = np.arange(h, dtype=np.float64)[:, None]
    dd = d[None, :] + 0.4 * np.sin(2 * np.pi * x / 97.0) + 0.2 * np.sin(2 * np.pi * y / 61.0)
    sd = (synth.SEED_BASE + seed + D) & ((1 << 64) - 1)
    tex = lambda u: 128.0 + SMOOTH_CONTRAST * (synth._tex(u, y, params) - 128.0)
    left = tex(x) + synth._hash_noise(sd, 0, h, w)
    right = tex(x - dd) + synth._hash_noise(sd, 1, h, w)
    return _u8(right), _u8(left)


SCENES = {"terrace": terrace, "smooth_terrace": smooth_terrace, "periodic": periodic}


def pad(right, left, D: int, off: int = 0):
    """The padded pictures wass_stereo hands to cv::StereoSGBM (wass_stereo.cpp:820-831), as test_sgm_gpu._pad."""
    h, w = right.shape
    offp, comp = max(off, 0), max(-off, 0)
    Wp = w + D + offp
    R = np.zeros((h, Wp), np.uint8); L = np.zeros((h, Wp), np.uint8)
    R[:, D:D + w] = right
    L[:, D + offp - comp:D + offp - comp + w] = left
    return R, L


# --------------------------------------------------------------------------- cases
Case = namedtuple("Case", "family scene D h ndirs win min_disp uniq d12 off")
Case.id = property(lambda c: f"{c.scene}-D{c.D}-h{c.h}-p{c.ndirs}-w{c.win}-m{c.min_disp}-u{c.uniq}-l{c.d12}" + (f"-o{c.off}" if c.off else ""))

ALL_D = [64, 128, 160, 256, 272, 384, 512, 640, 768, 896, 1024]          # every NP from 1 to 8; D no multiple of V at 160 and 272
PATHS = [5, 8]
SELECTION_ROWS = [(5, 10, 1), (13, 1, 1), (9, 15, 2), (3, 0, 0)]         # win, uniq_ratio, min_disp
PERIODIC_UNIQ = [0, 1, 10, 40, 99, 100]
LR_DIFFS = [-1, 0, 1, 2, 5]
# heights of test_sgm_gpu.CASES whose half chains hold two or more full checkpoint segments, per D
STEADY_H = {256: 64, 384: 48, 512: 64, 640: 40, 768: 40, 896: 40, 1024: 40}
FUSED5 = [(192, 131), (256, 37)]                                         # test_sgm_gpu._FUSED5_CASES: D, h


def periodic_height(D: int) -> int:
    return 40 if D <= 128 else 20


def selection_cases():
    return [Case("selection", "terrace", D, 20, n, win, m, u, LR_OFF, 0) for D in ALL_D for n in PATHS for (win, u, m) in SELECTION_ROWS]


def subpixel_cases():
    return [Case("subpixel", "smooth_terrace", D, 20, n, win, 1, 1, LR_OFF, 0) for D in ALL_D for n in PATHS for win in (5, 13)]


def periodic_cases():
    """Window 3: small costs, so that exact equalities in the uniqueness test are frequent; the two narrowest pictures are 40 rows high
    to hold enough pixels for them."""
    return [Case("periodic", "periodic", D, periodic_height(D), n, 3, 1, u, LR_OFF, 0) for D in ALL_D for n in PATHS for u in PERIODIC_UNIQ]


def lrcheck_cases():
    out = [Case("lrcheck", "terrace", D, 20, n, 5, 1, 1, l, 0) for D in ALL_D for n in PATHS for l in LR_DIFFS]
    return out + [Case("lrcheck", "terrace", 272, 20, 8, 5, 1, 1, -1, 3), Case("lrcheck", "terrace", 272, 20, 5, 5, 1, 1, -1, -4)]


def steady_cases():
    out = [Case("steady", "smooth_terrace", D, h, n, win, 1, 1, LR_OFF, 0) for D, h in STEADY_H.items() for n in PATHS for win in (13, 5)]
    return out + [Case("steady", "smooth_terrace", D, h, 5, win, 1, 1, LR_OFF, 0) for D, h in FUSED5 for win in (13, 5)]


def all_cases():
    return selection_cases() + subpixel_cases() + periodic_cases() + lrcheck_cases() + steady_cases()


def make(c: Case):
    """(right, left) of a case."""
    return SCENES[c.scene](c.D, c.h, c.min_disp)


def sgm_params(c: Case):
    """wass_sgm_params of a case: default_sgm_params' P1 and P2 for its window."""
    from wass_amd import default_sgm_params
    p = default_sgm_params(c.D, ndirs=c.ndirs, win=c.win, min_disp=c.min_disp, disp_offset=c.off)
    p.uniq_ratio = c.uniq
    p.disp12_max_diff = c.d12
    return p


def oracle_params(O, p):
    return O.SgbmParams(p.min_disp, p.num_disp, p.win, p.P1, p.P2, p.uniq_ratio, p.disp12_max_diff,
                        p.prefilter_cap, p.speckle_win, p.speckle_range, p.ndirs)


def run_oracle(O, c: Case):
    """(right, left, params, disp, stats, C, S, raw) of a case on the CPU oracle."""
    right, left = make(c)
    p = sgm_params(c)
    R, L = pad(right, left, c.D, c.off)
    disp, st, Co, So, rawo = O.sgbm_compute(R, L, oracle_params(O, p), dump=True)
    return right, left, p, disp, st, Co, So, rawo


# --------------------------------------------------------------------------- the selection, restated
MISTAKES = ("cyclic", "tie_high", "uniq_le", "exempt_wide", "exempt_narrow", "padded", "trunc", "rv_small_x", "lr_ge")


def winners(S, D, uniq, mistake=None):
    """Per pixel of S (h, width1, D): (best, minS, ok, a, c) -- the winning index (ties to the lowest d; -1 where every entry is
    0x7FFF), its cost, whether it passes the uniqueness test, and the costs of its two neighbours (0 where there is none)."""
    S = S.astype(np.int32)
    h, w1, _ = S.shape
    V = nslots(D)
    minS = S.min(-1)
    best = (D - 1 - np.argmin(S[..., ::-1], -1)) if mistake == "tie_high" else np.argmin(S, -1)
    best = np.where(minS >= INVALID_COST, -1, best)              # "if (Sval < minS)" never fires when every S is MAX_COST
    q = 100 - uniq
    T = (minS * 100)[..., None]
    low = (S * q <= T) if mistake == "uniq_le" else (S * q < T)
    reach = {"exempt_wide": 2, "exempt_narrow": 0}.get(mistake, 1)
    dist = np.abs(np.arange(D)[None, None, :] - best[..., None])
    ia, ic = best - 1, best + 1
    if mistake == "cyclic":                                      # the neighbour taken inside the winner's own lane of V slots
        ia = np.where(best % V == 0, best + V - 1, ia)
        ic = np.where(best % V == V - 1, best - V + 1, ic)
        dist = np.where((np.arange(D)[None, None, :] == ia[..., None]) | (np.arange(D)[None, None, :] == ic[..., None]), 1,
                        np.where(dist == 1, 2, dist))
    bad = (low & (dist > reach)).any(-1)
    if mistake == "padded" and D % (64 * V):
        # Slots D .. 64 V - 1 are no candidates.  While they hold 0x7FFF, counting them changes nothing for uniq_ratio <= 100: where
        # 0x7FFF * q < 100 minS, every real slot (S <= 0x7FFF, q >= 0) passes the same test, and one of them lies outside best +- 1.
        # The mistake that shows is counting them with what a register that was never loaded holds, zero.
        bad |= 0 < minS * 100
    take = lambda i: np.take_along_axis(S, np.clip(i, 0, D - 1)[..., None], -1)[..., 0]
    a = np.where((best >= 1) & (ia < D), take(ia), 0)
    c = np.where((best >= 0) & (best < D - 1) & (ic >= 0), take(ic), 0)
    return best, minS, ~bad, a, c


def select(S, params, mistake=None):
    """The raw disparity map (h, Wp) of Appendix A.5 from the aggregated volume S (h, width1, D): winner, uniqueness, sub-pixel
    interpolation, right-view map and left-right test.  `params` has min_disp, num_disp, uniq_ratio and disp12_max_diff;
    `mistake` names one deliberate error (MISTAKES) a rewrite of the selection kernels could make."""
    assert mistake is None or mistake in MISTAKES
    D, minD = params.num_disp, params.min_disp
    uniq = params.uniq_ratio if params.uniq_ratio >= 0 else 10
    d12 = params.disp12_max_diff if params.disp12_max_diff > 0 else 1
    h, w1, _ = S.shape
    minX1 = minD + D
    Wp = w1 + minX1
    INV = (minD - 1) * 16
    best, minS, ok, a, c = winners(S, D, uniq, mistake)
    ok = ok & (best >= 0)                                        # an all-0x7FFF pixel neither scatters nor gets a disparity
    # sub-pixel: C division (towards zero) of a numerator of either sign
    den2 = np.maximum(a + c - 2 * minS, 1)
    num = (a - c) * 16 + (0 if mistake == "trunc" else den2)
    frac = np.sign(num) * (np.abs(num) // (den2 * 2))
    d16 = best * 16 + np.where((best > 0) & (best < D - 1), frac, 0) + minD * 16
    # right-view map: the cheapest pixel that lands on a column, at equal cost the one with the larger x (it is visited first)
    yy, xx = np.nonzero(ok)
    X2 = xx + D - best[yy, xx]
    order = xx if mistake == "rv_small_x" else (w1 - 1 - xx)
    key = np.full(h * Wp, np.iinfo(np.int64).max, np.int64)
    np.minimum.at(key, yy * Wp + X2, minS[yy, xx].astype(np.int64) * 65536 + order)
    key = key.reshape(h, Wp)
    hit = key != np.iinfo(np.int64).max
    xw = np.where(hit, key % 65536, 0)
    xw = xw if mistake == "rv_small_x" else (w1 - 1 - xw)
    disp2 = np.where(hit, best[np.arange(h)[:, None], np.clip(xw, 0, w1 - 1)] + minD, INV)
    # left-right test on the fixed-point map, both roundings of the disparity
    raw = np.full((h, Wp), INV, np.int64)
    raw[:, minX1:] = np.where(ok, d16, INV)
    cols = np.arange(Wp)[None, :]
    rows = np.arange(h)[:, None]
    far = (lambda v: v >= d12) if mistake == "lr_ge" else (lambda v: v > d12)

    def fails(dr):
        x2 = cols - dr
        inside = (x2 >= 0) & (x2 < Wp)
        d2 = disp2[rows, np.clip(x2, 0, Wp - 1)]
        return inside & (d2 >= minD) & far(np.abs(d2 - dr))
    rej = (raw != INV) & fails(raw >> 4) & fails((raw + 15) >> 4)
    rej[:, :minX1] = False
    return np.where(rej, INV, raw).astype(np.int16)
