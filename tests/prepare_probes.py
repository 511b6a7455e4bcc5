"""Inputs of the prepare-stage edge suite: tests/test_prepare_edges.py holds them in place on the CPU (the direct restatement of
tests/prepare_direct.py against the C oracle, and what makes each probe a probe), tests/test_prepare_edges_gpu.py runs them through the
kernels of rectify.hip and clahe.hip.  Every probe is a dict with a name, a kind ("remap", "warp", "undistort", "clahe") and that kind's
arguments; probes() builds them once, read-only.  No global random state, no files.

  calibrated K   camera matrices whose closed-form inverse has ir[8] = (fx fy) * (1 / (fx fy)) != 1 in fp64, and one where it is 1;
  horizons       homographies whose denominator W reaches 0 exactly, comes within 2^-30 of it, and changes sign, one of them 300 x 5 so
                 that the warp's block is 204 columns wide; two affine warps whose x lies within an ulp of a 1/64-pixel tie, where the
                 per-block evaluation of the coordinates rounds differently from one evaluation per row;
  windows        every start of the 4 x 4 (bicubic) and 2 x 2 (bilinear) window from wholly outside through each partial count to wholly
                 inside, on both sides of both axes, at the fractions 0, 1/32, 16/32, 31/32, on sources 1, 2, 3, 4, 5 and 9 pixels wide
                 and tall; lattices on which all 1024 phases occur at a wholly-inside window; a map of exact ties; a map beyond int16;
  wrap           a 5000 x 5 undistortion whose coordinates leave int16 and wrap back into the picture;
  CLAHE          rectangular grids, tiles worked out by hand for seven residuals, a tile of area 510, tiny tiles, a picture smaller than
                 the grid."""
import functools
import itertools

import numpy as np

import prepare_direct as D

F = np.float32
SRC_W, SRC_H = 97, 61
FRACS = (0.0, 1 / 32, 16 / 32, 31 / 32)
SIZES = ((1, 1), (2, 3), (3, 2), (4, 5), (5, 4), (9, 9), (1, 9), (9, 1))         # every size of 1, 2, 3, 4, 5, 9 along each axis
RESIDUALS = (0, 1, 3, 85, 128, 129, 255)


def picture(w, h, seed=0):
    """values 1 .. 255: a tap inside the picture is never 0, a tap outside always"""
    return np.random.default_rng([seed, w, h]).integers(1, 256, (h, w), dtype=np.uint8)


def texture(w, h, seed=0, lo=40, span=90):
    """a narrow, uneven histogram: clipping has something to clip"""
    rng = np.random.default_rng([seed, w, h, 7])
    y, x = np.mgrid[0:h, 0:w]
    v = lo + span * (0.5 + 0.5 * np.sin(x / 5.3 + y / 9.1)) * (0.6 + 0.4 * np.cos(y / 4.7)) + rng.normal(0, 4, (h, w))
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


# ---- calibrated camera matrices ---------------------------------------------------------------------------------------------------------
def _K(fx, fy, cx, cy):
    return np.array([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]])


# name -> (K, w, h): found by drawing fx, fy from [500, 5000) (and one pair of short focal lengths, where the distortion moves a small
# picture's pixels by several pixels) and keeping those with ir[8] != 1; "round" is the form every earlier test used, ir[8] == 1
CAMERAS = {
    "diag1234": (_K(1234.5, 1234.5, 44.7, 35.2), 90, 70),
    "f3366": (_K(3366.3, 1714.0, 2499.7, 2.3), 5000, 5),
    "f3783": (_K(3783.4, 1290.5, 128.6, 16.2), 258, 33),
    "f1107": (_K(1107.9, 3746.7, 33.1, 20.6), 64, 48),
    "short": (_K(77.7, 80.3, 44.7, 35.2), 90, 70),
    "round": (_K(0.9 * 90, 0.92 * 90, 90 / 2 - 0.3, 70 / 2 + 0.2), 90, 70),
    "round2010": (_K(2010.0, 2005.0, 31.5, 24.25), 64, 48),
}
DISTS = {0: [], 4: [-0.2, 0.05, 0.001, -0.002], 5: [-0.25, 0.08, 0.002, -0.001, 0.01], 8: [0.1, -0.02, 0, 0, 0.003, 0.01, -0.005, 0.001],
         12: [-0.2, 0.05, 0.001, -0.002, 0.01, 0.0, 0.0, 0.0, 0.002, -0.001, 0.0015, 0.0005]}
# the table cache: A, B, A, C, A, B over (camera, w, h); A and B share K and differ in size.  Round matrices: the cache is not the refusal
CACHE_SEQUENCE = (("round", 90, 70), ("round", 64, 48), ("round", 90, 70), ("round2010", 90, 70), ("round", 90, 70), ("round", 64, 48))


def ir8(K):
    return D.inv33(K)[8]


def refused_fraction(n=20000, seed=0):
    """how many of n matrices with fx, fy uniform in [500, 5000) have ir[8] != 1"""
    rng = np.random.default_rng(seed)
    return sum(ir8(_K(fx, fy, 44.7, 35.2)) != 1.0 for fx, fy in rng.uniform(500, 5000, (n, 2))) / n


def wrap_case():
    w, h = 5000, 5
    return dict(name="wrap", kind="undistort", src=picture(w, h, 3), K=_K(0.9 * w, 0.92 * w, w / 2 - 0.3, 2.0), dist=[80.0, 0, 0, 0, 0])


# ---- warps ----------------------------------------------------------------------------------------------------------------------------------
def _inv(M):
    return np.array(D.inv33(M)).reshape(3, 3)


def horizon_cases():
    """name, M (destination to source), dw, dh, roi: the ROI's left edge is no multiple of bw0 and the ROI holds the column where W = 0"""
    e = 2.0 ** -30
    return [("horizon_zero", [[.5, 0, 0], [0, 1, 0], [-1 / 128, 0, 1]], 160, 40, (101, 3, 50, 30)),
            ("horizon_tiny", [[.5, 0, 0], [0, 1, 0], [-1 / 128, 0, 1 + e]], 160, 40, (101, 3, 50, 30)),
            ("horizon_204", [[.5, 0, 3], [0, .75, 2], [-1 / 128, 0, 1]], 300, 5, (77, 1, 150, 3))]


def tie_cases():
    """x = a * column + 1/64 + m1 (row - mid) with m1 far below an ulp of x: which side of the tie a pixel falls on is decided by the order
    in which the block's X0 and the offset inside the block are rounded"""
    out = []
    for name, a, s, dw, dh, roi in (("tie_64", 0.5, 0.11, 160, 40, (67, 5, 90, 30)), ("tie_204", 0.25, 0.3, 300, 5, (131, 1, 160, 3))):
        m1 = s * 2.0 ** -47
        out.append((name, [[a, m1, 1 / 64 - m1 * (dh // 2)], [0, 1, 0.25], [0, 0, 1]], dw, dh, roi))
    return out


def _warp(name, M, dw, dh, roi=None, src=None):
    return dict(name=name, kind="warp", src=picture(SRC_W, SRC_H, 1) if src is None else src, H=_inv(M), dw=dw, dh=dh, roi=roi)


def border_warps():
    """pure translations by -5 + fraction: the 2 x 2 window starts at -5 .. size + 4 along each axis"""
    out = []
    for sw, sh in SIZES:
        for fx, fy in itertools.product(FRACS, FRACS):
            out.append(_warp(f"border_warp_{sw}x{sh}_{int(fx * 32)}_{int(fy * 32)}", [[1, 0, -5 + fx], [0, 1, -5 + fy], [0, 0, 1]], sw + 10, sh + 10,
                             src=picture(sw, sh, 2)))
    return out


def lattice_warp():
    """x = 33/32 column + 2, y = 33/32 row + 1: phase (row % 32, column % 32), every window inside the 97 x 61 source"""
    return _warp("lattice_warp", [[33 / 32, 0, 2], [0, 33 / 32, 1], [0, 0, 1]], 64, 48, roi=(5, 3, 41, 37))


# ---- maps -------------------------------------------------------------------------------------------------------------------------------------
def _remap(name, src, mx, my, roi=None):
    return dict(name=name, kind="remap", src=src, mx=np.ascontiguousarray(mx, F), my=np.ascontiguousarray(my, F), roi=roi)


def border_maps():
    out = []
    for sw, sh in SIZES:
        xs = [i + f for i in range(-5, sw + 5) for f in FRACS]
        ys = [i + f for i in range(-5, sh + 5) for f in FRACS]
        mx, my = np.meshgrid(np.array(xs, F), np.array(ys, F))
        out.append(_remap(f"border_map_{sw}x{sh}", picture(sw, sh, 2), mx, my, roi=(3, 1, len(xs) - 7, len(ys) - 4)))
    return out


def _lattice(dw, dh, offset):
    y, x = np.mgrid[0:dh, 0:dw]
    ix, iy = 1 + (3 * x + 5 * y) % 90, 1 + (7 * x + 2 * y) % 55          # the window 0 .. 93 + 3, 0 .. 57 + 3: inside 97 x 61
    return ix + (x % 32) / 32 + offset, iy + (y % 32) / 32 + offset


def lattice_map():
    """128 x 96: every one of the 1024 phases twelve times, each time at another wholly-inside window"""
    mx, my = _lattice(128, 96, 0.0)
    return _remap("lattice_map", picture(SRC_W, SRC_H, 1), mx, my, roi=(31, 7, 65, 33))


def ties_map():
    """the same 1/64 of a pixel further: map * 32 is k + 0.5 exactly, in both axes"""
    mx, my = _lattice(64, 32, 1 / 64)
    return _remap("ties_map", picture(SRC_W, SRC_H, 1), mx, my)


def extreme_map():
    """beyond int16: rows 0-7 and 8-15 lie 65536 pixels off in x and in y and would wrap to where they came from; row 16 holds values
    whose integer part saturates, two of them beyond the int32 range of map * 32 (outside either way)"""
    rng = np.random.default_rng(8)
    mx = rng.integers(0, 95 * 32, (24, 60)) / 32
    my = rng.integers(0, 59 * 32, (24, 60)) / 32
    mx[0:8] += 65536
    my[8:16] -= 65536
    mx[16, :12] = [-1e6, 1e6, -40000, 40000, -1.5, -2.96875, 96.0, 97.96875, 98.0, 3e9, -3e9, 32768.5]
    my[17, :8] = [-1e6, 1e6, -2.96875, 61.0, 59.5, -1.0, 3e9, -3e9]
    return _remap("extreme_map", picture(SRC_W, SRC_H, 1), mx, my)


# ---- CLAHE ------------------------------------------------------------------------------------------------------------------------------------
def _clahe(name, src, clip, tx, ty):
    return dict(name=name, kind="clahe", src=src, clip=float(clip), tiles_x=tx, tiles_y=ty)


_SHAPE = {257: (257, 1), 258: (43, 6), 259: (37, 7), 260: (20, 13), 261: (29, 9), 342: (19, 18), 343: (49, 7), 385: (35, 11), 386: (193, 2),
          387: (43, 9), 512: (32, 16), 513: (27, 19)}


def hand_cases():
    """(probe, levels, residual): one tile, clip forced to 1 (clip limit 0.4 at an area below 640), filled with one level (area 257 + r) or
    with two (area 258 + r), so that 256 + r counts are cut off: a batch of 1 and the residual r"""
    out = []
    for r in RESIDUALS:
        w, h = _SHAPE[257 + r]
        out.append((_clahe(f"hand_const_r{r}", np.full((h, w), 100, np.uint8), 0.4, 1, 1), (100,), r))
        w, h = _SHAPE[258 + r]
        img = np.full((h, w), 100, np.uint8)
        img.ravel()[1::3] = 201
        out.append((_clahe(f"hand_two_r{r}", img, 0.4, 1, 1), (100, 201), r))
    return out


def hand_answer(levels, residual, area):
    """level -> output, from the definition: every level's count is cut to 1, every bin gets the batch of 1, bins 0, step, 2 step, ... one
    more; the table is rint(float32(cumulative) * (255.0f / area)) and a single tile blends with itself"""
    step = max(256 // residual, 1) if residual else 1
    out = {}
    for v in levels:
        extra = sum(1 for k in range(residual) if k * step < 256 and k * step <= v)
        cum = (v + 1) + sum(1 for u in levels if u <= v) + extra
        out[v] = int(np.clip(np.rint(F(cum) * (F(255) / F(area))), 0, 255))
    return out


def clahe_cases():
    out = [_clahe("grid_7x3", texture(70, 50), 2.0, 7, 3), _clahe("grid_3x7", texture(70, 50), 2.0, 3, 7),
           _clahe("grid_1x9", texture(33, 47), 3.0, 1, 9), _clahe("grid_9x1", texture(33, 47), 3.0, 9, 1),
           _clahe("grid_150x2", texture(70, 50), 2.0, 150, 2), _clahe("grid_2x150", texture(70, 50), 40.0, 2, 150),
           _clahe("ragged_5x4", texture(131, 67), 3.5, 5, 4),
           _clahe("area510", picture(30, 17, 5), 0.0, 1, 1), _clahe("area510_clip", picture(30, 17, 5), 4.0, 1, 1),
           _clahe("area510_2x2", picture(60, 34, 6), 0.0, 2, 2), _clahe("area510_3x2_clip", texture(90, 34, 6, 0, 250), 2.5, 3, 2),
           _clahe("tiny_clip", picture(12, 10, 7), 0.5, 1, 1), _clahe("tiny_noclip", picture(12, 10, 7), 0.0, 1, 1),
           _clahe("tiny_tiles", texture(24, 20), 1.0, 3, 2),
           _clahe("narrow_5x40", texture(5, 40), 2.0, 7, 3), _clahe("flat_2x31", texture(31, 2), 2.0, 3, 5), _clahe("one_pixel", picture(1, 1, 1), 2.0, 2, 3)]
    return out + [p for p, _, _ in hand_cases()]


# ---- everything, once ---------------------------------------------------------------------------------------------------------------------------
def undistort_cases():
    out = []
    for cam, (K, w, h) in CAMERAS.items():
        for n, dist in DISTS.items():
            out.append(dict(name=f"undistort_{cam}_{n}", kind="undistort", src=picture(w, h, 4), K=K, dist=list(dist), camera=cam))
    for cam in ("short", "round"):
        out.append(dict(name=f"undistort_{cam}_strong", kind="undistort", src=picture(90, 70, 4), K=CAMERAS[cam][0], dist=[3.0, -8.0, 0.1, 0.1, 5.0],
                        camera=cam))
    return out


def _freeze(p):
    for v in p.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def probes():
    """name -> probe, in a fixed order"""
    out = undistort_cases() + [wrap_case()]
    out += [_warp(*c) for c in horizon_cases() + tie_cases()] + [lattice_warp()] + border_warps()
    out += border_maps() + [lattice_map(), ties_map(), extreme_map()]
    out += clahe_cases()
    names = [p["name"] for p in out]
    assert len(set(names)) == len(names)
    return {p["name"]: _freeze(p) for p in out}


def of_kind(kind):
    return [p for p in probes().values() if p["kind"] == kind]


# the mistake -> the probes built for it
SWITCH_PROBES = {
    "truncate": ("ties_map", "horizon_204", "undistort_round_5"),
    "swap_phase": ("lattice_map", "lattice_warp", "undistort_round_strong"),
    "no_fixup": ("lattice_map",),               # the bilinear table needs the fix-up in its zero-phase entry alone, where no u8 result changes
    "saturate_undistort": ("wrap",),
    "wrap_remap": ("extreme_map", "horizon_tiny"),
    "one_block": ("tie_64", "tie_204"),
    "w0_as_inf": ("horizon_zero", "horizon_204"),
    "transpose_grid": ("grid_7x3", "grid_3x7", "grid_150x2"),
    "no_residual_step": ("hand_const_r3", "hand_two_r85", "hand_const_r128", "ragged_5x4"),
    "lut_half_up": ("area510", "area510_2x2"),
}
assert set(SWITCH_PROBES) == set(D.SWITCHES)


def run_direct(p, **switch):
    """the restatement's answer for a probe (the whole destination), with at most one mistake switched on"""
    k = p["kind"]
    if k == "remap":
        return D.remap_cubic(p["src"], p["mx"], p["my"], **switch)
    if k == "warp":
        return D.warp_linear(p["src"], p["H"], p["dw"], p["dh"], **switch)
    if k == "undistort":
        return D.undistort(p["src"], p["K"], p["dist"], **switch)
    return D.clahe(p["src"], p["clip"], p["tiles_x"], p["tiles_y"], **switch)


def run_oracle(O, p):
    k = p["kind"]
    if k == "remap":
        return O.remap_cubic(p["src"], p["mx"], p["my"])
    if k == "warp":
        return O.warp_perspective(p["src"], p["H"], p["dw"], p["dh"])
    if k == "undistort":
        return O.undistort(p["src"], p["K"], p["dist"] if len(p["dist"]) else [0.0] * 4)          # no coefficients: four zeros
    return O.clahe(p["src"], p["clip"], p["tiles_x"], p["tiles_y"])


_ORACLE = {}


def oracle_answer(O, p):
    """computed once per probe and shared, read-only"""
    if p["name"] not in _ORACLE:
        a = run_oracle(O, p)
        a.setflags(write=False)
        _ORACLE[p["name"]] = a
    return _ORACLE[p["name"]]


def crop(a, roi):
    x, y, w, h = roi
    return a[y:y + h, x:x + w]


def switch_bound(O, switch, name):
    """(bound, found on the oracle): the mistake misses the oracle in `found` pixels of the probe; a result that is right misses the
    mistaken variant in at least half of them, and in at least one"""
    p = probes()[name]
    found = int((run_direct(p, **{switch: True}) != oracle_answer(O, p)).sum())
    return max(found // 2, 1), found
