"""numpy restatements of the radiance chain (wass_amd.postproc: remap_lanczos4, radiance, bgimage, radiance_threshold), the table
builder, scene builders and deliberately wrong variants.  Test infrastructure only.

The Lanczos4 sampler restates OpenCV 4.5.5's imgwarp.cpp (interpolateLanczos4, initInterTab2D, remapLanczos4) from knowledge:
cv2 is not available where this was written, so the restatement is UNPINNED against the real OpenCV, like the cubic one of
oracle/rectify_oracle.c.  scripts/pin_with_opencv.py is where a pin would be made.  What is checked without OpenCV: the table
builder equals oracle.orc_inter_tab at ksize 2 and 4, the structure of the table at 8, and the sampler against a float64
Lanczos resampling (tests/test_radiance.py)."""
import math

import numpy as np

F = np.float32
BITS, TAB, SCALE = 5, 32, 1 << 15


# ---- the fixed-point tables -------------------------------------------------------------------------------------------------------
def tab1d(ksize: int, x) -> np.ndarray:
    """interpolateLinear / interpolateCubic / interpolateLanczos4 at phase x (float32), in float32 as the C code computes them"""
    x = F(x)
    if ksize == 2:
        return np.array([F(1) - x, x], F)
    if ksize == 4:
        A, one = F(-0.75), F(1)
        c0 = ((A * (x + one) - F(5) * A) * (x + one) + F(8) * A) * (x + one) - F(4) * A
        c1 = ((A + F(2)) * x - (A + F(3))) * x * x + one
        c2 = ((A + F(2)) * (one - x) - (A + F(3))) * (one - x) * (one - x) + one
        return np.array([c0, c1, c2, one - c0 - c1 - c2], F)
    assert ksize == 8
    c = np.zeros(8, F)
    if x < np.finfo(F).eps:
        c[3] = 1
        return c
    s45 = 0.70710678118654752440084436210485
    cs = [(1, 0), (-s45, -s45), (0, 1), (s45, -s45), (-1, 0), (s45, s45), (0, -1), (-s45, s45)]
    y0 = float(-(x + F(3))) * math.pi * 0.25
    s0, c0 = math.sin(y0), math.cos(y0)
    total = F(0)
    for i in range(8):
        y = float(-(x + F(3) - F(i))) * math.pi * 0.25
        c[i] = F((cs[i][0] * s0 + cs[i][1] * c0) / (y * y))
        total = F(total + c[i])
    inv = F(1) / total
    return (c * inv).astype(F)


def inter_tab(ksize: int, fixup: bool = True) -> np.ndarray:
    """initInterTab2D(fixpt=true): int16 [1024, ksize, ksize], phase (fy, fx) at fy * 32 + fx.  The weights are the float32
    products of the two 1-D tables, scaled by 2^15 and rounded half to even with saturation; where they do not sum to 2^15, the
    difference goes to the largest (or smallest) of the four entries [k/2, k/2 + 2)^2, scanned in OpenCV's order."""
    t1 = np.stack([tab1d(ksize, F(i) * F(1.0 / TAB)) for i in range(TAB)])
    prod = (t1[:, None, :, None] * t1[None, :, None, :]).astype(F) * F(SCALE)            # [fy, fx, ky, kx]
    whole = np.clip(np.rint(prod), -32768, 32767).astype(np.int32).reshape(TAB * TAB, ksize * ksize)
    if not fixup:
        return whole.reshape(TAB * TAB, ksize, ksize).astype(np.int16)
    # as the C code runs: phase by phase into zeroed storage; at ksize 2 the scan looks past the entry into storage that is still
    # zero, and what it writes there the next phase overwrites
    kk, k0 = ksize * ksize, ksize // 2
    flat = np.zeros(TAB * TAB * kk + 64, np.int32)
    for p in range(TAB * TAB):
        it = flat[p * kk:]
        it[:kk] = whole[p]
        diff = int(whole[p].sum()) - SCALE
        if diff == 0:
            continue
        M = m = k0 * ksize + k0
        for k1 in range(k0, k0 + 2):
            for k2 in range(k0, k0 + 2):
                at = k1 * ksize + k2
                if it[at] < it[m]:
                    m = at
                elif it[at] > it[M]:
                    M = at
        at = M if diff < 0 else m
        it[at] -= diff
    return flat[:TAB * TAB * kk].reshape(TAB * TAB, ksize, ksize).astype(np.int16)


_TABS = {}


def lanczos_tab(fixup: bool = True) -> np.ndarray:
    if fixup not in _TABS:
        _TABS[fixup] = inter_tab(8, fixup)
    return _TABS[fixup]


# ---- the sampler ------------------------------------------------------------------------------------------------------------------
def quantise(m, rounding: str = "even"):
    """(q int64, ok): q = round(m * 32) with the product in float32; ok is false where the product is NaN, infinite or outside
    the int32 range (the sampler gives 0 there)"""
    with np.errstate(invalid="ignore", over="ignore"):
        p = np.asarray(m, F) * F(TAB)
        ok = np.isfinite(p) & (np.abs(p) < F(2147483648.0))
        p = np.where(ok, p, F(0))
    q = np.rint(p) if rounding == "even" else np.trunc(p)
    return q.astype(np.int64), ok


def remap_lanczos4(img, mapx, mapy, tab=None, offset: int = 3, rounding: str = "even", swap_phase: bool = False) -> np.ndarray:
    """cv.remap(img u8, mapx, mapy, INTER_LANCZOS4, BORDER_CONSTANT 0), restated.  The keyword arguments make the wrong variants:
    offset 4, rounding 'trunc', a table without the fix-up, the x and y phase exchanged."""
    img = np.asarray(img, np.uint8)
    tab = lanczos_tab() if tab is None else tab
    sh, sw = img.shape
    shape = np.shape(mapx)
    X, okx = quantise(np.ravel(mapx), rounding)
    Y, oky = quantise(np.ravel(mapy), rounding)
    sx = np.clip(X >> BITS, -32768, 32767) - offset
    sy = np.clip(Y >> BITS, -32768, 32767) - offset
    fx, fy = X & (TAB - 1), Y & (TAB - 1)
    phase = fx * TAB + fy if swap_phase else fy * TAB + fx
    out = np.zeros(X.shape[0], np.uint8)
    for a in range(0, X.shape[0], 1 << 16):
        s = slice(a, a + (1 << 16))
        yy = sy[s, None] + np.arange(8)
        xx = sx[s, None] + np.arange(8)
        iny, inx = (yy >= 0) & (yy < sh), (xx >= 0) & (xx < sw)
        pix = img[np.clip(yy, 0, sh - 1)[:, :, None], np.clip(xx, 0, sw - 1)[:, None, :]].astype(np.int64)
        pix *= (iny[:, :, None] & inx[:, None, :])
        v = (pix * tab[phase[s]].astype(np.int64)).sum(axis=(1, 2))
        assert np.abs(v).max(initial=0) < 2 ** 31
        out[s] = np.clip((v + (1 << 14)) >> 15, 0, 255)
    out[~(okx & oky)] = 0
    return out.reshape(shape)


def lanczos_float(img, x, y):
    """float64 Lanczos (a = 4) resampling of img at the real positions (x, y), the 8 x 8 weights normalised to sum 1; positions whose
    window leaves the picture give NaN"""
    img = np.asarray(img, np.float64)
    sh, sw = img.shape
    x, y = np.ravel(x).astype(np.float64), np.ravel(y).astype(np.float64)
    ix, iy = np.floor(x).astype(int), np.floor(y).astype(int)

    def w(frac):
        d = frac[:, None] - (np.arange(8) - 3)
        k = np.sinc(d) * np.sinc(d / 4.0)
        return k / k.sum(axis=1, keepdims=True)

    wx, wy = w(x - ix), w(y - iy)
    inside = (ix - 3 >= 0) & (ix + 4 < sw) & (iy - 3 >= 0) & (iy + 4 < sh)
    ixc, iyc = np.where(inside, ix, 3), np.where(inside, iy, 3)
    pix = img[(iyc[:, None] + np.arange(8) - 3)[:, :, None], (ixc[:, None] + np.arange(8) - 3)[:, None, :]]
    v = (pix * wy[:, :, None] * wx[:, None, :]).sum(axis=(1, 2))
    return np.where(inside, v, np.nan)


# ---- the projection and the radiance ----------------------------------------------------------------------------------------------
def pcam(Pplane, Iw, Ih):
    to_norm = np.array([[2.0 / Iw, 0, -1, 0], [0, 2.0 / Ih, -1, 0], [0, 0, 1, 0], [0, 0, 0, 1]], dtype=float)
    return np.linalg.inv(to_norm) @ np.asarray(Pplane, float)


def project(Z, XX, YY, P, datascale=1e-3):
    """the maps as wass_amd computes them: zf = Z * float32(datascale) in float32, each row ((P0 X + P1 Y) + P2 z) + P3 in fp64"""
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        z = (np.asarray(Z, F) * F(datascale)).astype(np.float64)
        r = [((P[k, 0] * XX + P[k, 1] * YY) + P[k, 2] * z) + P[k, 3] for k in range(3)]
        return (r[0] / r[2]).astype(F), (r[1] / r[2]).astype(F)


def project_matmul(Z, XX, YY, P, divisor=1000.0):
    """the maps by one matrix product over homogeneous points, the heights DIVIDED by `divisor`: the reference's formulation"""
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        z = np.asarray(Z, F) / divisor
        pts = np.stack([XX.ravel(), YY.ravel(), z.ravel().astype(np.float64), np.ones(z.size)])
        uvw = P @ pts
        uv = uvw[:2] / uvw[2]
        return uv[0].reshape(z.shape).astype(F), uv[1].reshape(z.shape).astype(F)


def radiance(images, Z, XX, YY, Pplane, datascale=1e-3, **variant):
    out = np.empty(np.shape(Z), F)
    for t in range(len(Z)):
        P = pcam(Pplane, images[t].shape[1], images[t].shape[0])
        mx, my = project(Z[t], XX, YY, P, datascale)
        out[t] = remap_lanczos4(images[t], mx, my, **variant).astype(F) / F(255.0)
    return out


# ---- bgimage ----------------------------------------------------------------------------------------------------------------------
def reflect_index(k, n):
    """scipy.ndimage's 'reflect' (d c b a | a b c d | d c b a) for any integer k"""
    m = np.mod(k, 2 * n)
    return np.where(m < n, m, 2 * n - 1 - m)


def bgimage(x, size: int, update: str = "diff") -> np.ndarray:
    """scipy.ndimage.uniform_filter1d(x, size, axis=0, mode='reflect') of a float32 array, restated: the running sum in fp64.
    update: 'diff' tmp += new - old (scipy); 'two' tmp += new, then tmp -= old; 'divided' the increment divided by size."""
    x = np.asarray(x, F)
    n, s1 = x.shape[0], size // 2
    ext = x[reflect_index(np.arange(-s1, n + size - s1 - 1), n)].astype(np.float64)
    out = np.empty(x.shape, F)
    with np.errstate(invalid="ignore", over="ignore"):
        tmp = np.zeros(x.shape[1:], np.float64)
        for k in range(size):
            tmp = tmp + ext[k]
        if update == "divided":
            tmp = tmp / size
        out[0] = tmp if update == "divided" else tmp / size
        for t in range(1, n):
            new, old = ext[t + size - 1], ext[t - 1]
            if update == "diff":
                tmp = tmp + (new - old)
            elif update == "two":
                tmp = (tmp + new) - old
            else:
                tmp = tmp + (new - old) / size
            out[t] = tmp if update == "divided" else tmp / size
    return out


# (count, size): every size of the scipy comparison, counts below, at and far above the size, odd and even
BG_PAIRS = [(1, 1), (1, 7), (1, 2000), (2, 3), (3, 8), (5, 4), (7, 7), (9, 5), (17, 6), (33, 64), (64, 99), (100, 2000), (257, 64),
            (300, 99), (2500, 2000), (3000, 2000)]


def wide_series(count, nser, seed):
    """series of wide dynamic range (values from 1e-3 to 1e7 with both signs), where the order of the fp64 updates shows"""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((count, nser)) * 10.0 ** rng.uniform(-3, 7, (count, nser))).astype(F)


# ---- the threshold ----------------------------------------------------------------------------------------------------------------
def isub(I, Ibg):
    I, Ibg = np.asarray(I, F), np.asarray(Ibg, F)
    return I - (Ibg - np.amin(Ibg))


def counts_by_edges(v, edges):
    """the histogram the edges themselves define: edges[i] <= v < edges[i + 1], the last bin closed"""
    v = np.ravel(v)
    v = v[(v >= edges[0]) & (v <= edges[-1])]
    idx = np.minimum(np.searchsorted(edges, v, side="right") - 1, len(edges) - 2)
    return np.bincount(idx, minlength=len(edges) - 1).astype(np.int64)


def vats(values):
    """the VATS threshold of one frame from numpy's own histogram: the bin, from the peak on, farthest from the line through
    (peak, h[peak]) and (last, h[last]); the line in homogeneous form written out by hand"""
    h, edges = np.histogram(values, bins=30, density=True)
    x = np.arange(h.shape[0], dtype=np.float64)
    peak = int(np.argmax(h))
    x1, y1, x2, y2 = x[peak], h[peak], x[-1], h[-1]
    a, b, c = y1 - y2, x2 - x1, x1 * y2 - y1 * x2
    d = np.abs(a * x + b * h + c)
    return edges[int(np.argmax(d[peak:])) + peak + 1]


def threshold(I, Ibg, threshold_val=0.35, use_vats=False):
    mask, thr = np.empty(np.shape(I), np.uint8), np.empty(len(I), F)
    for t in range(len(I)):
        s = isub(I[t], Ibg[t])
        thr[t] = vats(s) if use_vats else F(threshold_val)
        mask[t] = s > thr[t]
    return mask, thr


# ---- scenes -----------------------------------------------------------------------------------------------------------------------
def picture(h, w, seed, noise=40.0):
    """a smooth uint8 picture with texture: every tap of a window matters"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    v = 128 + 70 * np.sin(x / 5.3 + seed) * np.cos(y / 4.1) + noise * rng.standard_normal((h, w))
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


def grid(H, W, du=0.25):
    xs, ys = (np.arange(W) - W / 2.0) * du, (np.arange(H) - H / 2.0) * du
    XX, YY = np.meshgrid(xs, ys)
    return np.ascontiguousarray(XX), np.ascontiguousarray(YY)


def heights(count, H, W, seed, amp=400.0):
    """a cube in millimetres"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    t = np.arange(count)[:, None, None]
    return (amp * np.sin(x / 7.0 + 0.3 * t) * np.cos(y / 9.0 - 0.2 * t) + 30.0 * rng.standard_normal((count, H, W))).astype(F)


def pplane(Iw, Ih, XX, YY, kind: str):
    """a P{cam}plane matrix under which the grid's footprint lies 'inside' the Iw x Ih picture, 'crossing' all four of its borders,
    or wholly 'outside'; a mild perspective, heights move the pixel"""
    xr, yr = XX.max() - XX.min(), YY.max() - YY.min()
    fill = {"inside": 0.8, "crossing": 1.3, "outside": 0.8}[kind]
    sx, sy = fill * Iw / xr, fill * Ih / yr
    ox, oy = Iw / 2.0 + 0.37, Ih / 2.0 - 0.21
    if kind == "outside":
        ox += 3.0 * Iw
    P = np.array([[sx, 0.07 * sx, 6.0, ox], [-0.05 * sy, sy, 4.0, oy], [2e-4 / xr, -3e-4 / yr, 0.004, 1.0], [0, 0, 0, 1.0]])
    P[0] += ox * np.array([2e-4 / xr, -3e-4 / yr, 0.004, 0.0])          # keep the centre where it is under the perspective
    P[1] += oy * np.array([2e-4 / xr, -3e-4 / yr, 0.004, 0.0])
    to_norm = np.array([[2.0 / Iw, 0, -1, 0], [0, 2.0 / Ih, -1, 0], [0, 0, 1, 0], [0, 0, 0, 1]], dtype=float)
    return to_norm @ P


def lattice_maps(h, w, sh, sw, seed):
    """h x w maps, the first 1024 cells on the k / 32 lattice with all 1024 phases (when h * w >= 1024), positions from well outside to
    well outside, and, after them, window starts from -9 to +1 and from size - 8 to size + 1 on both axes, wholly outside, and the undefined
    values: NaN, +-inf, +-1e30, +-2^26"""
    rng = np.random.default_rng(seed)
    n = h * w
    qx = rng.integers(-12 * 32, (sw + 12) * 32, n)
    qy = rng.integers(-12 * 32, (sh + 12) * 32, n)
    k = np.arange(min(n, 1024))
    qx[k] = (qx[k] & ~31) | (k & 31)                    # every phase at least once
    qy[k] = (qy[k] & ~31) | (k >> 5)
    # beyond the first 1024 cells a third of the positions sits exactly half-way between two lattice points (where rounding half to
    # even, half up and truncation part) and a third at 0.3 / 32 past one
    jx = np.where(np.arange(n) < 1024, 0.0, np.array([0.0, 0.5, 0.3])[np.arange(n) % 3])
    jy = np.where(np.arange(n) < 1024, 0.0, np.array([0.5, 0.3, 0.0])[np.arange(n) % 3])
    mx, my = ((qx + jx) / 32.0).astype(F), ((qy + jy) / 32.0).astype(F)
    edge = []
    for size in (sw, sh):
        starts = list(range(-9, 2)) + list(range(size - 8, size + 2))
        edge.append(np.array(starts) + 3 + 0.40625)     # window start + 3 = the position of tap 3; phase 13
    special = [np.nan, np.inf, -np.inf, 1e30, -1e30, 2.0 ** 26, -2.0 ** 26, -40.0, 5000.0]
    cases = [(a, b) for a in edge[0] for b in edge[1]] + [(s, 10.5) for s in special] + [(10.5, s) for s in special]
    if n >= 1024 + len(cases):
        for i, (a, b) in enumerate(cases):
            mx[1024 + i], my[1024 + i] = a, b
    else:                                               # a small output: the corners and the undefined values come first
        pick = [(a, b) for a in edge[0][[0, 9, 11, 20]] for b in edge[1][[0, 9, 11, 20]]] + cases[len(edge[0]) * len(edge[1]):]
        for i, (a, b) in enumerate(pick[:n]):
            mx[i], my[i] = a, b
    return mx.reshape(h, w), my.reshape(h, w)


def threshold_frames(H, W, seed):
    rng = np.random.default_rng(seed)
    bg = (0.3 + 0.1 * rng.uniform(size=(H, W))).astype(F)
    I = (bg + 0.05 * rng.standard_normal((H, W)) + (rng.uniform(size=(H, W)) > 0.97) * rng.uniform(0.2, 0.6, (H, W))).astype(F)
    return I, bg


# ---- the wrong variants of the sampler ---------------------------------------------------------------------------------------------
VARIANTS = {"offset 4": dict(offset=4), "truncation": dict(rounding="trunc"), "no fix-up": dict(tab=lanczos_tab(fixup=False)),
            "phase exchanged": dict(swap_phase=True)}
# the fraction of the cells of a lattice_maps case of 37 x 67 or more by which each mistake must miss.  Reasoning: a shifted
# window or exchanged phases change every cell whose window meets the picture (about half of these cases' cells do) unless the
# textured picture happens to agree, so a quarter; truncation differs where a coordinate is off the lattice and not already an
# integer below, a third of the cells past the first 1024 per axis, so a fiftieth; the fix-up moves one weight of a phase by a
# few units of 2^-15, which shows in the rounded grey level only now and then, so one cell in a thousand.
VARIANT_MISS = {"offset 4": 1 / 4, "truncation": 1 / 50, "no fix-up": 1 / 1000, "phase exchanged": 1 / 4}
