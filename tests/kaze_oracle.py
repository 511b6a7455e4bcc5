"""numpy restatement of the KAZE detector (include/wass_gpu.h "KAZE feature detector", DESIGN.md "Feature detector"): float32 in the
stated operation order for every stage made of + - x / sqrt, so that the device must give the same bits; the orientation and the
descriptor, which use atan2 / sin / cos / exp, take a dtype and have an fp64 twin that sets the tests' tolerance.

Written from the specification, not from wass_amd/features.py: the level table, FED steps, taps and weights are recomputed here.
"""
import math

import numpy as np

F = np.float32
SOFFSET, SDERIV = 1.6, 1.0
NBINS = 300

GAUSS25 = np.array([
    [0.02546481, 0.02350698, 0.01849125, 0.01239505, 0.00708017, 0.00344629, 0.00142946],
    [0.02350698, 0.02169968, 0.01706957, 0.01144208, 0.00653582, 0.00318132, 0.00131956],
    [0.01849125, 0.01706957, 0.01342740, 0.00900066, 0.00514126, 0.00250252, 0.00103800],
    [0.01239505, 0.01144208, 0.00900066, 0.00603332, 0.00344629, 0.00167749, 0.00069579],
    [0.00708017, 0.00653582, 0.00514126, 0.00344629, 0.00196855, 0.00095820, 0.00039744],
    [0.00344629, 0.00318132, 0.00250252, 0.00167749, 0.00095820, 0.00046640, 0.00019346],
    [0.00142946, 0.00131956, 0.00103800, 0.00069579, 0.00039744, 0.00019346, 0.00008024]], np.float32)


# ------------------------------------------------------------------------------------------------------------------- tables
def levels(n_octaves=4, n_sublevels=4):
    """list of dicts: esigma, etime (float32), sigma_size, octave, sublevel"""
    out = []
    for o in range(n_octaves):
        for s in range(n_sublevels):
            es = F(SOFFSET * 2.0 ** (s / n_sublevels + o))
            out.append({"esigma": es, "etime": F(0.5) * es * es, "sigma_size": int(np.rint(es)), "octave": o, "sublevel": s})
    return out


def fed_taus_unordered(T):
    T, tm = F(T), F(0.25)
    n = int(np.ceil(np.sqrt(F(3.0) * T / tm + F(0.25)) - F(0.5) - F(1e-8)) + F(0.5))
    scale = F(3.0) * T / (tm * F(n * (n + 1)))
    return np.array([np.float64(scale * tm) / (2.0 * math.cos(math.pi * (2 * k + 1) / (4 * n + 2)) ** 2) for k in range(n)]).astype(F)


def fed_taus(T, reorder=True):
    tauh = fed_taus_unordered(T)
    n = len(tauh)
    if not reorder or n == 1:
        return tauh
    kappa, prime = n // 2, n + 1
    while any(prime % d == 0 for d in range(2, prime)):
        prime += 1
    tau, k = [], 0
    for _ in range(n):
        while ((k + 1) * kappa) % prime - 1 >= n:
            k += 1
        tau.append(tauh[((k + 1) * kappa) % prime - 1])
        k += 1
    return np.array(tau, F)


def gaussian_taps(sigma):
    ksize = int(math.ceil(2.0 * (1.0 + (sigma - 0.8) / 0.3)))
    ksize += 1 - ksize % 2
    x = np.arange(ksize) - (ksize - 1) / 2.0
    t = np.exp(-(x ** 2) / (2.0 * sigma ** 2))
    return (t / t.sum()).astype(F)


def scharr_weights(s):
    w = F(10.0) / F(3.0)
    norm = F(1.0) / (F(2.0) * F(s) * (w + F(2.0)))
    return norm, w * norm


# ------------------------------------------------------------------------------------------------------------------- stencils
def convert(img):
    return img.astype(F) * F(1.0 / 255.0)


def gauss(src, taps, mode="edge"):
    src = np.asarray(src, F)
    h, w = src.shape
    r = len(taps) // 2
    p = np.pad(src, ((0, 0), (r, r)), mode=mode)
    acc = np.zeros((h, w), F)
    for j, t in enumerate(taps):
        acc = acc + F(t) * p[:, j:j + w]
    p = np.pad(acc, ((r, r), (0, 0)), mode=mode)
    out = np.zeros((h, w), F)
    for j, t in enumerate(taps):
        out = out + F(t) * p[j:j + h, :]
    return out


def _shifted(src, s, mode):
    h, w = src.shape
    p = np.pad(np.asarray(src, F), s, mode=mode)
    return lambda dy, dx: p[s + dy:s + dy + h, s + dx:s + dx + w]


def scharr_x(src, s, mode="reflect"):
    n, wn = scharr_weights(s)
    P = _shifted(src, s, mode)
    d = lambda r: P(r, s) - P(r, -s)
    return (n * d(-s) + wn * d(0)) + n * d(s)


def scharr_y(src, s, mode="reflect"):
    n, wn = scharr_weights(s)
    P = _shifted(src, s, mode)
    m = lambda r: (n * P(r, -s) + wn * P(r, 0)) + n * P(r, s)
    return m(s) - m(-s)


def contrast(img32, mode="reflect"):
    """(k, hmax, npoints, hist)"""
    g = gauss(img32, gaussian_taps(1.0))
    return contrast_of(scharr_x(g, 1, mode), scharr_y(g, 1, mode))


def contrast_of(lx, ly):
    """(k, hmax, npoints, hist) of two planes of first derivatives: what wass_kaze_contrast_dev and the host's scan of the bins give"""
    lx, ly = np.asarray(lx, F), np.asarray(ly, F)
    m = np.sqrt(lx * lx + ly * ly)[1:-1, 1:-1].ravel()
    hmax = m.max() if m.size else F(0)
    nz = m[m != 0]
    hist = np.zeros(NBINS, np.int64)
    if nz.size:
        b = np.minimum(np.floor(F(NBINS) * (nz / hmax)).astype(np.int64), NBINS - 1)
        np.add.at(hist, b, 1)
    nthr = int(F(nz.size) * F(0.7))
    run, k = 0, 0
    while run < nthr and k < NBINS:
        run += hist[k]
        k += 1
    kc = F(0.03) if (run < nthr or nz.size == 0) else hmax * (F(k) / F(NBINS))
    return kc, hmax, int(nz.size), hist


def flow_g2(lx, ly, k):
    return F(1.0) / (F(1.0) + (lx * lx + ly * ly) / (F(k) * F(k)))


def fed_step(L, c, tau):
    z = np.zeros_like(L)
    xpos, xneg, ypos, yneg = z.copy(), z.copy(), z.copy(), z.copy()
    xpos[:, :-1] = (c[:, 1:] + c[:, :-1]) * (L[:, 1:] - L[:, :-1])
    xneg[:, 1:] = (c[:, 1:] + c[:, :-1]) * (L[:, 1:] - L[:, :-1])
    ypos[:-1, :] = (c[1:, :] + c[:-1, :]) * (L[1:, :] - L[:-1, :])
    yneg[1:, :] = (c[1:, :] + c[:-1, :]) * (L[1:, :] - L[:-1, :])
    return L + (F(0.5) * F(tau)) * (((xpos - xneg) + ypos) - yneg)


def scale_space(img, n_octaves=4, n_sublevels=4, border="reflect", fed_reorder=True, sigma_sq=True):
    """Every plane of every level.  border / fed_reorder / sigma_sq switch on the mistakes the probe pictures must show."""
    lv = levels(n_octaves, n_sublevels)
    img32 = convert(np.asarray(img, np.uint8))
    k, hmax, npoints, hist = contrast(img32, border)
    out = {key: [] for key in ("Lt", "Lsmooth", "flow", "Lx", "Ly", "Lxx", "Lxy", "Lyy", "Ldet")}
    Lt = gauss(img32, gaussian_taps(SOFFSET))
    g1 = gaussian_taps(SDERIV)
    for i, l in enumerate(lv):
        if i == 0:
            Lsm, fl = gauss(Lt, g1), np.zeros_like(Lt)
        else:
            Lsm = gauss(Lt, g1)
            fl = flow_g2(scharr_x(Lsm, 1, border), scharr_y(Lsm, 1, border), k)
            for tau in fed_taus(l["etime"] - lv[i - 1]["etime"], fed_reorder):
                Lt = fed_step(Lt, fl, tau)
        s = l["sigma_size"]
        lx, ly = scharr_x(Lsm, s, border), scharr_y(Lsm, s, border)
        ss2 = F(s) * F(s) if sigma_sq else F(s)
        lxx, lxy, lyy = scharr_x(lx, s, border) * ss2, scharr_y(lx, s, border) * ss2, scharr_y(ly, s, border) * ss2
        for key, v in (("Lt", Lt), ("Lsmooth", Lsm), ("flow", fl), ("Lx", lx * F(s)), ("Ly", ly * F(s)), ("Lxx", lxx), ("Lxy", lxy), ("Lyy", lyy),
                       ("Ldet", lxx * lyy - lxy * lxy)):
            out[key].append(v)
    out = {key: np.stack(v) for key, v in out.items()}
    out.update(k=k, hmax=hmax, npoints=npoints, hist=hist, levels=lv)
    return out


# -------------------------------------------------------------------------------------------------------------------- extrema
def _round(v, rounding):
    if rounding == "even":
        return np.rint(v)
    if rounding == "away":
        return np.sign(v) * np.floor(np.abs(v) + F(0.5))
    assert rounding == "trunc"
    return np.trunc(v)


def extrema(ldet, lv, threshold=1e-4, strict=True, loose=None, rounding="even"):
    """n x 3 (level, y, x) sorted, and the values.  Mistakes: strict=False compares >= everywhere, loose=(dl, dy, dx) at that one
    neighbour; rounding "away" / "trunc" in the border rule instead of half to even"""
    N, h, w = ldet.shape
    found = []
    for l in range(1, N - 1):
        v = ldet[l, 1:-1, 1:-1]
        ok = (v > F(threshold)) & (v >= F(1e-5))
        for dl in (-1, 0, 1):
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    if dl == 0 and dy == 0 and dx == 0:
                        continue
                    nb = ldet[l + dl, 1 + dy:h - 1 + dy, 1 + dx:w - 1 + dx]
                    ok &= (v > nb) if strict and loose != (dl, dy, dx) else (v >= nb)
        r = F(3.0) * lv[l]["esigma"]
        ys, xs = np.nonzero(ok)
        ys, xs = ys + 1, xs + 1
        xf, yf = xs.astype(F), ys.astype(F)
        rnd = lambda t: _round(t, rounding)
        inside = (rnd(xf - r) >= 0) & (rnd(xf + r) < w) & (rnd(yf - r) >= 0) & (rnd(yf + r) < h)
        found += [(l, int(y), int(x)) for y, x in zip(ys[inside], xs[inside])]
    cand = np.array(sorted(found), np.int64).reshape(-1, 3)
    return cand, ldet[cand[:, 0], cand[:, 1], cand[:, 2]].astype(F)


def duplicates(cand, values, lv):
    """the accepted list (indices into cand) of the duplicate pass, plain loops"""
    acc = []
    for i, (l, y, x) in enumerate(cand.tolist()):
        hit = None
        for slot, j in enumerate(acc):
            lj, yj, xj = cand[j].tolist()
            d2 = F(F(xj) - F(x)) ** 2 + F(F(yj) - F(y)) ** 2
            if (lj == l and d2 < lv[l]["esigma"] ** 2) or (lj == l - 1 and d2 < F(lv[l]["sigma_size"]) ** 2):
                hit = slot
                break
        if hit is None:
            acc.append(i)
        elif cand[acc[hit]][0] == l - 1 and values[i] > values[acc[hit]]:
            acc[hit] = i
    return np.array(acc, np.int64)


def solve3(a, pivot="first"):
    """pivot: "first" of equal pivots (the rule); the mistakes "last" of equal pivots and "none" (no row exchange)"""
    a = [[F(v) for v in row] for row in a]
    for k in range(3):
        p = k
        for r in range(k + 1, 3):
            if pivot != "none" and (abs(a[r][k]) > abs(a[p][k]) or (pivot == "last" and abs(a[r][k]) == abs(a[p][k]))):
                p = r
        a[k], a[p] = a[p], a[k]
        if a[k][k] == 0:
            return None
        for r in range(k + 1, 3):
            f = a[r][k] / a[k][k]
            for c in range(k + 1, 4):
                a[r][c] = a[r][c] - f * a[k][c]
    d2 = a[2][3] / a[2][2]
    d1 = (a[1][3] - a[1][2] * d2) / a[1][1]
    d0 = ((a[0][3] - a[0][1] * d1) - a[0][2] * d2) / a[0][0]
    return d0, d1, d2


def refine(ldet, cand, pivot="first", bound="le"):
    """n x 5 float32: x + dx, y + dy, ds, |v|, kept.  Mistakes: pivot (solve3), bound="lt" refuses an offset of exactly 1"""
    out = np.zeros((len(cand), 5), F)
    h2, q = F(0.5), F(0.25)
    with np.errstate(all="ignore"):
        for i, (l, y, x) in enumerate(np.asarray(cand).tolist()):
            C, D, U = ldet[l], ldet[l - 1], ldet[l + 1]
            v = C[y, x]
            Dx, Dy, Ds = h2 * (C[y, x + 1] - C[y, x - 1]), h2 * (C[y + 1, x] - C[y - 1, x]), h2 * (U[y, x] - D[y, x])
            Dxx = (C[y, x + 1] + C[y, x - 1]) - F(2) * v
            Dyy = (C[y + 1, x] + C[y - 1, x]) - F(2) * v
            Dss = (U[y, x] + D[y, x]) - F(2) * v
            Dxy = q * ((C[y + 1, x + 1] + C[y - 1, x - 1]) - (C[y - 1, x + 1] + C[y + 1, x - 1]))
            Dxs = q * ((U[y, x + 1] + D[y, x - 1]) - (U[y, x - 1] + D[y, x + 1]))
            Dys = q * ((U[y + 1, x] + D[y - 1, x]) - (U[y - 1, x] + D[y + 1, x]))
            out[i] = (x, y, 0, abs(v), 0)
            d = solve3([[Dxx, Dxy, Dxs, -Dx], [Dxy, Dyy, Dys, -Dy], [Dxs, Dys, Dss, -Ds]], pivot)
            inside = (lambda t: abs(t) <= 1) if bound == "le" else (lambda t: abs(t) < 1)
            if d is not None and inside(d[0]) and inside(d[1]) and inside(d[2]):
                out[i] = (F(x) + d[0], F(y) + d[1], d[2], abs(v), 1)
    return out


def sizes(lv, level, ds, n_sublevels):
    return np.array([2.0 * SOFFSET * 2.0 ** (lv[int(l)]["octave"] + (lv[int(l)]["sublevel"] + float(F(d))) / n_sublevels) for l, d in zip(level, ds)],
                    np.float64).astype(F).reshape(-1)


# ---------------------------------------------------------------------------------------------------------------- orientation
_LATTICE = [(i, j) for i in range(-6, 7) for j in range(-6, 7) if i * i + j * j < 36]


def _fround(v):
    """(int)(v + 0.5): truncation towards zero"""
    return np.trunc(v + v.dtype.type(0.5)).astype(np.int64)


def orientation(kp, Lx, Ly, dtype=np.float32, flags=False, admissible=False, **mistakes):
    """angles of a keypoint table (x, y, size, level[, ...]); with flags also the fragile keypoints: a sample's angle within 1e-5 rad
    of a window edge, or a window of other members whose score is within 1e-6 (relative) of the best.  With admissible as well, a
    third value: per keypoint the angles a correct float32 implementation may give (empty where the keypoint is not fragile).  They
    are the angles of every window, with its samples within 1e-5 rad of one of its edges as computed, all counted in and all counted
    out, whose score reaches (within 1e-6) the largest score some window has whichever way its own near samples fall; 0 as well where
    that is 0.

    Mistakes (keywords, for the probes of tests/kaze_probes.py): transpose (the planes read at [x][y]; swapping i and j alone only
    reorders the symmetric lattice), floor (floor(v + 0.5) instead of the
    truncation), clamp (outside samples read the border instead of 0), zero_in (a >= 0 in the wrap-around windows), last_equal (the
    last of equal windows wins), no_wrap (ang2 = ang1 + pi / 3 always), no_high (a wrap-around window
    without its part below 2 pi), level0 (every keypoint reads level 0), size_floor
    ((int)(size / 2)), drop=q (sample q is not read)"""
    mk = lambda name, default=False: mistakes.pop(name, default)
    transpose, floor_, clamp, zero_in, last_equal = mk("transpose"), mk("floor"), mk("clamp"), mk("zero_in"), mk("last_equal")
    no_wrap, level0, size_floor, drop, no_high = mk("no_wrap"), mk("level0"), mk("size_floor"), mk("drop", None), mk("no_high")
    assert not mistakes, mistakes
    T = dtype
    N, h, w = Lx.shape
    two_pi, pi3, pi53 = T(6.2831853071795864769), T(1.0471975511965976), T(5.2359877559829887)
    ii = np.array([p[0] for p in _LATTICE])
    jj = np.array([p[1] for p in _LATTICE])
    g = GAUSS25[np.abs(ii), np.abs(jj)].astype(T)
    ang1s = []
    a = np.float32(0.0)
    while a < np.float32(6.2831853071795864769):
        ang1s.append(a)
        a = a + np.float32(0.15)
    ang1s = np.array(ang1s, np.float32).astype(T)              # the window starts are float32 sums on the device
    assert len(ang1s) == 42
    ang2s = np.where((ang1s + pi3 > two_pi) & (not no_wrap), ang1s - pi53, ang1s + pi3).astype(T)
    out, frag, adm = np.zeros(len(kp), T), np.zeros(len(kp), bool), [np.zeros(0, T) for _ in range(len(kp))]
    kp = np.asarray(kp, np.float32)

    def member(ang, a1, a2, force=None):
        """force: (near, value): samples of `near` are counted in (True) or out (False)"""
        if a1 < a2:
            m = (a1 < ang) & (ang < a2)
        else:
            m = (((ang >= 0) if zero_in else (ang > 0)) & (ang < a2)) | ((ang > a1) & (ang < two_pi) & (not no_high))
        if force is not None:
            m = np.where(force[0], force[1], m)
        return m

    def window(m, rx, ry):
        sx, sy = T(0), T(0)
        for t in np.flatnonzero(m):
            sx, sy = sx + rx[t], sy + ry[t]
        ba = np.arctan2(sy, sx).astype(T)
        return sx * sx + sy * sy, (ba + two_pi if ba < 0 else ba)

    for q in range(len(kp)):
        xf, yf = kp[q, 0], kp[q, 1]                                 # float32 coordinates, float32 sample positions, as on the device
        s = int(np.float32(kp[q, 2]) / np.float32(2.0) + (np.float32(0.0) if size_floor else np.float32(0.5)))
        lev = 0 if level0 else int(kp[q, 3])
        rnd = (lambda v: np.floor(v + v.dtype.type(0.5)).astype(np.int64)) if floor_ else _fround
        ix = rnd(xf + (ii * s).astype(np.float32))
        iy = rnd(yf + (jj * s).astype(np.float32))
        ok = (ix >= 0) & (ix < w) & (iy >= 0) & (iy < h)
        if clamp:
            ok[:] = True
        if drop is not None:
            ok[drop] = False
        cx, cy = np.clip(ix, 0, w - 1), np.clip(iy, 0, h - 1)
        if transpose:
            cx, cy = np.clip(iy, 0, w - 1), np.clip(ix, 0, h - 1)
        rx = np.where(ok, g * Lx[lev, cy, cx].astype(T), T(0))
        ry = np.where(ok, g * Ly[lev, cy, cx].astype(T), T(0))
        ang = np.arctan2(ry, rx).astype(T)
        ang = np.where(ang < 0, ang + two_pi, ang).astype(T)
        best, besta, members, scores = T(0), T(0), [], []
        for a1, a2 in zip(ang1s, ang2s):
            m = member(ang, a1, a2)
            sc, ba = window(m, rx, ry)
            members.append(m)
            scores.append(sc)
            if sc > best or (last_equal and sc == best and sc > 0):
                best = sc
                besta = ba
        out[q] = besta
        if flags:
            live = (rx != 0) | (ry != 0)
            edges = np.concatenate([ang1s, ang2s, [T(0), two_pi]]).astype(np.float64)
            near = np.abs(ang[live].astype(np.float64)[:, None] - edges[None, :]).min(initial=np.inf) < 1e-5
            b = int(np.argmax(scores))
            close = any(abs(float(sc) - float(best)) < 1e-6 * float(best) and not np.array_equal(m, members[b])
                        for m, sc in zip(members, scores)) if best > 0 else True
            frag[q] = bool(near or close)
            if admissible and frag[q]:
                a64 = ang.astype(np.float64)
                variants = []                                       # per window: [(score, angle), ...]
                for a1, a2, m, sc in zip(ang1s, ang2s, members, scores):
                    own = [float(a1), float(a2)] + ([0.0, float(two_pi)] if not a1 < a2 else [])
                    nr = live & (np.abs(a64[:, None] - np.array(own)[None, :]).min(axis=1) < 1e-5)
                    v = [window(m, rx, ry)]
                    if nr.any():
                        v += [window(member(ang, a1, a2, (nr, True)), rx, ry), window(member(ang, a1, a2, (nr, False)), rx, ry)]
                    variants.append(v)
                floor_score = max(min(float(sc) for sc, _ in v) for v in variants)
                ok_a = [ba for v in variants for sc, ba in v if float(sc) > 0 and float(sc) >= floor_score * (1.0 - 1e-6)]
                if floor_score == 0.0:
                    ok_a.append(T(0))
                adm[q] = np.array(ok_a, T)
    if flags and admissible:
        return out, frag, adm
    return (out, frag) if flags else out


# ----------------------------------------------------------------------------------------------------------------- descriptor
def descriptors(kp, Lx, Ly, dtype=np.float32, rotate_sign=1.0, **mistakes):
    """n x 64 of a keypoint table (x, y, size, level, angle).  rotate_sign = -1 rotates the pattern the wrong way (a probe).
    Further mistakes (keywords): swap_sub (sub / 4 and sub % 4 swapped), swap_kl (k and l swapped in the sample's position), swap_rr (rrx and rry written to
    the other array), zero_outside (a sample outside the picture reads 0 instead of the border), frac_after_clamp (the bilinear
    fraction taken from the clamped index)"""
    mk = lambda name: mistakes.pop(name, False)
    swap_sub, swap_kl, swap_rr, zero_outside, frac_after_clamp = mk("swap_sub"), mk("swap_kl"), mk("swap_rr"), mk("zero_outside"), mk("frac_after_clamp")
    assert not mistakes, mistakes
    T = dtype
    N, h, w = Lx.shape
    kp = np.asarray(kp, np.float32)
    out = np.zeros((len(kp), 64), T)
    sub = np.arange(16)
    i0, j0 = -12 + 5 * (sub // 4), -12 + 5 * (sub % 4)
    if swap_sub:
        i0, j0 = j0, i0
    r = np.arange(81)
    k = (i0[:, None] + r[None, :] // 9).astype(T)
    l = (j0[:, None] + r[None, :] % 9).astype(T)
    if swap_kl:
        k, l = l, k
    ky, kx = (i0 + 5).astype(T)[:, None], (j0 + 5).astype(T)[:, None]
    half = T(0.5)

    def gaussian(x, y, sig):
        return np.exp(-(x * x + y * y) / (T(2.0) * sig * sig)).astype(T)

    with np.errstate(all="ignore"):
        for q in range(len(kp)):
            xf, yf = T(kp[q, 0]), T(kp[q, 1])
            scale = T(int(np.float32(kp[q, 2]) / np.float32(2.0) + np.float32(0.5)))
            lev = int(kp[q, 3])
            ang = T(kp[q, 4]) * T(rotate_sign)
            co, si = np.cos(ang).astype(T), np.sin(ang).astype(T)
            xs = xf + (-kx * scale * si + ky * scale * co)
            ys = yf + (kx * scale * co + ky * scale * si)
            sy = yf + (l * scale * co + k * scale * si)
            sx = xf + (-l * scale * si + k * scale * co)
            g1 = gaussian(xs - sx, ys - sy, T(2.5) * scale)
            flx, fly = np.floor(sx), np.floor(sy)
            fx, fy = sx - flx, sy - fly
            y1, x1 = np.clip(fly.astype(np.int64), 0, h - 1), np.clip(flx.astype(np.int64), 0, w - 1)
            y2, x2 = np.clip(fly.astype(np.int64) + 1, 0, h - 1), np.clip(flx.astype(np.int64) + 1, 0, w - 1)
            if frac_after_clamp:
                fx, fy = sx - x1.astype(T), sy - y1.astype(T)
            one = T(1.0)
            w1, w2, w3, w4 = (one - fx) * (one - fy), fx * (one - fy), (one - fx) * fy, fx * fy
            PX, PY = Lx[lev].astype(T), Ly[lev].astype(T)
            if zero_outside:
                fi, fj = fly.astype(np.int64), flx.astype(np.int64)
                z = lambda P, yy, xx, oy, ox: np.where((fi + oy >= 0) & (fi + oy < h) & (fj + ox >= 0) & (fj + ox < w), P[yy, xx], T(0))
                rx = ((w1 * z(PX, y1, x1, 0, 0) + w2 * z(PX, y1, x2, 0, 1)) + w3 * z(PX, y2, x1, 1, 0)) + w4 * z(PX, y2, x2, 1, 1)
                ry = ((w1 * z(PY, y1, x1, 0, 0) + w2 * z(PY, y1, x2, 0, 1)) + w3 * z(PY, y2, x1, 1, 0)) + w4 * z(PY, y2, x2, 1, 1)
            else:
                rx = ((w1 * PX[y1, x1] + w2 * PX[y1, x2]) + w3 * PX[y2, x1]) + w4 * PX[y2, x2]
                ry = ((w1 * PY[y1, x1] + w2 * PY[y1, x2]) + w3 * PY[y2, x1]) + w4 * PY[y2, x2]
            rx, ry = g1 * rx, g1 * ry
            rry = rx * co + ry * si
            rrx = -rx * si + ry * co
            if swap_rr:
                rrx, rry = rry, rrx
            acc = np.zeros((16, 4), T)
            for t in range(81):
                acc[:, 0] = acc[:, 0] + rrx[:, t]
                acc[:, 1] = acc[:, 1] + rry[:, t]
                acc[:, 2] = acc[:, 2] + np.abs(rrx[:, t])
                acc[:, 3] = acc[:, 3] + np.abs(rry[:, t])
            cx, cy = (sub // 4).astype(T) + half, (sub % 4).astype(T) + half
            part = acc * gaussian(cx - T(2.0), cy - T(2.0), T(1.5))[:, None]
            ln = T(0)
            for t in range(16):
                ln = ln + (((part[t, 0] * part[t, 0] + part[t, 1] * part[t, 1]) + part[t, 2] * part[t, 2]) + part[t, 3] * part[t, 3])
            out[q] = (part / np.sqrt(ln).astype(T)).reshape(64)
    return out


# ------------------------------------------------------------------------------------------------------------------ detector
def detect(img, n_octaves=4, n_sublevels=4, threshold=1e-4, **mistakes):
    """dict: the scale space `ss`, candidates, values, kept (m x 3), refined (m x 5), and the keypoint table kp (x, y, size, level,
    angle) with response and descriptors of the refined points that are kept"""
    strict = mistakes.pop("strict", True)
    rotate_sign = mistakes.pop("rotate_sign", 1.0)
    ss = scale_space(img, n_octaves, n_sublevels, **mistakes)
    lv = ss["levels"]
    cand, values = extrema(ss["Ldet"], lv, threshold, strict)
    kept = cand[duplicates(cand, values, lv)].reshape(-1, 3)
    ref = refine(ss["Ldet"], kept)
    ok = ref[:, 4] != 0
    level = kept[ok, 0]
    size = sizes(lv, level, ref[ok, 2], n_sublevels)
    kp = np.column_stack([ref[ok, 0], ref[ok, 1], size, level.astype(F), np.zeros(len(level), F)]).astype(F).reshape(-1, 5)
    kp[:, 4] = orientation(kp, ss["Lx"], ss["Ly"])
    desc = descriptors(kp, ss["Lx"], ss["Ly"], rotate_sign=rotate_sign)
    return {"ss": ss, "candidates": cand, "values": values, "kept": kept, "refined": ref, "size_all": sizes(lv, kept[:, 0], ref[:, 2], n_sublevels),
            "kp": kp, "response": ref[ok, 3], "descriptors": desc}
