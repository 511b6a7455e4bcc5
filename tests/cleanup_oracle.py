"""Direct-form restatements of the disparity clean-up between SGM and triangulation (csrc/post.hip, csrc/post_opt.hip; rows a7-a9),
in numpy / scipy.ndimage only.  Written from the reference's lines (wass_stereo.cpp:617-733 the three helpers, :903-986 the resize /
mask / median / biggest-component step) and from the documented arithmetic of the OpenCV functions they call; they share no code
with oracle/*.c, which tests/test_cleanup_edges.py compares them with bit for bit.

Every function takes variant= : None is the right answer, a name is one deliberately wrong version (the mistakes a kernel could
make), used to show that a probe can tell the two apart.  Unknown names are refused.

chain(..., tile=(64, 32), halo=(hl, hr, hv)) evaluates the chain the way a tiled kernel does: every tile of tile[0] x tile[1] output
cells is computed from a buffer that carries hl more columns to the left, hr to the right and hv rows above and below; a cell whose
stencil leaves the buffer keeps its value.  With the halo a chain needs, the result equals the untiled one; "one cell short" is a
halo argument."""
import numpy as np
from scipy import ndimage

F = np.float32


def _check(variant, allowed):
    if variant is not None and variant not in allowed:
        raise ValueError(f"unknown variant {variant!r} (known: {sorted(allowed)})")


# ---------------------------------------------------------------------------------------------------------------- a7: the chain
def convert(d16, mindisp, numdisp, off=0, scale=1.0, variant=None):
    """clean_and_convert_disparity (:714-733): d/16 in float32; <= mindisp or > numdisp is invalid (0); + off in float32; * scale in double."""
    _check(variant, ())
    d = np.asarray(d16, np.int16).astype(F) / F(16.0)
    bad = (d <= F(mindisp)) | (d > F(numdisp))
    v = ((d + F(off)).astype(np.float64) * float(scale)).astype(F)
    return np.where(bad, F(0), v).astype(F)


def _dilate_cells(T, ok, variant):
    """One dilation of the buffer T; ok: the cells the rule applies to at all (the others keep their value).  A cell whose stencil
    (rows +-1, columns +0..+2) leaves the buffer keeps its value too."""
    th, tw = T.shape
    out = T.copy()
    if th < 3 or tw < 3:
        return out
    nb = lambda dy, dx: T[1 + dy:th - 1 + dy, 1 + dx:tw - 1 + dx]        # the neighbours of the cells (1..th-2, 1..tw-2)
    # the reference writes the result for the stencil centred on column k+1 into column k; "centre_k" is the stencil where one
    # would expect it, centred on the cell itself
    cols = slice(1, tw - 1) if variant == "centre_k" else slice(0, tw - 2)
    # t[-1], t[1], t[0], b[-1], b[1], b[0], c[-1], c[1]
    order = [nb(-1, -1), nb(-1, 1), nb(-1, 0), nb(1, -1), nb(1, 1), nb(1, 0), nb(0, -1), nb(0, 1)]
    if variant == "sorted":                                     # the same sum taken in ascending order of the values
        order = list(np.sort(np.stack([np.where(a > 0, a, F(0)) for a in order]), axis=0))
    avg = np.zeros(order[0].shape, F)
    n = np.zeros(order[0].shape, np.int32)
    for a in order:
        pos = a > 0
        avg = np.where(pos, (avg + a).astype(F), avg)
        n += pos
    enough = n >= 1 if variant == "ge1" else n > 1
    cur = T[1:th - 1, cols]
    with np.errstate(divide="ignore", invalid="ignore"):
        q = (avg / n.astype(F)).astype(F)
    out[1:th - 1, cols] = np.where(enough & (cur == 0) & ok[1:th - 1, cols], q, cur)
    return out


def dilate(f, variant=None):
    """matrix_dilate_zero<float> (:617-662): rows 1..h-2, output columns 0..w-3."""
    _check(variant, ("centre_k", "ge1", "sorted"))
    f = np.asarray(f, F)
    return _dilate_cells(f, np.ones(f.shape, bool), variant)


def _erode_cells(T, gy, gx, w, h, variant):
    """One erosion of the buffer T whose cell (ly, lx) is the picture's (gy[ly], gx[lx]).  Cells outside the picture keep their
    value; first / last row and column become 0; an inner cell becomes 0 where one of its 8 neighbours is 0; a cell whose stencil
    leaves the buffer keeps its value."""
    th, tw = T.shape
    Y, X = np.meshgrid(gy, gx, indexing="ij")
    inside = (Y >= 0) & (Y < h) & (X >= 0) & (X < w)
    border = inside & ((Y == 0) | (Y == h - 1) | (X == 0) | (X == w - 1))
    out = np.where(border, F(0), T).astype(F)
    if th >= 3 and tw >= 3:
        P = T == 0
        if variant == "four":
            z = P[:-2, 1:-1] | P[2:, 1:-1] | P[1:-1, :-2] | P[1:-1, 2:]
        else:
            z = (P[:-2, 1:-1] | P[:-2, :-2] | P[:-2, 2:] | P[2:, 1:-1] | P[2:, :-2] | P[2:, 2:] | P[1:-1, :-2] | P[1:-1, 2:])
        inner = (inside & ~border)[1:-1, 1:-1]
        out[1:-1, 1:-1] = np.where(inner & z, F(0), out[1:-1, 1:-1])
    return out


def erode(f, variant=None):
    """matrix_erode_zero<float> (:665-711)."""
    _check(variant, ("four",))
    f = np.asarray(f, F)
    h, w = f.shape
    return _erode_cells(f, np.arange(h), np.arange(w), w, h, variant)


def mask_step(nn, cub, variant=None, erode_variant=None):
    """:908-928: the cubic copy, zero where the eroded nearest copy is zero."""
    _check(variant, ("skip",))
    cub = np.asarray(cub, F)
    if variant == "skip":
        return cub.copy()
    return np.where(erode(nn, erode_variant) == 0, F(0), cub).astype(F)


def median(f, ks, variant=None):
    """cv::medianBlur on CV_32F, ks 3 or 5: the middle of the ks*ks values, border replicated."""
    _check(variant, ())
    f = np.asarray(f, F)
    r = ks // 2
    p = np.pad(f, r, mode="edge")
    h, w = f.shape
    win = np.stack([p[a:a + h, b:b + w] for a in range(ks) for b in range(ks)])
    return np.sort(win, axis=0)[ks * ks // 2]


def chain_halo(nd, ne, med):
    """(hl, hr, hv) a tile needs: a column per erosion, one for the mask's erosion and one per median ring on either side; a dilation
    looks two columns to the right (and none to the left) and one row up and down."""
    nd, ne, rm = max(nd, 0), max(ne, 0), (med // 2 if med >= 3 else 0)
    return ne + 1 + rm, 2 * nd + ne + 1 + rm, nd + ne + 1 + rm


def chain_lds_bytes(nd, ne, med, tile=(64, 32)):
    """two float32 buffers of the tile with its halo"""
    hl, hr, hv = chain_halo(nd, ne, med)
    return (tile[0] + hl + hr) * (tile[1] + 2 * hv) * 2 * 4


def chain(d16, mindisp, numdisp, off, scale, nd, ne, med, variant=None, tile=None, halo=None):
    """convert -> nd dilations -> ne erosions -> mask by one more erosion -> median (med 3 or 5; less: none)."""
    _check(variant, ("centre_k", "ge1", "sorted", "four", "skip", "median_tile_clamp"))
    dv = variant if variant in ("centre_k", "ge1", "sorted") else None
    ev = "four" if variant == "four" else None
    nd, ne = max(nd, 0), max(ne, 0)
    a = convert(d16, mindisp, numdisp, off, scale)
    if tile is None:
        if variant == "median_tile_clamp":
            raise ValueError("median_tile_clamp needs tile=")
        for _ in range(nd):
            a = dilate(a, dv)
        for _ in range(ne):
            a = erode(a, ev)
        a = mask_step(a, a, "skip" if variant == "skip" else None, ev)
        return median(a, med) if med >= 3 else a
    h, w = a.shape
    TX, TY = tile
    hl, hr, hv = chain_halo(nd, ne, med) if halo is None else halo
    tw, th = TX + hl + hr, TY + 2 * hv
    r = med // 2 if med >= 3 else 0
    out = np.zeros((h, w), F)
    for by in range(0, h, TY):
        for bx in range(0, w, TX):
            gx, gy = np.arange(bx - hl, bx - hl + tw), np.arange(by - hv, by - hv + th)
            Y, X = np.meshgrid(gy, gx, indexing="ij")
            inside = (Y >= 0) & (Y < h) & (X >= 0) & (X < w)
            T = np.where(inside, a[np.clip(Y, 0, h - 1), np.clip(X, 0, w - 1)], F(0)).astype(F)
            ok = (Y >= 1) & (Y < h - 1) & (X >= 0) & (X <= w - 3)
            for _ in range(nd):
                T = _dilate_cells(T, ok, dv)
            for s in range(ne + 1):
                E = _erode_cells(T, gy, gx, w, h, ev)
                if s == ne:
                    E = T.copy() if variant == "skip" else np.where(E == 0, F(0), T).astype(F)
                T = E
            flat = T.ravel()
            ys, xs = np.arange(by, min(by + TY, h)), np.arange(bx, min(bx + TX, w))
            if med >= 3:
                vals = []
                for dy in range(-r, r + 1):
                    for dx in range(-r, r + 1):
                        if variant == "median_tile_clamp":       # the border replicated at the tile's output area, not the picture's
                            yy = np.clip(ys + dy, ys[0], ys[-1]); xx = np.clip(xs + dx, xs[0], xs[-1])
                        else:
                            yy = np.clip(ys + dy, 0, h - 1); xx = np.clip(xs + dx, 0, w - 1)
                        # flat addressing, as a buffer in memory is addressed: a column that the halo does not hold is the
                        # neighbouring row's cell, not an error
                        idx = (yy[:, None] - gy[0]) * tw + (xx[None, :] - gx[0])
                        vals.append(flat[np.clip(idx, 0, flat.size - 1)])
                res = np.sort(np.stack(vals), axis=0)[med * med // 2]
            else:
                res = T[hv:hv + len(ys), hl:hl + len(xs)]
            out[ys[0]:ys[-1] + 1, xs[0]:xs[-1] + 1] = res
    return out


# ---------------------------------------------------------------------------------------------------------------- a9: Sobel, components
def _refl101(i, n):
    if n == 1:
        return np.zeros_like(i)
    i = np.abs(i)
    i = np.where(i >= n, 2 * n - 2 - i, i)
    return np.clip(i, 0, n - 1)


def sobel_sq(f, variant=None):
    """gx^2 + gy^2 of the 3 x 3 Sobel pair in float32, BORDER_REFLECT_101; per row: c - a and a + 2b + c, then gx = t0 + 2 t1 + t2,
    gy = u2 - u0."""
    _check(variant, ("replicate",))
    f = np.asarray(f, F)
    h, w = f.shape
    if variant == "replicate":
        ry = lambda i: np.clip(i, 0, h - 1)
        rx = lambda i: np.clip(i, 0, w - 1)
    else:
        ry = lambda i: _refl101(i, h)
        rx = lambda i: _refl101(i, w)
    x = np.arange(w)
    t, u = [], []
    for k in range(3):
        r = f[ry(np.arange(h) - 1 + k)]
        a, b, c = r[:, rx(x - 1)], r, r[:, rx(x + 1)]
        t.append((c - a).astype(F))
        u.append(((a + (b * F(2)).astype(F)).astype(F) + c).astype(F))
    gx = ((t[0] + (t[1] * F(2)).astype(F)).astype(F) + t[2]).astype(F)
    gy = (u[2] - u[0]).astype(F)
    return ((gx * gx).astype(F) + (gy * gy).astype(F)).astype(F)


def large_gradient(f, thr, variant=None):
    """:951-957: 1 where the squared Sobel magnitude is greater than the threshold."""
    _check(variant, ("ge", "replicate"))
    g = sobel_sq(f, "replicate" if variant == "replicate" else None)
    return (g >= F(thr) if variant == "ge" else g > F(thr)).astype(np.uint8)


EIGHT = np.ones((3, 3), int)
FOUR = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]])


def label_components(active, variant=None):
    """labels (0: none; 1.. in raster order of each component's first pixel) and the areas, 8-connected."""
    _check(variant, ("four", "row_wrap"))
    active = np.asarray(active, bool)
    h, w = active.shape
    lab, n = ndimage.label(active, FOUR if variant == "four" else EIGHT)
    if variant == "row_wrap":                                   # a raster index i - 1 that runs from column 0 into the row above:
        root = np.arange(n + 1)                                 # the last cell of a row joined with the first cell of the next

        def find(i):
            while root[i] != i:
                i = root[i]
            return i
        for y in range(h - 1):
            p, q = find(lab[y, w - 1]), find(lab[y + 1, 0])
            if p and q and p != q:
                root[max(p, q)] = min(p, q)
        lab = np.array([find(i) for i in range(n + 1)])[lab]
    # number the components in raster order of their first pixel, whatever order the labelling used
    ids, first = np.unique(lab.ravel(), return_index=True)
    ids, first = ids[ids != 0], first[ids != 0]
    new = np.zeros(n + 1, np.int64)
    new[ids[np.argsort(first, kind="stable")]] = np.arange(1, len(ids) + 1)
    lab = new[lab]
    area = np.bincount(lab.ravel(), minlength=len(ids) + 1)
    area[0] = 0
    return lab, area


def biggest_component(f, thr, variant=None):
    """:947-986: zero where the gradient is large, then keep the largest 8-connected component of the non-zero cells; of equal areas
    the one whose first pixel comes first in raster order (the loop at :972-980 replaces on '>' only).  Returns (map, area, mask)."""
    _check(variant, ("four", "tie_last", "ge", "replicate", "row_wrap"))
    f = np.asarray(f, F)
    lg = large_gradient(f, thr, variant if variant in ("ge", "replicate") else None)
    out = np.where(lg != 0, F(0), f).astype(F)
    lab, area = label_components(out != 0, variant if variant in ("four", "row_wrap") else None)
    if len(area) <= 1:
        return np.zeros_like(out), 0, lg
    big = int(area.max())
    winners = np.flatnonzero(area == big)
    best = winners[-1] if variant == "tie_last" else winners[0]
    return np.where(lab == best, out, F(0)).astype(F), big, lg


def filter_speckles(img, new_val, max_size, max_diff, variant=None):
    """cv::filterSpeckles on CV_16S: a plain flood fill from every unvisited pixel != new_val in raster order over the 4 neighbours
    that are != new_val and differ by at most max_diff from the pixel they are reached from; a region of at most max_size pixels
    becomes new_val."""
    _check(variant, ("eight", "lt", "wrap16"))
    img = np.asarray(img, np.int16)
    h, w = img.shape
    v = img.astype(np.int64)
    out = img.copy()
    seen = v == new_val
    if variant == "eight":
        steps = [(-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1)]
    else:
        steps = [(-1, 0), (0, -1), (0, 1), (1, 0)]

    def diff(a, b):
        d = a - b
        if variant == "wrap16":                                 # the difference taken in 16 bits
            d = (d + 32768) % 65536 - 32768
        return abs(d)
    for y0 in range(h):
        for x0 in range(w):
            if seen[y0, x0]:
                continue
            seen[y0, x0] = True
            region = [(y0, x0)]
            k = 0
            while k < len(region):
                y, x = region[k]; k += 1
                for dy, dx in steps:
                    yy, xx = y + dy, x + dx
                    if 0 <= yy < h and 0 <= xx < w and not seen[yy, xx] and diff(v[y, x], v[yy, xx]) <= max_diff:
                        seen[yy, xx] = True
                        region.append((yy, xx))
            small = len(region) < max_size if variant == "lt" else len(region) <= max_size
            if small:
                for y, x in region:
                    out[y, x] = new_val
    return out


# ---------------------------------------------------------------------------------------------------------------- a9: resizers
def _cubic_axis(n_dst, scale):
    """first source index - 1 ... and the four float32 weights of cv::interpolateCubic (A = -0.75) for every destination index"""
    d = np.arange(n_dst, dtype=np.float64)
    f = ((d + 0.5) * float(scale) - 0.5).astype(F)
    s = np.floor(f).astype(np.int64)
    f = (f - s.astype(F)).astype(F)
    A = F(-0.75)
    one, two, three, four, five, eight = (F(v) for v in (1, 2, 3, 4, 5, 8))
    m = lambda a, b: (a * b).astype(F)
    ad = lambda a, b: (a + b).astype(F)
    sb = lambda a, b: (a - b).astype(F)
    f1 = ad(f, one)
    c0 = sb(m(ad(m(sb(m(A, f1), m(five, A)), f1), m(eight, A)), f1), m(four, A))
    c1 = ad(m(m(sb(m(ad(A, two), f), ad(A, three)), f), f), one)
    g = sb(one, f)
    c2 = ad(m(m(sb(m(ad(A, two), g), ad(A, three)), g), g), one)
    c3 = sb(sb(sb(one, c0), c1), c2)
    return s, np.stack([c0, c1, c2, c3], axis=1)


def _taps(s, n_src, variant=None):
    idx = s[:, None] - 1 + np.arange(4)[None, :]
    if variant == "no_right_clamp":                              # the last column is not clamped: the tap runs into the next row
        return np.maximum(idx, 0)
    return np.clip(idx, 0, n_src - 1)


def resize_cubic_u8(src, dw, dh, scale_x, scale_y, variant=None):
    """cv::resize INTER_CUBIC on CV_8UC1: weights rounded (half to even) to 11 fractional bits and saturated to int16, rows and
    columns in integers, (acc + 2^21) >> 22, saturated to 0..255."""
    _check(variant, ("no_right_clamp",))
    src = np.ascontiguousarray(src, np.uint8)
    sh, sw = src.shape
    sx, cx = _cubic_axis(dw, scale_x)
    sy, cy = _cubic_axis(dh, scale_y)
    q = lambda c: np.clip(np.rint((c * F(2048.0)).astype(F)).astype(np.int64), -32768, 32767)
    qx, qy = q(cx), q(cy)
    tx, ty = _taps(sx, sw, variant), _taps(sy, sh)
    flat = src.ravel().astype(np.int64)
    acc = np.zeros((dh, dw), np.int64)
    for k in range(4):
        hs = np.zeros((dh, dw), np.int64)
        for j in range(4):
            idx = np.minimum(ty[:, k][:, None] * sw + tx[:, j][None, :], flat.size - 1)
            hs += flat[idx] * qx[:, j][None, :]
        acc += hs * qy[:, k][:, None]
    return np.clip((acc + (1 << 21)) >> 22, 0, 255).astype(np.uint8)


def resize_f32(src, dw, dh, cubic, variant=None):
    """cv::resize(src, dst, Size(dw, dh), 0, 0, ...) on CV_32FC1; nearest: floor(d * scale) clamped; cubic: four taps times their
    weights summed left to right per row, then the four rows top to bottom, all in float32."""
    _check(variant, ())
    src = np.ascontiguousarray(src, F)
    sh, sw = src.shape
    scx, scy = sw / dw, sh / dh
    if not cubic:
        ix = np.clip(np.floor(np.arange(dw) * scx).astype(np.int64), 0, sw - 1)
        iy = np.clip(np.floor(np.arange(dh) * scy).astype(np.int64), 0, sh - 1)
        return src[iy][:, ix]
    sx, cx = _cubic_axis(dw, scx)
    sy, cy = _cubic_axis(dh, scy)
    tx, ty = _taps(sx, sw), _taps(sy, sh)
    rows = []
    for k in range(4):
        r = src[ty[:, k]]
        p = [(r[:, tx[:, j]] * cx[:, j][None, :]).astype(F) for j in range(4)]
        rows.append((((p[0] + p[1]).astype(F) + p[2]).astype(F) + p[3]).astype(F))
    p = [(rows[k] * cy[:, k][:, None]).astype(F) for k in range(4)]
    return (((p[0] + p[1]).astype(F) + p[2]).astype(F) + p[3]).astype(F)


def postprocess_ex(d16, mindisp, numdisp, off, dense_scale, nd, ne, med, ow, oh, cc_threshold=0):
    """:853-986 with every option: the chain with the two resized copies between the erosions and the mask."""
    a = convert(d16, mindisp, numdisp, off, 1.0 / dense_scale)
    for _ in range(max(nd, 0)):
        a = dilate(a)
    for _ in range(max(ne, 0)):
        a = erode(a)
    if (oh, ow) == a.shape:
        nn = cub = a
    else:
        nn, cub = resize_f32(a, ow, oh, False), resize_f32(a, ow, oh, True)
    a = mask_step(nn, cub)
    if med >= 3:
        a = median(a, med)
    if cc_threshold > 0:
        a = biggest_component(a, cc_threshold)[0]
    return a
