"""Direct-form numpy restatement of the prepare stage: the three resamplers of wass_amd/csrc/rectify.hip (bicubic remap through two float32
maps, perspective warp, undistortion; both of the latter bilinear) and the contrast equalisation of wass_amd/csrc/clahe.hip.  Test
infrastructure only, written from the statement in NOTES/oracle_and_pins.md ("Rectification (f1) is restated ...") and from the header
comments of the two kernels' files; it shares no code with oracle/*.c, which tests/test_prepare_edges.py holds it bit-equal to on every
probe of tests/prepare_probes.py.

Everything is integer arithmetic on int64 arrays or IEEE arithmetic of the stated width, one rounding per operation (numpy fuses nothing):

  tables      the 1-D coefficients in float32 (linear: 1 - x, x; cubic: Keys, A = -0.75, the last one 1 - c0 - c1 - c2), their products
              times 2^15 rounded to nearest even and saturated to int16, and the sum fix-up: where an entry does not sum to 2^15 the
              difference goes to the largest (sum too small) or the smallest (sum too large) of the four weights at [k/2, k/2 + 2)^2 of the
              entry's own storage, which for the bilinear table reaches past the entry into weights not yet written (zeros);
  coordinates in 1/32 pixel, round to nearest even: float32(map) * 32.0f for the remap; (X0 + M0 x1) * (32 / W) per block of bw0 columns
              for the warp, W == 0 giving 0, clamped to the int32 range; the fp64 polynomial of per-column and per-row normalised
              coordinates for the undistortion, whose tables are built per stripe of max(1, 4096 / w) rows and divided by _w;
  window      X >> 5, saturated to int16 by the remap and the warp and wrapped to int16 by the undistortion; phase (Y & 31) * 32 + (X & 31);
  tap sum     (sum + 2^14) >> 15, clamped to 0 .. 255, taps outside the picture 0;
  CLAHE       the histogram of each tile of the reflect-101 extended picture, clipped, the excess redistributed (a batch to every bin, the
              residual one count each to bins 0, step, 2 step, ... with step = max(256 / residual, 1)), the table
              rint(float32(cumulative) * (255.0f / area)), and the float32 blend of the four neighbouring tables.

A float32 map product beyond the int32 range saturates here (the kernel's conversion); the probes hold such values only where every tap
lies outside either way.  NaN maps are left out: their rounding is undefined in the reference.

SWITCHES names the mistakes a test must be able to see; each function takes those that apply to it as keyword arguments."""
import numpy as np

F = np.float32
SWITCHES = ("truncate", "swap_phase", "no_fixup", "saturate_undistort", "wrap_remap", "one_block", "w0_as_inf", "transpose_grid",
            "no_residual_step", "lut_half_up")


# ---- tables -------------------------------------------------------------------------------------------------------------------------------
def coeffs_1d(ksize):
    """[32, ksize] float32: the weights along one axis at the fractions 0, 1/32, ..., 31/32"""
    x = np.arange(32, dtype=F) * F(1.0 / 32)
    if ksize == 2:
        return np.stack([F(1) - x, x], 1)
    A = F(-0.75)
    x1, u = x + F(1), F(1) - x
    c0 = ((A * x1 - F(5) * A) * x1 + F(8) * A) * x1 - F(4) * A
    c1 = ((A + F(2)) * x - (A + F(3))) * x * x + F(1)
    c2 = ((A + F(2)) * u - (A + F(3))) * u * u + F(1)
    c3 = F(1) - c0 - c1 - c2
    out = np.stack([c0, c1, c2, c3], 1)
    assert out.dtype == F
    return out


_TABLES = {}


def weight_table(ksize, no_fixup=False):
    """[1024, ksize, ksize] int64, entry fy * 32 + fx, weight [ky, kx]"""
    key = (ksize, bool(no_fixup))
    if key in _TABLES:
        return _TABLES[key]
    c = coeffs_1d(ksize)
    kk, k0 = ksize * ksize, ksize // 2
    flat = np.zeros(1024 * kk + 64, np.int64)                         # the entries in the order they are written, zeros behind them
    for fy in range(32):
        for fx in range(32):
            at = (fy * 32 + fx) * kk
            prod = c[fy][:, None] * c[fx][None, :]
            assert prod.dtype == F
            q = np.clip(np.rint(prod * F(32768)), -32768, 32767).astype(np.int64)
            flat[at:at + kk] = q.ravel()
            diff = int(q.sum()) - 32768
            if diff and not no_fixup:
                places = [at + k1 * ksize + k2 for k1 in (k0, k0 + 1) for k2 in (k0, k0 + 1)]
                lo = hi = places[0]
                for p in places:
                    if flat[p] < flat[lo]:
                        lo = p
                    elif flat[p] > flat[hi]:
                        hi = p
                flat[hi if diff < 0 else lo] -= diff
    tab = flat[:1024 * kk].reshape(1024, ksize, ksize)
    tab.setflags(write=False)
    _TABLES[key] = tab
    return tab


# ---- the sampler ------------------------------------------------------------------------------------------------------------------------
def sat16(v):
    return np.clip(v, -32768, 32767)


def wrap16(v):
    return (v + 32768) % 65536 - 32768


def _round(v, truncate):
    return np.trunc(v) if truncate else np.rint(v)


def tap_sum(src, X, Y, tab, wrap, swap_phase=False):
    """src u8 [sh, sw]; X, Y int64 in 1/32 pixel; the window's second tap (cubic) or first tap (linear) is at (X >> 5, Y >> 5)"""
    src = np.asarray(src, np.uint8).astype(np.int64)
    sh, sw = src.shape
    k = tab.shape[1]
    fit = wrap16 if wrap else sat16
    sx, sy = fit(X >> 5) - (k // 2 - 1), fit(Y >> 5) - (k // 2 - 1)
    a = (X & 31) * 32 + (Y & 31) if swap_phase else (Y & 31) * 32 + (X & 31)
    w = tab[a]
    total = np.zeros(X.shape, np.int64)
    for i in range(k):
        for j in range(k):
            yy, xx = sy + i, sx + j
            inside = (yy >= 0) & (yy < sh) & (xx >= 0) & (xx < sw)
            total += np.where(inside, src[np.clip(yy, 0, sh - 1), np.clip(xx, 0, sw - 1)], 0) * w[..., i, j]
    return np.clip((total + (1 << 14)) >> 15, 0, 255).astype(np.uint8)


# ---- remap, bicubic -----------------------------------------------------------------------------------------------------------------------
def remap_coords(mx, my, truncate=False):
    out = []
    for m in (mx, my):
        v = np.asarray(m, F) * F(32)
        assert v.dtype == F
        out.append(np.clip(_round(v.astype(np.float64), truncate), -2147483648.0, 2147483647.0).astype(np.int64))
    return out


def remap_cubic(src, mx, my, truncate=False, swap_phase=False, no_fixup=False, wrap_remap=False):
    X, Y = remap_coords(mx, my, truncate)
    return tap_sum(src, X, Y, weight_table(4, no_fixup), wrap_remap, swap_phase)


# ---- warp, bilinear ------------------------------------------------------------------------------------------------------------------------
def inv33(m):
    """the closed form of a 3 x 3 inverse in fp64, one rounding per operation, cofactor times 1 / det"""
    m = [float(v) for v in np.ravel(m)]
    d = m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6])
    d = 1.0 / d
    return [(m[4] * m[8] - m[5] * m[7]) * d, (m[2] * m[7] - m[1] * m[8]) * d, (m[1] * m[5] - m[2] * m[4]) * d,
            (m[5] * m[6] - m[3] * m[8]) * d, (m[0] * m[8] - m[2] * m[6]) * d, (m[2] * m[3] - m[0] * m[5]) * d,
            (m[3] * m[7] - m[4] * m[6]) * d, (m[1] * m[6] - m[0] * m[7]) * d, (m[0] * m[4] - m[1] * m[3]) * d]


def block_width(dw, dh):
    return min(1024 // min(16, dh), dw)


def warp_terms(H, dw, dh, one_block=False):
    """(numerator of x, numerator of y, W) as fp64 [dh, dw]: what the warp divides, evaluated per block of bw0 columns"""
    m = inv33(H)
    bw0 = dw if one_block else block_width(dw, dh)
    x = np.arange(dw)
    bx = ((x // bw0) * bw0).astype(np.float64)
    x1 = (x % bw0).astype(np.float64)
    y = np.arange(dh, dtype=np.float64)[:, None]
    X0 = m[0] * bx + m[1] * y + m[2]
    Y0 = m[3] * bx + m[4] * y + m[5]
    W0 = m[6] * bx + m[7] * y + m[8]
    return X0 + m[0] * x1, Y0 + m[3] * x1, W0 + m[6] * x1


def warp_coords(H, dw, dh, truncate=False, one_block=False, w0_as_inf=False):
    nx, ny, W = warp_terms(H, dw, dh, one_block)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        s = 32.0 / W if w0_as_inf else np.where(W != 0.0, 32.0 / np.where(W != 0.0, W, 1.0), 0.0)
        # fmin / fmax: a NaN (0 * inf, with w0_as_inf only) gives the other operand
        fX = np.fmax(-2147483648.0, np.fmin(2147483647.0, nx * s))
        fY = np.fmax(-2147483648.0, np.fmin(2147483647.0, ny * s))
    return _round(fX, truncate).astype(np.int64), _round(fY, truncate).astype(np.int64)


def warp_linear(src, H, dw, dh, truncate=False, swap_phase=False, wrap_remap=False, one_block=False, w0_as_inf=False):
    X, Y = warp_coords(H, dw, dh, truncate, one_block, w0_as_inf)
    return tap_sum(src, X, Y, weight_table(2), wrap_remap, swap_phase)


# ---- undistortion, bilinear ------------------------------------------------------------------------------------------------------------------
def undistort_tables(K, w, h, divide=True):
    """(xs [w], ys [h]): the normalised coordinates per column and per row; divide=False is the form without * (1 / _w)"""
    K = [float(v) for v in np.ravel(K)]
    xs, ys = np.empty(w), np.empty(h)
    rows = min(max(1, 4096 // max(w, 1)), h)
    for y0 in range(0, h, rows):
        A = list(K)
        A[5] = K[5] - y0
        ir = inv33(A)
        for i in range(min(rows, h - y0)):
            ww = 1.0 / (i * ir[7] + ir[8]) if divide else 1.0
            ys[y0 + i] = (i * ir[4] + ir[5]) * ww
            if y0 == 0 and i == 0:                       # ir[1] = ir[7] = 0: every row of every stripe holds the same column sequence
                _x = i * ir[1] + ir[2]
                for j in range(w):
                    xs[j] = _x * ww
                    _x += ir[0]
    return xs, ys


def undistort_coords(K, dist, w, h, truncate=False, divide=True):
    K = np.asarray(K, np.float64).reshape(3, 3)
    k = np.zeros(12)
    k[:len(np.ravel(dist))] = np.ravel(dist)
    xs, ys = undistort_tables(K, w, h, divide)
    x, y = xs[None, :], ys[:, None]
    x2, y2 = x * x, y * y
    r2, _2xy = x2 + y2, 2 * x * y
    kr = (1 + ((k[4] * r2 + k[1]) * r2 + k[0]) * r2) / (1 + ((k[7] * r2 + k[6]) * r2 + k[5]) * r2)
    xd = x * kr + k[2] * _2xy + k[3] * (r2 + 2 * x2) + k[8] * r2 + k[9] * r2 * r2
    yd = y * kr + k[2] * (r2 + 2 * y2) + k[3] * _2xy + k[10] * r2 + k[11] * r2 * r2
    u, v = K[0, 0] * xd + K[0, 2], K[1, 1] * yd + K[1, 2]
    iu = _round(np.clip(u * 32, -2147483648.0, 2147483647.0), truncate).astype(np.int64)
    iv = _round(np.clip(v * 32, -2147483648.0, 2147483647.0), truncate).astype(np.int64)
    return iu, iv


def undistort(src, K, dist, truncate=False, swap_phase=False, saturate_undistort=False):
    h, w = np.asarray(src).shape
    iu, iv = undistort_coords(K, dist, w, h, truncate)
    return tap_sum(src, iu, iv, weight_table(2), not saturate_undistort, swap_phase)


# ---- CLAHE ---------------------------------------------------------------------------------------------------------------------------------
def reflect101(i, n):
    i = np.array(i, np.int64)
    if n == 1:
        return np.zeros_like(i)
    while ((i < 0) | (i >= n)).any():
        i = np.where(i < 0, -i, i)
        i = np.where(i >= n, 2 * n - 2 - i, i)
    return i


def clahe_geometry(w, h, tiles_x, tiles_y, clip_limit):
    """(tile width, tile height, clip): a picture that is no multiple of the grid in either axis is extended in both"""
    if w % tiles_x == 0 and h % tiles_y == 0:
        ew, eh = w, h
    else:
        ew, eh = w + (tiles_x - w % tiles_x), h + (tiles_y - h % tiles_y)
    tw, th = ew // tiles_x, eh // tiles_y
    clip = max(int(clip_limit * (tw * th) / 256), 1) if clip_limit > 0.0 else 0
    return tw, th, clip


def clahe_hist(values, clip, no_residual_step=False):
    """the clipped and redistributed 256-bin histogram of one tile"""
    hist = np.bincount(np.ravel(values), minlength=256).astype(np.int64)
    if clip > 0:
        excess = int(np.maximum(hist - clip, 0).sum())
        hist = np.minimum(hist, clip)
        batch, residual = divmod(excess, 256)
        hist += batch
        if residual:
            step = 1 if no_residual_step else max(256 // residual, 1)
            bins = np.arange(residual) * step
            hist[bins[bins < 256]] += 1
    return hist


def clahe_luts(src, clip_limit, tiles_x, tiles_y, transpose_grid=False, no_residual_step=False, lut_half_up=False):
    """[tiles_y * tiles_x, 256] int64, tile ty * tiles_x + tx"""
    src = np.asarray(src, np.uint8)
    h, w = src.shape
    tw, th, clip = clahe_geometry(w, h, tiles_x, tiles_y, clip_limit)
    scale = F(255) / F(tw * th)
    luts = np.empty((tiles_x * tiles_y, 256), np.int64)
    for t in range(tiles_x * tiles_y):
        tx, ty = (t % tiles_y, t // tiles_y) if transpose_grid else (t % tiles_x, t // tiles_x)
        rows, cols = reflect101(ty * th + np.arange(th), h), reflect101(tx * tw + np.arange(tw), w)
        cum = np.cumsum(clahe_hist(src[rows][:, cols], clip, no_residual_step)).astype(F) * scale
        assert cum.dtype == F
        r = np.floor(cum.astype(np.float64) + 0.5) if lut_half_up else np.rint(cum)
        luts[t] = np.clip(r, 0, 255).astype(np.int64)
    return luts


def clahe(src, clip_limit, tiles_x, tiles_y, transpose_grid=False, no_residual_step=False, lut_half_up=False):
    src = np.asarray(src, np.uint8)
    h, w = src.shape
    tw, th, _ = clahe_geometry(w, h, tiles_x, tiles_y, clip_limit)
    lut = clahe_luts(src, clip_limit, tiles_x, tiles_y, transpose_grid, no_residual_step, lut_half_up).astype(F)

    def axis(n, size, tiles):
        f = np.arange(n, dtype=F) * (F(1) / F(size)) - F(0.5)
        t1 = np.floor(f)
        a = f - t1
        t1 = t1.astype(np.int64)
        return np.maximum(t1, 0), np.minimum(t1 + 1, tiles - 1), a, F(1) - a

    ty1, ty2, ya, ya1 = (v[:, None] for v in axis(h, th, tiles_y))
    tx1, tx2, xa, xa1 = (v[None, :] for v in axis(w, tw, tiles_x))
    v = src.astype(np.int64)
    res = (lut[ty1 * tiles_x + tx1, v] * xa1 + lut[ty1 * tiles_x + tx2, v] * xa) * ya1 + \
          (lut[ty2 * tiles_x + tx1, v] * xa1 + lut[ty2 * tiles_x + tx2, v] * xa) * ya
    assert res.dtype == F
    return np.clip(np.rint(res), 0, 255).astype(np.uint8)
