"""Inputs of the clean-up edge suite (tests/test_cleanup_edges.py holds them in place on the CPU, tests/test_cleanup_edges_gpu.py runs
them through the kernels).  Every probe is a pure function of its arguments: no global random state, no files."""
import numpy as np

TILE = (64, 32)                                                   # the fused chain kernel's output tile
NUMDISP, MINDISP = 128, 1

SHAPES = [(1, 1), (2, 2), (3, 3), (2, 40), (40, 2), (63, 31), (64, 32), (65, 33), (129, 65), (257, 97)]
LATTICE_SHAPES = [(129, 65), (257, 97)]
# (dilations, erosions, median): (9, 9, 5) is the largest setting whose tile fits 64 KiB of LDS, (10, 9, 5) the first that does not
STEPS = [(0, 0, 0), (1, 2, 0), (1, 2, 3), (1, 2, 5), (3, 3, 5), (0, 3, 3), (3, 0, 5), (9, 9, 5), (10, 9, 5)]
HOLE_FRACTIONS = [0.05, 0.20, 0.50]
OFFSETS = [0, 3, -2]
MIN_DISPS = [0, 1, 3]
COMPONENT_SHAPES = [(255, 9), (256, 9), (257, 9), (97, 61), (512, 64), (1024, 256)]


def random_holes(w, h, frac, seed=0):
    """int16 fixed-point disparities in 1/16 steps, most of them valid for (MINDISP, NUMDISP); `frac` of the cells are holes (-16, what
    SGM writes), and a few sit exactly on and next to the two limits of clean_and_convert."""
    rng = np.random.default_rng([seed, w, h, int(frac * 1000)])
    d = rng.integers(16 * 2, 16 * 100, (h, w)).astype(np.int16)
    d[rng.random((h, w)) < frac] = -16
    edge = np.array([16 * MINDISP, 16 * MINDISP + 1, 16 * NUMDISP, 16 * NUMDISP + 1, 0, 16 * 3, 16 * 3 + 1], np.int16)
    m = rng.random((h, w)) < 0.02
    d[m] = edge[rng.integers(0, len(edge), int(m.sum()))]
    return d


def seams(n, t):
    return list(range(t, n, t))


def lattice_places(w, h, reach=3):
    """(x, y, size) of the holes of the seam lattice: along every tile seam a staircase that crosses it, one hole per offset
    -reach..reach from the seam, single cells and 2 x 2 blocks in turn, far enough apart not to touch."""
    out = []
    k = 0
    span = 2 * reach + 1
    for X in seams(w, TILE[0]) + [w - 1 - reach]:                # (the last entry: the same staircase against the picture's right edge)
        for m in range(0, max(1, (h - 4) // (5 * span)) + 1):
            for d in range(-reach, reach + 1):
                y = 2 + 5 * (d + reach) + 5 * span * m
                if 0 <= X + d < w - 1 and y < h - 1:
                    out.append((X + d, y, 1 + k % 2)); k += 1
    for Y in seams(h, TILE[1]) + [h - 1 - reach]:
        for m in range(0, max(1, (w - 4) // (5 * span)) + 1):
            for d in range(-reach, reach + 1):
                x = 3 + 5 * (d + reach) + 5 * span * m
                if 0 <= Y + d < h - 1 and x < w - 1:
                    out.append((x, Y + d, 1 + k % 2)); k += 1
    return out


def texture(w, h):
    y, x = np.mgrid[0:h, 0:w]
    return (16 * (20 + (7 * x + 13 * y) % 50)).astype(np.int16)


def halo_edge_holes(w, h, nd, ne, med):
    """Holes (x0, y0, x1, y1, inclusive) whose fate after the chain (nd, ne, med) hangs on the outermost cell of a tile's halo, one per
    side and seam.  A dilation closes a rectangular hole by two columns from the right and by a row from above and from below,
    never from the left; an erosion then widens what is left by a cell all round, the median looks med/2 further.  So
      right: a hole 2 nd wide and 2 nd + 1 high that ends one column before the halo's last: it closes in exactly nd steps, and only
             if the first step saw the last column (nd = 0: the last column itself is the hole);
      above / below: the same turned, 2 nd high and 2 nd + 1 wide, one row inside the halo's first / last row;
      left:  a hole that nd dilations shrink to the single cell in the halo's first column.
    A tile that carries one column or row less leaves the first three open and never sees the fourth."""
    rm = med // 2 if med >= 3 else 0
    hl, hr, hv = ne + 1 + rm, 2 * nd + ne + 1 + rm, nd + ne + 1 + rm
    out = []
    ya, yb = 8 + nd, min(h - 1, TILE[1]) + 8 + nd                 # rows of the right / left probes (second tile row where there is one)
    for X in seams(w, TILE[0]):
        last = X - 1 + hr                                       # last halo column of the tile that ends at X - 1
        out.append((last - 2 * nd, ya - nd, last - 1, ya + nd) if nd else (last, ya, last, ya))
        first = X - hl                                          # first halo column of the tile that starts at X
        out.append((first, yb - nd, first + 2 * nd, yb + nd))
    xa, xb = 10, min(w - 1, TILE[0]) + 24
    for Y in seams(h, TILE[1]):
        first, last = Y - hv, Y - 1 + hv
        out.append((xa, first + 1, xa + 2 * nd, first + 2 * nd) if nd else (xa, first, xa, first))
        out.append((xb, last - 2 * nd, xb + 2 * nd, last - 1) if nd else (xb, last, xb, last))
    m = ne + 2 + rm                                             # keep clear of what the picture's own border does
    return [r for r in out if r[0] >= m and r[1] >= m and r[2] < w - m - 2 and r[3] < h - m]


def seam_lattice(w, h, steps=(0, 0, 0), reach=3):
    """A textured valid map with single holes and 2 x 2 holes at -reach..reach cells from every tile seam, and the holes of
    halo_edge_holes for the chain `steps`.  The small holes are grown by what the chain's dilations will close again (2 nd columns
    to the right, nd rows up and down, at most 3 steps' worth), so that after them the single and 2 x 2 holes are left where they
    are meant to be."""
    nd, ne, med = steps
    grow = min(nd, 3)
    d = texture(w, h)
    edge = halo_edge_holes(w, h, nd, ne, med)
    # a small hole stays away from a halo-edge hole by what the chain spreads either of them, or it would cover the cells that show
    # whether the halo-edge hole was seen
    keep = 2 * (ne + 1 + (med // 2 if med >= 3 else 0)) + 2
    for x, y, s in lattice_places(w, h, reach):
        x0, y0, x1, y1 = x, max(y - grow, 0), x + s - 1 + 2 * grow, y + s - 1 + grow
        if any(x0 <= e[2] + keep and e[0] - keep <= x1 and y0 <= e[3] + keep and e[1] - keep <= y1 for e in edge):
            continue
        d[y0:y1 + 1, x0:x1 + 1] = -16
    for x0, y0, x1, y1 in edge:
        d[y0:y1 + 1, x0:x1 + 1] = -16
    return d


def seam_lattice_inverse(w, h, reach=3):
    """A zero map with single survivors and 2 x 2 survivors at the same places."""
    t = texture(w, h)
    d = np.full((h, w), -16, np.int16)
    for x, y, s in lattice_places(w, h, reach):
        d[y:y + s, x:x + s] = t[y:y + s, x:x + s]
    return d


# ---------------------------------------------------------------------------------------------------------------- median
def median_maps():
    """name -> float32-valued int16 maps for the median alone (dilate = erode = 0 still applies the mask step, so the values that
    matter sit away from the border on the larger maps; the small ones are all border)"""
    rng = np.random.default_rng(5)
    out = {}
    for w, h in ((1, 1), (2, 5), (5, 2), (4, 4)):
        out[f"small{w}x{h}"] = rng.integers(32, 1600, (h, w)).astype(np.int16)
    out["ties"] = (16 * (2 + rng.integers(0, 3, (21, 23)))).astype(np.int16)            # three values only: every window ties
    z = rng.integers(32, 1600, (21, 23)).astype(np.int16)
    z[rng.random((21, 23)) < 0.05] = -16                                                   # the mask step widens each to 3 x 3: the median flips between 0 and a value
    out["zeros"] = z
    return out


# ---------------------------------------------------------------------------------------------------------------- components
def _blank(w, h):
    return np.zeros((h, w), np.float32)


def comp_empty(w, h):
    return _blank(w, h)


def comp_full(w, h):
    return np.full((h, w), 7.0, np.float32)


def comp_two_equal(w, h):
    """Two components of the same area.  A starts in row 1 at column w-4 (first in raster order) and hangs down as a 3-wide bar; B
    starts one row lower at column 1, left of A's start: 'smallest column' or 'later label' would pick B."""
    f = _blank(w, h)
    n = min(h - 3, 4)
    f[1:1 + n, w - 4:w - 1] = 5.0
    f[2:2 + n, 1:4] = 6.0
    return f


def comp_three_sizes(w, h):
    f = _blank(w, h)
    f[1:3, 1:4] = 5.0                                            # 6
    f[1:4, w // 2:w // 2 + 4] = 6.0                              # 12: the winner, neither first nor last
    f[h - 3:h - 1, w - 4:w - 1] = 5.5                            # 6
    f[h - 2, 1] = 4.0                                            # 1
    return f


def comp_diagonal(w, h, anti=False):
    """One component joined through diagonals only, crossing the 256-thread block boundary (columns 255 | 256) where the map is that
    wide, else the middle; a lone 2-cell bar elsewhere is the runner-up."""
    f = _blank(w, h)
    n = min(h, w, 7)
    c = 255 if w >= 257 else w // 2
    x0 = max(min(c - n // 2, w - n), 0)
    for k in range(n):
        f[k, x0 + (n - 1 - k if anti else k)] = 5.0
    if w >= 6 and x0 >= 4:
        f[h - 1, 0:2] = 3.0
    return f


def comp_row_end(w, h):
    """Active at (y, w-1) and (y+1, 0) only: two components of one cell; a raster index that wraps would join them."""
    f = _blank(w, h)
    y = h // 2 - 1 if h >= 2 else 0
    f[y, w - 1] = 5.0
    if y + 1 < h:
        f[y + 1, 0] = 6.0
    return f


def comp_serpentine(w, h):
    """One 1-wide path: every even row full, joined to the next even row alternately at the right and the left end."""
    f = _blank(w, h)
    f[0::2, :] = 5.0
    for k, y in enumerate(range(1, h - 1, 2)):
        f[y, w - 1 if k % 2 == 0 else 0] = 5.0
    if h % 2 == 0:
        f[h - 1, :] = 0.0
    return f


def comp_spiral(w, h):
    """A 1-wide path that winds inwards from (0, 0), clockwise, leaving a 1-wide gap to its earlier turns: it goes straight while
    the next cell is free and the one after it is not part of the path, else turns right, and ends where it can do neither."""
    f = _blank(w, h)
    x = y = 0
    dx, dy = 1, 0
    f[0, 0] = 5.0
    while True:
        for _ in range(2):
            nx, ny, ax, ay = x + dx, y + dy, x + 2 * dx, y + 2 * dy
            if 0 <= nx < w and 0 <= ny < h and f[ny, nx] == 0 and not (0 <= ax < w and 0 <= ay < h and f[ay, ax] != 0):
                x, y = nx, ny
                f[y, x] = 5.0
                break
            dx, dy = -dy, dx
        else:
            return f


def comp_comb(w, h):
    """Teeth in every other column from row 0 down, joined only by the last row."""
    f = _blank(w, h)
    f[:, 0::2] = 5.0
    f[h - 1, :] = 5.0
    return f


def comp_checkerboard(w, h):
    y, x = np.mgrid[0:h, 0:w]
    return np.where((x + y) % 2 == 0, 5.0, 0.0).astype(np.float32)


COMPONENT_MAPS = {
    "empty": comp_empty, "full": comp_full, "two_equal": comp_two_equal, "three_sizes": comp_three_sizes,
    "diagonal": comp_diagonal, "antidiagonal": lambda w, h: comp_diagonal(w, h, True), "row_end": comp_row_end,
    "serpentine": comp_serpentine, "spiral": comp_spiral, "comb": comp_comb, "checkerboard": comp_checkerboard,
}
def component_expect(name, w, h):
    """(number of 8-connected components, area of the one kept) a map is built to have; None where the builder does not fix it."""
    even_rows = (h + 1) // 2
    return {
        "empty": (0, 0), "full": (1, w * h), "two_equal": (2, 3 * min(h - 3, 4)), "three_sizes": (4, 12),
        "diagonal": (2, 7), "antidiagonal": (2, 7), "row_end": (2, 1),
        "serpentine": (1, even_rows * w + even_rows - 1), "spiral": (1, None),
        "comb": (1, ((w + 1) // 2) * (h - 1) + w), "checkerboard": (1, (w * h + 1) // 2),
    }[name]


HARD_MAPS = ("serpentine", "spiral", "comb", "checkerboard", "diagonal", "antidiagonal")
# flat maps have no gradient away from their edges; the component tests use a threshold no edge of these heights reaches
COMPONENT_THR = 100000


def as_int16(f):
    """A component map as a speckle picture: 160 where active, new_val = 0 elsewhere."""
    return np.where(f != 0, 160, 0).astype(np.int16)


# ---------------------------------------------------------------------------------------------------------------- Sobel
def sobel_ramp(w=40, h=10):
    y, x = np.mgrid[0:h, 0:w]
    return (3 * x + 5).astype(np.float32)


def sobel_step(s, w=24, h=10):
    """0 left of the middle column, s from it on: the squared gradient on the two columns of the step is (4 s)^2 = 16 s^2."""
    f = np.zeros((h, w), np.float32)
    f[:, w // 2:] = s
    return f


# ---------------------------------------------------------------------------------------------------------------- speckles
def speckle_probes():
    """name -> (img, new_val, max_size, max_diff)"""
    out = {}
    a = np.zeros((12, 20), np.int16)
    a[2:5, 2:6] = 160                                           # 12 pixels: exactly max_size
    a[7:10, 2:6] = 160; a[10, 2] = 160                          # 13 pixels
    out["exact_size"] = (a, 0, 12, 16)
    c = np.full((5, 13), -16, np.int16)
    c[2, 2:11] = 160 + 16 * np.arange(9)                        # eight steps of 16: ends 128 apart, one region at max_diff 16
    out["chain16"] = (c, -16, 8, 16)
    out["chain15"] = (c, -16, 8, 15)
    d = np.zeros((8, 8), np.int16)
    for k in range(6):
        d[1 + k, 1 + k] = 160                                   # six equal values touching only diagonally
    out["diagonal"] = (d, 0, 5, 16)
    s = np.full((7, 11), 160, np.int16)
    s[:, 5] = -16                                               # a wall of new_val: two halves of 35, never joined through it
    out["split"] = (s, -16, 40, 400)
    e = np.zeros((6, 8), np.int16)
    e[1:5, 1:4] = 32767; e[1:5, 4:7] = -32768                   # 12 + 12: a 16-bit difference would read 65535 as -1
    out["extremes"] = (e, 0, 12, 16)
    out["extremes_big"] = (e, 0, 23, 16)
    return out


# ---------------------------------------------------------------------------------------------------------------- resizers
def picture(w, h, seed=0):
    rng = np.random.default_rng([seed, w, h])
    y, x = np.mgrid[0:h, 0:w]
    return np.clip(128 + 90 * np.sin(0.37 * x + 0.11 * y) + rng.integers(-40, 41, (h, w)), 0, 255).astype(np.uint8)


RESIZE_SOURCES = [(1, 1), (2, 3), (3, 3), (97, 61)]
RESIZE_FACTORS = [(0.5, 0.5), (0.73, 0.73), (1.37, 1.0), (2.0, 1.0)]          # (fx, fy): above 1 the reference stretches x only
RESIZE_DEST_WIDTHS = [255, 256, 257, 513]


def resize_cases():
    """(sw, sh, dw, dh): every source to the factors' sizes, to the block-edge widths and to 1 x 1."""
    out = []
    for sw, sh in RESIZE_SOURCES:
        for fx, fy in RESIZE_FACTORS:
            out.append((sw, sh, max(1, int(np.rint(sw * fx))), max(1, int(np.rint(sh * fy)))))
        out.append((sw, sh, 1, 1))
    for dw in RESIZE_DEST_WIDTHS:
        out.append((97, 61, dw, 33))
        out.append((3, 3, dw, 2))
    return sorted(set(out))


def float_resize_cases():
    """(ws, hs, dense_scale, ow, oh): the map is the small source, the output what the crop had before it was scaled"""
    out = []
    for ws, hs in RESIZE_SOURCES:
        for fx, fy in RESIZE_FACTORS:
            out.append((ws, hs, fx, max(1, int(np.rint(ws / fx))), max(1, int(np.rint(hs / fy)))))
    return out


# ---------------------------------------------------------------------------------------------------------------- masks
MASK_SIZES = [4, 8, 1020, 1024, 1028, 4100, 1, 2, 3, 5, 1023, 1025]


def mask_bytes(n):
    """253, 254 and 255 at every position modulo 4 (period 3 against period 4), the rest of the range in between."""
    i = np.arange(n)
    b = (253 + i % 3).astype(np.uint8)
    b[i % 7 == 6] = (i[i % 7 == 6] * 37 % 253).astype(np.uint8)
    return b


def file_mask_bytes(n):
    i = np.arange(n)
    return np.array([0, 1, 255], np.uint8)[(i // 2) % 3]
