"""Plain numpy / fp64 references and scene builders for the mesh stage tests (tests/test_mesh_edges.py, tests/test_mesh_edges_gpu.py).

The references restate the definitions of the reference program (wass_stereo/PovMesh.cpp, line numbers in the docstrings), not the
kernels of wass_amd/csrc/mesh.hip.  Each takes a keyword that switches ONE known mistake on (VARIANTS); the CPU tests show for
every probe scene that its variant changes the result, so a kernel with that mistake cannot pass the GPU test of that scene.

Arrays are (h, w) row major as everywhere in the project: valid uint8, z float64, p3d (h, w, 3) float64.
"""
import itertools

import numpy as np

VARIANTS = {
    "link": ("lt", "le"),               # |dz| < zgap  /  <=
    "tie": ("colmajor", "raster"),      # equal sizes: smallest u*h + v  /  smallest v*w + u
    "rank": ("floor", "ceil"),          # index of the order statistic
    "cols": ("interior", "all"),        # gap columns 1 .. w-2  /  0 .. w-1
    "above": ("three", "two"),          # neighbours -1, 0, +1 of the row above  /  -1, 0 only
    "count": ("lt", "le"),              # |distance| < thr  /  <=
}

# every launch edge of the stage, w x h ("What the mesh edge suite pins")
SMALL = [(1, 1), (1, 7), (7, 1), (2, 2), (3, 2), (3, 3), (5, 4), (16, 16), (17, 15), (257, 1), (63, 7), (64, 8), (65, 9),
         (255, 3), (256, 4), (257, 5), (128, 64), (129, 64), (3, 257), (4, 258), (5, 513)]
PCTS = (0.0, 3.0, 50.0, 98.7, 99.0, 100.0)


def pred(x):
    """the double just below x > 0"""
    return float(np.nextafter(x, 0.0))


def succ(x):
    return float(np.nextafter(x, np.inf))


def as_mesh(valid, z=None, x=None, y=None):
    """(valid uint8, p3d) C-contiguous; x, y default to the column and row numbers; invalid points are zeroed like a triangulated mesh"""
    valid = np.ascontiguousarray(valid, np.uint8)
    h, w = valid.shape
    p3d = np.zeros((h, w, 3))
    uu, vv = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    p3d[..., 0] = uu if x is None else x
    p3d[..., 1] = vv if y is None else y
    if z is not None:
        p3d[..., 2] = z
    p3d[valid == 0] = 0
    return valid, np.ascontiguousarray(p3d)


# ---------------------------------------------------------------------------------------------------------------- z-gap percentile
def zgaps(valid, z, cols="interior", above="three"):
    """PovMesh.cpp:888-922: |z - z(neighbour k in the row above)|, k = -1, 0, +1, for the valid points of columns 1 .. w-2 and rows
    1 .. h-1 whose neighbour is valid.  Unsorted."""
    v = np.asarray(valid) != 0
    z = np.asarray(z, np.float64)
    h, w = v.shape
    j0, j1 = (0, w) if cols == "all" else (1, w - 1)
    out = [np.zeros(0)]
    if h >= 2 and j1 > j0:
        vp = np.pad(v, ((0, 0), (1, 1)))
        zp = np.pad(z, ((0, 0), (1, 1)))
        for k in ((-1, 0, 1) if above == "three" else (-1, 0)):
            c = v[1:, j0:j1] & vp[:-1, j0 + 1 + k:j1 + 1 + k]
            with np.errstate(invalid="ignore"):
                out.append(np.abs(z[1:, j0:j1] - zp[:-1, j0 + 1 + k:j1 + 1 + k])[c])
    return np.concatenate(out)


def rank_index(pct, n, rank="floor"):
    """PovMesh.cpp:924: floor(pct / 100.0 * n), clamped to n - 1 (the reference reads out of bounds at 100 %)"""
    x = pct / 100.0 * float(n)
    return min(int(np.floor(x) if rank == "floor" else np.ceil(x)), n - 1)


def zgap_percentile(valid, z, pct, rank="floor", cols="interior", above="three"):
    """(value, number of gaps); (nan, 0) without a gap"""
    g = np.sort(zgaps(valid, z, cols=cols, above=above))
    if g.size == 0:
        return float("nan"), 0
    return float(g[rank_index(pct, g.size, rank)]), int(g.size)


# ------------------------------------------------------------------------------------------------------------ connected components
def links(valid, z, zgap, link="lt"):
    """(hl, vl): hl[i, j] = (i, j) -- (i, j+1) linked, vl[i, j] = (i, j) -- (i+1, j) linked (PovMesh.cpp:147-188: both valid and
    fabs(dz) < zgap)"""
    v = np.asarray(valid) != 0
    z = np.asarray(z, np.float64)
    cmp = np.less if link == "lt" else np.less_equal
    with np.errstate(invalid="ignore"):
        hl = v[:, 1:] & v[:, :-1] & cmp(np.abs(z[:, 1:] - z[:, :-1]), zgap)
        vl = v[1:] & v[:-1] & cmp(np.abs(z[1:] - z[:-1]), zgap)
    return hl, vl


def components(valid, z, zgap, link="lt"):
    """4-connected components under the link rule, by an iterative union-find over numpy arrays (hook the larger root under the
    smaller, then pointer jumping, until no edge joins two trees).
    Returns (labels (h, w) int64: raster index of the component's smallest pixel, -1 where invalid;
             roots, sizes, seeds: per component its label, its size and its smallest column-major index u*h + v)."""
    v = np.asarray(valid) != 0
    h, w = v.shape
    n = h * w
    hl, vl = links(valid, z, zgap, link)
    idx = np.arange(n).reshape(h, w)
    a = np.concatenate([idx[:, :-1][hl], idx[:-1][vl]])
    b = np.concatenate([idx[:, 1:][hl], idx[1:][vl]])
    parent = np.arange(n)
    while True:
        ra, rb = parent[a], parent[b]
        live = ra != rb
        if not live.any():
            break
        lo, hi = np.minimum(ra[live], rb[live]), np.maximum(ra[live], rb[live])
        np.minimum.at(parent, hi, lo)
        while True:                                             # pointer jumping: every node at its root
            pp = parent[parent]
            if np.array_equal(pp, parent):
                break
            parent = pp
    labels = np.where(v, parent.reshape(h, w), -1)
    flat = labels.ravel()
    ok = flat >= 0
    roots, inv, sizes = np.unique(flat[ok], return_inverse=True, return_counts=True)
    cm = (np.arange(n) % w) * h + (np.arange(n) // w)
    seeds = np.full(roots.size, n, np.int64)
    np.minimum.at(seeds, inv, cm[ok])
    return labels, roots, sizes, seeds


def component_order(valid, z, zgap, link="lt", tie="colmajor"):
    """the components from the one keep_biggest takes first to the one it would take last: (labels, list of (root, size))"""
    labels, roots, sizes, seeds = components(valid, z, zgap, link)
    second = seeds if tie == "colmajor" else roots                   # a root IS the component's smallest raster index
    order = np.lexsort((second, -sizes))
    return labels, [(int(roots[k]), int(sizes[k])) for k in order]


def keep_biggest(valid, z, zgap, link="lt", tie="colmajor"):
    """PovMesh.cpp:929-987: seeds are taken in column-major order and a component replaces the best only if strictly larger, so
    among the largest the one with the smallest column-major index wins.  (mask uint8, size); nothing valid: (zeros, 0)."""
    labels, order = component_order(valid, z, zgap, link, tie)
    if not order:
        return np.zeros(labels.shape, np.uint8), 0
    return (labels == order[0][0]).astype(np.uint8), order[0][1]


# ----------------------------------------------------------------------------------------------------------------- planes
def plane_distance(p3d, plane):
    """PovMesh.cpp:717-742: fabs(((a x + b y) + c z) + d) in fp64, one operation at a time"""
    a, b, c, d = (float(t) for t in plane)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.abs(((a * p3d[..., 0] + b * p3d[..., 1]) + c * p3d[..., 2]) + d)


def _inside(valid, p3d, plane, thr, count):
    with np.errstate(invalid="ignore"):
        dist = plane_distance(p3d, plane)
        return (np.asarray(valid) != 0) & (dist < thr if count == "lt" else dist <= thr)


def plane_count(valid, p3d, plane, thr, count="lt"):
    return int(_inside(valid, p3d, plane, thr, count).sum())


def crop(valid, p3d, plane, thr, count="lt"):
    """PovMesh.cpp:780-815: a valid point stays if its distance is < thr (a NaN distance goes).  (mask uint8, kept)"""
    m = _inside(valid, p3d, plane, thr, count)
    return m.astype(np.uint8), int(m.sum())


def plane_of(p3d, uv6):
    """PovMesh.cpp:693-712: the candidate of one sample triple {u1, v1, u2, v2, u3, v3}, operation by operation"""
    u1, v1, u2, v2, u3, v3 = (int(t) for t in uv6)
    p1, p2, p3 = p3d[v1, u1], p3d[v2, u2], p3d[v3, u3]
    with np.errstate(invalid="ignore", divide="ignore"):
        a, b = p2 - p1, p3 - p1
        n = np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])
        n = n / np.sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2])
        if n[2] < 0:
            n = n * -1.0
        d = -(n[0] * p1[0] + n[1] * p1[1] + n[2] * p1[2])
    return np.array([n[0], n[1], n[2], d])


def refinement_inliers(valid, p3d, every=10, central_third_only=False, xmin=-9999., xmax=9999., ymin=-9999., ymax=9999.,
                       max_distance=70.0):
    """PovMesh.cpp:590-606 + wass_stereo.cpp:2077-2085: every `every`-th point, in raster order, of the (central-third) window that
    passes refine_plane's tests"""
    h, w = valid.shape
    u0, u1, v0, v1 = (w // 4, w * 3 // 4, h // 4, h * 2 // 3) if central_third_only else (0, w - 1, 0, h - 1)
    uu, vv = np.meshgrid(np.arange(w), np.arange(h))
    x, y, z = p3d[..., 0], p3d[..., 1], p3d[..., 2]
    ok = (valid != 0) & (uu >= u0) & (uu <= u1) & (vv >= v0) & (vv <= v1) & (x > xmin) & (x < xmax) & (y > ymin) & (y < ymax) & \
         (np.sqrt(x * x + y * y + z * z) < max_distance)
    return p3d[ok][::every], int(ok.sum())


# ================================================================================================================ scene builders
def holes(w, h, seed=0, frac=0.1, rough=0.3):
    """a rough surface with `frac` random holes: (valid, z)"""
    rng = np.random.default_rng(1000 * w + h + seed)
    z = np.cumsum(rng.normal(0, 0.05, (h, w)), axis=0) + rng.normal(0, rough, (h, w))
    valid = (rng.random((h, w)) >= frac).astype(np.uint8)
    return valid, z


# ---- gaps ----
def gap_pairs(w, h, values):
    """Isolated pairs: pixel (i, j) and its upper RIGHT neighbour (i-1, j+1), z = (g, 0), nothing else valid near them: exactly one
    gap of value g per pair, reached through neighbour k = +1 only (the probe of above="two").  Pairs sit at columns 1, 4, 7 ...
    <= w-2 of the row pairs (0, 1), (3, 4), (6, 7) ..."""
    cols = list(range(1, w - 1, 3))
    rows = list(range(1, h, 3))
    slots = [(i, j) for i in rows for j in cols]
    assert len(values) <= len(slots), (len(values), len(slots))
    valid = np.zeros((h, w), np.uint8)
    z = np.zeros((h, w))
    for (i, j), g in zip(slots, values):
        valid[i, j] = valid[i - 1, j + 1] = 1
        z[i, j] = g
    return valid, z


def gap_consecutive(w, h, n, base=1.0):
    """n gaps that are n consecutive doubles from `base` up (n a multiple of 3): rows 3r (z = -(j % 3) ulp) and 3r+1
    (z = base + 3 m ulp for the m-th used pixel), so the three gaps of pixel m are base + (3 m + {0, 1, 2}) ulp, exactly.
    Only the last radix digit (9 bits) and the one before it differ."""
    assert n % 3 == 0 and 1.0 <= base < 1.5
    u = 2.0 ** -52
    valid = np.zeros((h, w), np.uint8)
    z = np.zeros((h, w))
    m = 0
    for r in range(0, h - 1, 3):
        valid[r, :] = 1
        z[r, :] = -(np.arange(w) % 3) * u
        for j in range(1, w - 1):
            if m == n // 3:
                break
            # gaps of (r+1, j): z - z[r, j-1 .. j+1] = base + (3 m + ((j-1) % 3, j % 3, (j+1) % 3)) ulp
            valid[r + 1, j] = 1
            z[r + 1, j] = base + 3 * m * u
            m += 1
    assert m == n // 3, "picture too small"
    return valid, z


def gap_values(name):
    """the value probes of the percentile on 65 x 9"""
    if name == "one":
        return [0.75]
    if name == "two":
        return [0.75, 0.25]
    if name == "zeros":
        return [0.0] * 60
    if name == "equal":
        return [0.1] * 60
    if name == "pow2":                                   # first digits decide; denormals (k < -1022) included
        return [2.0 ** k for k in range(-1074, 1024, 36)]
    if name == "inf":
        return [float("inf")] + [0.5 + 0.01 * k for k in range(40)]
    raise KeyError(name)


GAP_PROBES = ("one", "two", "zeros", "equal", "pow2", "inf")

# (n gaps, pct): pct / 100.0 * n exactly an integer in fp64, or just below one -- classified by test_mesh_edges.py
RANK_CASES = [(100, 99.0), (1000, 98.7), (100, 57.0), (100, 29.0), (1000, 50.0), (100, 58.0), (1000, 70.1), (7, 100.0), (3, 0.0)]


def rank_scene(n):
    """n isolated gaps with the distinct values 1 .. n in a scrambled order: (w, h, valid, z)"""
    w, h = (129, 9) if n <= 120 else (257, 37)
    vals = (np.random.default_rng(n).permutation(n) + 1).astype(np.float64)
    return (w, h) + gap_pairs(w, h, list(vals))


# ---- components ----
def _pow2_below(w):
    return 2.0 ** -int(np.floor(np.log2(w)))


def snake(w, h, zgap=1.0, transpose=False):
    """A one-pixel-wide snake (z = 0) through the whole picture: the even rows, joined alternately at the right and left end by one
    pixel of the odd rows.  The rest of the odd rows is filled with z = zgap exactly: next to the snake everywhere, never linked
    to it.  Probe of link="le" (everything would merge).  transpose: the same with columns."""
    if transpose:
        v, z, size = snake(h, w, zgap)
        return np.ascontiguousarray(v.T), np.ascontiguousarray(z.T), size
    valid = np.ones((h, w), np.uint8)
    z = np.zeros((h, w))
    for i in range(1, h, 2):
        z[i, :] = zgap
        z[i, w - 1 if (i // 2) % 2 == 0 else 0] = 0.0
    return valid, z, ((h + 1) // 2) * w + h // 2


def spiral(w, h, zgap=1.0):
    """a rectangular spiral corridor (z = 0) from the corner inwards, turns two pixels apart, the walls between them z = zgap
    exactly (probe of link="le").  Returns (valid, z, size of the corridor)."""
    valid = np.ones((h, w), np.uint8)
    z = np.full((h, w), zgap)
    top, left, bottom, right = 0, 0, h - 1, w - 1
    i = j = 0
    z[0, 0] = 0.0
    while True:
        if j >= right or top > bottom:
            break
        z[i, j:right + 1] = 0.0; j = right; top += 2                 # right along row i
        if i >= bottom or left > right:
            break
        z[i:bottom + 1, j] = 0.0; i = bottom; right -= 2             # down along column j
        if j <= left or top > bottom:
            break
        z[i, left:j + 1] = 0.0; j = left; bottom -= 2                # left along row i
        if i <= top or left > right:
            break
        z[top:i + 1, j] = 0.0; i = top; left += 2                    # up along column j
    return valid, z, int((z == 0.0).sum())


def checkerboard(w, h):
    """valid where (row + column) is odd: every component is one pixel; the first valid pixel is (0, 1) in raster order and (1, 0)
    in column-major order (probe of tie="raster")"""
    vv, uu = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    return ((uu + vv) % 2 == 1).astype(np.uint8), np.zeros((h, w))


def stripes(w, h):
    """a horizontal stripe in row 0 and a vertical stripe in column 0, equal areas, apart: raster order names the horizontal one,
    column-major order the vertical one (probe of tie="raster").  Returns (valid, z, area)."""
    L = min(w - 2, h - 2)
    valid = np.zeros((h, w), np.uint8)
    valid[0, 2:2 + L] = 1
    valid[2:2 + L, 0] = 1
    return valid, np.zeros((h, w)), L


def twins(w, h, L=6):
    """Two 2 x L rectangles, each with pixels in two different 256-pixel blocks of the raster order; the later one in raster order
    sits at column 0, the earlier one further right (probe of tie="raster").  Returns (valid, z, size, top row of either)."""
    def crosses(r, c):
        return (r * w + c) // 256 != ((r + 1) * w + c + L - 1) // 256
    ca = L + 2
    pairs = [(ra, rb) for ra in range(h - 1) for rb in range(ra + 1, h - 1) if crosses(ra, ca) and crosses(rb, 0)]
    assert pairs, (w, h)
    ra, rb = pairs[0]
    valid = np.zeros((h, w), np.uint8)
    valid[ra:ra + 2, ca:ca + L] = 1
    valid[rb:rb + 2, 0:L] = 1
    return valid, np.zeros((h, w)), 2 * L, (ra, rb)


def islands_on_block_starts(w, h, zgap=1.0, block=8192):
    """A solid picture (z = 0) in which the first pixel of every `block` pixels of the raster order is an island of its own
    (z = zgap exactly): the root of a counting block's first pixel is never the big component.  Probe of link="le".
    Returns (valid, z, size of the big component)."""
    valid = np.ones((h, w), np.uint8)
    z = np.zeros(h * w)
    z[::block] = zgap
    return valid, z.reshape(h, w), h * w - len(range(0, h * w, block))


def ramp(w, h):
    """A solid picture whose rows are components of their own although the raster neighbours across a row end are as close as the
    neighbours inside a row: z = (i w + j) s, s = 2^-floor(log2 w), zgap = s w exactly -- horizontal steps s < zgap, vertical steps
    = zgap (not linked; probe of link="le"), the step across a row end s.  A labelling that lets a run continue over a row end
    (runs wrap inside a wave when w < 64) merges everything.  Returns (valid, z, zgap)."""
    s = _pow2_below(w)
    z = (np.arange(h * w, dtype=np.float64) * s).reshape(h, w)
    return np.ones((h, w), np.uint8), z, s * w


COMPONENT_SHAPES = [(65, 9), (256, 4), (128, 64), (129, 64), (300, 41)]


# ---- the 16 link patterns of a 2 x 2 cell ----
def cell_heights(pattern, zgap=1.0):
    """Heights (TL, TR, BL, BR) of a 2 x 2 cell whose four links -- bit 0 top (TL-TR), bit 1 bottom (BL-BR), bit 2 left (TL-BL),
    bit 3 right (TR-BR) -- are present exactly as the bits of `pattern` say.  Found by search over multiples of zgap / 2; among
    the solutions the one with most absent links at |dz| == zgap exactly is taken (probe of link="le")."""
    best = None
    steps = [0.0, 0.5, 1.0, 1.5, 2.0, 2.5, 3.0]
    for tr, bl, br in itertools.product(steps, repeat=3):
        zs = (0.0, tr * zgap, bl * zgap, br * zgap)
        d = (abs(zs[0] - zs[1]), abs(zs[2] - zs[3]), abs(zs[0] - zs[2]), abs(zs[1] - zs[3]))
        if all((d[k] < zgap) == bool(pattern >> k & 1) for k in range(4)):
            score = sum(1 for k in range(4) if not (pattern >> k & 1) and d[k] == zgap)
            if best is None or score > best[0]:
                best = (score, zs)
    assert best is not None, pattern
    return best[1]


def cell_components(pattern):
    """by hand: a 4-cycle with L links has 4 - L components while it is a forest (L <= 3), one when closed"""
    L = bin(pattern).count("1")
    return max(1, 4 - L)


def link_cells_at(col, zgap=1.0, w=512):
    """the 16 patterns one under the other with the cell's left column at `col`: (valid, z, number of components = 33)"""
    h = 48
    valid = np.zeros((h, w), np.uint8)
    z = np.zeros((h, w))
    for p in range(16):
        tl, tr, bl, br = cell_heights(p, zgap)
        r = 3 * p
        valid[r:r + 2, col:col + 2] = 1
        z[r, col], z[r, col + 1], z[r + 1, col], z[r + 1, col + 1] = tl, tr, bl, br
    return valid, z, sum(cell_components(p) for p in range(16))


LINK_CELL_COLUMNS = (255, 256, 100)      # straddling a 256-pixel block boundary, at a block start, mid-block


# ---- link thresholds ----
def comb(w, h, zgap):
    """A spine (row 0 and column 0, z = 0) with teeth: below the spine at even columns >= 2 and right of it at even rows >= 2, one
    pixel each, with z cycling through pred(zgap), zgap, succ(zgap).  A tooth belongs to the spine's component iff its z < zgap:
    the size is spine + number of pred teeth.  Probe of link="le" (the teeth at zgap would join).
    Returns (valid, z, dict(spine=, pred=, at=, succ=))."""
    valid = np.zeros((h, w), np.uint8)
    z = np.zeros((h, w))
    valid[0, :] = 1
    valid[:, 0] = 1
    vals = (pred(zgap), zgap, succ(zgap))
    cnt = [0, 0, 0]
    k = 0
    teeth = [(1, j) for j in range(2, w, 2)] + ([(i, 1) for i in range(2, h, 2)] if w > 1 else [])
    for i, j in teeth:
        if i >= h or j >= w:
            continue
        valid[i, j] = 1
        z[i, j] = vals[k % 3]
        cnt[k % 3] += 1
        k += 1
    return valid, z, dict(spine=w + h - 1, pred=cnt[0], at=cnt[1], succ=cnt[2])


# ---- plane thresholds ----
LATTICE_SHAPES = [(63, 7), (64, 8), (65, 9), (257, 5), (2, 2)]


def lattice_samples(w, h):
    """three pixels that are not collinear: (0, 0), (w-1, 0), (0, h-1) -> uv (1, 6)"""
    return np.array([[0, 0, w - 1, 0, 0, h - 1]], np.int32)


def lattice(w, h, thr, kind="mixed"):
    """Integer X = column, Y = row; the three sample pixels at z = 0, so their plane is (0, 0, 1, 0) and a point's distance is |z|
    exactly.  kind:
      mixed    the other points cycle through thr, pred(thr), succ(thr), -thr, -pred(thr), 0 (equal in fp32 next to thr: they must
               go through the fp64 recount; probe of count="le")
      pred     every other point at pred(thr): a bound must not decide "all outside"
      at       every other point at thr: a bound must not decide "all inside" (probe of count="le")
      patches  whole 64 x 8 patches alternately at thr / 4 (strictly inside) and 4 thr (strictly outside): both shortcuts taken
    Returns (valid, p3d, counts dict by value class, inside = the number the plane must count)."""
    vals = {"mixed": (thr, pred(thr), succ(thr), -thr, -pred(thr), 0.0), "pred": (pred(thr),), "at": (thr,)}
    z = np.zeros((h, w))
    idx = np.arange(h * w).reshape(h, w)
    if kind == "patches":
        vv, uu = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
        z = np.where(((uu // 64) + (vv // 8)) % 2 == 0, thr / 4, 4 * thr)
    else:
        z = np.array(vals[kind])[idx % len(vals[kind])]
    for u, v in lattice_samples(w, h).reshape(3, 2):
        z[v, u] = 0.0
    valid, p3d = as_mesh(np.ones((h, w), np.uint8), z)
    az = np.abs(z)
    counts = dict(at=int((az == thr).sum()), pred=int((az == pred(thr)).sum()), succ=int((az == succ(thr)).sum()),
                  inside=int((az < pred(thr)).sum()), outside=int((az > succ(thr)).sum()))
    return valid, p3d, counts, int((az < thr).sum())


def lattice_far(w, h, thr, shift=1e6):
    """The lattice moved by `shift` in X and Y under a tilted plane z = 0.001 (X - shift) + 0.002 (Y - shift), the other points
    at distance thr (1 + k 1e-10), k = -3 .. 3, on both sides (the rounding of the fp64 sum, about 1e-10, decides near k = 0): |coordinate| 2^-21 exceeds thr / 2, so the fp32 pass can decide
    nothing near the band edge and every patch recounts.  Returns (valid, p3d)."""
    vv, uu = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    zp = 0.001 * uu + 0.002 * vv
    k = (np.arange(h * w).reshape(h, w) % 7) - 3
    sign = np.where((np.arange(h * w).reshape(h, w) // 7) % 2 == 0, 1.0, -1.0)
    cz = 1.0 / np.sqrt(1.0 + 0.001 ** 2 + 0.002 ** 2)               # the plane's c: a height offset t is a distance t c
    z = zp + sign * thr * (1.0 + k * 1e-10) / cz
    for u, v in lattice_samples(w, h).reshape(3, 2):
        z[v, u] = zp[v, u]
    return as_mesh(np.ones((h, w), np.uint8), z, x=uu + shift, y=vv + shift)


def lattice_nan(w, h, thr, axis):
    """a flat lattice strictly inside the band (z = thr / 4, samples at 0) with ONE valid point whose coordinate `axis` is NaN, in the
    middle of the picture: fabs(NaN) < thr is false, the reference never counts it.  Returns (valid, p3d, inside)."""
    z = np.full((h, w), thr / 4)
    for u, v in lattice_samples(w, h).reshape(3, 2):
        z[v, u] = 0.0
    valid, p3d = as_mesh(np.ones((h, w), np.uint8), z)
    p3d[h // 2, w // 2, axis] = np.nan
    return valid, p3d, h * w - 1


# ---- block counts, scan, pack ----
BLOCK_COUNTS = (1, 2, 64, 65, 128, 129, 192, 193, 256, 257, 1025)
BLOCK_WIDTH = 37                                               # does not divide 256
PATTERNS = ("all", "none", "last", "block_first", "block_last", "alternate", "random")


def block_shape(nb, w=BLOCK_WIDTH):
    """(w, h) with ceil(w h / 256) == nb"""
    h = (256 * nb) // w
    assert (w * h + 255) // 256 == nb
    return w, h


def pattern_valid(w, h, pattern, seed=0):
    n = w * h
    v = np.zeros(n, np.uint8)
    if pattern == "all":
        v[:] = 1
    elif pattern == "last":
        v[-1] = 1
    elif pattern == "block_first":
        v[::256] = 1
    elif pattern == "block_last":
        v[255::256] = 1
        v[-1] = 1
    elif pattern == "alternate":
        v[::2] = 1
    elif pattern == "random":
        v[:] = np.random.default_rng(n + seed).random(n) < 0.5
    elif pattern != "none":
        raise KeyError(pattern)
    return v.reshape(h, w)


def sea(w, h, seed=0, noise=0.05, flat_x=None):
    """a tilted noisy plane in front of the camera (the `_cloud()` of test_post_mesh_gpu.py at any size): (p3d, plane).
    flat_x: every point gets this x (a zero extent on that axis for the xyzC encoder; the plane then has a = 0)."""
    rng = np.random.default_rng(7 * w + h + seed)
    n = np.array([0.0 if flat_x is not None else 0.04, -0.45, 0.89])
    n /= np.linalg.norm(n)
    d = -18.0
    u, v = np.meshgrid(np.arange(w), np.arange(h))
    x = (u - w / 2) * 0.12 + rng.normal(0, 0.01, (h, w))
    y = (v - h / 2) * 0.1 + rng.normal(0, 0.01, (h, w))
    if flat_x is not None:
        x = np.full((h, w), float(flat_x))
    z = (-d - n[0] * x - n[1] * y) / n[2] + rng.normal(0, noise, (h, w))
    return np.ascontiguousarray(np.stack([x, y, z], -1)), np.array([*n, d])


# ---- the plane stages on a shared device record ----
RECORD_SHAPES = [(1, 1), (65, 9), (257, 5)]
EXACT_REFINE = dict(max_distance=1e4, weight_by_distance=False)       # every valid point of exact_sea is a refinement inlier, weight 1


def exact_sea(w, h, seed=0):
    """A rough tilted plane whose refinement gives the same bits in ANY summation order: x = column, y = row,
    z = 20 + (u + 2 v + k) / 8 with k in -4 .. 4, and the number of valid points the largest power of two <= w h.  With
    EXACT_REFINE the sums of pass 0 are integers / 8, the centroid is such a sum over a power of two, and the scatter sums are
    integers over (8 n)^2 that stay below 2^53 (tests/test_mesh_edges.py computes them in integers): no partial sum is ever
    rounded, so a tree of block sums and the reference's raster loop agree exactly.  Returns (valid, p3d)."""
    rng = np.random.default_rng(31 * w + h + seed)
    n = 1 << int(np.floor(np.log2(w * h)))
    valid = np.zeros(w * h, np.uint8)
    valid[rng.permutation(w * h)[:n]] = 1
    vv, uu = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    z = 20.0 + (uu + 2 * vv + rng.integers(-4, 5, (h, w))) / 8.0
    valid = valid.reshape(h, w)
    p3d = np.stack([uu.astype(np.float64), vv.astype(np.float64), z], -1)
    p3d[valid == 0] = 0
    return valid, np.ascontiguousarray(p3d)


def sparse_sea(w, h):
    """exact_sea(seed=1) with every 20th of its points valid, at most w h // 20: no plane can reach the w h / 10 inliers that ransac_find_plane asks
    for (PovMesh.cpp:773), so RANSAC reports "not found" -- except at 1 x 1, where the limit is 0 and nothing is valid."""
    valid, p3d = exact_sea(w, h, seed=1)
    keep = np.flatnonzero(valid.ravel())[::20][:(w * h) // 20]
    valid = np.zeros(w * h, np.uint8)
    valid[keep] = 1
    valid = valid.reshape(h, w)
    p3d[valid == 0] = 0
    return valid, p3d


def record_samples(w, h, rounds=64):
    """sample triples of three different pixels, uv (rounds, 6); the one pixel three times at 1 x 1"""
    if w * h < 3:
        return np.zeros((1, 6), np.int32)
    rng = np.random.default_rng(w + 1000 * h)
    px = np.array([rng.choice(w * h, 3, replace=False) for _ in range(rounds)])
    return np.ascontiguousarray(np.stack([px % w, px // w], -1).reshape(rounds, 6).astype(np.int32))
