"""numpy restatement of the LinearND interpolator (wass_amd/csrc/grid_linear.hip, DESIGN.md "LinearND") in two independent forms.

The definition (certify): given a proposed triangle for a node, the certificate and the canonical value with the kernel's
expressions in the kernel's order of operations -- numpy's elementwise fp64 products and sums are not contracted, like the library's.
It looks at EVERY point of the cloud, so it knows nothing of cells, rings or circle boxes.

A brute-force walk (walk): nearest point, its nearest point, apex, across the separating edge, every step over all points at
once, so its visiting order has nothing in common with the kernel's buckets.  The hull is found by gift wrapping, not by the
monotone chain.  interpolate() puts the two together: flags, values and the triangle per node."""
import numpy as np

EPS = 2.0 ** -53
EO = 5.0 * EPS          # |orient - exact| <= EO * S
EI = 12.0 * EPS         # |incircle - exact| <= EI * P
DEFAULT_STEPS = 256


def orient(ax, ay, bx, by, cx, cy):
    """(A - C) x (B - C), origin the last argument; returns (det, S)."""
    acx, acy, bcx, bcy = ax - cx, ay - cy, bx - cx, by - cy
    t1, t2 = acx * bcy, acy * bcx
    return t1 - t2, np.abs(t1) + np.abs(t2)


def incircle(ax, ay, bx, by, cx, cy, dx, dy):
    """> 0: D inside the circle through the counter-clockwise A, B, C; origin D; returns (det, permanent)."""
    adx, ady, bdx, bdy, cdx, cdy = ax - dx, ay - dy, bx - dx, by - dy, cx - dx, cy - dy
    bdxcdy, cdxbdy, alift = bdx * cdy, cdx * bdy, adx * adx + ady * ady
    cdxady, adxcdy, blift = cdx * ady, adx * cdy, bdx * bdx + bdy * bdy
    adxbdy, bdxady, clift = adx * bdy, bdx * ady, cdx * cdx + cdy * cdy
    perm = ((np.abs(bdxcdy) + np.abs(cdxbdy)) * alift + (np.abs(cdxady) + np.abs(adxcdy)) * blift) + (np.abs(adxbdy) + np.abs(bdxady)) * clift
    det = (alift * (bdxcdy - cdxbdy) + blift * (cdxady - adxcdy)) + clift * (adxbdy - bdxady)
    return det, perm


def nodes(xmin, xmax, ymin, ymax, W, H):
    return np.linspace(xmin, xmax, W), np.linspace(ymin, ymax, H)


def taken(x, y, xmin, xmax, ymin, ymax, mistake=None):
    """Indices (ascending) of the points that exist: inside the closed area, finite, the lowest index of equal (x, y).
    mistake (the probes of tests/test_linearnd.py only): "open" takes the area open, "last" lets the highest index stand."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    with np.errstate(invalid="ignore"):
        if mistake == "open":
            idx = np.flatnonzero((x > xmin) & (x < xmax) & (y > ymin) & (y < ymax))
        else:
            idx = np.flatnonzero((x >= xmin) & (x <= xmax) & (y >= ymin) & (y <= ymax))
    if idx.size == 0:
        return idx
    order = np.lexsort((-idx if mistake == "last" else idx, y[idx], x[idx]))
    s = idx[order]
    first = np.ones(s.size, bool)
    first[1:] = (x[s][1:] != x[s][:-1]) | (y[s][1:] != y[s][:-1])
    return np.sort(s[first])


def hull(X, Y):
    """Gift wrapping over the existing points: positions into X, Y of the hull's vertices, counter-clockwise, strict turns only;
    empty when fewer than three remain (all collinear)."""
    n = X.size
    if n < 3:
        return np.zeros(0, np.int64)
    start = int(np.lexsort((Y, X))[0])
    out, cur = [start], start
    for _ in range(n + 1):
        cand = (cur + 1) % n
        # the next vertex: no point right of cur -> next; of collinear ones the farthest
        for _ in range(n):
            o, _S = orient(X[cur], Y[cur], X[cand], Y[cand], X, Y)
            right = np.flatnonzero(o < 0)
            if right.size == 0:
                break
            cand = int(right[np.argmin(o[right])])
        o, _S = orient(X[cur], Y[cur], X[cand], Y[cand], X, Y)
        col = np.flatnonzero(o == 0)
        d = (X[col] - X[cur]) ** 2 + (Y[col] - Y[cur]) ** 2
        cand = int(col[np.argmax(d)])
        if cand == start or cand == cur:
            break
        out.append(cand)
        cur = cand
    return np.array(out, np.int64) if len(out) >= 3 else np.zeros(0, np.int64)


def outside_hull(X, Y, hv, qx, qy):
    """certainly beyond a hull edge: flag 1"""
    a, b = hv, np.roll(hv, -1)
    o, S = orient(X[a], Y[a], X[b], Y[b], qx, qy)
    return bool((o < -(EO * S)).any())


def certify(X, Y, Z, tri, qx, qy, mistake=None):
    """The definition.  tri: three positions into X, Y, Z (which are in ascending order of the original index).  Returns
    (flag 0 or 2, value).  mistake (probes only): "unsorted" takes the vertices in the order given, "left" looks only at the points
    left of the edge tri[0] -> tri[1]."""
    i, j, k = (int(t) for t in tri) if mistake == "unsorted" else sorted(int(t) for t in tri)
    o3, S3 = orient(X[i], Y[i], X[j], Y[j], X[k], Y[k])
    ok = abs(o3) > EO * S3
    sg = 1.0 if o3 > 0 else -1.0
    oi, Si = orient(X[j], Y[j], X[k], Y[k], qx, qy)
    oj, Sj = orient(X[k], Y[k], X[i], Y[i], qx, qy)
    ok3, Sk = orient(X[i], Y[i], X[j], Y[j], qx, qy)
    ok = ok and sg * oi >= EO * Si and sg * oj >= EO * Sj and sg * ok3 >= EO * Sk
    with np.errstate(all="ignore"):
        val = np.float64((oi * Z[i] + oj * Z[j]) + ok3 * Z[k]) / np.float64((oi + oj) + ok3)
    if not np.isfinite(val):
        return 2, np.nan
    if not ok:
        return 2, float(val)
    ic, P = incircle(X[i], Y[i], X[j], Y[j], X[k], Y[k], X, Y)
    out = sg * ic < -(EI * P)
    out[[i, j, k]] = True
    if mistake == "left":
        a, b = int(tri[0]), int(tri[1])
        out |= ~(orient(X[a], Y[a], X[b], Y[b], X, Y)[0] > 0)
    return (0 if out.all() else 2), float(val)


def _nearest(X, Y, px, py, skip=-1):
    dx, dy = X - px, Y - py
    d = dx * dx + dy * dy
    if skip >= 0:
        d = d.copy()
        d[skip] = np.inf
    return int(np.argmin(d))                       # the first of equal distances: the lowest index


def _apex(X, Y, a, b):
    o, _S = orient(X[a], Y[a], X[b], Y[b], X, Y)
    o[[a, b]] = -1.0
    left = np.flatnonzero(o > 0)
    if left.size == 0:
        return -1
    best = int(left[0])
    lx, ly = X[left], Y[left]
    for _ in range(left.size + 1):
        ic, _P = incircle(X[a], Y[a], X[b], Y[b], X[best], Y[best], lx, ly)
        inside = np.flatnonzero(ic > 0)
        if inside.size:
            best = int(left[inside[np.argmax(ic[inside])]])
            continue
        tie = left[ic == 0]
        if tie.size and int(tie[0]) < best:
            best = int(tie[0])
            continue
        return best
    return best


def walk(X, Y, qx, qy, max_steps=DEFAULT_STEPS):
    """Steps 2-4 over all points.  Returns (status, tri, steps): status 0 with a triangle that holds q by the plain signs, 2 when
    an apex search found nothing, 3 at the step cap."""
    a = _nearest(X, Y, qx, qy)
    b = _nearest(X, Y, X[a], Y[a], skip=a)
    o, _S = orient(X[a], Y[a], X[b], Y[b], qx, qy)
    if o < 0:
        a, b = b, a
    for step in range(max_steps):
        c = _apex(X, Y, a, b)
        if c < 0:
            if step == 0 and o == 0:
                a, b, o = b, a, 1.0
                continue
            return 2, None, step
        obc, _S = orient(X[b], Y[b], X[c], Y[c], qx, qy)
        oca, _S = orient(X[c], Y[c], X[a], Y[a], qx, qy)
        if obc >= 0 and oca >= 0:
            return 0, (a, b, c), step + 1
        if obc < 0:
            a = c
        else:
            b = c
        o = 1.0
    return 3, None, max_steps


def interpolate(x, y, z, xmin, xmax, ymin, ymax, W, H, max_steps=DEFAULT_STEPS, mistake=None):
    """out (H x W float64), flags (H x W uint8), tri (H x W x 3 original indices, -1 without a triangle), info dict."""
    x, y, z = (np.asarray(v, np.float64) for v in (x, y, z))
    keep = taken(x, y, xmin, xmax, ymin, ymax, mistake)
    X, Y, Z = x[keep], y[keep], z[keep]
    out = np.full((H, W), np.nan)
    flags = np.ones((H, W), np.uint8)
    tri = np.full((H, W, 3), -1, np.int64)
    info = {"n_taken": int(keep.size), "too_few": False, "max_steps": 0}
    hv = hull(X, Y)
    if hv.size < 3:
        info["too_few"] = True
        return out, flags, tri, info
    qxs, qys = nodes(xmin, xmax, ymin, ymax, W, H)
    for r in range(H):
        for c in range(W):
            qx, qy = qxs[c], qys[r]
            if outside_hull(X, Y, hv, qx, qy):
                continue
            status, t, steps = walk(X, Y, qx, qy, max_steps)
            info["max_steps"] = max(info["max_steps"], steps)
            if status != 0:
                flags[r, c] = status
                continue
            flags[r, c], out[r, c] = certify(X, Y, Z, t, qx, qy, mistake)
            tri[r, c] = np.sort(keep[list(t)])
    return out, flags, tri, info


# ---- the scenes of the tests: 5 points per cell of a 32 x 32 lattice over the unit square
def scene(kind, seed=1, n=5 * 32 * 32):
    rng = np.random.default_rng(seed)
    if kind == "uniform":
        p = rng.random((n, 2))
    elif kind == "hole":
        p = rng.random((2 * n, 2))
        p = p[(p[:, 0] - 0.5) ** 2 + (p[:, 1] - 0.5) ** 2 > 0.3 ** 2][:n]
    elif kind == "clump":
        p = np.concatenate([rng.normal((0.3, 0.6), 0.03, (n - 40, 2)), rng.random((40, 2))])
    else:
        raise ValueError(kind)
    z = np.sin(3.0 * p[:, 0]) + np.cos(2.0 * p[:, 1]) + 0.1 * rng.normal(size=p.shape[0])
    return p[:, 0].copy(), p[:, 1].copy(), z


SCENES = ("uniform", "hole", "clump")
UNIT = (0.0, 1.0, 0.0, 1.0)


def value_bound(x, y, z, tri):
    """What two correct evaluations of the plane through the triangles tri (.. x 3 indices) may differ by at any point inside:
    each computes three weights that sum to 1 from differences and products of the coordinates; a weight's error is a few roundings
    of products as large as S = the sum over the edges of |dx| |dy|, over twice the area.  16 eps (S / 2 area) max |z| covers the
    four roundings of each weight on either side, with a factor 2 to spare."""
    X, Y, Zv = x[tri], y[tri], np.abs(z[tri]).max(axis=-1)
    area2 = np.abs((X[..., 0] - X[..., 2]) * (Y[..., 1] - Y[..., 2]) - (Y[..., 0] - Y[..., 2]) * (X[..., 1] - X[..., 2]))
    S = sum(np.abs(X[..., a] - X[..., b]) * np.abs(Y[..., a] - Y[..., b]) for a, b in ((0, 1), (1, 2), (2, 0)))
    span = np.maximum(np.ptp(X, axis=-1), np.ptp(Y, axis=-1)) ** 2
    return 16.0 * EPS * (np.maximum(S, span) / area2) * Zv + 4.0 * EPS * Zv


# ---- exact scenes
def square_lattice(m=6):
    """m x m points on the integer lattice 0 .. m - 1 with z = 2x - 3y + 1: every triangulation gives that plane"""
    gx, gy = np.meshgrid(np.arange(m, dtype=np.float64), np.arange(m, dtype=np.float64))
    x, y = gx.ravel(), gy.ravel()
    return x, y, 2.0 * x - 3.0 * y + 1.0
