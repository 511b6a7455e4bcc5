"""numpy restatement of the reference's game-theoretic matcher (src/wass_match/GTMatcher.cpp, iidyn.cpp, wass_match.cpp), for the
tests of wass_amd.match.  Test infrastructure only: nothing in wass_amd imports it.

The dynamics takes the order of its sums as a parameter ("sequential" is the reference's, "pairwise" numpy's, "reversed" the
reference's from the far end, "tree" the kernel's own fixed tree, which predicts the GPU's bits on the CPU) and the mistakes the
probe scenes are there to catch as switches, all off by default.
"""
import numpy as np

EPS = np.finfo(np.float64).eps
MAX_ITERS = 50000
TOLL = 1e-20


def bound(n):
    """8 N eps: the rounding of an N-term fp64 dot product, times 8"""
    return 8.0 * n * EPS


# ------------------------------------------------------------------------------------------------------------------------ sums
def _sum(v, how):
    if v.size == 0:
        return np.float64(0.0)
    if how == "sequential":
        return np.cumsum(v)[-1]
    if how == "reversed":
        return np.cumsum(v[::-1])[-1]
    if how == "pairwise":
        return np.sum(v)
    if how == "tree":
        return _tree_sum(v)
    raise ValueError(how)


def _fold64(w):
    """the butterfly over a wave: lanes l and l ^ 32, then ^ 16 ... (axis -1 has 64 entries); wave_all of wass_amd/csrc/reduce.h"""
    m = 32
    while m >= 1:
        w = w[..., :m] + w[..., m:2 * m]
        m >>= 1
    return w[..., 0]


def _tree_sum(v):
    """the kernel's tree: 1024 threads, thread t sums elements t, t + 1024, ... in order, a butterfly over each wave of 64, the
    sixteen waves in order; a problem of at most 64 elements is summed in order, like the reference (orders: wass_amd/csrc/reduce.h)"""
    if v.size <= 64:
        return np.cumsum(v)[-1]
    pad = np.zeros(8192)
    pad[:v.size] = v
    per_thread = np.cumsum(pad.reshape(8, 1024), axis=0)[-1]
    return np.cumsum(_fold64(per_thread.reshape(16, 64)))[-1]


def matvec(A, x, how):
    n = A.shape[0]
    y = np.empty(n)
    step = max(1, (1 << 22) // max(n, 1))
    for r0 in range(0, n, step):
        P = A[r0:r0 + step] * x[None, :]
        if how == "sequential":
            y[r0:r0 + step] = np.cumsum(P, axis=1)[:, -1]
        elif how == "reversed":
            y[r0:r0 + step] = np.cumsum(P[:, ::-1], axis=1)[:, -1]
        elif how == "tree" and n <= 64:
            y[r0:r0 + step] = np.cumsum(P, axis=1)[:, -1]
        elif how == "tree":                                  # one wave per row: lane l sums columns l, l + 64, ... in order
            Q = np.zeros((P.shape[0], -(-n // 64) * 64))
            Q[:, :n] = P
            y[r0:r0 + step] = _fold64(np.cumsum(Q.reshape(P.shape[0], -1, 64), axis=1)[:, -1, :])
        else:
            y[r0:r0 + step] = P.sum(axis=1)
    return y


# -------------------------------------------------------------------------------------------------------------------- dynamics
def create_population(n):
    """gt_create_population: rand() / RAND_MAX is an integer division, so every entry is 1.0 before the division by the sum"""
    x = np.ones(n)
    return x / np.float64(n)


def simplexify(x, how):
    x = np.where(x >= 0, x, 0.0)
    return x / _sum(x, how)


def iidyn(A, x0=None, toll=TOLL, max_iters=MAX_ITERS, summation="sequential", ties="first", min_over="positive", do_simplexify=True):
    """gt_iidyn.  Returns (population, steps, last error)."""
    A = np.ascontiguousarray(A, np.float64)
    n = A.shape[0]
    x = create_population(n) if x0 is None else np.array(x0, np.float64)
    with np.errstate(all="ignore"):
        x = simplexify(x, summation)
        Ax = matvec(A, x, summation)
        toll2 = toll * toll
        niter, err = 0, np.finfo(np.float64).max
        while niter < max_iters:
            if ties == "first":
                max_idx = int(np.argmax(Ax))
            else:
                max_idx = n - 1 - int(np.argmax(Ax[::-1]))
            if not Ax[max_idx] > -np.inf:
                max_idx = -1
            masked = Ax if min_over == "all" else np.where(x > 0, Ax, np.inf)
            if ties == "first":
                min_idx = int(np.argmin(masked))
            else:
                min_idx = n - 1 - int(np.argmin(masked[::-1]))
            minv = masked[min_idx]
            if not minv < np.inf:
                min_idx = -1
            xAx = _sum(Ax * x, summation)
            maxv = (Ax[max_idx] if max_idx >= 0 else -np.inf) - xAx
            minv = xAx - minv
            idx, delta = max_idx, maxv
            if maxv < minv:
                idx, delta = min_idx, -minv
            tmp = xAx - Ax
            tmp = np.where(tmp > x, x, tmp)
            err = _sum(tmp * tmp, summation)
            if err < toll2 or idx < 0:
                break
            den = A[idx, idx] - Ax[idx] - delta
            do_remove = False
            if delta >= 0:
                mu = np.float64(1.0)
                if den < 0:
                    t = -delta / den
                    if mu > t:
                        mu = t
                    if mu < 0:
                        mu = np.float64(0.0)
            else:
                mu = x[idx] / (x[idx] - 1)
                do_remove = True
                if den < 0:
                    t = -delta / den
                    if mu < t:
                        mu = t
                        do_remove = False
                    if mu > 0:
                        mu = np.float64(0.0)
            x = x * (1 - mu)
            x[idx] = 0.0 if do_remove else x[idx] + mu
            if do_simplexify:
                x = simplexify(x, summation)
            Ax = mu * (A[idx] - Ax) + Ax
            niter += 1
    return x, niter, float(err)


def group(x, pop_threshold=0.7):
    """the winners of match_group, in candidate order"""
    return np.flatnonzero(x > np.max(x) * pop_threshold)


def threshold_margin(x, pop_threshold=0.7):
    """the smallest relative distance of a population value from the group threshold"""
    thr = np.max(x) * pop_threshold
    return np.inf if thr == 0 else float(np.min(np.abs(x - thr)) / thr)


# ---------------------------------------------------------------------------------------------------------------------- payoff
def ang_diff(first, second, dtype):
    d = dtype(second) - dtype(first)
    pi = dtype(np.pi)
    while d < -pi:
        d += dtype(2.0) * pi
    while d > pi:
        d -= dtype(2.0) * pi
    return d


def payoff_entries(fa, fb, cand, I, J, lam, dtype=np.float64, geo="max"):
    """entries (I, J) of compute_payoff_matrix (index arrays that broadcast against each other).  fa, fb: n x 4 float32 (x y scale
    angle); cand: N x 2.  With dtype=np.longdouble the same expression in extended precision (the float32 inputs and pi widened
    exactly), which is what the oracle's own rounding is measured against.  Returns (payoff, geometric error, excluded)."""
    fa, fb, cand = np.asarray(fa, np.float32), np.asarray(fb, np.float32), np.asarray(cand).reshape(-1, 2)
    n = cand.shape[0]
    S, T = fa[cand[:, 0]].astype(dtype), fb[cand[:, 1]].astype(dtype)
    rot = np.array([ang_diff(T[i, 3], S[i, 3], dtype) for i in range(n)], dtype)
    ca, sn = np.cos(rot), np.sin(rot)
    ds = T[:, 2] / S[:, 2]
    scx, scy = S[:, 0] * ds, S[:, 1] * ds
    dx = T[:, 0] - (scx * ca - scy * sn)
    dy = T[:, 1] - (scx * sn + scy * ca)
    # a1 = candidate I, a2 = candidate J
    c1, s1, x1, y1, k1 = ca[I], sn[I], dx[I], dy[I], ds[I]
    c2, s2, x2, y2, k2 = ca[J], sn[J], dx[J], dy[J], ds[J]
    s1x, s1y, t1x, t1y = S[I, 0], S[I, 1], T[I, 0], T[I, 1]
    s2x, s2y, t2x, t2y = S[J, 0], S[J, 1], T[J, 0], T[J, 1]
    eX = t2x - (k1 * (s2x * c1 - s2y * s1) + x1)
    eY = t2y - (k1 * (s2x * s1 + s2y * c1) + y1)
    eX2 = t1x - (k2 * (c2 * s1x - s2 * s1y) + x2)
    eY2 = t1y - (k2 * (s2 * s1x + c2 * s1y) + y2)
    e1, e2 = eX * eX + eY * eY, eX2 * eX2 + eY2 * eY2
    ge = np.where(e1 < e2, e2, e1) if geo == "max" else np.where(e1 < e2, e1, e2)
    P = np.exp(-dtype(lam) * ge)
    excl = (cand[I, 0] == cand[J, 0]) | (cand[I, 1] == cand[J, 1])
    P = np.where(excl, dtype(0), P)
    return P, ge, excl


def payoff(fa, fb, cand, lam, dtype=np.float64, geo="max"):
    """the whole N x N matrix, in slabs of rows"""
    n = np.asarray(cand).reshape(-1, 2).shape[0]
    P, G, E = np.empty((n, n), dtype), np.empty((n, n), dtype), np.empty((n, n), bool)
    J = np.arange(n)[None, :]
    step = max(1, (1 << 21) // n)
    for r0 in range(0, n, step):
        I = np.arange(r0, min(n, r0 + step))[:, None]
        P[r0:r0 + step], G[r0:r0 + step], E[r0:r0 + step] = payoff_entries(fa, fb, cand, I, J, lam, dtype, geo)
    return P, G, E


# ------------------------------------------------------------------------------------------------------------------ candidates
def knn(desc_a, desc_b, k):
    """exact k nearest in fp64; ties to the lower index.  Returns (idx, fp64 squared distances, the gap to the next neighbour)"""
    a, b = np.asarray(desc_a, np.float64), np.asarray(desc_b, np.float64)
    D = ((a[:, None, :] - b[None, :, :]) ** 2).sum(axis=2)
    order = np.argsort(D, axis=1, kind="stable")
    kk = min(k, b.shape[0])
    idx = order[:, :kk].astype(np.int32)
    sd = np.take_along_axis(D, order, axis=1)
    return idx, sd[:, :kk], sd


def dist_f32(desc_a, desc_b, idx):
    """the float32 squared distances of the chosen neighbours, differences squared and summed in index order"""
    a, b = np.asarray(desc_a, np.float32), np.asarray(desc_b, np.float32)
    out = np.zeros(idx.shape, np.float32)
    for t in range(a.shape[1]):
        df = a[:, t][:, None] - b[idx, t]
        out = out + df * df
    return out


def candidates(idx):
    """candidate i * k + j is (i, nn[j])"""
    na, kk = idx.shape
    return np.stack([np.repeat(np.arange(na, dtype=np.int32), kk), idx.reshape(-1).astype(np.int32)], axis=1)


def nndr_matches(idx, dist, k, nndr):
    """the match list of generate_candidates: d0 < NNDR * d1, only when k > 1"""
    if k <= 1 or idx.shape[1] < 2:
        return np.zeros((0, 2), np.int32)
    keep = dist[:, 0].astype(np.float32) < np.float32(nndr) * dist[:, 1].astype(np.float32)
    rows = np.flatnonzero(keep)
    return np.stack([rows.astype(np.int32), idx[rows, 0].astype(np.int32)], axis=1)


# ------------------------------------------------------------------------------------------------------------------ host logic
def remove_candidates(cand, winners):
    """match_group's removal loop (GTMatcher.cpp:300-315): a removed candidate is overwritten with the last one, the list shrinks
    and slot i is not looked at again"""
    cm = [tuple(int(v) for v in c) for c in np.asarray(cand).reshape(-1, 2)]
    wins = [tuple(int(v) for v in w) for w in np.asarray(winners).reshape(-1, 2)]
    i = 0
    while i < len(cm):
        for s, t in wins:
            if cm[i][0] == s or cm[i][1] == t:
                cm[i] = cm[-1]
                cm.pop()
                break
        i += 1
    return np.array(cm, np.int32).reshape(-1, 2)


def remove_candidates_all(cand, winners):
    """what a `correct` removal would leave: no candidate that uses a winning feature, the order kept"""
    cand = np.asarray(cand).reshape(-1, 2)
    winners = np.asarray(winners).reshape(-1, 2)
    keep = ~(np.isin(cand[:, 0], winners[:, 0]) | np.isin(cand[:, 1], winners[:, 1]))
    return cand[keep].astype(np.int32)


def gt_match(fa_xysa, fb_xysa, desc_a, desc_b, lam=1e-5, pop_threshold=0.7, min_group_size=5, max_rounds=20, k=3, skip_gt=False, nndr=0.25,
             toll=TOLL, max_iters=MAX_ITERS, summation="sequential", dynamics=None):
    """wass_match.cpp's round loop.  Returns (matches M x 2, rounds as a list of (N, steps, group size))."""
    idx, d64, _ = knn(desc_a, desc_b, k)
    if skip_gt:
        return nndr_matches(idx, dist_f32(desc_a, desc_b, idx), k, nndr), []
    cand = candidates(idx)
    run = dynamics or (lambda A: iidyn(A, None, toll, max_iters, summation))
    matches, rounds = [], []
    left = max_rounds
    while True:
        if cand.shape[0] == 0:                               # the reference is undefined here; the product stops
            break
        P, _, _ = payoff(fa_xysa, fb_xysa, cand, lam)
        x, steps, _ = run(P)
        g = group(x, pop_threshold)
        win = cand[g]
        matches.extend(win.tolist())
        rounds.append((int(cand.shape[0]), int(steps), int(g.size)))
        cand = remove_candidates(cand, win)
        go = g.size >= min_group_size
        more = left != 0
        left -= 1
        if not (more and go):
            break
    return np.array(matches, np.int32).reshape(-1, 2), rounds


# ---------------------------------------------------------------------------------------------------------------------- inputs
def random_symmetric(n, density, seed):
    """mrand's kind of matrix: zero diagonal, symmetric, an entry present with probability `density` and then uniform in (0, 1)"""
    rng = np.random.default_rng(seed)
    U = rng.random((n, n))
    M = np.where(rng.random((n, n)) <= density, U, 0.0)
    M = np.triu(M, 1)
    return M + M.T


def cliques(sizes, interleave=False):
    """disjoint 0/1 cliques of the given sizes; a size of 1 is an isolated strategy"""
    n = sum(sizes)
    label = np.concatenate([np.full(s, i) for i, s in enumerate(sizes)])
    if interleave:
        label = np.arange(n) % len(sizes)
    A = (label[:, None] == label[None, :]).astype(np.float64)
    np.fill_diagonal(A, 0.0)
    return A


def scene(seed, n=80, dim=64, outliers=0.5, noise=0.3):
    """two feature sets under a similarity transform, `outliers` of B's features moved somewhere else.  Returns (fa, fb, desc_a,
    desc_b, truth) with fa, fb n x 4 float32 (x y scale angle) and truth[i] = True where feature i of A kept its partner i of B."""
    rng = np.random.default_rng(seed)
    theta, s, t = rng.uniform(-0.6, 0.6), rng.uniform(0.8, 1.25), rng.uniform(-80, 80, 2)
    xy = rng.uniform(50, 1950, (n, 2))
    sc = rng.uniform(2, 12, n)
    an = rng.uniform(0, 2 * np.pi, n)
    R = np.array([[np.cos(theta), -np.sin(theta)], [np.sin(theta), np.cos(theta)]])
    xy_b = (s * (R @ xy.T)).T + t + rng.normal(0, noise, (n, 2))
    sc_b = sc * s
    an_b = np.mod(an - theta, 2 * np.pi)                     # compute_affine rotates by src.angle - targ.angle
    truth = np.ones(n, bool)
    out = rng.permutation(n)[:int(n * outliers)]
    truth[out] = False
    xy_b[out] = rng.uniform(50, 1950, (out.size, 2))
    sc_b[out] = rng.uniform(2, 12, out.size)
    an_b[out] = rng.uniform(0, 2 * np.pi, out.size)
    desc_a = rng.normal(0, 1, (n, dim))
    desc_a /= np.linalg.norm(desc_a, axis=1, keepdims=True)
    desc_b = desc_a + rng.normal(0, 0.02, (n, dim))
    desc_b /= np.linalg.norm(desc_b, axis=1, keepdims=True)
    fa = np.column_stack([xy, sc, an]).astype(np.float32)
    fb = np.column_stack([xy_b, sc_b, an_b]).astype(np.float32)
    return fa, fb, desc_a.astype(np.float32), desc_b.astype(np.float32), truth


# the probe matrices of the dynamics: every one of them is also held to the conditions of tests/test_match.py
GPU_SIZES = (1, 2, 3, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049)
DENSITIES = (0.05, 0.5, 1.0)
PROBE_STEPS = 300
BIG_N, BIG_STEPS, BIG_LAMBDA = 8192, 50, 1e-5


def random_seed(n, density):
    return 1000 * n + int(round(density * 100))


def big_scene():
    """2048 features under a similarity transform with four candidates each, the first the true partner: N = 8192, the cap"""
    fa, fb, _, _, _ = scene(99, n=2048, outliers=0.25)
    i = np.arange(2048, dtype=np.int32)
    cand = np.stack([np.repeat(i, 4), ((i[:, None] + np.array([0, 37, 411, 1201])[None, :]) % 2048).reshape(-1).astype(np.int32)], axis=1)
    return fa, fb, cand


def tie_probe():
    """exact ties among more strategies than one wave holds: two cliques of 40 that tie, and one of 60 with larger payoffs, which wins"""
    return cliques([40, 40, 60]) * np.repeat([1.0, 1.0, 1.5], [40, 40, 60])[:, None]


def batch_problems(golden_scene0):
    """five problems of different size for the batch tests; the fourth (6 features, 3 of them true) ends in its first round"""
    return [golden_scene0, scene(21, n=60)[:4], scene(22, n=33)[:4], scene(23, n=6)[:4], scene(24, n=100)[:4]]


BATCH_LAMBDA = 1e-4
