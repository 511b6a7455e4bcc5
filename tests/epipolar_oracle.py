"""numpy oracle of the essential-matrix filter (wass_amd/epipolar.py, csrc/epipolar.hip): test infrastructure only.

  five_point        an independent five-point solver: the null space from np.linalg.svd, the ten monomials of degree 3 eliminated, the
                    solutions read off the real eigenvectors of the 10 x 10 action matrix of the multiplication by x.  No polynomial
                    in one unknown, no root isolation: it shares nothing with the kernel but the problem.
  sampson_err ...   the scoring in the operation order include/wass_gpu.h states, so that err and the counts can be compared exactly
  find_essential    best of all hypotheses, the largest count, ties to the lowest (sample, solution)
  recover_pose, epipolar_error_stats   restated on their own
  rig, scene        a synthetic calibrated rig over a slanted sea (or an exactly planar one), with pixel noise and outliers

Conventions (wass_match.cpp:252-280): x0 = K0^-1 (u0, v0, 1), x1 = K1^-1 (u1, v1, 1), x1' E x0 = 0, a point X of camera 0 is
R X + T in camera 1, E = [T]x R.
"""
import functools
import itertools

import numpy as np

EPS = np.finfo(np.float64).eps
KAPPA_MAX = 1.0e5          # a sample is admitted when the 10 x 10 block is conditioned better than this ...
SEPARATION = 1.0e-4        # ... and the action matrix's eigenvalues are this far apart, relatively
BOUND_FACTOR = 16.0        # the kernel's elimination and root finder have constants of their own

# the reference's acceptance numbers (test/verify_matcher.m:5-8)
MIN_MATCHES, MAX_EPI_ERROR, T_MAX_ERR, R_MAX_ERR = 400, 0.5, 2e-2, 5e-3


# ------------------------------------------------------------------------------------------------------------------------- rig
def skew(t):
    return np.array([[0.0, -t[2], t[1]], [t[2], 0.0, -t[0]], [-t[1], t[0], 0.0]])


def rodrigues(r):
    th = np.linalg.norm(r)
    if th == 0.0:
        return np.eye(3)
    k = skew(r / th)
    return np.eye(3) + np.sin(th) * k + (1.0 - np.cos(th)) * (k @ k)


def rig(seed=0, f=2500.0, angle=0.15, size=(2456, 2058)):
    """K0, K1, R, T (|T| = 1: the baseline), the picture size.  Camera 1 sits one baseline to the side of camera 0, turned by about
    `angle` rad, mostly about the vertical axis, towards it."""
    rng = np.random.default_rng([seed, 101])
    w, h = size
    K0 = np.array([[f, 0.0, w / 2 + rng.uniform(-20, 20)], [0.0, f * rng.uniform(0.995, 1.005), h / 2 + rng.uniform(-20, 20)], [0.0, 0.0, 1.0]])
    K1 = np.array([[f * rng.uniform(0.99, 1.01), 0.0, w / 2 + rng.uniform(-20, 20)], [0.0, f * rng.uniform(0.99, 1.01), h / 2 + rng.uniform(-20, 20)],
                   [0.0, 0.0, 1.0]])
    axis = np.array([0.1, 1.0, 0.05]) + rng.uniform(-0.1, 0.1, 3)
    R = rodrigues(angle * rng.uniform(0.8, 1.2) * axis / np.linalg.norm(axis))
    T = np.array([-1.0, 0.0, 0.0]) + rng.uniform(-0.15, 0.15, 3)
    T /= np.linalg.norm(T)
    return K0, K1, R, T, size


def essential(R, T):
    E = skew(T) @ R
    return E / np.linalg.norm(E)


def scene(the_rig, m, seed, noise=0.0, outliers=0.0, planar=False):
    """m matches of the rig: sea points 6 to 40 baselines away on a slanted plane below the cameras, a few baselines above and below
    it (planar: exactly on it).  Returns the pixel positions (float32 M x 2 each, what matches_unfiltered.txt holds), the normalised
    points of the noise-free pixels before their rounding to float32 (fp64 M x 2 each: exact inliers of the true E), and which
    matches are inliers.  noise: pixels, Gaussian, on both pictures; outliers: the share replaced by uniform positions in picture 1."""
    K0, K1, R, T, (w, h) = the_rig
    rng = np.random.default_rng([seed, 202, int(planar)])
    P = np.zeros((0, 3))
    while P.shape[0] < m:
        n = 4 * m
        z = rng.uniform(6.0, 40.0, n)
        x = rng.uniform(-0.5, 0.5, n) * z
        y = 2.0 + 0.02 * z + (0.0 if planar else 1.0) * rng.uniform(-3.0, 3.0, n)
        Q = np.stack([x, y, z], axis=1)
        p0 = Q @ K0.T
        Q1 = Q @ R.T + T
        p1 = Q1 @ K1.T
        ok = (Q1[:, 2] > 1.0)
        for p, d in ((p0, Q[:, 2]), (p1, Q1[:, 2])):
            ok &= (p[:, 0] / d > 5) & (p[:, 0] / d < w - 5) & (p[:, 1] / d > 5) & (p[:, 1] / d < h - 5)
        P = np.concatenate([P, Q[ok]])
    P = P[:m]
    u0 = (P @ K0.T)
    u0 = u0[:, :2] / u0[:, 2:]
    u1 = (P @ R.T + T) @ K1.T
    u1 = u1[:, :2] / u1[:, 2:]
    x0, x1 = normalise(u0, K0), normalise(u1, K1)
    inl = np.ones(m, bool)
    n_out = int(round(outliers * m))
    if n_out:
        bad = rng.permutation(m)[:n_out]
        inl[bad] = False
        u1[bad] = np.stack([rng.uniform(5, w - 5, n_out), rng.uniform(5, h - 5, n_out)], axis=1)
        x1[bad] = normalise(u1[bad], K1)
    if noise:
        u0 = u0 + rng.normal(0.0, noise, u0.shape)
        u1 = u1 + rng.normal(0.0, noise, u1.shape)
    return u0.astype(np.float32), u1.astype(np.float32), x0, x1, inl


def normalise(px, K):
    """K^-1 (u, v, 1), its first two entries: wass_match.cpp:272-276"""
    Ki = np.linalg.inv(K)
    p = np.concatenate([np.asarray(px, np.float64), np.ones((len(px), 1))], axis=1) @ Ki.T
    return np.ascontiguousarray(p[:, :2])


# ------------------------------------------------------------------------------------------------------------------ five-point
_CUBIC = [e for e in itertools.product(range(4), repeat=3) if sum(e) == 3]                       # the ten monomials that go
_BASIS = [(2, 0, 0), (1, 1, 0), (1, 0, 1), (0, 2, 0), (0, 1, 1), (0, 0, 2), (1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, 0)]


def _pmul(A, B):
    """product of two polynomials in (x, y, z) held as S x (d+1)^3 arrays of coefficients by exponent"""
    na, nb = A.shape[1], B.shape[1]
    out = np.zeros((A.shape[0],) + (na + nb - 1,) * 3)
    for i, j, k in itertools.product(range(nb), repeat=3):
        if i + j + k < nb:
            out[:, i:i + na, j:j + na, k:k + na] += A * B[:, i, j, k][:, None, None, None]
    return out


def constraints(q0, q1):
    """S samples of five matches (S x 5 x 2 each) -> the null-space basis (S x 4 x 9: X Y Z W) and the ten cubic constraints as
    S x 10 x 4 x 4 x 4 coefficient arrays"""
    q0, q1 = np.asarray(q0, np.float64), np.asarray(q1, np.float64)
    S = q0.shape[0]
    a = np.concatenate([q0, np.ones((S, 5, 1))], axis=2)
    b = np.concatenate([q1, np.ones((S, 5, 1))], axis=2)
    Q = (b[:, :, :, None] * a[:, :, None, :]).reshape(S, 5, 9)
    basis = np.linalg.svd(Q)[2][:, 5:, :]
    ent = np.zeros((S, 9, 2, 2, 2))
    ent[:, :, 1, 0, 0], ent[:, :, 0, 1, 0], ent[:, :, 0, 0, 1], ent[:, :, 0, 0, 0] = basis[:, 0], basis[:, 1], basis[:, 2], basis[:, 3]
    e = [[ent[:, 3 * r + c] for c in range(3)] for r in range(3)]
    eet = [[sum(_pmul(e[i][k], e[j][k]) for k in range(3)) for j in range(3)] for i in range(3)]
    tr = eet[0][0] + eet[1][1] + eet[2][2]
    out = []
    for i in range(3):
        for j in range(3):
            out.append(sum(_pmul(2.0 * eet[i][k], e[k][j]) for k in range(3)) - _pmul(tr, e[i][j]))
    det = (_pmul(_pmul(e[1][1], e[2][2]) - _pmul(e[1][2], e[2][1]), e[0][0]) - _pmul(_pmul(e[1][0], e[2][2]) - _pmul(e[1][2], e[2][0]), e[0][1])
           + _pmul(_pmul(e[1][0], e[2][1]) - _pmul(e[1][1], e[2][0]), e[0][2]))
    out.append(det)
    return basis, np.stack(out, axis=1)


def five_point(q0, q1):
    """S samples -> per sample a dict: E (n x 3 x 3, norm 1), kappa (condition number of the 10 x 10 block of the eliminated
    monomials), eig (the ten eigenvalues), admitted (kappa <= KAPPA_MAX and the eigenvalues SEPARATION apart, relatively)"""
    basis, cons = constraints(q0, q1)
    S = cons.shape[0]
    A3 = np.stack([cons[:, :, i, j, k] for i, j, k in _CUBIC], axis=2)
    A2 = np.stack([cons[:, :, i, j, k] for i, j, k in _BASIS], axis=2)
    out = []
    for s in range(S):
        rec = {"E": np.zeros((0, 3, 3)), "kappa": np.inf, "eig": np.zeros(0), "admitted": False}
        out.append(rec)
        if not np.isfinite(A3[s]).all():
            continue
        rec["kappa"] = np.linalg.cond(A3[s])
        if not np.isfinite(rec["kappa"]) or rec["kappa"] > 1e15:
            continue
        red = -np.linalg.solve(A3[s], A2[s])                 # a cubic monomial = red[its index] . basis
        Mx = np.zeros((10, 10))
        for i, (a, b, c) in enumerate(_BASIS):
            t = (a + 1, b, c)
            if sum(t) == 3:
                Mx[i] = red[_CUBIC.index(t)]
            else:
                Mx[i, _BASIS.index(t)] = 1.0
        w, V = np.linalg.eig(Mx)
        rec["eig"] = w
        d = np.abs(w[:, None] - w[None, :]) + np.eye(10) * 1e300
        big = np.maximum(np.abs(w)[:, None], np.abs(w)[None, :])
        rec["admitted"] = bool(rec["kappa"] <= KAPPA_MAX and (d >= SEPARATION * big).all())
        sols = []
        for k in np.argsort(w.real):
            if w[k].imag != 0.0:
                continue
            v = V[:, k].real
            # v = (x^2, xy, xz, y^2, yz, z^2, x, y, z, 1) up to scale: the entries of the symmetric 4 x 4 matrix h h' with
            # h = (x, y, z, 1).  Its dominant eigenvector uses all ten entries and divides by none of them.
            H = v[[[0, 1, 2, 6], [1, 3, 4, 7], [2, 4, 5, 8], [6, 7, 8, 9]]]
            hw, hv = np.linalg.eigh(H)
            h = hv[:, np.argmax(np.abs(hw))]
            with np.errstate(all="ignore"):
                E = h @ basis[s]
                E = E / np.linalg.norm(E)
            if np.isfinite(E).all():
                sols.append(E.reshape(3, 3))
        rec["E"] = np.array(sols).reshape(-1, 3, 3)
    return out


def distance(E, F):
    """between two essential matrices of norm 1, up to sign"""
    return min(np.linalg.norm(E - F), np.linalg.norm(E + F))


def residuals(E, q0, q1):
    """of one solution of norm 1: the largest of |x1' E x0| over the five matches, |det E| and |2 E E' E - tr(E E') E|"""
    a = np.concatenate([q0, np.ones((5, 1))], axis=1)
    b = np.concatenate([q1, np.ones((5, 1))], axis=1)
    epi = np.abs(np.einsum("ni,ij,nj->n", b, E, a)).max()
    return max(epi, abs(np.linalg.det(E)), np.abs(2.0 * E @ E.T @ E - np.trace(E @ E.T) * E).max())


# --------------------------------------------------------------------------------------------------------------------- scoring
def sampson_err(E, x0, x1):
    """float32 err of every match under one model, operation by operation as the header states it"""
    E = np.asarray(E, np.float64).reshape(9)
    ax, ay, bx, by = x0[:, 0], x0[:, 1], x1[:, 0], x1[:, 1]
    with np.errstate(all="ignore"):
        l0 = (E[0] * ax + E[1] * ay) + E[2]
        l1 = (E[3] * ax + E[4] * ay) + E[5]
        l2 = (E[6] * ax + E[7] * ay) + E[8]
        r0 = (E[0] * bx + E[3] * by) + E[6]
        r1 = (E[1] * bx + E[4] * by) + E[7]
        num = (bx * l0 + by * l1) + l2
        den = ((l0 * l0 + l1 * l1) + r0 * r0) + r1 * r1
        return ((num * num) / den).astype(np.float32)


def threshold(t):
    return np.float32(np.float64(t) * np.float64(t))


def inlier_mask(E, x0, x1, t):
    with np.errstate(invalid="ignore"):
        return sampson_err(E, x0, x1) <= threshold(t)


def score_models(E, x0, x1, t):
    return np.array([int(inlier_mask(e, x0, x1, t).sum()) for e in np.asarray(E).reshape(-1, 3, 3)], np.int32)


def find_essential(x0, x1, t, samples, tie="first", compare="le", squared=True):
    """The best of all hypotheses.  Returns a dict: E, mask, count, sample, solution, rec (the winning sample's five_point record).
    tie / compare / squared are there for the probes of tests/test_epipolar.py: the mistakes the scenes must notice."""
    samples = np.asarray(samples)
    recs = five_point(x0[samples], x1[samples])
    thr = threshold(t) if squared else np.float32(t)
    best = {"E": np.zeros((3, 3)), "mask": np.zeros(len(x0), bool), "count": -1, "sample": -1, "solution": -1, "rec": None}
    for r, rec in enumerate(recs):
        for s, E in enumerate(rec["E"][:10]):
            err = sampson_err(E, x0, x1)
            with np.errstate(invalid="ignore"):
                mask = err <= thr if compare == "le" else err < thr
            n = int(mask.sum())
            if n > best["count"] or (tie == "last" and n == best["count"]):
                best = {"E": E, "mask": mask, "count": n, "sample": r, "solution": s, "rec": rec, "err": err}
    return best


def margin(err, t):
    """the smallest relative distance of an err to the threshold"""
    thr = np.float64(threshold(t))
    e = err[np.isfinite(err)].astype(np.float64)
    return np.abs(e - thr).min() / thr


# ------------------------------------------------------------------------------------------------------------------------ pose
def triangulate(P0, P1, x0, x1):
    """DLT: the homogeneous point of every match, M x 4"""
    A = np.stack([x0[:, 0:1] * P0[2] - P0[0], x0[:, 1:2] * P0[2] - P0[1], x1[:, 0:1] * P1[2] - P1[0], x1[:, 1:2] * P1[2] - P1[1]], axis=1)
    return np.linalg.svd(A)[2][:, 3, :]


def recover_pose(E, x0, x1, mask, distance=50.0):
    """cv::recoverPose restated: the four decompositions in OpenCV's order, the first with the most points in front of both
    cameras and nearer than `distance`"""
    U, _, Vt = np.linalg.svd(np.asarray(E, np.float64).reshape(3, 3))
    if np.linalg.det(U) < 0:
        U = -U
    if np.linalg.det(Vt) < 0:
        Vt = -Vt
    W = np.array([[0.0, 1.0, 0.0], [-1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    R1, R2, t = U @ W @ Vt, U @ W.T @ Vt, U[:, 2]
    P0 = np.eye(3, 4)
    best = None
    for R, tt in ((R1, t), (R2, t), (R1, -t), (R2, -t)):
        P1 = np.concatenate([R, tt[:, None]], axis=1)
        Q = triangulate(P0, P1, x0, x1)
        with np.errstate(all="ignore"):
            good = Q[:, 2] * Q[:, 3] > 0
            Q = Q / Q[:, 3:]
            good &= Q[:, 2] < distance
            z1 = (Q @ P1.T)[:, 2]
            good &= (z1 > 0) & (z1 < distance)
        good &= np.asarray(mask, bool)
        if best is None or good.sum() > best[2].sum():
            best = (R, tt, good)
    return best


def epipolar_error_stats(F, p0, p1):
    """evaluate_epipolar_error (epipolar.cpp:7-39) restated with numpy's own sums: avg, std, min, max"""
    l = np.concatenate([np.asarray(p0, np.float64), np.ones((len(p0), 1))], axis=1)
    r = np.concatenate([np.asarray(p1, np.float64), np.ones((len(p1), 1))], axis=1)
    Fl, Fr = l @ F.T, r @ F
    e = 0.5 * (np.abs((Fl * r).sum(1) / np.sqrt(Fl[:, 0] ** 2 + Fl[:, 1] ** 2)) + np.abs((Fr * l).sum(1) / np.sqrt(Fr[:, 0] ** 2 + Fr[:, 1] ** 2)))
    return float(e.mean()), float(np.sqrt(((e - e.mean()) ** 2).mean())), float(e.min()), float(e.max())


def fundamental(E, K0, K1):
    return np.linalg.inv(K1).T @ np.asarray(E).reshape(3, 3) @ np.linalg.inv(K0)


def pipeline(loc_a, loc_b, K0, K1, samples, max_epi_distance=0.5):
    """the whole filter on the oracle alone: a dict with E, mask, R, T, pose_mask, stats, kept"""
    x0, x1 = normalise(loc_a, K0), normalise(loc_b, K1)
    t = max_epi_distance / ((K0[0, 0] + K0[1, 1]) / 2)
    best = find_essential(x0, x1, t, samples)
    R, T, good = recover_pose(best["E"], x0, x1, best["mask"])
    stats = epipolar_error_stats(fundamental(best["E"], K0, K1), np.asarray(loc_a)[good], np.asarray(loc_b)[good])
    return {"E": best["E"], "mask": best["mask"], "R": R, "T": T, "pose_mask": good, "stats": stats, "kept": int(good.sum()), "best": best, "t": t}


# --------------------------------------------------------------------------------------------------------- the tests' scenes
SOLVER_SAMPLES = 256
SCORE_M = (5, 6, 63, 64, 65, 257)
ROUNDS = (1, 63, 64, 65, 1024)
NOISY = dict(m=600, noise=0.2, outliers=0.3, rounds=1024, rig_seed=3, seed=12)
SELECT = dict(rig_seed=5, outliers=0.3, rounds=128)


@functools.lru_cache(maxsize=None)
def solver_scene(planar):
    """256 noise-free samples of five matches of one scene, the truth, the oracle's records and its own error against the truth"""
    g = rig(7 + int(planar))
    _, _, x0, x1, _ = scene(g, 400, 31, planar=planar)
    rng = np.random.default_rng([77, int(planar)])
    samples = np.array([rng.permutation(400)[:5] for _ in range(SOLVER_SAMPLES)], np.int32)
    recs = five_point(x0[samples], x1[samples])
    Et = essential(g[2], g[3])
    dist = np.array([min([distance(E, Et) for E in r["E"]], default=np.inf) for r in recs])
    return {"x0": x0, "x1": x1, "samples": samples, "recs": recs, "Et": Et, "dist": dist}


def solver_bound_factor():
    """c of the bound c kappa eps: BOUND_FACTOR times the largest distance / (kappa eps) the oracle itself shows against the true E
    on the admitted samples of both scenes"""
    worst = 0.0
    for planar in (False, True):
        sc = solver_scene(planar)
        for r, d in zip(sc["recs"], sc["dist"]):
            if r["admitted"]:
                worst = max(worst, d / (r["kappa"] * EPS))
    return BOUND_FACTOR * worst


@functools.lru_cache(maxsize=None)
def select_scene(m, seed=0):
    """exact inliers plus 30 % outliers, in normalised coordinates; the threshold of a 0.5 px distance"""
    g = rig(SELECT["rig_seed"])
    _, _, x0, x1, inl = scene(g, m, 41 + seed, outliers=SELECT["outliers"])
    t = 0.5 / ((g[0][0, 0] + g[0][1, 1]) / 2)
    return g, x0, x1, inl, t


@functools.lru_cache(maxsize=None)
def noisy_scene():
    g = rig(NOISY["rig_seed"])
    loc_a, loc_b, _, _, inl = scene(g, NOISY["m"], NOISY["seed"], noise=NOISY["noise"], outliers=NOISY["outliers"])
    return g, loc_a, loc_b, inl


def score_probe(m, seed=0):
    """m matches and a few models for the exact scoring tests: the true E, two perturbed ones, a model of zeros; matches moved onto
    err == float32(t * t) and one float32 ulp either side under the true E, and one NaN match (m >= 6)."""
    g = rig(9)
    _, _, x0, x1, _ = scene(g, m, 51 + seed, outliers=0.3)
    t = 0.5 / ((g[0][0, 0] + g[0][1, 1]) / 2)
    Et = essential(g[2], g[3])
    rng = np.random.default_rng([m, seed, 5])
    models = np.stack([Et, Et + 1e-4 * rng.normal(size=(3, 3)), Et.T, np.zeros((3, 3)), -Et + 1e-6 * rng.normal(size=(3, 3))])
    x1 = x1.copy()
    thr = threshold(t)
    targets = [thr, np.nextafter(thr, np.float32(0)), np.nextafter(thr, np.float32(1))]
    placed = []
    for k, want in enumerate(targets[:max(0, min(3, m - 2))]):
        j = k
        # move match j across the epipolar line of x0[j] until its float32 err is exactly `want`: bisection on the offset
        a = np.concatenate([x0[j], [1.0]])
        line = Et @ a
        n = line[:2] / np.linalg.norm(line[:2])
        base = x1[j] - n * ((line[:2] @ x1[j] + line[2]) / np.linalg.norm(line[:2]))
        lo, hi = 0.0, 4.0 * t
        for _ in range(200):
            mid = 0.5 * (lo + hi)
            e = sampson_err(Et, x0[j:j + 1], (base + mid * n)[None])[0]
            if e < want:
                lo = mid
            elif e > want:
                hi = mid
            else:
                break
        x1[j] = base + mid * n
        placed.append((j, want, sampson_err(Et, x0[j:j + 1], x1[j:j + 1])[0]))
    if m >= 6:
        x1[m - 1, 0] = np.nan
    return x0, x1, models, t, placed
