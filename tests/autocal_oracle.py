"""numpy oracle of the autocalibration (wass_amd/autocalibrate.py, csrc/autocal.hip): test infrastructure only.

  triangulate, project, linearize   the per-point formulas in the operation order include/wass_gpu.h states, so that the kernels'
                                    per-point results can be compared exactly
  jacobian_cs                       the Jacobian on its own: complex-step differentiation of a projection written with the
                                    quaternion product; it shares nothing with the kernel's closed form
  lm                                Levenberg-Marquardt with the rules DESIGN.md states, on dense normal equations (or, above
                                    DENSE_MAX points, the Schur complement from numpy's own inverses and solver)
  choose_pose, select_points, relative_pose, pose_distance
  ba_scene                          a scene of the synthetic rig of tests/epipolar_oracle.py for the bundle adjustment

A camera is 15 numbers: R0 (9), v (3), t (3); parameters are ordered v0 t0 v1 t1, then the points.
"""
import numpy as np

import epipolar_oracle as EO

EPS = np.finfo(np.float64).eps
DENSE_MAX = 150
MARGIN = 64.0    # see DESIGN.md, "Autocalibration": the yardstick is one draw of a rounding-noise magnitude, the result another


def gamma(n):
    return n * EPS / (1.0 - n * EPS)


# ----------------------------------------------------------------------------------------------------------------- stated order
def triangulate(R, T, x0, x1):
    """M x 3: the least-squares point of the two rays, NaN where the determinant is zero or not finite"""
    R, T = np.asarray(R, np.float64).reshape(3, 3), np.asarray(T, np.float64).reshape(3)
    p0, p1, q0, q1 = x0[:, 0], x0[:, 1], x1[:, 0], x1[:, 1]
    with np.errstate(all="ignore"):
        r2 = [q0 * R[2, k] - R[0, k] for k in range(3)]
        r3 = [q1 * R[2, k] - R[1, k] for k in range(3)]
        b2, b3 = T[0] - T[2] * q0, T[1] - T[2] * q1
        a = (1.0 + r2[0] * r2[0]) + r3[0] * r3[0]
        b = r2[0] * r2[1] + r3[0] * r3[1]
        c = (r2[0] * r2[2] - p0) + r3[0] * r3[2]
        d = (1.0 + r2[1] * r2[1]) + r3[1] * r3[1]
        e = (r2[1] * r2[2] - p1) + r3[1] * r3[2]
        f = ((p0 * p0 + p1 * p1) + r2[2] * r2[2]) + r3[2] * r3[2]
        y = [r2[k] * b2 + r3[k] * b3 for k in range(3)]
        C00, C01, C02 = d * f - e * e, c * e - b * f, b * e - c * d
        C11, C12, C22 = a * f - c * c, b * c - a * e, a * d - b * b
        det = (a * C00 + b * C01) + c * C02
        X = ((C00 * y[0] + C01 * y[1]) + C02 * y[2]) / det
        Y = ((C01 * y[0] + C11 * y[1]) + C12 * y[2]) / det
        Z = ((C02 * y[0] + C12 * y[1]) + C22 * y[2]) / det
    out = np.stack([X, Y, Z], axis=1)
    out[~((det != 0.0) & np.isfinite(det))] = np.nan
    return out


def count_valid(pts, mask, bound=1.0):
    with np.errstate(invalid="ignore"):
        return int((np.asarray(mask, bool) & (pts[:, 2] > bound)).sum())


def derived(cam):
    """R0, v, t, w, 1 / w, Rj of one camera"""
    cam = np.asarray(cam, np.float64).reshape(15)
    R0, v, t = cam[:9].reshape(3, 3), cam[9:12], cam[12:15]
    s = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]
    with np.errstate(all="ignore"):
        w = np.sqrt(1.0 - s)
        iw = 1.0 / w
    vx = np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])
    I = np.eye(3)
    Rl = I + 2.0 * (w * vx + (np.outer(v, v) - s * I))
    Rj = np.stack([(Rl[r, 0] * R0[0] + Rl[r, 1] * R0[1]) + Rl[r, 2] * R0[2] for r in range(3)])
    return R0, v, t, w, iw, Rj


def _project(Rj, t, M):
    X = [((Rj[r, 0] * M[:, 0] + Rj[r, 1] * M[:, 1]) + Rj[r, 2] * M[:, 2]) + t[r] for r in range(3)]
    iz = 1.0 / X[2]
    return iz, X[0] * iz, X[1] * iz


def residuals(cams, pts, obs):
    """N x 4: ex0 ey0 ex1 ey1"""
    out = []
    with np.errstate(all="ignore"):
        for q in range(2):
            _, _, t, _, _, Rj = derived(cams[q])
            _, px, py = _project(Rj, t, pts)
            out += [obs[:, 2 * q] - px, obs[:, 2 * q + 1] - py]
    return np.stack(out, axis=1)


def error(cams, pts, obs):
    r = residuals(cams, pts, obs)
    return float((r * r).sum())


def cam_rows(cam, M, uv):
    """ax, ay (N x 6), bx, by (N x 3), ex, ey of one camera in the stated order"""
    R0, v, t, w, iw, Rj = derived(cam)
    with np.errstate(all="ignore"):
        iz, px, py = _project(Rj, t, M)
        ex, ey = uv[:, 0] - px, uv[:, 1] - py
        Y = [(R0[r, 0] * M[:, 0] + R0[r, 1] * M[:, 1]) + R0[r, 2] * M[:, 2] for r in range(3)]
        c = [v[1] * Y[2] - v[2] * Y[1], v[2] * Y[0] - v[0] * Y[2], v[0] * Y[1] - v[1] * Y[0]]
        h = (v[0] * Y[0] + v[1] * Y[1]) + v[2] * Y[2]
        g = [w * Y[r] + c[r] for r in range(3)]
        G = [iw * c[r] + Y[r] for r in range(3)]
        z = np.zeros_like(h)
        gx = [[z, -g[2], g[1]], [g[2], z, -g[0]], [-g[1], g[0], z]]
        D = [[2.0 * (((h if r == k else 0.0) - G[r] * v[k]) - gx[r][k]) for k in range(3)] for r in range(3)]
        ax = [iz * (D[0][k] - px * D[2][k]) for k in range(3)] + [iz, z, -(px * iz)]
        ay = [iz * (D[1][k] - py * D[2][k]) for k in range(3)] + [z, iz, -(py * iz)]
        bx = [iz * (Rj[0, k] - px * Rj[2, k]) for k in range(3)]
        by = [iz * (Rj[1, k] - py * Rj[2, k]) for k in range(3)]
    return np.stack(ax, 1), np.stack(ay, 1), np.stack(bx, 1), np.stack(by, 1), ex, ey


def linearize(cams, pts, obs):
    """dict: res (N x 4), V (N x 3 x 3), eb (N x 3), W (N x 2 x 6 x 3) bit for bit as the kernel states them; the terms of the sums
    Ut (N x 2 x 6 x 6), eat (N x 12), e2 (N); A (N x 2 x 2 x 6) and B (N x 2 x 2 x 3)"""
    n = pts.shape[0]
    res, W, Ut, eat = np.zeros((n, 4)), np.zeros((n, 2, 6, 3)), np.zeros((n, 2, 6, 6)), np.zeros((n, 12))
    A, B = np.zeros((n, 2, 2, 6)), np.zeros((n, 2, 2, 3))
    V = eb = e2 = None
    with np.errstate(all="ignore"):
        for q in range(2):
            ax, ay, bx, by, ex, ey = cam_rows(cams[q], pts, obs[:, 2 * q:2 * q + 2])
            A[:, q, 0], A[:, q, 1], B[:, q, 0], B[:, q, 1] = ax, ay, bx, by
            res[:, 2 * q], res[:, 2 * q + 1] = ex, ey
            Vq = bx[:, :, None] * bx[:, None, :] + by[:, :, None] * by[:, None, :]
            ebq = bx * ex[:, None] + by * ey[:, None]
            eq = ex * ex + ey * ey
            V, eb, e2 = (Vq, ebq, eq) if q == 0 else (V + Vq, eb + ebq, e2 + eq)
            W[:, q] = ax[:, :, None] * bx[:, None, :] + ay[:, :, None] * by[:, None, :]
            Ut[:, q] = ax[:, :, None] * ax[:, None, :] + ay[:, :, None] * ay[:, None, :]
            eat[:, 6 * q:6 * q + 6] = ax * ex[:, None] + ay * ey[:, None]
    return dict(res=res, V=V, eb=eb, W=W, Ut=Ut, eat=eat, e2=e2, A=A, B=B)


def vinv(V, mu):
    """(V + mu I)^-1 by the cofactor rule, N x 3 x 3"""
    with np.errstate(all="ignore"):
        a, b, c, d, e, f = V[:, 0, 0] + mu, V[:, 0, 1], V[:, 0, 2], V[:, 1, 1] + mu, V[:, 1, 2], V[:, 2, 2] + mu
        C00, C01, C02 = d * f - e * e, c * e - b * f, b * e - c * d
        C11, C12, C22 = a * f - c * c, b * c - a * e, a * d - b * b
        det = (a * C00 + b * C01) + c * C02
        i = 1.0 / det
        out = np.stack([C00 * i, C01 * i, C02 * i, C01 * i, C11 * i, C12 * i, C02 * i, C12 * i, C22 * i], axis=1).reshape(-1, 3, 3)
    return out


def schur_terms(L, mu):
    """per point the terms T (N x 12 x 12) and r (N x 12) of the reduced system's sums, in the stated order, and Vi"""
    Vi = vinv(L["V"], mu)
    Wt = L["W"].reshape(-1, 12, 3)
    with np.errstate(all="ignore"):
        Y = (Wt[:, :, 0:1] * Vi[:, None, 0, :] + Wt[:, :, 1:2] * Vi[:, None, 1, :]) + Wt[:, :, 2:3] * Vi[:, None, 2, :]
        T = (Y[:, :, None, 0] * Wt[:, None, :, 0] + Y[:, :, None, 1] * Wt[:, None, :, 1]) + Y[:, :, None, 2] * Wt[:, None, :, 2]
        eb = L["eb"]
        r = (Y[:, :, 0] * eb[:, None, 0] + Y[:, :, 1] * eb[:, None, 1]) + Y[:, :, 2] * eb[:, None, 2]
    return T, r, Vi


def back_substitute(L, Vi, da):
    """db (N x 3) from a given da, in the stated order"""
    Wt = L["W"].reshape(-1, 12, 3)
    with np.errstate(all="ignore"):
        acc = Wt[:, 0, :] * da[0]
        for p in range(1, 12):
            acc = acc + Wt[:, p, :] * da[p]
        g = L["eb"] - acc
        return np.stack([(Vi[:, r, 0] * g[:, 0] + Vi[:, r, 1] * g[:, 1]) + Vi[:, r, 2] * g[:, 2] for r in range(3)], axis=1)


def moved(cams, da):
    out = np.array(cams, np.float64).copy()
    out[0, 9:15] = out[0, 9:15] + da[0:6]
    out[1, 9:15] = out[1, 9:15] + da[6:12]
    return out


# ------------------------------------------------------------------------------------------------- an independent Jacobian
def _quat_to_R(q):
    a, b, c, d = q
    return np.array([[a * a + b * b - c * c - d * d, 2 * (b * c - a * d), 2 * (b * d + a * c)],
                     [2 * (b * c + a * d), a * a - b * b + c * c - d * d, 2 * (c * d - a * b)],
                     [2 * (b * d - a * c), 2 * (c * d + a * b), a * a - b * b - c * c + d * d]])


def project_any(R0, v, t, M):
    """the projection from its definition, for real or complex arguments: the quaternion (sqrt(1 - v.v), v) as a matrix, times R0"""
    w = np.sqrt(1.0 - (v[0] * v[0] + v[1] * v[1] + v[2] * v[2]))
    X = _quat_to_R([w, v[0], v[1], v[2]]) @ (R0 @ M) + t
    return np.array([X[0] / X[2], X[1] / X[2]])


def jacobian_cs(cam, M, h=1e-30):
    """(A 2 x 6, B 2 x 3) of one camera at one point by complex-step differentiation"""
    cam = np.asarray(cam, np.float64)
    R0 = cam[:9].reshape(3, 3)
    x = np.concatenate([cam[9:15], M]).astype(complex)
    J = np.zeros((2, 9))
    for k in range(9):
        y = x.copy()
        y[k] += 1j * h
        J[:, k] = project_any(R0.astype(complex), y[0:3], y[3:6], y[6:9]).imag / h
    return J[:, :6], J[:, 6:]


def jacobian_fd(cam, M, h=1e-6):
    cam = np.asarray(cam, np.float64)
    R0 = cam[:9].reshape(3, 3)
    x = np.concatenate([cam[9:15], M])
    J = np.zeros((2, 9))
    for k in range(9):
        a, b = x.copy(), x.copy()
        a[k] += h
        b[k] -= h
        J[:, k] = (project_any(R0, a[0:3], a[3:6], a[6:9]) - project_any(R0, b[0:3], b[3:6], b[6:9])) / (2 * h)
    return J[:, :6], J[:, 6:]


# ------------------------------------------------------------------------------------------------------------------------- LM
def dense_jacobian(L):
    n = L["A"].shape[0]
    J = np.zeros((4 * n, 12 + 3 * n))
    for q in range(2):
        for r in range(2):
            J[2 * q + r::4, 6 * q:6 * q + 6] = L["A"][:, q, r]
            for k in range(3):
                J[2 * q + r::4, 12 + k::3][np.arange(n), np.arange(n)] = L["B"][:, q, r, k]
    return J


def solve_step(L, mu, damping="additive", fix_cam0=False):
    """(da 12, db N x 3) of (J'J + damping) dp = J'e, or None when the system cannot be solved"""
    n = L["A"].shape[0]
    e = L["res"].reshape(-1)
    with np.errstate(all="ignore"):
        if n <= DENSE_MAX:
            J = dense_jacobian(L)
            if fix_cam0:
                J = J[:, 6:]
            H, g = J.T @ J, J.T @ e
            H[np.diag_indices_from(H)] += mu if damping == "additive" else mu * np.diag(H)
            if not np.isfinite(H).all():
                return None
            try:
                np.linalg.cholesky(H)
                dp = np.linalg.solve(H, g)
            except np.linalg.LinAlgError:
                return None
            if fix_cam0:
                dp = np.concatenate([np.zeros(6), dp])
            return dp[:12], dp[12:].reshape(n, 3)
        U = np.zeros((12, 12))
        U[:6, :6], U[6:, 6:] = L["Ut"][:, 0].sum(0), L["Ut"][:, 1].sum(0)
        ea = L["eat"].sum(0)
        V = L["V"].copy()
        dU = np.diag(U).copy()
        if damping == "additive":
            U[np.diag_indices(12)] += mu
            V[:, [0, 1, 2], [0, 1, 2]] += mu
        else:
            U[np.diag_indices(12)] += mu * dU
            V[:, [0, 1, 2], [0, 1, 2]] *= 1.0 + mu
        if not (np.isfinite(V).all() and np.isfinite(U).all()):
            return None
        try:
            Vi = np.linalg.inv(V)
            Wt = L["W"].reshape(n, 12, 3)
            Y = Wt @ Vi
            S = U - np.einsum("npk,nqk->pq", Y, Wt)
            rhs = ea - np.einsum("npk,nk->p", Y, L["eb"])
            if fix_cam0:
                da = np.concatenate([np.zeros(6), np.linalg.solve(S[6:, 6:], rhs[6:])])
                np.linalg.cholesky(S[6:, 6:])
            else:
                np.linalg.cholesky(S)
                da = np.linalg.solve(S, rhs)
        except np.linalg.LinAlgError:
            return None
        db = np.einsum("nrk,nk->nr", Vi, L["eb"] - np.einsum("npk,p->nk", Wt, da))
        return da, db


def lm(cams, pts, obs, max_iters=1000, damping="additive", fix_cam0=False, tau=1e-3, eps=1e-12):
    """the rules of DESIGN.md ("Autocalibration"); returns (cams, pts, info)"""
    cams, pts = np.array(cams, np.float64).copy(), np.array(pts, np.float64).copy()
    mu, nu, stop, it, solves = 0.0, 2, 0, 0, 0
    err = err0 = float("nan")
    while it < max_iters and not stop:
        L = linearize(cams, pts, obs)
        err = float(L["e2"].sum())
        if it == 0:
            err0 = err
        if not np.isfinite(err):
            stop = 7
            break
        ea, U = L["eat"].sum(0), L["Ut"].sum(0)
        if fix_cam0:
            ea = ea.copy()
            ea[:6] = 0.0
        ginf = max(np.abs(ea).max(), np.abs(L["eb"]).max())
        if ginf <= eps:
            stop = 1
            break
        if err <= eps * eps:
            stop = 6
            break
        if it == 0:
            mu = tau * max(np.diag(U[0]).max(), np.diag(U[1]).max(), L["V"][:, [0, 1, 2], [0, 1, 2]].max())
        while True:
            solves += 1
            sol = solve_step(L, mu, damping, fix_cam0)
            if sol is not None and np.isfinite(sol[0]).all():
                da, db = sol
                dp2 = float((da * da).sum() + (db * db).sum())
                p2 = float((cams[:, 9:15] ** 2).sum() + (pts * pts).sum())
                if dp2 <= eps * eps * p2:
                    stop = 2
                    break
                if dp2 >= (p2 + eps) / 1e-24:
                    stop = 4
                    break
                cn, pn = moved(cams, da), pts + db
                errn = error(cn, pn, obs)
                if not np.isfinite(errn):
                    stop = 7
                    break
                dF = err - errn
                if damping == "additive":
                    dL = float((da * (mu * da + ea)).sum() + (db * (mu * db + L["eb"])).sum())
                else:
                    dL = float((da * (mu * np.concatenate([np.diag(U[0]), np.diag(U[1])]) * da + ea)).sum()
                               + (db * (mu * L["V"][:, [0, 1, 2], [0, 1, 2]] * db + L["eb"])).sum())
                if dL > 0.0 and dF > 0.0:
                    t = 2.0 * dF / dL - 1.0
                    mu *= max(1.0 - t * t * t, 1.0 / 3.0)
                    nu = 2
                    cams, pts, err = cn, pn, errn
                    break
            mu *= nu
            nu2 = (nu << 1) & 0xFFFFFFFF
            if nu2 <= nu or not np.isfinite(mu):
                stop = 5
                break
            nu = nu2
        it += 1
    if not stop:
        stop = 3
    return cams, pts, dict(err0=err0, err1=err, iters=it, reason=stop, mu=mu, solves=solves)


# ------------------------------------------------------------------------------------------------------------------------ pose
def choose_pose(counts, R4):
    best, best_n, best_r = -1, 0, 0.0
    for i in range(4):
        if counts[i] > best_n or (counts[i] == best_n and R4[i][0][0] > best_r):
            best, best_n, best_r = i, counts[i], R4[i][0][0]
    return best


def select_points(pts, mask):
    with np.errstate(invalid="ignore"):
        return np.asarray(mask, bool) & ~(pts[:, 2] < 0)


def cam_R(cam):
    return derived(cam)[5]


def relative_pose(cams):
    R0, R1 = cam_R(cams[0]), cam_R(cams[1])
    R = R1 @ R0.T
    T = R1 @ (-R0.T @ cams[0, 12:15]) + cams[1, 12:15]
    return R, T / np.linalg.norm(T)


def pose_distance(Ra, Ta, Rb, Tb):
    """the larger of |Ra - Rb| (Frobenius) and |Ta - Tb| of two unit-baseline poses"""
    return max(float(np.linalg.norm(Ra - Rb)), float(np.linalg.norm(np.ravel(Ta) - np.ravel(Tb))))


def make_cams(R0, T0, R1, T1, v0=(0, 0, 0), v1=(0, 0, 0)):
    return np.stack([np.concatenate([np.ravel(R0), v0, np.ravel(T0)]), np.concatenate([np.ravel(R1), v1, np.ravel(T1)])]).astype(np.float64)


def ba_scene(n, seed, noise=0.0, rot_deg=0.0, t_off=0.0):
    """(cams, pts, obs, R, T, extra): n points of the rig; observations with `noise` pixels of Gaussian noise; camera 1 started
    rot_deg off in rotation and t_off (a share of the baseline) off in translation; the points triangulated from the start pose"""
    the_rig = EO.rig(seed)
    K0, K1, R, T, _ = the_rig
    _, _, x0, x1, _ = EO.scene(the_rig, n, seed)
    rng = np.random.default_rng([seed, 303])
    if noise:
        x0 = x0 + rng.normal(0.0, noise / K0[0, 0], x0.shape)
        x1 = x1 + rng.normal(0.0, noise / K1[0, 0], x1.shape)
    axis = rng.normal(size=3)
    Rs = EO.rodrigues(np.deg2rad(rot_deg) * axis / np.linalg.norm(axis)) @ R
    Ts = T + t_off * rng.normal(size=3) / np.sqrt(3.0)
    pts = triangulate(Rs, Ts, x0, x1)
    return make_cams(np.eye(3), np.zeros(3), Rs, Ts), pts, np.concatenate([x0, x1], axis=1), R, T, dict(K0=K0, K1=K1, x0=x0, x1=x1)


# --------------------------------------------------------------------------------------------------- the independent minimiser
import functools


def scipy_minimum(cams, pts, obs):
    """scipy.optimize.least_squares (trust-region reflective, exact solves) on the same residuals: (cams, pts, cost)"""
    from scipy.optimize import least_squares
    n = pts.shape[0]

    def unpack(x):
        c = cams.copy()
        c[0, 9:15], c[1, 9:15] = x[0:6], x[6:12]
        return c, x[12:].reshape(n, 3)

    x0 = np.concatenate([cams[0, 9:15], cams[1, 9:15], pts.reshape(-1)])
    r = least_squares(lambda x: residuals(*unpack(x), obs).reshape(-1), x0, jac=lambda x: -dense_jacobian(linearize(*unpack(x), obs)), method="trf",
                      ftol=1e-15, xtol=1e-15, gtol=1e-15, max_nfev=2000)
    c, p = unpack(r.x)
    return c, p, 2.0 * float(r.cost)


NOISY_SEED, NOISY_PX, START_DEG, START_T = 3, 0.2, 1.0, 0.02


@functools.lru_cache(maxsize=None)
def noisy_case(n):
    """the noisy scene of n points with the oracle's minimum and, up to DENSE_MAX points, scipy's: dict(cams, pts, obs, R, T,
    oracle=(cams, pts, info), scipy_cost, scipy_pose, d_cost, d_pose); d_cost (relative) and d_pose are the oracle-versus-scipy
    differences, the yardstick of the GPU test.  Above DENSE_MAX points scipy's dense steps take 20 s: the yardstick is then the one
    of DENSE_MAX // 5 * 4 points and scipy_cost, scipy_pose are the oracle's."""
    cams, pts, obs, R, T, _ = ba_scene(n, NOISY_SEED, NOISY_PX, START_DEG, START_T)
    oc, op, info = lm(cams, pts, obs)
    Ro, To = relative_pose(oc)
    if n <= DENSE_MAX:
        sc, sp, cost = scipy_minimum(cams, pts, obs)
        Rs, Ts = relative_pose(sc)
        d_cost, d_pose = abs(cost - info["err1"]) / cost, pose_distance(Ro, To, Rs, Ts)
    else:
        small = noisy_case(DENSE_MAX // 5 * 4)
        cost, Rs, Ts, d_cost, d_pose = info["err1"], Ro, To, small["d_cost"], small["d_pose"]
    return dict(cams=cams, pts=pts, obs=obs, R=R, T=T, oracle=(oc, op, info), scipy_cost=cost, scipy_pose=(Rs, Ts), d_cost=d_cost, d_pose=d_pose)


@functools.lru_cache(maxsize=None)
def clean_case(n=120):
    """the noise-free scene started 1 degree and 2 % off: dict(cams, pts, obs, R, T, oracle, d_truth)"""
    cams, pts, obs, R, T, _ = ba_scene(n, NOISY_SEED, 0.0, START_DEG, START_T)
    oc, op, info = lm(cams, pts, obs)
    Ro, To = relative_pose(oc)
    return dict(cams=cams, pts=pts, obs=obs, R=R, T=T, oracle=(oc, op, info), d_truth=pose_distance(Ro, To, R, T))


# -------------------------------------------------------------------------------------------------------------- the whole chain
def pose_candidates(E):
    U, _, Vt = np.linalg.svd(E)
    U, Vt = (-U if np.linalg.det(U) < 0 else U), (-Vt if np.linalg.det(Vt) < 0 else Vt)
    W = np.array([[0.0, 1.0, 0.0], [-1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    R1, R2, t = U @ W @ Vt, U @ W.T @ Vt, U[:, 2]
    return np.stack([R1, R1, R2, R2]), np.stack([t, -t, t, -t])


def calibrate(p0, p1, K0, K1, samples):
    """the chain on the CPU from pooled pixel matches (float64) and a sample table: dict(code, R, T, before, after, n)"""
    x0, x1 = EO.normalise(p0, K0), EO.normalise(p1, K1)
    best = EO.find_essential(x0, x1, 1.5 / K0[0, 0], samples)
    E, mask = best["E"], best["mask"]
    R4, T4 = pose_candidates(E)
    pts4 = [triangulate(R4[k], T4[k], x0, x1) for k in range(4)]
    k = choose_pose([count_valid(p, mask) for p in pts4], R4)
    if k < 0:
        return dict(code=-1)
    keep = select_points(pts4[k], mask)
    if keep.sum() < 24:
        return dict(code=-1, n=int(keep.sum()))
    q0, q1 = p0[keep], p1[keep]
    before = EO.epipolar_error_stats(EO.fundamental(E, K0, K1), q0, q1)
    cams, _, info = lm(make_cams(np.eye(3), np.zeros(3), R4[k], T4[k]), pts4[k][keep], np.concatenate([x0[keep], x1[keep]], axis=1))
    R, T = relative_pose(cams)
    after = EO.epipolar_error_stats(EO.fundamental(EO.skew(T) @ R, K0, K1), q0, q1)
    return dict(code=0 if after[0] < before[0] else -1, R=R, T=T, before=before, after=after, n=int(keep.sum()), info=info)


E2E = dict(rig_seed=4, frames=3, m=40, noise=0.3, rounds=64)


def e2e_frames():
    """(K0, K1, R, T, [(p0, p1) float32 per frame]) of the end-to-end test"""
    the_rig = EO.rig(E2E["rig_seed"])
    K0, K1, R, T, _ = the_rig
    return K0, K1, R, T, [EO.scene(the_rig, E2E["m"], 50 + f, noise=E2E["noise"])[:2] for f in range(E2E["frames"])]


def v_to_one_case(n=65):
    """a hand-made start: camera 1's local rotation already at |v| = 0.97 (R0 chosen so that the pose is the scene's, turned 0.6 rad
    about the axis of v): the first step asks for |v| > 1"""
    cams, pts, obs, _, _, _ = ba_scene(n, 7, noise=0.2, rot_deg=0.5, t_off=0.01)
    Rs = cams[1, :9].reshape(3, 3).copy()
    cams[1, 9:12] = [0.0, 0.97, 0.0]
    cams[1, :9] = np.eye(3).ravel()
    cams[1, :9] = (cam_R(cams[1]).T @ EO.rodrigues(np.array([0.0, -0.6, 0.0])) @ Rs).ravel()
    return cams, pts, obs


REJECT = dict(rig_seed=1, seed=109, frames=3, m=10, noise=1.0, rounds=64)


def reject_frames():
    """a scene on which the bundle adjustment does not lower the epipolar error: 30 matches with 1 px of noise; the essential matrix
    of 64 samples already has the lower symmetric epipolar distance in pixels, and the minimum of the reprojection error in
    normalised coordinates lies 7 % above it (tests/test_autocal.py holds the oracle to that)"""
    the_rig = EO.rig(REJECT["rig_seed"])
    K0, K1, R, T, _ = the_rig
    a, b = EO.scene(the_rig, REJECT["frames"] * REJECT["m"], REJECT["seed"], noise=REJECT["noise"])[:2]
    m = REJECT["m"]
    return K0, K1, R, T, [(a[f * m:(f + 1) * m], b[f * m:(f + 1) * m]) for f in range(REJECT["frames"])]
