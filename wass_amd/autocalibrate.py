"""wass_autocalibrate on the GPU (src/wass_autocalibrate/wass_autocalibrate.cpp, sba_driver.cpp): the matches_epionly.txt of many
frames are pooled, one essential matrix is found over all of them (epipolar.find_essential), one of its four poses is chosen by
triangulating every match (csrc/autocal.hip), a bundle adjustment of the two cameras and the points refines it (csrc/autocal.hip:
one thread per point, the Levenberg-Marquardt loop on the host), and ext_R.xml, ext_T.xml and H.xml are written into every
workspace when the epipolar error went down.

    python -m wass_amd.autocalibrate WORKSPACES_FILE

A camera of the bundle adjustment is 15 numbers: R0 (9, the fixed initial rotation), v (3, the vector part of the unit quaternion
(sqrt(1 - |v|^2), v) multiplied onto it) and t (3); its rotation is R(v) R0.  sba's loop and cv::findHomography are restated from
knowledge: DESIGN.md section 8, items 31 onwards.  There is no CPU path: without the library or a GPU every function that runs a
kernel raises.
"""
from __future__ import annotations

import ctypes as C
import os
import sys
from dataclasses import dataclass

import numpy as np

from . import epipolar, gridding
from .epipolar import ROUNDS, epipolar_error_stats, write_opencv_matrix
from .match import _context

LIN_ROWS = 49            # WASS_AC_LIN_ROWS
LIN_SUMS = 57            # WASS_AC_LIN_SUMS
MAX_N = 1 << 22          # WASS_AC_MAX_N
MIN_MATCHES = 8          # wass_autocalibrate.cpp:165
MIN_POINTS = 24          # wass_autocalibrate.cpp:284
STOP_REASONS = {1: "small gradient", 2: "small step", 3: "iterations", 4: "step too large", 5: "damping overflow", 6: "small error",
                7: "not finite"}


@dataclass
class Linearization:
    """ba_linearize's result.  Per point: res (N x 4: ex0 ey0 ex1 ey1), V (N x 3 x 3), eb (N x 3), W (N x 2 x 6 x 3).  Reduced: U (2 x
    6 x 6), ea (12), err = |e|^2, grad_pts = max |eb| and diag_pts = max diag V."""
    res: np.ndarray
    V: np.ndarray
    eb: np.ndarray
    W: np.ndarray
    U: np.ndarray
    ea: np.ndarray
    err: float
    grad_pts: float
    diag_pts: float


@dataclass
class Step:
    """ba_step's result: ok (False: the factorisation failed, a rejected step), da (12), db (N x 3), err (|e|^2 at the candidate), dL,
    and S (12 x 12), rhs (12) of the reduced system, cams and pts of the candidate, dp2 = |dp|^2 and p2 = |p|^2"""
    ok: bool
    da: np.ndarray
    db: np.ndarray
    err: float
    dL: float
    S: np.ndarray
    rhs: np.ndarray
    cams: np.ndarray
    pts: np.ndarray
    dp2: float
    p2: float


@dataclass
class BAResult:
    R0: np.ndarray
    T0: np.ndarray
    R1: np.ndarray
    T1: np.ndarray
    pts: np.ndarray
    iters: int
    reason: int
    err0: float
    err1: float


# ---------------------------------------------------------------------------------------------------------------------- checks
def _doubles(a, n):
    a = np.ascontiguousarray(np.asarray(a, np.float64).reshape(-1))
    if a.shape[0] != n:
        raise ValueError(f"{a.shape[0]} numbers where {n} are expected")
    return a


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _problem(cams, pts, obs):
    cams = np.ascontiguousarray(np.asarray(cams, np.float64))
    if cams.shape != (2, 15):
        raise ValueError("cameras are 2 x 15: R0, v, t")
    pts, obs = np.ascontiguousarray(np.asarray(pts, np.float64)), np.ascontiguousarray(np.asarray(obs, np.float64))
    if pts.ndim != 2 or pts.shape[1] != 3 or obs.shape != (pts.shape[0], 4):
        raise ValueError("points are N x 3 and observations N x 4")
    if not 1 <= pts.shape[0] <= MAX_N:
        raise ValueError(f"{pts.shape[0]} points: 1 .. {MAX_N}")
    return cams, pts, obs


def make_cams(R0, T0, R1, T1, v0=(0.0, 0.0, 0.0), v1=(0.0, 0.0, 0.0)) -> np.ndarray:
    """the 2 x 15 camera array of the kernels"""
    return np.stack([np.concatenate([_doubles(R0, 9), _doubles(v0, 3), _doubles(T0, 3)]),
                     np.concatenate([_doubles(R1, 9), _doubles(v1, 3), _doubles(T1, 3)])])


def cam_rotation(cam) -> np.ndarray:
    """R(v) R0 of one camera, in the order include/wass_gpu.h states"""
    cam = _doubles(cam, 15)
    R0, v = cam[:9].reshape(3, 3), cam[9:12]
    s = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]
    with np.errstate(invalid="ignore"):
        w = np.sqrt(1.0 - s)
    vx = np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])
    I = np.eye(3)
    Rl = I + 2.0 * (w * vx + (np.outer(v, v) - s * I))
    return np.stack([(Rl[r, 0] * R0[0] + Rl[r, 1] * R0[1]) + Rl[r, 2] * R0[2] for r in range(3)])


def wass_ac_scratch_bytes(n: int) -> int:
    """device memory the context keeps for a bundle adjustment of n points (no GPU needed)"""
    from . import _lib
    return _lib.scratch_bytes("ac", (int(n),), f"n = {n}: 1 .. {MAX_N} points")


# --------------------------------------------------------------------------------------------------------------------- kernels
def pose_candidates(E):
    """decomposeEssentialMat as epipolar.recover_pose does it, the candidates in wass_autocalibrate's order (R1, t) (R1, -t) (R2, t)
    (R2, -t): (R4 4 x 3 x 3, T4 4 x 3)"""
    E = np.asarray(E, np.float64)
    if E.shape != (3, 3):
        raise ValueError("a model is 3 x 3")
    U, _, Vt = np.linalg.svd(E)
    if np.linalg.det(U) < 0:
        U = -U
    if np.linalg.det(Vt) < 0:
        Vt = -Vt
    W = np.array([[0.0, 1.0, 0.0], [-1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    R1, R2, t = U @ W @ Vt, U @ W.T @ Vt, U[:, 2].copy()
    return np.stack([R1, R1, R2, R2]), np.stack([t, -t, t, -t])


def triangulate_candidates(R4, T4, x0, x1, mask, ctx=None):
    """k_ac_triangulate: (pts 4 x M x 3, counts int32 4): per candidate and match the least-squares point of the two rays, per
    candidate the matches with mask set and z > 1"""
    R4, T4 = _doubles(R4, 36), _doubles(T4, 12)
    a, b = np.ascontiguousarray(np.asarray(x0, np.float64)), np.ascontiguousarray(np.asarray(x1, np.float64))
    if a.ndim != 2 or a.shape[1] != 2 or a.shape != b.shape or not 1 <= a.shape[0] <= MAX_N:
        raise ValueError(f"matches are two M x 2 arrays of normalised points, 1 .. {MAX_N} of them")
    mk = np.ascontiguousarray(np.asarray(mask).reshape(-1) != 0).astype(np.uint8)
    if mk.shape[0] != a.shape[0]:
        raise ValueError("one mask entry per match")
    import torch
    ctx = _context(ctx)
    dev = torch.device("cuda", ctx.device_id)
    d0, d1, dm = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev), torch.from_numpy(mk).to(dev)
    d_p = torch.empty((4, a.shape[0], 3), dtype=torch.float64, device=dev)
    counts = (C.c_int32 * 4)()
    torch.cuda.synchronize()
    ctx._check(ctx._lib.wass_ac_triangulate_dev(ctx._h, d0.data_ptr(), d1.data_ptr(), dm.data_ptr(), a.shape[0], _dp(R4), _dp(T4), d_p.data_ptr(),
                                                counts))
    return d_p.cpu().numpy(), np.array(list(counts), np.int32)


def choose_pose(counts, R4) -> int:
    """wass_autocalibrate.cpp:198-220: the largest count; equal counts go to the larger R[0, 0]; both start at 0, so a candidate
    without a valid point and without a positive R[0, 0] is never taken.  -1: none was."""
    best, best_n, best_r = -1, 0, 0.0
    for i in range(4):
        n, r = int(counts[i]), float(np.asarray(R4)[i][0][0])
        if n > best_n or (n == best_n and r > best_r):
            best, best_n, best_r = i, n, r
    return best


def _upload(ctx, pts, obs):
    import torch
    dev = torch.device("cuda", ctx.device_id)
    return torch, dev, torch.from_numpy(pts).to(dev), torch.from_numpy(obs).to(dev)


def ba_linearize(cams, pts, obs, ctx=None) -> Linearization:
    """k_ac_linearize at (cams, pts): residuals, the blocks of J'J and J'e"""
    cams, pts, obs = _problem(cams, pts, obs)
    ctx = _context(ctx)
    torch, dev, d_p, d_o = _upload(ctx, pts, obs)
    n = pts.shape[0]
    d_l = torch.empty((LIN_ROWS, n), dtype=torch.float64, device=dev)
    sums = np.zeros(LIN_SUMS)
    torch.cuda.synchronize()
    ctx._check(ctx._lib.wass_ac_linearize_dev(ctx._h, _dp(cams), d_p.data_ptr(), d_o.data_ptr(), n, d_l.data_ptr(), _dp(sums)))
    lin = d_l.cpu().numpy()
    V = np.empty((n, 3, 3))
    for r, (a, b) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
        V[:, a, b] = V[:, b, a] = lin[4 + r]
    U = np.zeros((2, 6, 6))
    for q in range(2):
        for a in range(6):
            for b in range(a + 1):
                U[q, a, b] = U[q, b, a] = sums[21 * q + a * (a + 1) // 2 + b]
    return Linearization(lin[0:4].T.copy(), V, lin[10:13].T.copy(), lin[13:49].T.reshape(n, 2, 6, 3).copy(), U, sums[42:54].copy(), float(sums[54]),
                         float(sums[55]), float(sums[56]))


def ba_step(cams, pts, obs, mu, ctx=None) -> Step:
    """one Schur step at the damping mu: the reduced 12 x 12 system, its Cholesky solve, the back-substitution and the candidate's
    error"""
    cams, pts, obs = _problem(cams, pts, obs)
    ctx = _context(ctx)
    torch, dev, d_p, d_o = _upload(ctx, pts, obs)
    n = pts.shape[0]
    d_db = torch.zeros((n, 3), dtype=torch.float64, device=dev)
    d_pn = d_p.clone()
    S, rhs, da, cn, scal = np.zeros((12, 12)), np.zeros(12), np.zeros(12), np.zeros((2, 15)), np.zeros(4)
    ok = C.c_int(0)
    torch.cuda.synchronize()
    ctx._check(ctx._lib.wass_ac_step_dev(ctx._h, _dp(cams), d_p.data_ptr(), d_o.data_ptr(), n, float(mu), _dp(S), _dp(rhs), _dp(da), d_db.data_ptr(),
                                         d_pn.data_ptr(), _dp(cn), _dp(scal), C.byref(ok)))
    return Step(bool(ok.value), da, d_db.cpu().numpy(), float(scal[0]), float(scal[3]), S, rhs, cn, d_pn.cpu().numpy(), float(scal[1]), float(scal[2]))


def ba_error(cams, pts, obs, ctx=None, residuals: bool = False):
    """|e|^2 at (cams, pts); with residuals=True also the N x 4 residuals"""
    cams, pts, obs = _problem(cams, pts, obs)
    ctx = _context(ctx)
    torch, dev, d_p, d_o = _upload(ctx, pts, obs)
    n = pts.shape[0]
    d_r = torch.empty((4, n), dtype=torch.float64, device=dev) if residuals else None
    err = np.zeros(1)
    torch.cuda.synchronize()
    ctx._check(ctx._lib.wass_ac_error_dev(ctx._h, _dp(cams), d_p.data_ptr(), d_o.data_ptr(), n, d_r.data_ptr() if residuals else None, _dp(err)))
    return (float(err[0]), d_r.cpu().numpy().T.copy()) if residuals else float(err[0])


def bundle_adjust_cams(cams, pts, obs, max_iters: int = 1000, ctx=None):
    """the Levenberg-Marquardt loop from any start: (cams 2 x 15, pts N x 3, info) with info = dict(err0, err1, iters, reason, mu,
    grad, dp2, solves); the parameters are those of the last accepted step"""
    cams, pts, obs = _problem(cams, pts, obs)
    ctx = _context(ctx)
    torch, dev, d_p, d_o = _upload(ctx, pts, obs)
    cams, info = cams.copy(), np.zeros(8)
    torch.cuda.synchronize()
    ctx._check(ctx._lib.wass_ac_bundle_dev(ctx._h, _dp(cams), d_p.data_ptr(), d_o.data_ptr(), pts.shape[0], int(max_iters), _dp(info)))
    return cams, d_p.cpu().numpy(), dict(err0=float(info[0]), err1=float(info[1]), iters=int(info[2]), reason=int(info[3]), mu=float(info[4]),
                                         grad=float(info[5]), dp2=float(info[6]), solves=int(info[7]))


def bundle_adjust(R, T, pts3d, x0, x1, max_iters: int = 1000, ctx=None) -> BAResult:
    """sba_driver: camera 0 starts at the identity, camera 1 at (R, T), both free; x0, x1 are the normalised observations"""
    cams = make_cams(np.eye(3), np.zeros(3), R, T)
    obs = np.concatenate([np.asarray(x0, np.float64).reshape(-1, 2), np.asarray(x1, np.float64).reshape(-1, 2)], axis=1)
    cams, pts, info = bundle_adjust_cams(cams, pts3d, obs, max_iters, ctx)
    return BAResult(cam_rotation(cams[0]), cams[0, 12:15].copy(), cam_rotation(cams[1]), cams[1, 12:15].copy(), pts, info["iters"], info["reason"],
                    info["err0"], info["err1"])


# ------------------------------------------------------------------------------------------------------------------------ host
def relative_pose(R0, T0, R1, T1):
    """wass_autocalibrate.cpp:330-335: R = R1 R0', T = R1 (-R0' T0) + T1, T / |T|"""
    R0, R1 = np.asarray(R0, np.float64), np.asarray(R1, np.float64)
    R0i = R0.T
    T0i = -R0i @ np.asarray(T0, np.float64).reshape(3)
    R = R1 @ R0i
    T = R1 @ T0i + np.asarray(T1, np.float64).reshape(3)
    return R, T / np.linalg.norm(T)


def skew(t):
    return np.array([[0.0, -t[2], t[1]], [t[2], 0.0, -t[0]], [-t[1], t[0], 0.0]])


def fundamental(E, K0, K1):
    return np.linalg.inv(np.asarray(K1, np.float64)).T @ np.asarray(E, np.float64) @ np.linalg.inv(np.asarray(K0, np.float64))


def structure_error_stats(pts3d, p0, p1, R, T, K0, K1):
    """evaluate_structure_error (epipolar.cpp:42-80): per point half the sum of the two reprojection distances in pixels; (avg, std,
    min, max) with sequential sums and the population standard deviation"""
    P = np.asarray(pts3d, np.float64).reshape(-1, 3)
    p0, p1 = np.asarray(p0, np.float64).reshape(-1, 2), np.asarray(p1, np.float64).reshape(-1, 2)
    n = P.shape[0]
    big = float(np.finfo(np.float64).max)
    if n == 0:
        return float("nan"), float("nan"), big, -big
    with np.errstate(all="ignore"):
        a = P @ np.asarray(K0, np.float64).T
        b = (P @ np.asarray(R, np.float64).T + np.asarray(T, np.float64).reshape(3)) @ np.asarray(K1, np.float64).T
        a, b = a / a[:, 2:3], b / b[:, 2:3]
        e = 0.5 * (np.sqrt(((a[:, :2] - p0) ** 2).sum(1)) + np.sqrt(((b[:, :2] - p1) ** 2).sum(1)))
    avg = 0.0
    for v in e.tolist():
        avg += v
    avg /= float(n)
    var = 0.0
    for v in e.tolist():
        var += (v - avg) * (v - avg)
    return avg, float(np.sqrt(var / n)), float(e.min()), float(e.max())


def _hartley(p):
    c = p.mean(0)
    d = np.abs(p - c).mean(0)
    s = 1.0 / np.where(d > 0, d, 1.0)
    return np.array([[s[0], 0.0, -s[0] * c[0]], [0.0, s[1], -s[1] * c[1]], [0.0, 0.0, 1.0]])


def homography_lsq(p0, p1, steps: int = 10) -> np.ndarray:
    """cv::findHomography(p0, p1, 0) from knowledge: the DLT on points normalised per axis (centroid to the origin, mean absolute
    deviation to 1), the eigenvector of the smallest eigenvalue of L'L, then Gauss-Newton steps on the reprojection error in
    picture 1 over the eight parameters of H / H[2, 2]; a step that does not lower the error ends the refinement."""
    p0, p1 = np.asarray(p0, np.float64).reshape(-1, 2), np.asarray(p1, np.float64).reshape(-1, 2)
    if p0.shape != p1.shape or p0.shape[0] < 4:
        raise ValueError("at least four pairs of points")
    T0, T1 = _hartley(p0), _hartley(p1)
    a = p0 * [T0[0, 0], T0[1, 1]] + [T0[0, 2], T0[1, 2]]
    b = p1 * [T1[0, 0], T1[1, 1]] + [T1[0, 2], T1[1, 2]]
    n = a.shape[0]
    z, o = np.zeros(n), np.ones(n)
    L = np.concatenate([np.stack([a[:, 0], a[:, 1], o, z, z, z, -b[:, 0] * a[:, 0], -b[:, 0] * a[:, 1], -b[:, 0]], axis=1),
                        np.stack([z, z, z, a[:, 0], a[:, 1], o, -b[:, 1] * a[:, 0], -b[:, 1] * a[:, 1], -b[:, 1]], axis=1)])
    h = np.linalg.eigh(L.T @ L)[1][:, 0]
    H = np.linalg.inv(T1) @ h.reshape(3, 3) @ T0
    H = H / H[2, 2]

    def residual(h8):
        Hm = np.append(h8, 1.0).reshape(3, 3)
        q = np.concatenate([p0, np.ones((n, 1))], axis=1) @ Hm.T
        return (q[:, :2] / q[:, 2:3] - p1), q

    h8 = H.reshape(-1)[:8].copy()
    r, q = residual(h8)
    cost = float((r * r).sum())
    for _ in range(int(steps)):
        iw = 1.0 / q[:, 2]
        u, v = q[:, 0] * iw, q[:, 1] * iw
        x, y = p0[:, 0], p0[:, 1]
        Jx = np.stack([x * iw, y * iw, iw, z, z, z, -x * u * iw, -y * u * iw], axis=1)
        Jy = np.stack([z, z, z, x * iw, y * iw, iw, -x * v * iw, -y * v * iw], axis=1)
        J = np.concatenate([Jx, Jy])
        try:
            d = np.linalg.solve(J.T @ J, -J.T @ np.concatenate([r[:, 0], r[:, 1]]))
        except np.linalg.LinAlgError:
            break
        r2, q2 = residual(h8 + d)
        c2 = float((r2 * r2).sum())
        if not c2 < cost:
            break
        h8, r, q, cost = h8 + d, r2, q2, c2
    return np.append(h8, 1.0).reshape(3, 3)


# ----------------------------------------------------------------------------------------------------------------------- files
def load_workspaces(list_file):
    """the whitespace-separated tokens of the list file that are existing directories"""
    with open(os.fspath(list_file)) as f:
        return [t for t in f.read().split() if os.path.isdir(t)]


def _read_matches64(path):
    with open(path) as fh:
        tok = fh.read().split()
    m = int(tok[0])
    v = np.array(tok[1:1 + 4 * m], np.float64).reshape(m, 4)
    return v[:, 0:2].copy(), v[:, 2:4].copy()


def pool_matches(workdirs):
    """(p0, p1, x0, x1, K0, K1): every workspace's matches_epionly.txt as float64 pixels, and normalised with the full inverse of the
    first workspace's intrinsics.  A workspace without the file is skipped with a message."""
    K0 = K1 = None
    a, b = [np.zeros((0, 2))], [np.zeros((0, 2))]
    for wd in workdirs:
        if K0 is None:
            K0 = gridding.read_opencv_matrix(os.path.join(wd, "intrinsics_00000000.xml"), "intr")
            K1 = gridding.read_opencv_matrix(os.path.join(wd, "intrinsics_00000001.xml"), "intr")
        try:
            pa, pb = _read_matches64(os.path.join(wd, "matches_epionly.txt"))
        except OSError:
            print(f"wass_amd.autocalibrate: unable to load matches from {os.path.join(wd, 'matches_epionly.txt')}, skipping", file=sys.stderr)
            continue
        a.append(pa)
        b.append(pb)
    p0, p1 = np.concatenate(a), np.concatenate(b)
    if K0 is None:
        return p0, p1, np.zeros((0, 2)), np.zeros((0, 2)), None, None
    return p0, p1, _normalise(p0, K0), _normalise(p1, K1), np.asarray(K0, np.float64), np.asarray(K1, np.float64)


def _normalise(px, K):
    Ki = np.linalg.inv(np.asarray(K, np.float64))
    return np.ascontiguousarray((np.concatenate([px, np.ones((px.shape[0], 1))], axis=1) @ Ki.T)[:, :2])


def select_points(pts, mask):
    """wass_autocalibrate.cpp:258-279: the matches with mask set whose point is not behind camera 0 (z < 0 is dropped; -0.0 and NaN
    stay), in match order"""
    with np.errstate(invalid="ignore"):
        return np.asarray(mask, bool) & ~(np.asarray(pts)[:, 2] < 0)


@dataclass
class Calibration:
    """autocalibrate's result; code 0 on success, -1 otherwise (then R, T, H may be None)"""
    code: int
    R: np.ndarray = None
    T: np.ndarray = None
    H: np.ndarray = None
    err_before: tuple = None
    err_after: tuple = None
    structure: tuple = None
    ba: BAResult = None
    n_points: int = 0


def autocalibrate(p0, p1, x0, x1, K0, K1, rounds: int = ROUNDS, ctx=None, progress=None) -> Calibration:
    """everything between the pooled matches and the files"""
    say = (lambda s: None) if progress is None else progress
    if p0.shape[0] < MIN_MATCHES:
        print("wass_amd.autocalibrate: not enough matches to continue", file=sys.stderr)
        return Calibration(-1)
    best = epipolar.find_essential(x0, x1, 1.5 / K0[0, 0], rounds, None, ctx)
    R4, T4 = pose_candidates(best.E)
    pts4, counts = triangulate_candidates(R4, T4, x0, x1, best.mask, ctx)
    k = choose_pose(counts, R4)
    if k < 0:
        print("wass_amd.autocalibrate: no pose candidate has a valid point", file=sys.stderr)
        return Calibration(-1)
    R, T = R4[k], T4[k]
    keep = select_points(pts4[k], best.mask)
    n = int(keep.sum())
    if n < MIN_POINTS:
        print("wass_amd.autocalibrate: too few inlier points for the bundle adjustment", file=sys.stderr)
        return Calibration(-1, n_points=n)
    q0, q1, y0, y1, P = p0[keep], p1[keep], x0[keep], x1[keep], pts4[k][keep]
    structure = structure_error_stats(P, q0, q1, R, T, K0, K1)
    before = epipolar_error_stats(fundamental(best.E, K0, K1), q0, q1)
    say("[P|70|100]")
    ba = bundle_adjust(R, T, P, y0, y1, 1000, ctx)
    R, T = relative_pose(ba.R0, ba.T0, ba.R1, ba.T1)
    after = epipolar_error_stats(fundamental(skew(T) @ R, K0, K1), q0, q1)
    H = homography_lsq(q0, q1)
    if not after[0] < before[0]:
        print("wass_amd.autocalibrate: SBA failed.", file=sys.stderr)
        return Calibration(-1, R, T.reshape(3, 1), H, before, after, structure, ba, n)
    return Calibration(0, R, T.reshape(3, 1), H, before, after, structure, ba, n)


def autocalibrate_workdirs(list_file, rounds: int = ROUNDS, ctx=None) -> int:
    """The file-level entry: pools the workspaces the list file names, calibrates and, on success, writes ext_R.xml, ext_T.xml and
    H.xml into every workspace.  Returns 0, or -1 for an unreadable list, too few matches or points, or a bundle adjustment that
    did not lower the epipolar error; then nothing is written."""
    try:
        workdirs = load_workspaces(list_file)
    except OSError as ex:
        print(f"wass_amd.autocalibrate: unable to load {list_file}: {ex}", file=sys.stderr)
        return -1
    say = lambda s: print(s, flush=True)      # noqa: E731
    say("[P|20|100]")
    try:
        p0, p1, x0, x1, K0, K1 = pool_matches(workdirs)
    except (OSError, ValueError, IndexError) as ex:
        print(f"wass_amd.autocalibrate: {ex}", file=sys.stderr)
        return -1
    say("[P|50|100]")
    r = autocalibrate(p0, p1, x0, x1, K0, K1, rounds, ctx, say)
    if r.code != 0:
        return -1
    for wd in workdirs:
        write_opencv_matrix(os.path.join(wd, "ext_R.xml"), "ext_R", r.R)
        write_opencv_matrix(os.path.join(wd, "ext_T.xml"), "ext_T", r.T)
        write_opencv_matrix(os.path.join(wd, "H.xml"), "H", r.H)
    say("[P|100|100]")
    return 0


def main(argv=None) -> int:
    argv = sys.argv[1:] if argv is None else list(argv)
    if len(argv) == 0:
        print("usage: python -m wass_amd.autocalibrate WORKSPACES_FILE")
        return 0
    if len(argv) != 1:
        print("Invalid arguments", file=sys.stderr)
        return -1
    return autocalibrate_workdirs(argv[0])


if __name__ == "__main__":
    sys.exit(main())
