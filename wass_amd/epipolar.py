"""The essential-matrix filter of wass_match on the GPU (src/wass_match/wass_match.cpp:250-358, src/wass_lib/epipolar.cpp:7-39): from
matches_unfiltered.txt to matches_epionly.txt, matches.txt, matcher_stats.csv, ext_R.xml and ext_T.xml.

The kernels (csrc/epipolar.hip) solve the five-point problem of every sample, score every model against every match and pick the
best one, for several pairs of pictures in one chain of launches; the host keeps what is small: the sample table (cv::RNG and
getSubset's redraw loop, restated), cv::recoverPose (one 3 x 3 SVD per pair and four tiny triangulations per match) and the
statistics.  OpenCV's parts are restated from knowledge: DESIGN.md section 8, items 22 onwards.

Conventions (wass_match.cpp:252-280): x0 = K0^-1 (u0, v0, 1), x1 = K1^-1 (u1, v1, 1), x1' E x0 = 0, the threshold is
t = max_epi_distance / ((K0[0, 0] + K0[1, 1]) / 2), F = K1^-T E K0^-1.

Host arrays are numpy, device arrays torch tensors passed by raw pointer.  There is no CPU path: without the library or a GPU
every function that runs a kernel raises.
"""
from __future__ import annotations

import ctypes as C
import functools
import os
import sys
from dataclasses import dataclass

import numpy as np

from . import gridding
from . import match as _match
from .match import MatchResult, _context, _ints

MAX_SOL = 10             # WASS_EPI_MAX_SOL
MAX_ROUNDS = 65536       # WASS_EPI_MAX_ROUNDS
MAX_M = 1 << 22          # WASS_EPI_MAX_M
ROUNDS = 1024            # the smallest multiple of the workgroup above the reference's cap of 1000 iterations
RNG_STATE = 2 ** 64 - 1  # cv::RNG rng((uint64)-1) of RANSACPointSetRegistrator::run


@dataclass
class Essential:
    """find_essential's result: E (3 x 3, Frobenius norm 1), mask (bool M) and err (float32 M, the squared Sampson distances) of the
    best model, count = mask.sum(), and where it came from: sample (row of the table) and solution (0 .. 9); -1 when no sample
    gave a solution (then E is zero)"""
    E: np.ndarray
    mask: np.ndarray
    err: np.ndarray
    count: int
    sample: int
    solution: int


@dataclass
class EpipolarResult:
    """epipolar_filter's result.  E, F: 3 x 3; mask_epi: the inliers of E (matches_epionly.txt); mask: those that also pass
    recoverPose's test (matches.txt); R, T: ext_R, ext_T (T a 3 x 1 column of norm 1); stats: (avg, std, min, max) of the
    epipolar error in pixels over `mask`; best: the Essential record"""
    E: np.ndarray
    F: np.ndarray
    mask_epi: np.ndarray
    mask: np.ndarray
    R: np.ndarray
    T: np.ndarray
    stats: tuple
    threshold: float
    best: Essential


# --------------------------------------------------------------------------------------------------------------------- samples
def ransac_samples(m: int, rounds: int = ROUNDS, state: int = RNG_STATE) -> np.ndarray:
    """rounds x 5 int32, five distinct indices below m per row: cv::RNG (multiply-with-carry, state = (uint32)state * 4164903690 +
    (state >> 32), the low word is the draw) with uniform(0, m) = next() % m, and RANSACPointSetRegistrator::getSubset's loop,
    which draws an index again while it repeats an earlier one of its row.  One stream through all rows: the table of fewer rounds
    is a prefix.  There is no adaptive stop: the best of all rounds dominates the best of any prefix."""
    m, rounds = int(m), int(rounds)
    if m < 5:
        raise ValueError(f"{m} matches: five distinct ones are needed")
    if rounds < 1:
        raise ValueError(f"rounds = {rounds}: at least one")
    return _sample_table(m, rounds, int(state) & (2 ** 64 - 1)).copy()


@functools.lru_cache(maxsize=64)
def _sample_table(m: int, rounds: int, s: int) -> np.ndarray:
    """the table depends on (m, rounds, state) alone: the pairs of a sequence share it"""
    out = np.empty((rounds, 5), np.int32)
    for r in range(rounds):
        row = []
        while len(row) < 5:
            s = (s & 0xFFFFFFFF) * 4164903690 + (s >> 32)
            j = (s & 0xFFFFFFFF) % m
            if j not in row:
                row.append(j)
        out[r] = row
    return out


# ---------------------------------------------------------------------------------------------------------------------- checks
def _points(x0, x1):
    a, b = np.asarray(x0, np.float64), np.asarray(x1, np.float64)
    if a.ndim != 2 or a.shape[1] != 2 or a.shape != b.shape:
        raise ValueError("matches are two M x 2 arrays of normalised points")
    if a.shape[0] < 5:
        raise ValueError(f"{a.shape[0]} matches: at least five")
    if a.shape[0] > MAX_M:
        raise ValueError(f"{a.shape[0]} matches: at most {MAX_M}")
    return np.ascontiguousarray(a), np.ascontiguousarray(b)


def _samples(samples, m):
    s = np.asarray(samples)
    if s.ndim != 2 or s.shape[1] != 5 or s.shape[0] < 1 or not np.issubdtype(s.dtype, np.integer):
        raise ValueError("samples are an R x 5 integer array with R >= 1")
    if s.shape[0] > MAX_ROUNDS:
        raise ValueError(f"{s.shape[0]} samples: at most {MAX_ROUNDS}")
    if s.min() < 0 or s.max() >= m:
        raise ValueError("a sample names a match outside the pair")
    return np.ascontiguousarray(s, np.int32)


def _threshold(t):
    t = float(t)
    if not t >= 0.0:
        raise ValueError(f"threshold = {t}: a distance, not negative")
    return t


def _models(E):
    e = np.asarray(E, np.float64)
    if e.shape == (3, 3):
        e = e[None]
    if e.ndim != 3 or e.shape[1:] != (3, 3) or e.shape[0] < 1:
        raise ValueError("models are K x 3 x 3")
    if e.shape[0] > MAX_ROUNDS * MAX_SOL:
        raise ValueError(f"{e.shape[0]} models: at most {MAX_ROUNDS * MAX_SOL}")
    return np.ascontiguousarray(e)


def _doubles(v):
    return (C.c_double * len(v))(*[float(t) for t in v])


def _upload(pairs, dev):
    """the points of several pairs side by side, padded to the largest: two B x Mmax x 2 tensors, the sizes, the stride"""
    import torch
    ms = [a.shape[0] for a, _ in pairs]
    mmax = max(ms)
    h0, h1 = np.zeros((len(pairs), mmax, 2)), np.zeros((len(pairs), mmax, 2))
    for p, (a, b) in enumerate(pairs):
        h0[p, :ms[p]], h1[p, :ms[p]] = a, b
    return torch.from_numpy(h0).to(dev), torch.from_numpy(h1).to(dev), ms, 2 * mmax


def scratch_bytes(batch: int, rounds: int = ROUNDS) -> int:
    """device memory the context keeps for find_essential over `batch` pairs of `rounds` samples (no GPU needed)"""
    from . import _lib
    return _lib.scratch_bytes("epi", (int(batch), int(rounds)), f"batch = {batch}, rounds = {rounds}: 1 .. 65535 pairs of 1 .. {MAX_ROUNDS} samples")


# --------------------------------------------------------------------------------------------------------------------- kernels
def five_point(x0, x1, samples, ctx=None):
    """k_epi_solve5 on its own: for every sample (R x 5 indices) up to ten essential matrices.  Returns (E float64 R x 10 x 3 x 3, nsol
    int32 R): the first nsol[r] slots of E[r] hold the solutions, norm 1, by ascending root; the others are zero."""
    a, b = _points(x0, x1)
    s = _samples(samples, a.shape[0])
    import torch
    ctx = _context(ctx)
    dev = torch.device("cuda", ctx.device_id)
    d0, d1, ms, stride = _upload([(a, b)], dev)
    d_s = torch.from_numpy(s).to(dev)
    R = s.shape[0]
    d_E = torch.empty((R, MAX_SOL, 3, 3), dtype=torch.float64, device=dev)
    d_n = torch.empty(R, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    ctx._check(ctx._lib.wass_epi_solve5_dev(ctx._h, d0.data_ptr(), d1.data_ptr(), stride, d_s.data_ptr(), 5 * R, _ints(ms), R, 1, d_E.data_ptr(),
                                            d_n.data_ptr()))
    return d_E.cpu().numpy(), d_n.cpu().numpy()


def score_models(E, x0, x1, t, ctx=None) -> np.ndarray:
    """k_epi_score on its own: the int32 inlier count of every model (K x 3 x 3) over the matches, err <= float32(t * t)"""
    a, b = _points(x0, x1)
    e = _models(E)
    t = _threshold(t)
    import torch
    ctx = _context(ctx)
    dev = torch.device("cuda", ctx.device_id)
    d0, d1, ms, stride = _upload([(a, b)], dev)
    d_E = torch.from_numpy(e).to(dev)
    d_c = torch.empty(e.shape[0], dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    ctx._check(ctx._lib.wass_epi_score_dev(ctx._h, d_E.data_ptr(), e.shape[0], None, d0.data_ptr(), d1.data_ptr(), stride, _ints(ms), _doubles([t]), 1,
                                           d_c.data_ptr()))
    return d_c.cpu().numpy()


def inlier_mask(E, x0, x1, t, ctx=None):
    """k_epi_mask on its own: (mask bool M, err float32 M) of one model"""
    a, b = _points(x0, x1)
    e = np.ascontiguousarray(np.asarray(E, np.float64))
    if e.shape != (3, 3):
        raise ValueError("a model is 3 x 3")
    t = _threshold(t)
    import torch
    ctx = _context(ctx)
    dev = torch.device("cuda", ctx.device_id)
    d0, d1, ms, stride = _upload([(a, b)], dev)
    d_E = torch.from_numpy(e).to(dev)
    d_m = torch.empty(ms[0], dtype=torch.uint8, device=dev)
    d_e = torch.empty(ms[0], dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    ctx._check(ctx._lib.wass_epi_mask_dev(ctx._h, d_E.data_ptr(), d0.data_ptr(), d1.data_ptr(), stride, _ints(ms), _doubles([t]), 1, d_m.data_ptr(),
                                          d_e.data_ptr(), ms[0]))
    return d_m.cpu().numpy().astype(bool), d_e.cpu().numpy()


def find_essential_batch(pairs, t, rounds: int = ROUNDS, samples=None, ctx=None):
    """find_essential for several pairs in one chain of launches.  pairs: a list of (x0, x1); t: one threshold or one per pair;
    samples: None (ransac_samples(M, rounds) per pair) or one table per pair, all of `rounds` rows.  Pair i of a batch gives bit
    for bit what it gives alone."""
    pts = [_points(a, b) for a, b in pairs]
    if not pts:
        return []
    ts = [_threshold(v) for v in (t if isinstance(t, (list, tuple, np.ndarray)) else [t] * len(pts))]
    if len(ts) != len(pts):
        raise ValueError("one threshold per pair")
    if samples is None:
        if not 1 <= int(rounds) <= MAX_ROUNDS:
            raise ValueError(f"rounds = {rounds}: 1 .. {MAX_ROUNDS}")
        tabs = [ransac_samples(a.shape[0], int(rounds)) for a, _ in pts]
    else:
        if len(samples) != len(pts):
            raise ValueError("one sample table per pair")
        tabs = [_samples(s, a.shape[0]) for s, (a, _) in zip(samples, pts)]
        if len({s.shape[0] for s in tabs}) != 1:
            raise ValueError("every pair of a batch has the same number of samples")
    R, B = tabs[0].shape[0], len(pts)
    import torch
    ctx = _context(ctx)
    dev = torch.device("cuda", ctx.device_id)
    d0, d1, ms, stride = _upload(pts, dev)
    mmax = stride // 2
    d_s = torch.from_numpy(np.ascontiguousarray(np.stack(tabs))).to(dev)
    d_m = torch.empty((B, mmax), dtype=torch.uint8, device=dev)
    d_e = torch.empty((B, mmax), dtype=torch.float32, device=dev)
    E = np.zeros((B, 3, 3))
    idx, cnt = (C.c_int * B)(), (C.c_int * B)()
    torch.cuda.synchronize()
    ctx._check(ctx._lib.wass_epi_find_dev(ctx._h, d0.data_ptr(), d1.data_ptr(), stride, d_s.data_ptr(), 5 * R, _ints(ms), _doubles(ts), R, B,
                                          E.ctypes.data, idx, cnt, d_m.data_ptr(), d_e.data_ptr(), mmax))
    hm, he = d_m.cpu().numpy().astype(bool), d_e.cpu().numpy()
    out = []
    for p in range(B):
        k = int(idx[p])
        out.append(Essential(E[p].copy(), hm[p, :ms[p]].copy(), he[p, :ms[p]].copy(), int(cnt[p]), k // MAX_SOL if k >= 0 else -1,
                             k % MAX_SOL if k >= 0 else -1))
    return out


def find_essential(x0, x1, t, rounds: int = ROUNDS, samples=None, ctx=None) -> Essential:
    """cv::findEssentialMat(..., RANSAC, ., t) without the adaptive stop: every sample of the table is solved and every model scored
    against every match; the largest count wins, ties go to the lowest (sample, solution)."""
    return find_essential_batch([(x0, x1)], t, rounds, None if samples is None else [samples], ctx)[0]


# ------------------------------------------------------------------------------------------------------------------------ host
def triangulate(P0, P1, x0, x1) -> np.ndarray:
    """cv::triangulatePoints: per match the right singular vector of the smallest singular value of the 4 x 4 DLT matrix; M x 4"""
    A = np.stack([x0[:, 0:1] * P0[2] - P0[0], x0[:, 1:2] * P0[2] - P0[1], x1[:, 0:1] * P1[2] - P1[0], x1[:, 1:2] * P1[2] - P1[1]], axis=1)
    return np.linalg.svd(A)[2][:, 3, :]


def recover_pose(E, x0, x1, mask, distance: float = 50.0):
    """cv::recoverPose on the host, numpy fp64.  decomposeEssentialMat: E = U S V', U and V' forced to determinant +1, R1 = U W V',
    R2 = U W' V', t = U[:, 2]; the candidates in OpenCV's order (R1, t) (R2, t) (R1, -t) (R2, -t); per candidate the matches whose
    triangulated point lies at 0 < z < distance in both cameras, ANDed with `mask`; the first candidate with the largest count
    wins.  Returns (R, t, mask)."""
    a, b = _points(x0, x1)
    mask = np.asarray(mask, bool).reshape(-1)
    if mask.shape[0] != a.shape[0]:
        raise ValueError("one mask entry per match")
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
    P0 = np.eye(3, 4)
    best = None
    for R, tt in ((R1, t), (R2, t), (R1, -t), (R2, -t)):
        P1 = np.concatenate([R, tt[:, None]], axis=1)
        Q = triangulate(P0, P1, a, b)
        with np.errstate(all="ignore"):
            good = Q[:, 2] * Q[:, 3] > 0
            Q = Q / Q[:, 3:4]
            good &= Q[:, 2] < distance
            z1 = Q @ P1[2]
            good &= (z1 > 0) & (z1 < distance)
        good &= mask
        n = int(good.sum())
        if best is None or n > best[0]:
            best = (n, R, tt, good)
    return best[1], best[2], best[3]


def epipolar_error_stats(F, p0, p1):
    """evaluate_epipolar_error (epipolar.cpp:7-39): per match half the sum of the two point-to-line distances in pixels; (avg, std,
    min, max) with the reference's sequential sums and the population standard deviation.  No match: the reference divides by zero."""
    F = np.asarray(F, np.float64)
    p0, p1 = np.asarray(p0, np.float64).reshape(-1, 2), np.asarray(p1, np.float64).reshape(-1, 2)
    n = min(p0.shape[0], p1.shape[0])
    if n == 0:
        return float("nan"), float("nan"), float(np.finfo(np.float64).max), -float(np.finfo(np.float64).max)
    l = np.concatenate([p0[:n], np.ones((n, 1))], axis=1)
    r = np.concatenate([p1[:n], np.ones((n, 1))], axis=1)
    Ft = F.T
    Fl = np.stack([(F[i, 0] * l[:, 0] + F[i, 1] * l[:, 1]) + F[i, 2] * l[:, 2] for i in range(3)], axis=1)
    Fr = np.stack([(Ft[i, 0] * r[:, 0] + Ft[i, 1] * r[:, 1]) + Ft[i, 2] * r[:, 2] for i in range(3)], axis=1)
    dl = (Fl[:, 0] * r[:, 0] + Fl[:, 1] * r[:, 1]) + Fl[:, 2] * r[:, 2]
    dr = (Fr[:, 0] * l[:, 0] + Fr[:, 1] * l[:, 1]) + Fr[:, 2] * l[:, 2]
    e = 0.5 * (np.abs(dl / np.sqrt(Fl[:, 0] * Fl[:, 0] + Fl[:, 1] * Fl[:, 1])) + np.abs(dr / np.sqrt(Fr[:, 0] * Fr[:, 0] + Fr[:, 1] * Fr[:, 1])))
    avg = 0.0
    for v in e.tolist():
        avg += v
    avg /= float(n)
    var = 0.0
    for v in e.tolist():
        var += (v - avg) * (v - avg)
    return avg, float(np.sqrt(var / n)), float(e.min()), float(e.max())


def normalise(px, K) -> np.ndarray:
    """K^-1 (u, v, 1) per point, its first two entries (wass_match.cpp:257-276)"""
    Ki = np.linalg.inv(np.asarray(K, np.float64))
    p = np.asarray(px, np.float32).astype(np.float64).reshape(-1, 2)
    return np.ascontiguousarray((np.concatenate([p, np.ones((p.shape[0], 1))], axis=1) @ Ki.T)[:, :2])


def _intrinsics(K):
    K = np.asarray(K, np.float64)
    if K.shape != (3, 3):
        raise ValueError("intrinsics are 3 x 3")
    return K


def epipolar_filter_batch(pairs, max_epi_distance: float = 0.5, rounds: int = ROUNDS, ctx=None):
    """epipolar_filter for several pairs of pictures: pairs is a list of (loc_a, loc_b, K0, K1) or (MatchResult, K0, K1).  One chain
    of launches for all of them; pair i gives bit for bit what it gives alone."""
    items = []
    for it in pairs:
        if isinstance(it[0], MatchResult):
            if len(it) != 3:
                raise ValueError("a pair is (MatchResult, K0, K1) or (loc_a, loc_b, K0, K1)")
            loc_a, loc_b, K0, K1 = it[0].loc_a, it[0].loc_b, it[1], it[2]
        else:
            if len(it) != 4:
                raise ValueError("a pair is (MatchResult, K0, K1) or (loc_a, loc_b, K0, K1)")
            loc_a, loc_b, K0, K1 = it
        loc_a, loc_b = np.asarray(loc_a, np.float32).reshape(-1, 2), np.asarray(loc_b, np.float32).reshape(-1, 2)
        if loc_a.shape != loc_b.shape:
            raise ValueError("the two position arrays differ in shape")
        if loc_a.shape[0] < 5:
            raise ValueError(f"{loc_a.shape[0]} matches: at least five")
        K0, K1 = _intrinsics(K0), _intrinsics(K1)
        focal = (K0[0, 0] + K0[1, 1]) * 0.5
        items.append((loc_a, loc_b, K0, K1, normalise(loc_a, K0), normalise(loc_b, K1), float(max_epi_distance) / focal))
    if not items:
        return []
    best = find_essential_batch([(it[4], it[5]) for it in items], [it[6] for it in items], rounds, None, ctx)
    out = []
    for (loc_a, loc_b, K0, K1, x0, x1, t), b in zip(items, best):
        R, T, mask = recover_pose(b.E, x0, x1, b.mask)
        F = np.linalg.inv(K1).T @ b.E @ np.linalg.inv(K0)
        stats = epipolar_error_stats(F, loc_a[mask], loc_b[mask])
        out.append(EpipolarResult(b.E, F, b.mask, mask, R, T.reshape(3, 1), stats, t, b))
    return out


def epipolar_filter(loc_a, loc_b=None, K0=None, K1=None, max_epi_distance: float = 0.5, rounds: int = ROUNDS, ctx=None) -> EpipolarResult:
    """What wass_match does after matches_unfiltered.txt: findEssentialMat (RANSAC, threshold max_epi_distance / focal), recoverPose,
    F and the epipolar error of the matches kept.  loc_a, loc_b: M x 2 float32 pixel positions, or a MatchResult in place of both
    (then K0, K1 follow it)."""
    if isinstance(loc_a, MatchResult):
        if K1 is None:
            loc_b, K0, K1 = None, loc_b, K0
        return epipolar_filter_batch([(loc_a, K0, K1)], max_epi_distance, rounds, ctx)[0]
    return epipolar_filter_batch([(loc_a, loc_b, K0, K1)], max_epi_distance, rounds, ctx)[0]


# ----------------------------------------------------------------------------------------------------------------------- files
def write_opencv_matrix(path, node: str, a) -> None:
    """cv::FileStorage << node << Mat for a float64 matrix, in the XML layout gridding.read_opencv_matrix reads; 17 significant
    digits, so the matrix reads back bit for bit"""
    a = np.asarray(a, np.float64)
    if a.ndim != 2:
        raise ValueError("a matrix has two dimensions")
    vals = ["%.16e" % v for v in a.reshape(-1)]
    lines = ["    " + " ".join(vals[i:i + 3]) for i in range(0, len(vals), 3)]
    with open(os.fspath(path), "w") as f:
        f.write('<?xml version="1.0"?>\n<opencv_storage>\n<%s type_id="opencv-matrix">\n  <rows>%d</rows>\n  <cols>%d</cols>\n  <dt>d</dt>\n  <data>\n'
                % (node, a.shape[0], a.shape[1]))
        f.write("\n".join(lines))
        f.write("</data></%s>\n</opencv_storage>\n" % node)


def read_config(path) -> dict:
    """KEY=value lines of a matcher_config.txt; # starts a comment"""
    cfg = {}
    with open(os.fspath(path)) as f:
        for line in f:
            line = line.split("#", 1)[0].strip()
            if "=" in line:
                k, v = line.split("=", 1)
                cfg[k.strip()] = v.strip()
    return cfg


def filter_workdir(workdir, config=None, rounds: int = ROUNDS, ctx=None) -> int:
    """The file-level entry: reads matches_unfiltered.txt and intrinsics_0000000{0,1}.xml of `workdir`, writes matches_epionly.txt,
    matches.txt, matcher_stats.csv, ext_R.xml and ext_T.xml there and prints [P|100|100].  config: a KEY=value file;
    MATCHER_MAX_EPI_DISTANCE is read from it (0.5 without).  Returns 0, or -1 on a missing file or fewer than five matches."""
    wd = os.fspath(workdir)
    max_epi = 0.5
    try:
        if config is not None:
            max_epi = float(read_config(config).get("MATCHER_MAX_EPI_DISTANCE", max_epi))
        loc_a, loc_b = _match.read_matches(os.path.join(wd, "matches_unfiltered.txt"))
        K0 = gridding.read_opencv_matrix(os.path.join(wd, "intrinsics_00000000.xml"), "intr")
        K1 = gridding.read_opencv_matrix(os.path.join(wd, "intrinsics_00000001.xml"), "intr")
    except (OSError, ValueError, IndexError) as ex:
        print(f"wass_amd.epipolar: {ex}", file=sys.stderr)
        return -1
    if loc_a.shape[0] < 5:
        print(f"wass_amd.epipolar: {loc_a.shape[0]} matches, five are needed", file=sys.stderr)
        return -1
    r = epipolar_filter(loc_a, loc_b, K0, K1, max_epi, rounds, ctx)
    _match.write_matches(os.path.join(wd, "matches_epionly.txt"), loc_a[r.mask_epi], loc_b[r.mask_epi])
    g = _match._g15
    with open(os.path.join(wd, "matcher_stats.csv"), "w") as f:
        f.write("N.Matches;Avg. Error;Std. Error;Min. Error;Max. Error\n")
        f.write(f"{int(r.mask.sum())};{g(r.stats[0])};{g(r.stats[1])};{g(r.stats[2])};{g(r.stats[3])}\n")
    write_opencv_matrix(os.path.join(wd, "ext_R.xml"), "ext_R", r.R)
    write_opencv_matrix(os.path.join(wd, "ext_T.xml"), "ext_T", r.T)
    _match.write_matches(os.path.join(wd, "matches.txt"), loc_a[r.mask], loc_b[r.mask])
    print("[P|100|100]", flush=True)
    return 0


def main(argv=None) -> int:
    argv = sys.argv[1:] if argv is None else list(argv)
    if not 1 <= len(argv) <= 2:
        print("usage: python -m wass_amd.epipolar WORKDIR [CONFIG]", file=sys.stderr)
        return -1
    if not os.path.isdir(argv[0]):
        print(f"{argv[0]} does not exist, aborting.", file=sys.stderr)
        return -1
    return filter_workdir(argv[0], argv[1] if len(argv) > 1 else None)


if __name__ == "__main__":
    sys.exit(main())
