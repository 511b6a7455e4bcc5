"""The autocalibration without a GPU: the numpy oracle (tests/autocal_oracle.py) against independent checks, the host parts of
wass_amd/autocalibrate.py, the files and exit codes, and the probe scenes of tests/test_autocal_gpu.py against the mistakes they
are there to catch."""
import os

import numpy as np
import pytest

import autocal_oracle as O
import epipolar_oracle as EO
from wass_amd import autocalibrate as AC
from wass_amd import epipolar as EP
from wass_amd import match

V_OFF = np.array([[0.05, -0.1, 0.02], [-0.2, 0.1, 0.3]])


def make_workdirs(root, K0, K1, frames, skip_last=True):
    """one workspace per frame of (p0, p1) float32 matches, optionally one without matches_epionly.txt, and the list file, which
    also names a directory that does not exist"""
    dirs = []
    for f, (a, b) in enumerate(frames):
        wd = root / ("%06d_wd" % f)
        wd.mkdir()
        EP.write_opencv_matrix(wd / "intrinsics_00000000.xml", "intr", K0)
        EP.write_opencv_matrix(wd / "intrinsics_00000001.xml", "intr", K1)
        match.write_matches(str(wd / "matches_epionly.txt"), a, b)
        dirs.append(wd)
    if skip_last:
        wd = root / "empty_wd"
        wd.mkdir()
        EP.write_opencv_matrix(wd / "intrinsics_00000000.xml", "intr", K0)
        EP.write_opencv_matrix(wd / "intrinsics_00000001.xml", "intr", K1)
        dirs.append(wd)
    lst = root / "workspaces.txt"
    lst.write_text("\n".join(str(d) for d in dirs) + "\n" + str(root / "not_there") + "\n")
    return dirs, lst


# ------------------------------------------------------------------------------------------------------------------ the oracle
@pytest.mark.parametrize("off", [False, True])
def test_jacobians_agree(off):
    """the stated closed form, the complex-step Jacobian of the quaternion form and central differences of it: at v = 0 and away"""
    cams, pts, obs, _, _, _ = O.ba_scene(24, 7, noise=0.2, rot_deg=0.5, t_off=0.01)
    if off:
        cams[:, 9:12] = V_OFF
    L = O.linearize(cams, pts, obs)
    for i in range(0, 24, 5):
        for q in range(2):
            A, B = O.jacobian_cs(cams[q], pts[i])
            Af, Bf = O.jacobian_fd(cams[q], pts[i])
            sa, sb = np.abs(A).max(), np.abs(B).max()
            assert np.abs(A - Af).max() <= 1e-7 * sa and np.abs(B - Bf).max() <= 1e-7 * sb          # h^2 f''' / 6 and eps / h at h = 1e-6
            assert np.abs(A - L["A"][i, q]).max() <= 64 * O.EPS * sa and np.abs(B - L["B"][i, q]).max() <= 64 * O.EPS * sb
    # the residuals of the two forms of the projection
    for q in range(2):
        R0 = cams[q, :9].reshape(3, 3)
        p = np.stack([O.project_any(R0, cams[q, 9:12], cams[q, 12:15], m) for m in pts])
        assert np.abs((obs[:, 2 * q:2 * q + 2] - p) - L["res"][:, 2 * q:2 * q + 2]).max() <= 64 * O.EPS


def test_blocks_are_the_dense_normal_equations():
    cams, pts, obs, _, _, _ = O.ba_scene(24, 7, noise=0.2, rot_deg=0.5, t_off=0.01)
    cams[:, 9:12] = V_OFF
    L = O.linearize(cams, pts, obs)
    J = O.dense_jacobian(L)
    H, g = J.T @ J, J.T @ L["res"].reshape(-1)
    tol = 64 * O.EPS * np.abs(H).max()
    for q in range(2):
        assert np.abs(H[6 * q:6 * q + 6, 6 * q:6 * q + 6] - L["Ut"][:, q].sum(0)).max() <= tol
    assert np.abs(H[0:6, 6:12]).max() == 0.0
    for i in range(24):
        assert np.abs(H[12 + 3 * i:15 + 3 * i, 12 + 3 * i:15 + 3 * i] - L["V"][i]).max() <= tol
        assert np.abs(H[0:12, 12 + 3 * i:15 + 3 * i] - L["W"][i].reshape(12, 3)).max() <= tol
    assert np.abs(g[:12] - L["eat"].sum(0)).max() <= tol and np.abs(g[12:] - L["eb"].reshape(-1)).max() <= tol
    # the Schur step in the stated order solves the same damped system
    mu = 1e-3 * np.diag(H).max()
    T, r, Vi = O.schur_terms(L, mu)
    U = np.zeros((12, 12))
    U[:6, :6], U[6:, 6:] = L["Ut"][:, 0].sum(0), L["Ut"][:, 1].sum(0)
    da = np.linalg.solve(U + mu * np.eye(12) - T.sum(0), L["eat"].sum(0) - r.sum(0))
    db = O.back_substitute(L, Vi, da)
    dp = np.linalg.solve(H + mu * np.eye(H.shape[0]), g)
    assert np.abs(da - dp[:12]).max() <= 1e-9 * np.abs(dp).max() and np.abs(db.reshape(-1) - dp[12:]).max() <= 1e-9 * np.abs(dp).max()


def test_oracle_minimum_against_scipy():
    """an independent minimiser on the same residuals: the cost agrees to 1e-10 of itself and the relative pose to 1e-8 (the cost is
    flat to second order at the minimum, both stop at gradients far below that); what is found is the GPU test's yardstick"""
    c = O.noisy_case(120)
    info = c["oracle"][2]
    print("oracle vs scipy at N = 120: relative cost difference", c["d_cost"], "pose difference", c["d_pose"], info)
    assert info["reason"] in (1, 2) and info["err1"] < info["err0"] and info["iters"] < 100
    assert c["d_cost"] <= 1e-10 and c["d_pose"] <= 1e-8
    Ro, To = O.relative_pose(c["oracle"][0])
    assert O.pose_distance(Ro, To, c["R"], c["T"]) <= 2 * EO.T_MAX_ERR          # 0.2 px of noise: the reference's acceptance bars
    big = O.noisy_case(1025)
    assert big["oracle"][2]["reason"] in (1, 2) and big["d_pose"] == c["d_pose"]


def test_oracle_recovers_the_truth_without_noise():
    c = O.clean_case(120)
    print("noise-free: distance to the truth", c["d_truth"], c["oracle"][2])
    start = O.pose_distance(*O.relative_pose(c["cams"]), c["R"], c["T"])
    assert start >= 1e-2 and c["d_truth"] <= 1e-9
    assert c["oracle"][2]["err1"] <= 1e-20


def test_v_to_one_case_on_the_oracle():
    cams, pts, obs = O.v_to_one_case()
    L = O.linearize(cams, pts, obs)
    mu0 = 1e-3 * max(L["Ut"].sum(0)[:, range(6), range(6)].max(), L["V"][:, [0, 1, 2], [0, 1, 2]].max())
    da, _ = O.solve_step(L, mu0)
    v1 = cams[1, 9:12] + da[6:9]
    assert (v1 * v1).sum() > 1.0 + 1e-3                       # far enough past 1 that no rounding brings it back
    c2, p2, info = O.lm(cams, pts, obs)
    assert info["reason"] == 7 and info["iters"] == 1 and np.array_equal(c2, cams) and np.array_equal(p2, pts) and np.isfinite(info["err1"])


# ------------------------------------------------------------------------------------------------------------- the pose choice
def test_pose_choice():
    R4 = np.stack([np.eye(3) * s for s in (0.5, 0.5, 0.25, 0.25)])
    for win in range(4):                                       # the largest count wherever it stands
        counts = [3, 3, 3, 3]
        counts[win] = 9
        assert AC.choose_pose(counts, R4) == win == O.choose_pose(counts, R4)
    import itertools
    for perm in itertools.permutations([1, 2, 3, 4]):
        assert AC.choose_pose(perm, R4) == perm.index(4) == O.choose_pose(perm, R4)
    assert AC.choose_pose([5, 5, 5, 5], R4) == 0                # equal counts and equal R[0, 0]: the first (strict >)
    R4b = np.stack([np.eye(3) * s for s in (0.25, 0.25, 0.5, 0.5)])
    assert AC.choose_pose([5, 5, 5, 5], R4b) == 2 == O.choose_pose([5, 5, 5, 5], R4b)      # a tie decided by R[0, 0]
    assert AC.choose_pose([0, 0, 0, 0], R4b) == 2               # a tie at 0: R[0, 0] > 0.0 still decides
    assert AC.choose_pose([0, 0, 0, 0], -R4b) == -1 == O.choose_pose([0, 0, 0, 0], -R4b)   # nothing beats the starting values 0 / 0.0
    assert AC.choose_pose([0, 0, 1, 0], -R4b) == 2


def test_candidates_come_in_the_references_order():
    K0, K1, R, T, _ = EO.rig(0)
    R4, T4 = AC.pose_candidates(EO.essential(R, T))
    Ro, To = O.pose_candidates(EO.essential(R, T))
    assert np.allclose(R4, Ro) and np.allclose(T4, To)
    assert np.array_equal(R4[0], R4[1]) and np.array_equal(R4[2], R4[3]) and np.array_equal(T4[0], -T4[1]) and np.array_equal(T4[0], T4[2])
    assert np.array_equal(T4[1], T4[3]) and not np.allclose(R4[0], R4[2])


def pose_probe(near):
    """rig 0: the true pose is candidate 1, (R1, -t).  near: 40 points between 0.5 and 0.9 baselines from camera 0"""
    the_rig = EO.rig(0)
    K0, K1, R, T, _ = the_rig
    if near:
        rng = np.random.default_rng(0)
        P = np.stack([rng.uniform(-0.2, 0.2, 40), rng.uniform(-0.2, 0.2, 40), rng.uniform(0.5, 0.9, 40)], axis=1)
        Q = P @ R.T + T
        x0, x1 = P[:, :2] / P[:, 2:], Q[:, :2] / Q[:, 2:]
    else:
        _, _, x0, x1, _ = EO.scene(the_rig, 65, 11)
    R4, T4 = O.pose_candidates(EO.essential(R, T))
    return R, T, R4, T4, x0, x1


def test_probe_notices_a_swapped_candidate_order():
    R, T, R4, T4, x0, x1 = pose_probe(False)
    mask = np.ones(x0.shape[0], bool)
    counts = [O.count_valid(O.triangulate(R4[k], T4[k], x0, x1), mask) for k in range(4)]
    k = O.choose_pose(counts, R4)
    assert k == 1 and O.pose_distance(R4[k], T4[k], R, T) <= 1e-9
    order = [0, 2, 1, 3]                                         # cv::recoverPose's order: (R1, t) (R2, t) (R1, -t) (R2, -t)
    wrong = O.choose_pose([counts[j] for j in order], R4)
    assert wrong != k and O.pose_distance(R4[wrong], T4[wrong], R, T) > 0.1


def test_probe_notices_z_above_0_in_place_of_1():
    R, T, R4, T4, x0, x1 = pose_probe(True)
    mask = np.ones(x0.shape[0], bool)
    pts = [O.triangulate(R4[k], T4[k], x0, x1) for k in range(4)]
    right, wrong = [O.count_valid(p, mask, 1.0) for p in pts], [O.count_valid(p, mask, 0.0) for p in pts]
    assert right != wrong and O.choose_pose(right, R4) != O.choose_pose(wrong, R4)
    assert O.choose_pose(wrong, R4) == 1 and O.choose_pose(right, R4) == 2        # the reference's rule takes the twisted pose here


def test_probe_notices_z_above_0_in_place_of_not_below():
    pts = np.array([[0, 0, 0.0], [0, 0, -0.0], [0, 0, np.nan], [0, 0, 5e-324], [0, 0, -5e-324], [0, 0, 3.0], [0, 0, 2.0]])
    mask = np.array([1, 1, 1, 1, 1, 1, 0], bool)
    keep = AC.select_points(pts, mask)
    assert keep.tolist() == [True, True, True, True, False, True, False] == O.select_points(pts, mask).tolist()
    with np.errstate(invalid="ignore"):
        assert (mask & (pts[:, 2] > 0)).tolist() != keep.tolist()


def test_probe_notices_multiplicative_damping_and_a_fixed_camera():
    cams, pts, obs, _, _, _ = O.ba_scene(65, 7, noise=0.2, rot_deg=0.5, t_off=0.01)
    L = O.linearize(cams, pts, obs)
    mu = 1e-3 * max(L["Ut"].sum(0)[:, range(6), range(6)].max(), L["V"][:, [0, 1, 2], [0, 1, 2]].max())
    da, db = O.solve_step(L, mu)
    dm, _ = O.solve_step(L, mu, damping="multiplicative")
    df, _ = O.solve_step(L, mu, fix_cam0=True)
    scale = np.abs(da).max()
    assert np.abs(da - dm).max() >= 1e-3 * scale                # far above the backward-error bound the GPU's step is held to
    assert np.abs(da[:6]).max() >= 1e-3 * scale and not df[:6].any() and np.abs(da - df).max() >= 1e-3 * scale
    # the three variants walk different ways to the same relative pose: only the step tests can tell them apart
    ends = [O.relative_pose(O.lm(cams, pts, obs, **kw)[0]) for kw in (dict(), dict(damping="multiplicative"), dict(fix_cam0=True))]
    for Rv, Tv in ends[1:]:
        assert O.pose_distance(Rv, Tv, *ends[0]) <= 1e-7


# ------------------------------------------------------------------------------------------------- statistics and homography
def test_structure_error_stats_on_hand_made_points():
    K = np.array([[100.0, 0, 50], [0, 100, 40], [0, 0, 1]])
    P = np.array([[0.0, 0, 2], [2.0, 0, 4]])
    p0, p1 = np.array([[53.0, 44], [100, 40]]), np.array([[100.0, 40], [125, 46]])
    avg, std, lo, hi = AC.structure_error_stats(P, p0, p1, np.eye(3), np.array([1.0, 0, 0]), K, K)
    assert (avg, std, lo, hi) == (2.75, 0.25, 2.5, 3.0)
    big = np.finfo(np.float64).max
    e = AC.structure_error_stats(np.zeros((0, 3)), np.zeros((0, 2)), np.zeros((0, 2)), np.eye(3), np.zeros(3), K, K)
    assert np.isnan(e[0]) and e[2:] == (big, -big)


def test_relative_pose_and_fundamental():
    K0, K1, R, T, _ = EO.rig(1)
    G = EO.rodrigues(np.array([0.1, -0.2, 0.05]))                 # a common change of frame and scale leaves the relative pose alone
    c = np.array([0.3, -0.1, 0.2])
    R0, T0 = G, c
    R1, T1 = R @ G, R @ c + 2.5 * T
    Rr, Tr = AC.relative_pose(R0, T0, R1, T1)
    assert O.pose_distance(Rr, Tr, R, T) <= 64 * O.EPS
    F = AC.fundamental(AC.skew(Tr) @ Rr, K0, K1)
    p0, p1, _, _, _ = EO.scene(EO.rig(1), 30, 5)
    assert EP.epipolar_error_stats(F, p0, p1)[3] <= 1e-3         # float32 pixels


def test_homography_lsq_on_planar_points():
    """exactly planar points: the homography maps them to 1e-9 of the picture size; with noise the refinement does not raise the
    reprojection error of the DLT start"""
    the_rig = EO.rig(2)
    size = max(the_rig[4])
    rng = np.random.default_rng(5)
    Ht = np.array([[0.9, 0.05, 30.0], [-0.04, 1.1, -20.0], [1e-5, -2e-5, 1.0]])
    p0 = rng.uniform(0, size, (60, 2))
    q = np.concatenate([p0, np.ones((60, 1))], axis=1) @ Ht.T
    p1 = q[:, :2] / q[:, 2:]
    H = AC.homography_lsq(p0, p1)
    assert H[2, 2] == 1.0 and np.abs(H - Ht).max() <= 1e-9 * size
    m = np.concatenate([p0, np.ones((60, 1))], axis=1) @ H.T
    assert np.abs(m[:, :2] / m[:, 2:] - p1).max() <= 1e-9 * size
    noisy = p1 + rng.normal(0, 0.5, p1.shape)

    def cost(Hm):
        mm = np.concatenate([p0, np.ones((60, 1))], axis=1) @ Hm.T
        return ((mm[:, :2] / mm[:, 2:] - noisy) ** 2).sum()
    assert cost(AC.homography_lsq(p0, noisy)) <= cost(AC.homography_lsq(p0, noisy, steps=0)) <= cost(Ht) * 1.5
    with pytest.raises(ValueError):
        AC.homography_lsq(p0[:3], p1[:3])


# ------------------------------------------------------------------------------------------------------- files and exit codes
def test_usage_and_argument_errors(capsys, tmp_path):
    assert AC.main([]) == 0
    assert "usage" in capsys.readouterr().out.lower()
    assert AC.main(["a", "b"]) == -1
    assert AC.main([str(tmp_path / "no_such_list.txt")]) == -1
    assert "[P|" not in capsys.readouterr().out


def test_pooling_skips_and_too_few_matches_write_nothing(capsys, tmp_path):
    K0, K1, R, T, frames = O.e2e_frames()
    dirs, lst = make_workdirs(tmp_path, K0, K1, [(a[:3], b[:3]) for a, b in frames[:2]])
    assert AC.load_workspaces(lst) == [str(d) for d in dirs]           # the directory that is not there is no workspace
    p0, p1, x0, x1, k0, k1 = AC.pool_matches(AC.load_workspaces(lst))
    assert "skipping" in capsys.readouterr().err
    assert p0.dtype == np.float64 and p0.shape == (6, 2) and np.array_equal(k0, K0) and np.array_equal(k1, K1)
    want = np.concatenate([frames[0][0][:3], frames[1][0][:3]])
    assert np.array_equal(p0.astype(np.float32), want)                  # the file's 15 digits, read as float64: not the float32 widened
    assert np.array_equal(p0, np.array([[float(format(float(v), ".15g")) for v in row] for row in want])) and not np.array_equal(p0, want)
    assert np.array_equal(x0, EO.normalise(p0, K0)) and np.array_equal(x1, EO.normalise(p1, K1))
    before = {d: sorted(os.listdir(d)) for d in dirs}
    assert AC.autocalibrate_workdirs(lst) == -1                          # six matches: fewer than eight, before any kernel runs
    out = capsys.readouterr().out.split()
    assert out == ["[P|20|100]", "[P|50|100]"]
    assert {d: sorted(os.listdir(d)) for d in dirs} == before
    empty = tmp_path / "empty.txt"
    empty.write_text("\n")
    assert AC.autocalibrate_workdirs(empty) == -1
    broken = tmp_path / "b"
    broken.mkdir()
    (tmp_path / "broken.txt").write_text(str(broken))
    assert AC.autocalibrate_workdirs(tmp_path / "broken.txt") == -1      # no intrinsics in the first workspace


def test_end_to_end_scene_passes_the_acceptance_on_the_oracle():
    """the scene of the GPU's end-to-end test: on the CPU chain the epipolar error goes down by a third, not by luck"""
    K0, K1, R, T, frames = O.e2e_frames()
    p0 = np.concatenate([a for a, _ in frames]).astype(np.float64)
    p1 = np.concatenate([b for _, b in frames]).astype(np.float64)
    r = O.calibrate(p0, p1, K0, K1, EP.ransac_samples(p0.shape[0], O.E2E["rounds"]))
    assert r["code"] == 0 and r["n"] >= 100 and r["after"][0] <= 0.8 * r["before"][0]
    assert O.pose_distance(r["R"], r["T"], R, T) <= EO.T_MAX_ERR
    few = O.calibrate(p0[:23], p1[:23], K0, K1, EP.ransac_samples(23, O.E2E["rounds"]))
    assert few["code"] == -1 and few["n"] < 24


def test_reject_scene_fails_the_acceptance_on_the_oracle():
    K0, K1, R, T, frames = O.reject_frames()
    p0 = np.concatenate([a for a, _ in frames]).astype(np.float64)
    p1 = np.concatenate([b for _, b in frames]).astype(np.float64)
    r = O.calibrate(p0, p1, K0, K1, EP.ransac_samples(p0.shape[0], O.REJECT["rounds"]))
    assert r["code"] == -1 and r["n"] >= 24 and r["info"]["reason"] in (1, 2) and r["after"][0] >= 1.05 * r["before"][0]


def test_scratch_bytes_and_symbols():
    from wass_amd import _lib
    assert {s for s in _lib.SYMBOLS if s.startswith("wass_ac_")} == {"wass_ac_scratch_bytes", "wass_ac_triangulate_dev", "wass_ac_linearize_dev",
                                                                    "wass_ac_step_dev", "wass_ac_error_dev", "wass_ac_bundle_dev"}
    assert AC.wass_ac_scratch_bytes(1) < AC.wass_ac_scratch_bytes(1025) < AC.wass_ac_scratch_bytes(20000)
    assert AC.wass_ac_scratch_bytes(20000) >= 8 * 20000 * (49 + 6 + 3 + 3)
    for bad in (0, -1, (1 << 22) + 1):
        with pytest.raises(ValueError):
            AC.wass_ac_scratch_bytes(bad)
    assert np.array_equal(AC.cam_rotation(np.concatenate([np.eye(3).ravel(), V_OFF[1], np.zeros(3)])),
                          O.cam_R(np.concatenate([np.eye(3).ravel(), V_OFF[1], np.zeros(3)])))
