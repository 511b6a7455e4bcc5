"""The autocalibration on the GPU (wass_amd/autocalibrate.py, csrc/autocal.hip) against the numpy oracle (tests/autocal_oracle.py).
The scenes, the yardsticks and the oracle itself are held to their conditions on the CPU by tests/test_autocal.py.

Bounds.  Per-point results are compared bit for bit.  A sum of N terms is held within gamma_N * sum |terms| of the correctly
rounded sum (math.fsum), gamma_N = N eps / (1 - N eps): the bound of any summation order.  The 12 x 12 solve is held by its
backward error: Cholesky gives (S + dS) da = rhs with |dS| <= gamma_{3n+1} |L||L'| and || |L||L'| ||_2 <= n (1 - n gamma_{n+1})^-1
||S||_2 (Higham, Accuracy and Stability of Numerical Algorithms, theorems 10.3 and 10.4, n = 12), plus the rounding of the
residual formed here.  The loop's results are held within MARGIN times the oracle's own distance to its yardstick.

With both cameras free the projection has seven gauge freedoms, so the reduced system at mu = 0 is singular for every probe: the
entry takes no gauge constraint, and the mu = 0 case checks what holds all the same: the per-point inverse through db when the
factorisation succeeds, a rejected step otherwise, and no fault either way."""
import math
import os

import numpy as np
import pytest

import autocal_oracle as O
import epipolar_oracle as EO
from test_autocal import make_workdirs
from wass_amd import autocalibrate as AC
from wass_amd import epipolar as EP
from wass_amd import gridding

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 24, 63, 64, 65, 255, 256, 257, 1025)
V_OFF = np.array([[0.05, -0.1, 0.02], [-0.2, 0.1, 0.3]])


def same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def fsum(terms):
    """the correctly rounded sum over the first axis, and the sum of the absolute values"""
    t = terms.reshape(terms.shape[0], -1)
    s = np.array([math.fsum(t[:, k]) for k in range(t.shape[1])]).reshape(terms.shape[1:])
    return s, np.abs(terms).sum(0)


def probe(n, off=False):
    cams, pts, obs, _, _, _ = O.ba_scene(n, 7, noise=0.2, rot_deg=0.5, t_off=0.01)
    if off:
        cams[:, 9:12] = V_OFF
    return cams, pts, obs


# --------------------------------------------------------------------------------------------------------------- triangulation
def tri_probe(m):
    """matches of the rig under the four candidates of the true E, every fifth outside the mask, the second a NaN match (the hand-made
    edge cases are test_triangulation_edges')"""
    the_rig = EO.rig(2)
    _, _, x0, x1, _ = EO.scene(the_rig, m, 11)
    x0, x1 = x0.copy(), x1.copy()
    mask = np.ones(m, bool)
    mask[::5] = False
    if m > 1:
        x0[1] = np.nan
    return x0, x1, mask, AC.pose_candidates(EO.essential(the_rig[2], the_rig[3]))


@pytest.mark.parametrize("m", [1, 63, 64, 65, 257, 1025])
def test_triangulation_is_exact(gpu_ctx, m):
    x0, x1, mask, (R4, T4) = tri_probe(m)
    pts, counts = AC.triangulate_candidates(R4, T4, x0, x1, mask, ctx=gpu_ctx)
    for k in range(4):
        ref = O.triangulate(R4[k], T4[k], x0, x1)
        assert same(pts[k], ref), (m, k)
        assert counts[k] == O.count_valid(ref, mask)
    if m >= 63:
        assert counts.max() > 0 and np.isnan(pts[:, 1]).all()
    _, c0 = AC.triangulate_candidates(R4, T4, x0, x1, np.zeros(m, bool), ctx=gpu_ctx)
    assert not c0.any()


def test_triangulation_edges(gpu_ctx):
    """camera 1 at the identity one unit to the side: the point (X, Y, Z) is seen at (X / Z, Y / Z) and ((X - 1) / Z, Y / Z).  Matches
    built for z = 1 and its neighbours, z = 0 and -0.0 (both rays parallel: the system is singular there), and a match on the
    baseline.  The oracle states what comes out; here the counts and bits agree, and a NaN point counts nowhere."""
    R4, T4 = np.stack([np.eye(3)] * 4), np.array([[-1.0, 0, 0], [1.0, 0, 0], [-1.0, 0, 0], [0, -1.0, 0]])
    zs = np.array([1.0, np.nextafter(1.0, 2.0), np.nextafter(1.0, 0.0), 2.0, 0.5, 1.0, 1.0])
    X = np.stack([0.25 * np.ones_like(zs), 0.5 * np.ones_like(zs), zs], axis=1)
    x0 = X[:, :2] / X[:, 2:]
    x1 = (X[:, :2] - [1.0, 0.0]) / X[:, 2:]
    x0 = np.concatenate([x0, [[0.3, 0.2], [0.3, 0.2], [1e308, 0.0], [0.0, 0.0]]])      # equal rays: parallel, z = 0 / 0 or -0.0
    x1 = np.concatenate([x1, [[0.3, 0.2], [0.3, -0.2], [1e308, 0.0], [0.0, 0.0]]])
    mask = np.ones(x0.shape[0], bool)
    pts, counts = AC.triangulate_candidates(R4, T4, x0, x1, mask, ctx=gpu_ctx)
    for k in range(4):
        ref = O.triangulate(R4[k], T4[k], x0, x1)
        assert same(pts[k], ref), k
        assert counts[k] == O.count_valid(ref, mask)
        keep = AC.select_points(pts[k], mask)
        assert np.array_equal(keep, O.select_points(ref, mask))
    assert np.isnan(pts[0]).any() and (pts[0][:, 2] > 1).any() and (pts[0][:, 2] <= 1).any()


# --------------------------------------------------------------------------------------------------------------- linearisation
@pytest.mark.parametrize("off", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_linearize(gpu_ctx, n, off):
    cams, pts, obs = probe(n, off)
    G, L = AC.ba_linearize(cams, pts, obs, ctx=gpu_ctx), O.linearize(cams, pts, obs)
    assert same(G.res, L["res"]) and same(G.V, L["V"]) and same(G.eb, L["eb"]) and same(G.W, L["W"])
    g = O.gamma(n)
    for got, terms in ((G.U, L["Ut"]), (G.ea, L["eat"]), (np.float64(G.err), L["e2"])):
        ref, mag = fsum(terms)
        assert (np.abs(got - ref) <= g * mag).all(), n
    assert G.grad_pts == np.abs(L["eb"]).max() and G.diag_pts == L["V"][:, [0, 1, 2], [0, 1, 2]].max()
    e, r = AC.ba_error(cams, pts, obs, ctx=gpu_ctx, residuals=True)
    assert same(r, L["res"]) and abs(e - fsum(L["e2"])[0]) <= g * L["e2"].sum()


# ------------------------------------------------------------------------------------------------------------------------ step
def check_step(G, L, cams, pts, obs, mu, n):
    T, r, Vi = O.schur_terms(L, mu)
    T = np.tril(T) + np.transpose(np.tril(T, -1), (0, 2, 1))          # the kernel forms the lower triangle, Y_p . W_q for q <= p
    g = O.gamma(n + 2)
    U, Um = np.zeros((12, 12)), np.zeros((12, 12))
    for q in range(2):
        U[6 * q:6 * q + 6, 6 * q:6 * q + 6], Um[6 * q:6 * q + 6, 6 * q:6 * q + 6] = fsum(L["Ut"][:, q])
    Ts, Tm = fsum(T)
    assert np.array_equal(G.S, G.S.T)
    assert (np.abs(G.S - (U + mu * np.eye(12) - Ts)) <= g * (Um + mu * np.eye(12) + Tm) + g * np.abs(G.S)).all()
    rs, rm = fsum(r)
    es, em = fsum(L["eat"])
    assert (np.abs(G.rhs - (es - rs)) <= g * (em + rm)).all()
    if not G.ok:
        assert not G.da.any() and G.err == 0.0
        return
    k = 12
    bound = O.gamma(3 * k + 1) * k / (1.0 - k * O.gamma(k + 1)) * np.linalg.norm(G.S, 2) * np.linalg.norm(G.da)
    bound += O.gamma(k + 1) * np.linalg.norm(np.abs(G.S) @ np.abs(G.da) + np.abs(G.rhs))
    assert np.linalg.norm(G.S @ G.da - G.rhs) <= bound
    db = O.back_substitute(L, Vi, G.da)
    assert same(G.db, db) and same(G.pts, pts + db) and same(G.cams, O.moved(cams, G.da))
    res = O.residuals(G.cams, G.pts, obs)
    e2 = (res[:, 0] * res[:, 0] + res[:, 1] * res[:, 1]) + (res[:, 2] * res[:, 2] + res[:, 3] * res[:, 3])
    assert abs(G.err - math.fsum(e2)) <= O.gamma(n) * e2.sum()
    d2 = (db[:, 0] * db[:, 0] + db[:, 1] * db[:, 1]) + db[:, 2] * db[:, 2]
    assert abs(G.dp2 - (math.fsum(d2) + (G.da ** 2).sum())) <= O.gamma(n + 12) * (d2.sum() + (G.da ** 2).sum())
    dl = np.concatenate([(db * (mu * db + L["eb"])).reshape(-1), G.da * (mu * G.da + L["eat"].sum(0))])
    assert abs(G.dL - math.fsum(dl)) <= O.gamma(3 * n + 24) * np.abs(dl).sum() + 2 * O.gamma(n) * np.abs(G.da) @ np.abs(L["eat"]).sum(0)


@pytest.mark.parametrize("which", ["zero", "initial", "1e12"])
@pytest.mark.parametrize("n", SIZES)
def test_step(gpu_ctx, n, which):
    cams, pts, obs = probe(n, off=(n % 2 == 1))
    L = O.linearize(cams, pts, obs)
    mu0 = 1e-3 * max(L["Ut"].sum(0)[:, range(6), range(6)].max(), L["V"][:, [0, 1, 2], [0, 1, 2]].max())
    mu = {"zero": 0.0, "initial": mu0, "1e12": 1e12}[which]
    G = AC.ba_step(cams, pts, obs, mu, ctx=gpu_ctx)
    if which != "zero":
        assert G.ok
    check_step(G, L, cams, pts, obs, mu, n)


def test_step_rejects_what_is_not_positive_definite(gpu_ctx):
    cams, pts, obs = probe(65)
    bad = pts.copy()
    bad[40] = np.nan
    G = AC.ba_step(cams, bad, obs, 1e-3, ctx=gpu_ctx)
    assert not G.ok and not G.da.any()
    c2 = cams.copy()
    c2[1, 9:12] = [0.9, 0.9, 0.9]                      # |v| > 1: w is NaN
    assert not AC.ba_step(c2, pts, obs, 1e-3, ctx=gpu_ctx).ok
    ok = AC.ba_step(cams, pts, obs, 1e-3, ctx=gpu_ctx)            # and the context works on
    assert ok.ok and np.isfinite(ok.db).all()


# ----------------------------------------------------------------------------------------------------------------- determinism
def test_two_runs_and_a_prefix_give_the_same_bits(gpu_ctx):
    cams, pts, obs = probe(257, off=True)
    a, b = AC.ba_linearize(cams, pts, obs, ctx=gpu_ctx), AC.ba_linearize(cams, pts, obs, ctx=gpu_ctx)
    for f in ("res", "V", "eb", "W", "U", "ea"):
        assert same(getattr(a, f), getattr(b, f)), f
    assert a.err == b.err
    s, t = AC.ba_step(cams, pts, obs, 1e-2, ctx=gpu_ctx), AC.ba_step(cams, pts, obs, 1e-2, ctx=gpu_ctx)
    assert same(s.S, t.S) and same(s.da, t.da) and same(s.db, t.db) and s.err == t.err and s.dL == t.dL
    r1, r2 = AC.bundle_adjust_cams(cams, pts, obs, 30, ctx=gpu_ctx), AC.bundle_adjust_cams(cams, pts, obs, 30, ctx=gpu_ctx)
    assert same(r1[0], r2[0]) and same(r1[1], r2[1]) and r1[2] == r2[2]
    # the entries take a count, not a mask: the first 100 points alone give the per-point bits they give among the 257; the sums
    # differ, as they should
    c = AC.ba_linearize(cams, pts[:100], obs[:100], ctx=gpu_ctx)
    for f in ("res", "V", "eb", "W"):
        assert same(getattr(a, f)[:100], getattr(c, f)), f


# ------------------------------------------------------------------------------------------------------------------- the loop
def gpu_pose(R, T, pts, obs, ctx):
    r = AC.bundle_adjust(R, T, pts, obs[:, :2], obs[:, 2:], ctx=ctx)
    assert np.isfinite(r.R0).all() and np.isfinite(r.R1).all() and np.isfinite(r.pts).all()
    return r, AC.relative_pose(r.R0, r.T0, r.R1, r.T1)


def test_bundle_adjust_noise_free(gpu_ctx):
    """N = 120, camera 1 started 1 degree and 2 % off: the pose comes back to the truth as closely as the oracle's, times MARGIN"""
    c = O.clean_case(120)
    r, (R, T) = gpu_pose(c["cams"][1, :9].reshape(3, 3), c["cams"][1, 12:15], c["pts"], c["obs"], gpu_ctx)
    d = O.pose_distance(R, T, c["R"], c["T"])
    print("noise-free: gpu", d, "oracle", c["d_truth"], "iters", r.iters, "reason", r.reason, "err", r.err0, r.err1)
    assert d <= O.MARGIN * max(c["d_truth"], 4 * O.EPS)                # the floor: the rounding of the entries of R and T themselves
    assert r.reason in (1, 2, 6) and r.err1 <= r.err0 and r.iters <= 1000


@pytest.mark.parametrize("n", [120, 1025])
def test_bundle_adjust_noisy(gpu_ctx, n):
    c = O.noisy_case(n)
    r, (R, T) = gpu_pose(c["cams"][1, :9].reshape(3, 3), c["cams"][1, 12:15], c["pts"], c["obs"], gpu_ctx)
    Ro, To = O.relative_pose(c["oracle"][0])
    dc, dp = abs(r.err1 - c["scipy_cost"]) / c["scipy_cost"], O.pose_distance(R, T, Ro, To)
    print("noisy", n, ": cost", r.err1, "rel. diff", dc, "yardstick", c["d_cost"], "pose diff", dp, "yardstick", c["d_pose"], "iters", r.iters, r.reason)
    # the floors: the cost is a sum of 4 N squares (gamma_4N of itself), the pose entries of size one (a few eps)
    assert dc <= O.MARGIN * max(c["d_cost"], O.gamma(4 * n)) and dp <= O.MARGIN * max(c["d_pose"], 4 * O.EPS)
    assert r.reason in (1, 2) and r.err1 <= r.err0


def test_v_driven_to_one_ends_with_reason_7(gpu_ctx):
    """the hand-made start of the oracle (held there: its first step asks for |v| > 1): the candidate's error is NaN and the loop
    ends with the start parameters, in which there is no NaN"""
    cams, pts, obs = O.v_to_one_case()
    c2, p2, info = AC.bundle_adjust_cams(cams, pts, obs, ctx=gpu_ctx)
    assert info["reason"] == 7 and info["iters"] == 1 and same(c2, cams) and same(p2, pts)
    assert info["err1"] == info["err0"] and np.isfinite(info["err1"]) and np.isfinite(c2).all() and np.isfinite(p2).all()


def test_scratch_bytes_grow_with_n():
    assert AC.wass_ac_scratch_bytes(1) < AC.wass_ac_scratch_bytes(1025) < AC.wass_ac_scratch_bytes(20000)
    assert AC.wass_ac_scratch_bytes(20000) >= 8 * 20000 * (49 + 6 + 3 + 3)
    with pytest.raises(ValueError):
        AC.wass_ac_scratch_bytes(0)


# ------------------------------------------------------------------------------------------------------------------ end to end
def test_end_to_end(gpu_ctx, tmp_path, capsys):
    K0, K1, R, T, frames = O.e2e_frames()
    dirs, lst = make_workdirs(tmp_path, K0, K1, frames)
    assert AC.autocalibrate_workdirs(lst, rounds=O.E2E["rounds"], ctx=gpu_ctx) == 0
    out = capsys.readouterr()
    marks = [l for l in out.out.split() if l.startswith("[P|")]
    assert marks == ["[P|20|100]", "[P|50|100]", "[P|70|100]", "[P|100|100]"]
    assert "skipping" in out.err
    first = {}
    for wd in dirs:
        for name, node, shape in (("ext_R.xml", "ext_R", (3, 3)), ("ext_T.xml", "ext_T", (3, 1)), ("H.xml", "H", (3, 3))):
            m = gridding.read_opencv_matrix(wd / name, node)
            assert m.shape == shape
            assert same(m, first.setdefault(name, m))
            assert open(wd / name).read() == open(dirs[0] / name).read()
    Rg, Tg = first["ext_R.xml"], first["ext_T.xml"].reshape(3)
    assert abs(np.linalg.norm(Tg) - 1.0) <= 4 * O.EPS and np.abs(Rg @ Rg.T - np.eye(3)).max() <= 64 * O.EPS
    assert O.pose_distance(Rg, Tg, R, T) <= 2 * EO.T_MAX_ERR


def test_failure_writes_nothing(gpu_ctx, tmp_path):
    """too few points for the bundle adjustment (23 matches): -1, and no file appears"""
    K0, K1, R, T, frames = O.e2e_frames()
    dirs, lst = make_workdirs(tmp_path, K0, K1, [(frames[0][0][:23], frames[0][1][:23])], skip_last=False)
    before = sorted(os.listdir(dirs[0]))
    assert AC.autocalibrate_workdirs(lst, rounds=O.E2E["rounds"], ctx=gpu_ctx) == -1
    assert sorted(os.listdir(dirs[0])) == before


def test_a_bundle_adjustment_that_does_not_help_changes_nothing(gpu_ctx, tmp_path, capsys):
    """the oracle's reject scene: -1, "SBA failed", and the files a matcher left are as they were"""
    K0, K1, R, T, frames = O.reject_frames()
    dirs, lst = make_workdirs(tmp_path, K0, K1, frames, skip_last=False)
    for wd in dirs:
        EP.write_opencv_matrix(wd / "ext_R.xml", "ext_R", np.eye(3))
        EP.write_opencv_matrix(wd / "ext_T.xml", "ext_T", np.array([[1.0], [0.0], [0.0]]))
    before = {wd: {f: open(wd / f).read() for f in sorted(os.listdir(wd))} for wd in dirs}
    assert AC.autocalibrate_workdirs(lst, rounds=O.REJECT["rounds"], ctx=gpu_ctx) == -1
    out = capsys.readouterr()
    assert "SBA failed" in out.err and "[P|70|100]" in out.out and "[P|100|100]" not in out.out
    assert {wd: {f: open(wd / f).read() for f in sorted(os.listdir(wd))} for wd in dirs} == before


def test_pictures_to_calibration(gpu_ctx, tmp_path, capsys):
    """two synthetic frames through features.match_workdir and epipolar.filter_workdir, then the autocalibration over both: the exit
    code, and the files that go with it"""
    from PIL import Image
    from wass_amd import features as FE
    from wass_amd import synth
    dirs = []
    for f, frame in enumerate((2, 3)):
        wd = tmp_path / ("%06d_wd" % f)
        (wd / "undistorted").mkdir(parents=True)
        left, right = synth.make_relief_pair(640, 400, frame)
        g = synth.rig_geometry(640, 400)
        Image.fromarray(left).save(wd / "undistorted" / "00000000.png")
        Image.fromarray(right).save(wd / "undistorted" / "00000001.png")
        EP.write_opencv_matrix(wd / "intrinsics_00000000.xml", "intr", g["K_left"])
        EP.write_opencv_matrix(wd / "intrinsics_00000001.xml", "intr", g["K_right"])
        (wd / "cfg.txt").write_text("NUM_FEATURES_PER_IMAGE=2000\nFEATURE_N_OCTAVES=4\nMATCHER_MAX_ROUNDS=1\n")
        assert FE.match_workdir(wd, wd / "cfg.txt", ctx=gpu_ctx) == 0
        assert EP.filter_workdir(wd, ctx=gpu_ctx) == 0
        dirs.append(wd)
    lst = tmp_path / "workspaces.txt"
    lst.write_text(" ".join(str(d) for d in dirs))
    left_by_matcher = {wd: open(wd / "ext_R.xml").read() for wd in dirs}
    capsys.readouterr()
    code = AC.autocalibrate_workdirs(lst, ctx=gpu_ctx)
    marks = [l for l in capsys.readouterr().out.split() if l.startswith("[P|")]
    assert code in (0, -1) and marks[:2] == ["[P|20|100]", "[P|50|100]"]
    if code == 0:
        assert marks[-1] == "[P|100|100]"
        for name in ("ext_R.xml", "ext_T.xml", "H.xml"):
            assert open(dirs[0] / name).read() == open(dirs[1] / name).read()
        assert gridding.read_opencv_matrix(dirs[0] / "H.xml", "H").shape == (3, 3)
    else:
        assert not (dirs[0] / "H.xml").exists() and {wd: open(wd / "ext_R.xml").read() for wd in dirs} == left_by_matcher
