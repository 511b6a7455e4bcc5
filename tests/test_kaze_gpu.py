"""The KAZE detector on the GPU (wass_amd/features.py, csrc/kaze.hip) against the numpy oracle (tests/kaze_oracle.py).

Every stencil kernel launches 64 x 4 tiles (64 threads along x, 4 rows).  The pictures (tests/kaze_pictures.py, width x height):
33 x 29 (one tile across, a ragged last row of tiles), 64 x 64 (exact tiles), 65 x 63 (ragged in both directions), 130 x 67 (several
tiles), 257 x 40 (a wide strip of exact rows), all with 2 octaves x 2 sublevels (reach up to 5 pixels); 96 x 80 with the defaults,
where the 22-pixel taps cross every tile edge and reflect off every border; 160 x 128 and a 300 x 200 sea picture end to end.
tests/test_kaze.py holds each picture to its conditions on the oracle alone.

Stages made of + - x / sqrt are compared bit for bit.  The orientation and the descriptor use atan2f / sinf / cosf / expf: their
tolerance is half a float32 ulp of the value's scale plus four times the largest difference between the oracle's float32 and
fp64 runs on the same keypoints, computed here and printed with the margin."""
import numpy as np
import pytest

import kaze_oracle as KO
import kaze_pictures as P
from wass_amd import features as FE

pytestmark = pytest.mark.gpu

_runs = {}


def run(gpu_ctx, name):
    """the device's planes and extrema of a named picture, computed once"""
    if name not in _runs:
        no, ns = P.options(name)
        pyr = FE.KazePyramid(P.picture(name), FE.KazeOptions(1e-4, no, ns), gpu_ctx, keep=True)
        _runs[name] = (pyr, FE.kaze_scale_space(pyr), FE.kaze_response(pyr), FE.kaze_extrema(pyr))
    return _runs[name]


EXACT = [n for n in P.NAMES]


@pytest.mark.parametrize("name", EXACT)
def test_scale_space_is_exact(gpu_ctx, name):
    ref = P.oracle(name)["ss"]
    _, ss, _, _ = run(gpu_ctx, name)
    assert ss["hmax"] == ref["hmax"] and ss["npoints"] == ref["npoints"] and np.array_equal(ss["hist"], ref["hist"])
    assert ss["k"] == ref["k"]
    for key in ("Lsmooth", "flow", "Lt"):
        bad = int((ss[key] != ref[key]).sum())
        assert np.array_equal(ss[key], ref[key]), f"{key}: {bad} values differ"


@pytest.mark.parametrize("name", EXACT)
def test_response_is_exact(gpu_ctx, name):
    ref = P.oracle(name)["ss"]
    _, _, rs, _ = run(gpu_ctx, name)
    for key in ("Lx", "Ly", "Lxx", "Lxy", "Lyy", "Ldet"):
        bad = int((rs[key] != ref[key]).sum())
        assert np.array_equal(rs[key], ref[key]), f"{key}: {bad} values differ"


@pytest.mark.parametrize("name", EXACT)
def test_extrema_are_exact(gpu_ctx, name):
    ref = P.oracle(name)
    _, _, _, ex = run(gpu_ctx, name)
    assert ex["status"] == 0
    assert np.array_equal(ex["candidates"], ref["candidates"]) and np.array_equal(ex["values"], ref["values"])
    assert np.array_equal(ex["kept"], ref["kept"])
    assert np.array_equal(ex["refined"], ref["refined"]) and np.array_equal(ex["size"], ref["size_all"])


def test_probes_say_what_they_are_for(gpu_ctx):
    assert run(gpu_ctx, "constant")[1]["k"] == np.float32(0.03) and len(run(gpu_ctx, "constant")[3]["candidates"]) == 0
    assert run(gpu_ctx, "inside")[3]["candidates"].tolist() == [[2, 31, 10]]
    assert run(gpu_ctx, "outside")[3]["candidates"].tolist() == []


def _angle_diff(a, b):
    d = np.abs(a.astype(np.float64) - b.astype(np.float64))
    return np.minimum(d, 2 * np.pi - d)


@pytest.mark.parametrize("name", P.ORIENTED)
def test_orientation_of_the_oracles_keypoints(gpu_ctx, name):
    ref = P.oracle(name)
    ss, kp = ref["ss"], ref["kp"]
    a32, fragile, admissible = KO.orientation(kp, ss["Lx"], ss["Ly"], np.float32, flags=True, admissible=True)
    a64 = KO.orientation(kp, ss["Lx"], ss["Ly"], np.float64)
    keep = ~fragile
    assert fragile.mean() <= 0.05 and keep.sum() >= 50
    got = FE.kaze_orientation(kp[:, :4], run(gpu_ctx, name)[0])
    tol = 0.5 * float(np.spacing(np.float32(2 * np.pi))) + 4.0 * _angle_diff(a32[keep], a64[keep]).max()
    err = _angle_diff(got[keep], a32[keep]).max()
    # a fragile keypoint is not compared with the oracle's one choice, but with every angle a correct float32 run may give
    ferr = max([_angle_diff(admissible[q], got[q]).min() for q in np.flatnonzero(fragile)], default=0.0)
    print(f"{name}: {keep.sum()} keypoints, largest difference {err:.3g} rad, tolerance {tol:.3g} rad; {fragile.sum()} fragile keypoints, "
          f"{ferr:.3g} rad off their nearest admissible angle")
    assert (got >= 0).all() and (got < np.float32(2 * np.pi) + 1e-6).all()
    assert err <= tol
    assert ferr <= tol


@pytest.mark.parametrize("name", P.ORIENTED)
def test_descriptors_of_the_oracles_keypoints(gpu_ctx, name):
    ref = P.oracle(name)
    ss, kp = ref["ss"], ref["kp"]
    d64 = KO.descriptors(kp, ss["Lx"], ss["Ly"], np.float64)
    tol = 0.5 * float(np.spacing(np.float32(1.0))) + 4.0 * np.abs(ref["descriptors"].astype(np.float64) - d64).max()
    got = FE.kaze_descriptors(kp, run(gpu_ctx, name)[0])
    err = np.abs(got.astype(np.float64) - ref["descriptors"]).max()
    print(f"{name}: {len(kp)} keypoints, largest difference {err:.3g}, tolerance {tol:.3g}")
    assert got.shape == (len(kp), 64) and np.abs(np.linalg.norm(got.astype(np.float64), axis=1) - 1).max() < 1e-6
    assert err <= tol


# ---------------------------------------------------------------------------------------------------------------- kaze_detect
def same_keypoints(a, b):
    return all(np.array_equal(getattr(a, k), getattr(b, k)) for k in ("x", "y", "size", "angle", "response", "level", "descriptors")) \
        and a.status == b.status


def test_detect_equals_the_stages_chained_by_hand(gpu_ctx):
    name = "interior"
    pyr, _, _, ex = run(gpu_ctx, name)
    ok = ex["refined"][:, 4] != 0
    r, level = ex["refined"][ok], ex["kept"][ok, 0]
    table = np.column_stack([r[:, 0], r[:, 1], ex["size"][ok], level.astype(np.float32)]).astype(np.float32)
    angle = FE.kaze_orientation(table, pyr)
    desc = FE.kaze_descriptors(np.column_stack([table, angle]).astype(np.float32), pyr)
    kp = FE.kaze_detect(P.picture(name), ctx=gpu_ctx)
    assert len(kp) == ok.sum() >= 50 and kp.status == 0
    assert np.array_equal(kp.x, r[:, 0]) and np.array_equal(kp.y, r[:, 1]) and np.array_equal(kp.size, table[:, 2])
    assert np.array_equal(kp.response, r[:, 3]) and np.array_equal(kp.level, level)
    assert np.array_equal(kp.angle, angle) and np.array_equal(kp.descriptors, desc)
    # and the oracle's own keypoints are the same points
    ref = P.oracle(name)
    assert np.array_equal(kp.table()[:, :4], ref["kp"][:, :4])


def test_detect_lists_tensors_and_repeats(gpu_ctx):
    import torch
    opts = FE.KazeOptions(1e-4, 2, 2)
    pics = [P.picture("blobs65x63"), P.picture("blobs130x67"), P.picture("blobs64x64")[:63, :]]
    pics[2] = np.ascontiguousarray(np.pad(pics[2], ((0, 0), (0, 1)), mode="edge"))      # a second picture of 65 x 63
    assert pics[0].shape == pics[2].shape != pics[1].shape
    singles = [FE.kaze_detect(p, opts, gpu_ctx) for p in pics]
    assert all(len(s) >= 4 for s in singles)
    for got, one in zip(FE.kaze_detect(pics, opts, gpu_ctx), singles):
        assert same_keypoints(got, one)
    assert same_keypoints(FE.kaze_detect(torch.from_numpy(pics[1]).cuda(), opts, gpu_ctx), singles[1])
    assert same_keypoints(FE.kaze_detect(pics[1], opts, gpu_ctx), singles[1])
    as_float = pics[1].astype(np.float32) / np.float32(255.0)
    assert same_keypoints(FE.kaze_detect(as_float, opts, gpu_ctx), singles[1])


def test_candidate_cap_is_a_status(gpu_ctx):
    pyr, _, _, ex = run(gpu_ctx, "interior")
    n = len(ex["candidates"])
    assert n > 8
    rc, cand, vals = pyr.candidates(cap=8)
    assert rc == FE.CAP_REACHED and cand.shape == (8, 3) and vals.shape == (8,)
    full = {tuple(c) for c in ex["candidates"].tolist()}
    assert all(tuple(c) in full for c in cand.tolist())                     # whichever arrived first, they are candidates
    assert FE.kaze_detect(P.picture("interior"), ctx=gpu_ctx, cap=8).status == FE.CAP_REACHED
    rc, cand, _ = pyr.candidates(cap=n)
    assert rc == 0 and np.array_equal(cand, ex["candidates"])               # the buffers are as good as before


def test_argument_errors(gpu_ctx):
    with pytest.raises(ValueError, match="image"):
        FE.kaze_detect(np.zeros((20, 20), np.uint8), ctx=gpu_ctx)            # 22-pixel reach
    with pytest.raises(ValueError, match="image"):
        FE.kaze_detect(np.zeros((64, 64), np.int32), ctx=gpu_ctx)
    with pytest.raises(ValueError, match="image"):
        FE.kaze_detect(np.zeros((3, 64, 64), np.uint8), ctx=gpu_ctx)
    with pytest.raises(ValueError, match="options"):
        FE.kaze_detect(np.zeros((64, 64), np.uint8), FE.KazeOptions(1e-4, 1, 2), ctx=gpu_ctx)
    pyr = run(gpu_ctx, "blobs64x64")[0]
    with pytest.raises(ValueError, match="keypoints"):
        pyr.descriptors(np.zeros((3, 4), np.float32))
    with pytest.raises(ValueError, match="keypoints"):
        pyr.orientation(np.array([[5, 5, 4, 9]], np.float32))
    for bad in ([5, 5, 1e9, 1], [5, 5, -1, 1], [1e9, 5, 4, 1], [5, -3, 4, 1], [5, 64, 4, 1]):        # (int) of such a float is undefined on the device
        with pytest.raises(ValueError, match="keypoints"):
            pyr.orientation(np.array([bad], np.float32))
    with pytest.raises(ValueError, match="cap"):
        pyr.candidates(cap=0)


# ------------------------------------------------------------------------------------------------------------------ end to end
def relief_pair(w=640, h=400, frame=2):
    """synth.make_relief_pair and its rig (focal length 0.9 w): at half the swell's length and 25 % of stretch the descriptors of the
    oracle no longer pair up (16 of 987 keypoints pass a ratio test at w = 640, against 175)"""
    from wass_amd import synth
    left, right = synth.make_relief_pair(w, h, frame)
    return left, right, synth.rig_geometry(w, h)


# The bars of tests/test_epipolar_gpu.py belong to its noisy scene: 0.2 px of noise at a focal length of 2500 px, 8e-5 rad, over 420
# inliers.  The detector places a keypoint of these pictures within 0.12 px (median |dy| of the matches), so the pose test needs a
# focal length of 1440 px (1600 x 1000) to stand where the bars were set; measured at 640 x 400, 576 px: |R - I| 0.006, |T - Tgt| 0.026.
POSE_SIZE = (1600, 1000)
POSE_FEATURES = 600     # N = 1800 candidates
ROUNDS = 5              # of the matcher: its dynamics run their 50 000 steps in every round, 0.4 s each; the large groups come first


def test_pictures_to_pose(gpu_ctx):
    """detect_features -> gt_match -> epipolar_filter on a synthetic rectified pair: R = I and T = +-(1, 0, 0) within the bars
    tests/test_epipolar_gpu.py holds its noisy scene to"""
    import epipolar_oracle as EO
    from wass_amd import epipolar as EP
    from wass_amd import match
    left, right, g = relief_pair(*POSE_SIZE)
    fa, fb = FE.detect_features(left, POSE_FEATURES, ctx=gpu_ctx), FE.detect_features(right, POSE_FEATURES, ctx=gpu_ctx)
    m = match.gt_match(fa, fb, max_rounds=ROUNDS, ctx=gpu_ctx)
    r = EP.epipolar_filter(m, g["K_left"], g["K_right"], ctx=gpu_ctx)
    dR = np.abs(r.R - np.eye(3)).max()
    dT = min(np.abs(r.T[:, 0] - g["T"]).max(), np.abs(r.T[:, 0] + g["T"]).max())
    dy = np.abs(m.loc_a[:, 1] - m.loc_b[:, 1])
    print(f"{len(fa)} and {len(fb)} features, {len(m.matches)} matches (median |dy| {np.median(dy):.3g} px), {r.mask.sum()} kept; "
          f"|R - I| {dR:.3g}, |T - Tgt| {dT:.3g}, avg epipolar error {r.stats[0]:.3g} px")
    assert dR <= EO.R_MAX_ERR and dT <= EO.T_MAX_ERR and r.stats[0] <= EO.MAX_EPI_ERROR


def test_match_workdir_then_filter_workdir(gpu_ctx, tmp_path, capsys):
    from PIL import Image
    from wass_amd import epipolar as EP
    from wass_amd import match
    left, right, g = relief_pair()
    (tmp_path / "undistorted").mkdir()
    Image.fromarray(left).save(tmp_path / "undistorted" / "00000000.png")
    Image.fromarray(right).save(tmp_path / "undistorted" / "00000001.png")
    EP.write_opencv_matrix(tmp_path / "intrinsics_00000000.xml", "intr", g["K_left"])
    EP.write_opencv_matrix(tmp_path / "intrinsics_00000001.xml", "intr", g["K_right"])
    (tmp_path / "cfg.txt").write_text("NUM_FEATURES_PER_IMAGE=2000\nFEATURE_N_OCTAVES=4\nMATCHER_MAX_ROUNDS=1\n")
    assert FE.match_workdir(tmp_path, tmp_path / "cfg.txt", ctx=gpu_ctx) == 0
    out = capsys.readouterr().out.split()
    assert out == ["[P|10|100]", "[P|20|100]"]
    loc_a, loc_b = match.read_matches(tmp_path / "matches_unfiltered.txt")
    m = match.gt_match(FE.detect_features(left, ctx=gpu_ctx), FE.detect_features(right, ctx=gpu_ctx), max_rounds=1, ctx=gpu_ctx)
    assert len(loc_a) >= 5 and np.array_equal(loc_a, m.loc_a) and np.array_equal(loc_b, m.loc_b)
    assert EP.filter_workdir(tmp_path, ctx=gpu_ctx) == 0
    for name in ("matches_epionly.txt", "matches.txt", "matcher_stats.csv", "ext_R.xml", "ext_T.xml"):
        assert (tmp_path / name).stat().st_size > 0
    (tmp_path / "undistorted" / "00000001.png").unlink()
    assert FE.match_workdir(tmp_path, ctx=gpu_ctx) == -1
