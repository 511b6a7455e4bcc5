"""The essential-matrix filter without a GPU: the numpy oracle (tests/epipolar_oracle.py) against the ground truth of its synthetic
rig, the conditions every input of the GPU tests (tests/test_epipolar_gpu.py) has to meet on the oracle alone, the probes that show
each scene notices the mistake it is there to catch, and the host side of wass_amd.epipolar: the sample table, recover_pose, the
statistics, the files and the argument checks that need no device."""
import numpy as np
import pytest

import epipolar_oracle as O
from wass_amd import epipolar as EP
from wass_amd import gridding


# ---------------------------------------------------------------------------------------------------------------------- oracle
@pytest.mark.parametrize("planar", [False, True])
def test_oracle_contains_the_true_E(planar):
    """Noise-free samples: the true E is among the solutions.  The bound is 4580 kappa eps per admitted sample, ten times the
    constant recorded when the solver was designed (458); at least 90 % of the 256 samples must be admitted."""
    sc = O.solver_scene(planar)
    adm = np.array([r["admitted"] for r in sc["recs"]])
    kappa = np.array([r["kappa"] for r in sc["recs"]])
    ratio = sc["dist"][adm] / (kappa[adm] * O.EPS)
    print(f"planar {planar}: {adm.sum()} of {adm.size} admitted, largest distance {sc['dist'][adm].max():.3g}, in kappa eps {ratio.max():.3g}")
    assert adm.sum() >= 0.9 * O.SOLVER_SAMPLES
    assert (ratio <= 4580.0).all()
    assert all(2 <= len(r["E"]) <= 10 and len(r["E"]) % 2 == 0 for r, a in zip(sc["recs"], adm) if a)


@pytest.mark.parametrize("planar", [False, True])
def test_oracle_residuals(planar):
    """every solution of an admitted sample satisfies the five constraints, det E = 0 and the trace identity within c kappa eps"""
    sc = O.solver_scene(planar)
    c = O.solver_bound_factor()
    worst = 0.0
    for r, s in zip(sc["recs"], sc["samples"]):
        if not r["admitted"]:
            continue
        for E in r["E"]:
            assert abs(np.linalg.norm(E) - 1.0) <= 4 * O.EPS
            res = O.residuals(E, sc["x0"][s], sc["x1"][s])
            worst = max(worst, res / (r["kappa"] * O.EPS))
            assert res <= c * r["kappa"] * O.EPS
    print(f"planar {planar}: c = {c:.4g}, largest residual {worst:.3g} kappa eps")


def test_bound_factor_is_the_oracles_own():
    c = O.solver_bound_factor()
    assert 16.0 <= c <= 16.0 * 4580.0


# ------------------------------------------------------------------------------------------------------------------------ pose
def _candidates(E):
    U, _, Vt = np.linalg.svd(E)
    U = -U if np.linalg.det(U) < 0 else U
    Vt = -Vt if np.linalg.det(Vt) < 0 else Vt
    W = np.array([[0.0, 1.0, 0.0], [-1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    R1, R2, t = U @ W @ Vt, U @ W.T @ Vt, U[:, 2]
    return [(R1, t), (R2, t), (R1, -t), (R2, -t)]


def test_recover_pose_returns_the_truth():
    winners = set()
    for k in range(24):
        g = O.rig(100 + k, angle=0.15 if k % 3 else 0.4)
        _, _, x0, x1, _ = O.scene(g, 40, k)
        E = O.essential(g[2], g[3]) * (-1.0 if k % 2 else 1.0)
        mask = np.ones(40, bool)
        mask[k % 40] = False
        R, T, good = EP.recover_pose(E, x0, x1, mask)
        assert np.abs(R - g[2]).max() <= 1e-9 and np.abs(T - g[3]).max() <= 1e-9
        assert good.sum() == 39 and not good[k % 40]
        Ro, To, go = O.recover_pose(E, x0, x1, mask)
        assert np.abs(R - Ro).max() <= 1e-12 and np.abs(T - To).max() <= 1e-12 and np.array_equal(good, go)
        hits = [i for i, (Rc, tc) in enumerate(_candidates(E)) if np.abs(Rc - R).max() <= 1e-12 and np.abs(tc - T).max() <= 1e-12]
        assert len(hits) == 1
        winners.add(hits[0])
    assert len(winners) >= 2, winners


def test_recover_pose_distance_and_mask():
    g = O.rig(3)
    _, _, x0, x1, _ = O.scene(g, 60, 2)
    E = O.essential(g[2], g[3])
    depth = (O.triangulate(np.eye(3, 4), np.concatenate([g[2], g[3][:, None]], axis=1), x0, x1))
    z = depth[:, 2] / depth[:, 3]
    cut = float(np.median(z))
    _, _, good = EP.recover_pose(E, x0, x1, np.ones(60, bool), distance=cut)
    assert 0 < good.sum() < 60 and np.array_equal(good, O.recover_pose(E, x0, x1, np.ones(60, bool), distance=cut)[2])
    assert not (good & (z > cut * 1.001)).any()


# ------------------------------------------------------------------------------------------------------------------ statistics
def test_epipolar_error_stats():
    g, loc_a, loc_b, inl = O.noisy_scene()
    F = O.fundamental(O.essential(g[2], g[3]), g[0], g[1])
    got = EP.epipolar_error_stats(F, loc_a[inl], loc_b[inl])
    want = O.epipolar_error_stats(F, loc_a[inl], loc_b[inl])
    # a distance is a sum of three terms as large as a pixel coordinate (3000 px at most) over the line's norm: the two orders of
    # summation differ by a few eps of that, whatever the distance itself
    atol = 16 * O.EPS * 3000.0
    assert np.allclose(got, want, rtol=1e-12, atol=atol)
    assert 0.05 < got[0] < 0.5 and got[2] <= got[0] <= got[3] and got[1] > 0          # 0.2 px of noise
    F2 = 3.0 * F                                                                         # the error does not depend on the scale of F
    assert np.allclose(EP.epipolar_error_stats(F2, loc_a[inl], loc_b[inl]), want, rtol=1e-12, atol=atol)
    one = EP.epipolar_error_stats(F, loc_a[:1], loc_b[:1])
    assert one[1] == 0.0 and one[0] == one[2] == one[3]


# --------------------------------------------------------------------------------------------------------------------- samples
def test_sample_table():
    for m in (5, 6, 64, 600):
        s = EP.ransac_samples(m, 100)
        assert s.shape == (100, 5) and s.dtype == np.int32 and s.min() >= 0 and s.max() < m
        assert all(len(set(r)) == 5 for r in s.tolist())
        assert np.array_equal(s, EP.ransac_samples(m, 100))
        assert np.array_equal(EP.ransac_samples(m, 260)[:100], s)
    assert not np.array_equal(EP.ransac_samples(64, 10), EP.ransac_samples(64, 10, state=12345))
    # the first draws of cv::RNG(2^64 - 1) by hand: state = lo * 4164903690 + hi
    s, want = 2 ** 64 - 1, []
    while len(want) < 5:
        s = (s & 0xFFFFFFFF) * 4164903690 + (s >> 32)
        if (s & 0xFFFFFFFF) % 1000 not in want:
            want.append((s & 0xFFFFFFFF) % 1000)
    assert EP.ransac_samples(1000, 1)[0].tolist() == want
    with pytest.raises(ValueError):
        EP.ransac_samples(4, 10)
    with pytest.raises(ValueError):
        EP.ransac_samples(10, 0)


# ---------------------------------------------------------------------------------------------------------------------- probes
def test_score_probes_sit_where_they_should():
    """the matches placed at err == float32(t t) and one ulp either side are there, bit for bit, and the masks say so"""
    for m in O.SCORE_M:
        x0, x1, models, t, placed = O.score_probe(m)
        thr = O.threshold(t)
        assert len(placed) == min(3, m - 2)
        for j, want, got in placed:
            assert got == want, (m, j)
        mask = O.inlier_mask(models[0], x0, x1, t)
        assert mask[0]                                       # at the threshold: an inlier
        if len(placed) == 3:
            assert placed[1][1] < thr < placed[2][1] and mask[1] and not mask[2]
        if m >= 6:
            assert not mask[m - 1] and np.isnan(O.sampson_err(models[0], x0, x1)[m - 1])
        assert O.score_models(models[3], x0, x1, t)[0] == 0  # the model of zeros


def test_every_probe_scene_notices_its_mistake():
    x0, x1, models, t, placed = O.score_probe(257)
    Et = models[0]
    right = O.score_models(Et, x0, x1, t)[0]
    assert right >= 170
    assert O.score_models(Et.T, x0, x1, t)[0] < right // 4, "a transposed E goes unnoticed"
    assert O.score_models(Et, x1, x0, t)[0] < right // 4, "swapped pictures go unnoticed"
    err = O.sampson_err(Et, x0, x1)
    thr = O.threshold(t)
    with np.errstate(invalid="ignore"):
        assert (err < thr).sum() == right - 1, "< for <= goes unnoticed"
        assert (err <= np.float32(t)).sum() > right, "an unsquared threshold goes unnoticed"
    for m in (64, 257):
        g, a, b, inl, tt = O.select_scene(m)
        table = tie_table(m)
        first, last = O.find_essential(a, b, tt, table), O.find_essential(a, b, tt, table, tie="last")
        assert first["sample"] == 0 and last["sample"] > 0 and first["count"] == last["count"] == inl.sum(), "a last-index tie rule goes unnoticed"


def tie_table(m):
    """a sample table of the selection scene whose first two rows (and a later one) are all-inlier"""
    _, _, _, inl, _ = O.select_scene(m)
    s = EP.ransac_samples(m, O.SELECT["rounds"])
    clean = [r for r in range(len(s)) if inl[s[r]].all()]
    dirty = [r for r in range(len(s)) if not inl[s[r]].all()]
    assert len(clean) >= 3 and len(dirty) >= 3
    return s[clean[:2] + dirty[:3] + clean[2:3]]


# ------------------------------------------------------------------------------------------------ conditions on the GPU inputs
@pytest.mark.parametrize("m", [64, 257])
def test_selection_scenes_meet_their_conditions(m):
    g, x0, x1, inl, t = O.select_scene(m)
    for table in (EP.ransac_samples(m, O.SELECT["rounds"]), tie_table(m)):
        b = O.find_essential(x0, x1, t, table)
        assert b["rec"]["admitted"] and b["count"] == inl.sum() and np.array_equal(b["mask"], inl)
        assert O.margin(b["err"], t) > 1e-6
        assert O.distance(b["E"], O.essential(g[2], g[3])) <= O.solver_bound_factor() * b["rec"]["kappa"] * O.EPS


def test_noisy_scene_meets_half_of_each_bar_on_the_oracle():
    g, loc_a, loc_b, _ = O.noisy_scene()
    r = O.pipeline(loc_a, loc_b, g[0], g[1], EP.ransac_samples(O.NOISY["m"], O.NOISY["rounds"]))
    dR, dT = np.abs(r["R"] - g[2]).max(), np.abs(r["T"] - g[3]).max()
    print(f"oracle: |R - Rgt| {dR:.3g}, |T - Tgt| {dT:.3g}, avg epipolar error {r['stats'][0]:.3g} px, {r['kept']} matches kept")
    assert dR <= O.R_MAX_ERR / 2 and dT <= O.T_MAX_ERR / 2 and r["stats"][0] <= O.MAX_EPI_ERROR / 2 and r["kept"] >= O.MIN_MATCHES


# ----------------------------------------------------------------------------------------------------------------------- files
def test_opencv_matrix_round_trip(tmp_path):
    rng = np.random.default_rng(1)
    for node, a in (("ext_R", O.rodrigues(rng.normal(size=3))), ("ext_T", rng.normal(size=(3, 1))), ("m", rng.normal(size=(2, 5)) * 1e-300)):
        p = tmp_path / f"{node}.xml"
        EP.write_opencv_matrix(p, node, a)
        back = gridding.read_opencv_matrix(p, node)
        assert back.dtype == np.float64 and back.shape == a.shape and np.array_equal(back, a)
    text = (tmp_path / "ext_R.xml").read_text()
    assert text.startswith('<?xml version="1.0"?>\n<opencv_storage>\n<ext_R type_id="opencv-matrix">') and "<dt>d</dt>" in text
    with pytest.raises(ValueError):
        EP.write_opencv_matrix(tmp_path / "x.xml", "x", np.zeros(3))


def test_workdir_errors_need_no_device(tmp_path, capsys):
    assert EP.filter_workdir(tmp_path) == -1                 # nothing there
    g, loc_a, loc_b, _ = O.noisy_scene()
    from wass_amd import match
    match.write_matches(tmp_path / "matches_unfiltered.txt", loc_a[:4], loc_b[:4])
    assert EP.filter_workdir(tmp_path) == -1                 # no intrinsics
    EP.write_opencv_matrix(tmp_path / "intrinsics_00000000.xml", "intr", g[0])
    EP.write_opencv_matrix(tmp_path / "intrinsics_00000001.xml", "intr", g[1])
    assert EP.filter_workdir(tmp_path) == -1                 # four matches
    assert EP.main([str(tmp_path / "absent")]) == -1 and EP.main([]) == -1
    assert "[P|100|100]" not in capsys.readouterr().out
    cfg = tmp_path / "matcher_config.txt"
    cfg.write_text("# comment\nMATCHER_LAMBDA=0.00001\nMATCHER_MAX_EPI_DISTANCE = 0.75 # px\n")
    assert EP.read_config(cfg)["MATCHER_MAX_EPI_DISTANCE"] == "0.75"


def test_scratch_bytes():
    one, many = EP.scratch_bytes(1), EP.scratch_bytes(16)
    assert one >= 1024 * 10 * (72 + 4) + 1024 * 4 and 15 * one < many <= 16 * one          # the models, their counts, the solution counts
    assert EP.scratch_bytes(1, 64) < one
    for b, r in ((0, 1024), (1, 0), (65536, 1), (1, EP.MAX_ROUNDS + 1)):
        with pytest.raises(ValueError):
            EP.scratch_bytes(b, r)


def test_argument_checks_that_need_no_device():
    x = np.zeros((6, 2))
    good = np.arange(5)[None]
    for bad in (lambda: EP.five_point(x[:4], x[:4], good), lambda: EP.five_point(x, x[:5], good), lambda: EP.five_point(x, x, [[0, 1, 2, 3, 6]]),
                lambda: EP.five_point(x, x, [[0, 1, 2, 3, -1]]), lambda: EP.five_point(x, x, np.zeros((0, 5), int)),
                lambda: EP.five_point(x, x, np.zeros((2, 4), int)), lambda: EP.score_models(np.zeros((2, 3)), x, x, 1e-3),
                lambda: EP.score_models(np.zeros((3, 3)), x, x, -1.0), lambda: EP.inlier_mask(np.zeros((2, 3, 3)), x, x, 1e-3),
                lambda: EP.find_essential(x, x, 1e-3, rounds=0), lambda: EP.find_essential(x[:4], x[:4], 1e-3),
                lambda: EP.find_essential(np.zeros((6, 3)), np.zeros((6, 3)), 1e-3),
                lambda: EP.epipolar_filter(np.zeros((4, 2)), np.zeros((4, 2)), np.eye(3), np.eye(3)),
                lambda: EP.epipolar_filter(np.zeros((6, 2)), np.zeros((6, 2)), np.eye(2), np.eye(3)),
                lambda: EP.recover_pose(np.eye(3), x, x, np.ones(5, bool))):
        with pytest.raises(ValueError):
            bad()
