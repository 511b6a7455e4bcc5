"""The essential-matrix filter on the GPU (wass_amd/epipolar.py, csrc/epipolar.hip) against the numpy oracle
(tests/epipolar_oracle.py).  Every input used here is held to its conditions on the oracle alone by tests/test_epipolar.py: the
admitted share of the solver samples, the winners and margins of the selection scenes, half of each of the reference's bars on
the noisy scene, the placed matches of the scoring probes."""
import numpy as np
import pytest

import epipolar_oracle as O
from test_epipolar import tie_table
from wass_amd import epipolar as EP
from wass_amd import gridding, match

pytestmark = pytest.mark.gpu


def same(a, b):
    return np.array_equal(a, b, equal_nan=True)


# --------------------------------------------------------------------------------------------------------------------- scoring
@pytest.mark.parametrize("m", O.SCORE_M)
def test_scoring_is_exact(gpu_ctx, m):
    """counts, mask and err equal the oracle's from the same bits of E: matches at err == float32(t t) and one ulp either side, a
    NaN match, a model of zeros"""
    x0, x1, models, t, placed = O.score_probe(m)
    assert np.array_equal(EP.score_models(models, x0, x1, t, ctx=gpu_ctx), O.score_models(models, x0, x1, t))
    for E in models:
        mask, err = EP.inlier_mask(E, x0, x1, t, ctx=gpu_ctx)
        assert err.dtype == np.float32 and same(err, O.sampson_err(E, x0, x1))
        assert np.array_equal(mask, O.inlier_mask(E, x0, x1, t))
    assert np.array_equal(EP.score_models(models[0], x0, x1, t, ctx=gpu_ctx), O.score_models(models[:1], x0, x1, t))


@pytest.mark.parametrize("rounds", [63, 65])
def test_scoring_over_model_tiles(gpu_ctx, rounds):
    """the models of `rounds` samples (630 and 650: across the 256-model workgroups), empty slots included, over 257 matches"""
    _, x0, x1, _, t = O.select_scene(257)
    E, nsol = EP.five_point(x0, x1, EP.ransac_samples(257, rounds), ctx=gpu_ctx)
    models = E.reshape(-1, 3, 3)
    assert (nsol > 0).any() and (nsol < 10).any()
    assert np.array_equal(EP.score_models(models, x0, x1, t, ctx=gpu_ctx), O.score_models(models, x0, x1, t))


# ---------------------------------------------------------------------------------------------------------------------- solver
def check_solutions(E, nsol):
    assert E.dtype == np.float64 and np.isfinite(E).all() and (0 <= nsol).all() and (nsol <= 10).all()
    for r in range(E.shape[0]):
        assert np.abs(np.linalg.norm(E[r, :nsol[r]], axis=(1, 2)) - 1.0).max(initial=0.0) <= 4 * O.EPS
        assert not E[r, nsol[r]:].any()


@pytest.mark.parametrize("planar", [False, True])
def test_solver_against_the_oracle(gpu_ctx, planar):
    """On the admitted samples: as many solutions as the oracle, each within c kappa eps of one of the oracle's up to sign, the
    residuals within the same bound.  c is 16 times the oracle's own largest distance / (kappa eps) to the true E (about 6.1e3).
    Measured on an MI355X: see DESIGN.md, "Essential-matrix filter"."""
    sc = O.solver_scene(planar)
    c = O.solver_bound_factor()
    E, nsol = EP.five_point(sc["x0"], sc["x1"], sc["samples"], ctx=gpu_ctx)
    check_solutions(E, nsol)
    worst_pair = worst_res = worst_true = 0.0
    for r, (rec, s) in enumerate(zip(sc["recs"], sc["samples"])):
        if not rec["admitted"]:
            continue
        assert nsol[r] == len(rec["E"]), f"sample {r}: {nsol[r]} solutions, the oracle has {len(rec['E'])}"
        b = rec["kappa"] * O.EPS
        for k in range(nsol[r]):
            worst_pair = max(worst_pair, min(O.distance(E[r, k], F) for F in rec["E"]) / b)
            worst_res = max(worst_res, O.residuals(E[r, k], sc["x0"][s], sc["x1"][s]) / b)
        worst_true = max(worst_true, min(O.distance(E[r, k], sc["Et"]) for k in range(nsol[r])) / b)
    print(f"planar {planar}: in kappa eps: to the oracle's solutions {worst_pair:.4g}, residuals {worst_res:.4g}, to the true E {worst_true:.4g}; "
          f"bound {c:.4g}")
    assert worst_pair <= c and worst_res <= c and worst_true <= c


@pytest.mark.parametrize("rounds", O.ROUNDS)
def test_solver_does_not_depend_on_the_launch(gpu_ctx, rounds):
    """the first `rounds` samples alone give what they give among 1024: across the workgroup of 64 and its edges"""
    _, x0, x1, _, _ = O.select_scene(257)
    table = EP.ransac_samples(257, 1024)
    whole = solver_1024(gpu_ctx, x0, x1, table)
    E, nsol = EP.five_point(x0, x1, table[:rounds], ctx=gpu_ctx)
    check_solutions(E, nsol)
    assert np.array_equal(E, whole[0][:rounds]) and np.array_equal(nsol, whole[1][:rounds])


_whole = {}


def solver_1024(ctx, x0, x1, table):
    if "r" not in _whole:
        _whole["r"] = EP.five_point(x0, x1, table, ctx=ctx)
    return _whole["r"]


def test_solver_equal_and_degenerate_samples(gpu_ctx):
    _, x0, x1, _, _ = O.select_scene(64)
    table = np.array([[3, 9, 20, 41, 60], [1, 2, 3, 4, 5], [3, 9, 20, 41, 60], [7, 7, 9, 30, 31], [5, 5, 5, 5, 5], [60, 41, 20, 9, 3]], np.int32)
    E, nsol = EP.five_point(x0, x1, table, ctx=gpu_ctx)
    check_solutions(E, nsol)
    assert np.array_equal(E[0], E[2]) and nsol[0] == nsol[2] and nsol[0] >= 2
    x0n = x0.copy()
    x0n[9, 0] = np.nan                                       # a match that is not a number: no solution, nothing non-finite
    En, nn = EP.five_point(x0n, x1, table, ctx=gpu_ctx)
    check_solutions(En, nn)
    assert nn[0] == 0 and np.array_equal(En[1], E[1])


# ------------------------------------------------------------------------------------------------------------------- selection
@pytest.mark.parametrize("m", [64, 257])
def test_selection(gpu_ctx, m):
    g, x0, x1, inl, t = O.select_scene(m)
    for table, first in ((EP.ransac_samples(m, O.SELECT["rounds"]), None), (tie_table(m), 0)):
        want = O.find_essential(x0, x1, t, table)
        got = EP.find_essential(x0, x1, t, samples=table, ctx=gpu_ctx)
        assert got.sample == want["sample"] and (first is None or got.sample == first)
        assert got.count == want["count"] == inl.sum() and np.array_equal(got.mask, want["mask"])
        assert O.distance(got.E, want["E"]) <= O.solver_bound_factor() * want["rec"]["kappa"] * O.EPS
        E, nsol = EP.five_point(x0, x1, table, ctx=gpu_ctx)
        assert 0 <= got.solution < nsol[got.sample] and np.array_equal(E[got.sample, got.solution], got.E)
        assert np.array_equal(got.mask, O.inlier_mask(got.E, x0, x1, t)) and same(got.err, O.sampson_err(got.E, x0, x1))
        counts = EP.score_models(E.reshape(-1, 3, 3), x0, x1, t, ctx=gpu_ctx)
        valid = (np.arange(10)[None] < nsol[:, None]).reshape(-1)
        assert got.sample * 10 + got.solution == int(np.flatnonzero(valid & (counts == counts[valid].max()))[0])       # the lowest index
    default = EP.find_essential(x0, x1, t, rounds=O.SELECT["rounds"], ctx=gpu_ctx)
    assert default.sample == got_sample_of(x0, x1, t, m) and default.count == inl.sum()


def got_sample_of(x0, x1, t, m):
    return O.find_essential(x0, x1, t, EP.ransac_samples(m, O.SELECT["rounds"]))["sample"]


def test_five_matches(gpu_ctx):
    """M = 5: every sample is the five matches in some order; the first solution with the largest count wins"""
    _, x0, x1, _, t = O.select_scene(64)
    x0, x1 = x0[[3, 9, 20, 41, 60]], x1[[3, 9, 20, 41, 60]]
    r = EP.find_essential(x0, x1, t, rounds=1, ctx=gpu_ctx)
    assert r.sample == 0 and r.solution >= 0 and r.count == 5 and r.mask.all()
    r6 = EP.find_essential(np.concatenate([x0, x0[:1] + 0.3]), np.concatenate([x1, x1[:1]]), t, rounds=64, ctx=gpu_ctx)
    assert r6.count >= 5


# ------------------------------------------------------------------------------------------------------------------ end to end
def test_noisy_scene_meets_the_references_bars(gpu_ctx):
    g, loc_a, loc_b, _ = O.noisy_scene()
    r = EP.epipolar_filter(loc_a, loc_b, g[0], g[1], rounds=O.NOISY["rounds"], ctx=gpu_ctx)
    dR, dT = np.abs(r.R - g[2]).max(), np.abs(r.T[:, 0] - g[3]).max()
    print(f"|R - Rgt| {dR:.3g}, |T - Tgt| {dT:.3g}, avg epipolar error {r.stats[0]:.3g} px, {r.mask.sum()} matches kept of {r.mask_epi.sum()}")
    assert dR <= O.R_MAX_ERR and dT <= O.T_MAX_ERR and r.stats[0] <= O.MAX_EPI_ERROR and r.mask.sum() >= O.MIN_MATCHES
    x0, x1 = EP.normalise(loc_a, g[0]), EP.normalise(loc_b, g[1])
    assert np.array_equal(r.mask_epi, O.inlier_mask(r.E, x0, x1, r.threshold)) and r.best.count == r.mask_epi.sum()
    assert not (r.mask & ~r.mask_epi).any() and r.T.shape == (3, 1) and abs(np.linalg.norm(r.T) - 1.0) <= 1e-12
    assert np.allclose(r.F, O.fundamental(r.E, g[0], g[1]), rtol=1e-12, atol=0)
    mr = match.MatchResult(np.zeros((len(loc_a), 2), np.int32), loc_a, loc_b)
    again = EP.epipolar_filter(mr, g[0], g[1], rounds=O.NOISY["rounds"], ctx=gpu_ctx)
    assert np.array_equal(again.E, r.E) and np.array_equal(again.mask, r.mask) and again.stats == r.stats


def results_equal(a, b):
    return (all(np.array_equal(getattr(a, k), getattr(b, k)) for k in ("E", "F", "mask_epi", "mask", "R", "T")) and a.stats == b.stats
            and (a.best.sample, a.best.solution, a.best.count) == (b.best.sample, b.best.solution, b.best.count) and same(a.best.err, b.best.err))


def test_batch_equals_singles(gpu_ctx):
    pairs = []
    for k, m in enumerate((65, 257, 130)):
        g = O.rig(20 + k)
        loc_a, loc_b, _, _, _ = O.scene(g, m, 60 + k, noise=0.2, outliers=0.3)
        pairs.append((loc_a, loc_b, g[0], g[1]))
    singles = [EP.epipolar_filter(*p, rounds=128, ctx=gpu_ctx) for p in pairs]
    assert len({s.threshold for s in singles}) == 3 and all(s.best.count >= 0.5 * len(p[0]) for s, p in zip(singles, pairs))
    for order in ((0, 1, 2), (2, 0, 1)):
        got = EP.epipolar_filter_batch([pairs[i] for i in order], rounds=128, ctx=gpu_ctx)
        for i, r in zip(order, got):
            assert results_equal(r, singles[i]), f"pair {i} in the order {order}"
    assert EP.epipolar_filter_batch([], ctx=gpu_ctx) == []


def test_filter_workdir(gpu_ctx, tmp_path, capsys):
    g, loc_a, loc_b, _ = O.noisy_scene()
    match.write_matches(tmp_path / "matches_unfiltered.txt", loc_a, loc_b)
    EP.write_opencv_matrix(tmp_path / "intrinsics_00000000.xml", "intr", g[0])
    EP.write_opencv_matrix(tmp_path / "intrinsics_00000001.xml", "intr", g[1])
    (tmp_path / "cfg.txt").write_text("MATCHER_MAX_EPI_DISTANCE=0.5\n")
    assert EP.filter_workdir(tmp_path, tmp_path / "cfg.txt", ctx=gpu_ctx) == 0
    assert capsys.readouterr().out.strip().endswith("[P|100|100]")
    r = EP.epipolar_filter(loc_a, loc_b, g[0], g[1], ctx=gpu_ctx)
    assert np.array_equal(gridding.read_opencv_matrix(tmp_path / "ext_R.xml", "ext_R"), r.R)
    assert np.array_equal(gridding.read_opencv_matrix(tmp_path / "ext_T.xml", "ext_T"), r.T)
    for name, mask in (("matches.txt", r.mask), ("matches_epionly.txt", r.mask_epi)):
        a, b = match.read_matches(tmp_path / name)
        assert np.array_equal(a, loc_a[mask]) and np.array_equal(b, loc_b[mask])
    head, row = (tmp_path / "matcher_stats.csv").read_text().splitlines()
    assert head == "N.Matches;Avg. Error;Std. Error;Min. Error;Max. Error"
    vals = row.split(";")
    assert int(vals[0]) == r.mask.sum() and [float(v) for v in vals[1:]] == [float(format(v, ".15g")) for v in r.stats]
    wide = tmp_path / "wide.txt"
    wide.write_text("MATCHER_MAX_EPI_DISTANCE=2.0\n")
    assert EP.filter_workdir(tmp_path, wide, ctx=gpu_ctx) == 0
    assert len(match.read_matches(tmp_path / "matches_epionly.txt")[0]) > r.mask_epi.sum()
    (tmp_path / "intrinsics_00000001.xml").unlink()
    assert EP.filter_workdir(tmp_path, ctx=gpu_ctx) == -1
    four = tmp_path / "four"
    four.mkdir()
    match.write_matches(four / "matches_unfiltered.txt", loc_a[:4], loc_b[:4])
    EP.write_opencv_matrix(four / "intrinsics_00000000.xml", "intr", g[0])
    EP.write_opencv_matrix(four / "intrinsics_00000001.xml", "intr", g[1])
    assert EP.filter_workdir(four, ctx=gpu_ctx) == -1


def test_argument_errors(gpu_ctx):
    _, x0, x1, _, t = O.select_scene(64)
    good = EP.ransac_samples(64, 4)
    for bad in (lambda: EP.five_point(x0[:4], x1[:4], good, ctx=gpu_ctx), lambda: EP.five_point(x0, x1[:60], good, ctx=gpu_ctx),
                lambda: EP.five_point(x0, x1, [[0, 1, 2, 3, 64]], ctx=gpu_ctx), lambda: EP.five_point(x0, x1, good[:, :4], ctx=gpu_ctx),
                lambda: EP.find_essential(x0, x1, t, rounds=0, ctx=gpu_ctx), lambda: EP.find_essential(x0, x1, -t, ctx=gpu_ctx),
                lambda: EP.find_essential_batch([(x0, x1), (x0, x1)], t, samples=[good, good[:2]], ctx=gpu_ctx),
                lambda: EP.score_models(np.zeros((0, 3, 3)), x0, x1, t, ctx=gpu_ctx), lambda: EP.inlier_mask(np.zeros(9), x0, x1, t, ctx=gpu_ctx),
                lambda: EP.epipolar_filter(x0[:4], x1[:4], np.eye(3), np.eye(3), ctx=gpu_ctx)):
        with pytest.raises(ValueError):
            bad()
    # the library's own check: an index past the pair is refused after a launch that read nothing out of bounds
    import torch
    import wass_amd
    d = [torch.from_numpy(np.ascontiguousarray(v)).cuda() for v in (x0, x1, np.array([[0, 1, 2, 3, 64]], np.int32))]
    d_E, d_n = torch.empty(90, dtype=torch.float64, device="cuda"), torch.empty(1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    with pytest.raises(wass_amd.WassError):
        gpu_ctx._check(gpu_ctx._lib.wass_epi_solve5_dev(gpu_ctx._h, d[0].data_ptr(), d[1].data_ptr(), 128, d[2].data_ptr(), 5, match._ints([64]), 1, 1,
                                                        d_E.data_ptr(), d_n.data_ptr()))
    assert int(d_n.cpu()[0]) == 0 and not d_E.cpu().numpy().any()
