"""The feature matcher without a GPU: the numpy oracle (tests/match_oracle.py) against the reference's own compiled dynamics
(tests/golden/match_iidyn.npz, recorded by tests/golden/make_golden_match.py), the conditions every probe input of the CPU and GPU
tests has to meet, closed forms of the payoff, and the host logic, files and argument checks of wass_amd.match."""
import os
import struct

import numpy as np
import pytest

import match_oracle as M
from wass_amd import match

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "match_iidyn.npz")
ORDERS = ("sequential", "pairwise", "reversed")
FULL_SCENE = 1                                               # the scene the GPU runs to the end


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


def scene_payoff(golden, s):
    fa, fb, da, db = (golden[f"scene{s}_{k}"] for k in ("fa", "fb", "da", "db"))
    idx, _, _ = M.knn(da, db, 3)
    return M.payoff(fa, fb, M.candidates(idx), float(golden[f"scene{s}_lambda"]))[0]


def check_orders(A, iters, label):
    """the condition on a probe matrix: the three orders of the sums agree within 8 N eps and in the group, and no population value
    lies within a relative 1e-6 of the group threshold"""
    n = A.shape[0]
    runs = {how: M.iidyn(A, max_iters=iters, summation=how)[0] for how in ORDERS}
    ref = runs["sequential"]
    for how in ORDERS[1:]:
        d = np.abs(runs[how] - ref).max()
        assert d <= M.bound(n), f"{label}: {how} sums move the population by {d:g} > {M.bound(n):g}"
        assert np.array_equal(M.group(runs[how]), M.group(ref)), f"{label}: {how} sums change the group"
    assert M.threshold_margin(ref) > 1e-6, f"{label}: a population value sits on the group threshold"
    return ref


# ------------------------------------------------------------------------------------------- the oracle against the reference
def test_random_matrices_match_the_recorded_reference(golden):
    worst = 0.0
    for n in golden["random_sizes"]:
        for d in golden["densities"]:
            key = f"random_{n}_{int(round(d * 100))}"
            A = M.random_symmetric(int(n), float(d), M.random_seed(int(n), float(d)))
            assert A.sum() == golden[key + "_sum"], f"{key}: the seeded matrix is not the recorded one"
            x, _, _ = M.iidyn(A, max_iters=int(golden["random_steps"]))
            xr = golden[key + "_x"]
            worst = max(worst, np.abs(x - xr).max() / M.bound(int(n)))
            assert np.abs(x - xr).max() <= M.bound(int(n)), key
            assert np.array_equal(M.group(x), M.group(xr)), key
    print(f"largest |oracle - reference| / (8 N eps) over the random matrices: {worst:g}")


def test_scenes_match_the_recorded_reference_and_hold_true_matches(golden):
    for s in range(4):
        P = scene_payoff(golden, s)
        x, _, _ = M.iidyn(P, max_iters=int(golden["random_steps"]))
        xr = golden[f"scene{s}_short_x"]
        assert np.abs(x - xr).max() <= M.bound(P.shape[0])
        assert np.array_equal(M.group(x), M.group(xr))
        idx, _, _ = M.knn(golden[f"scene{s}_da"], golden[f"scene{s}_db"], 3)
        cand = M.candidates(idx)
        win = cand[M.group(golden[f"scene{s}_full_x"])]
        assert win.shape[0] >= 5 and golden[f"scene{s}_truth"][win[:, 0]].all() and np.array_equal(win[:, 0], win[:, 1])


def test_full_scene_matches_the_recorded_reference_in_every_order(golden):
    P = scene_payoff(golden, FULL_SCENE)
    x = check_orders(P, int(golden["max_iters"]), "full scene")
    xr = golden[f"scene{FULL_SCENE}_full_x"]
    assert np.abs(x - xr).max() <= M.bound(P.shape[0])
    assert np.array_equal(M.group(x), M.group(xr))


def test_clique_and_degenerate_cases_match_the_recording(golden):
    for name in golden["special_names"]:
        A, xr = golden[f"special_{name}_A"], golden[f"special_{name}_x"]
        x, steps, _ = M.iidyn(A)
        assert np.array_equal(x > 0, xr > 0), name
        assert np.abs(x - xr).max() <= M.bound(A.shape[0]), name
        assert steps == int(golden[f"special_{name}_steps"]), name       # same order of sums: the oracle is the reference here
    third, eighth = 1.0 / 3.0, 0.125
    assert np.allclose(golden["special_cliques_3_3_x"], [0, 0, 0, third, third, third], atol=1e-15) and golden["special_cliques_3_3_steps"] == 38
    assert np.allclose(golden["special_cliques_4_4_1_x"], [eighth] * 8 + [0.0], atol=1e-15) and golden["special_cliques_4_4_1_x"][8] == 0 and golden["special_cliques_4_4_1_steps"] == 1
    for name, n in (("zeros_5", 5), ("single", 1)):
        assert golden[f"special_{name}_steps"] == 0 and np.allclose(golden[f"special_{name}_x"], np.full(n, 1.0 / n), atol=1e-15)


# ----------------------------------------------------------------------------------------------- conditions on the probe inputs
@pytest.mark.parametrize("n", M.GPU_SIZES)
def test_random_probe_matrices_meet_the_conditions(n):
    for d in M.DENSITIES:
        A = M.random_symmetric(n, d, M.random_seed(n, d))
        x = check_orders(A, M.PROBE_STEPS, f"N = {n}, density {d}")
        t = M.iidyn(A, max_iters=M.PROBE_STEPS, summation="tree")[0]      # the kernel's own tree, predicted on the CPU
        assert np.abs(t - x).max() <= M.bound(n) and np.array_equal(M.group(t), M.group(x))


def test_scene_and_special_probe_matrices_meet_the_conditions(golden):
    for s in range(4):
        check_orders(scene_payoff(golden, s), M.PROBE_STEPS, f"scene {s}")
    for name in golden["special_names"]:
        A = golden[f"special_{name}_A"]
        runs = [M.iidyn(A, summation=how, max_iters=2000)[0] for how in ORDERS]
        for x in runs[1:]:
            assert np.array_equal(x > 0, runs[0] > 0) and np.abs(x - runs[0]).max() <= M.bound(A.shape[0]), name
        assert M.threshold_margin(runs[0]) > 1e-6


def test_tie_probe_and_matcher_scenes_meet_the_conditions(golden):
    x = check_orders(M.tie_probe(), M.PROBE_STEPS, "tie probe")
    assert np.array_equal(np.flatnonzero(x > 0), np.arange(80, 140))
    scenes = [(tuple(golden[f"scene{s}_{k}"] for k in ("fa", "fb", "da", "db")), float(golden[f"scene{s}_lambda"])) for s in range(4)]
    scenes += [(p, M.BATCH_LAMBDA) for p in M.batch_problems(scenes[0][0])]
    for i, ((fa, fb, da, db), lam) in enumerate(scenes):
        # every round's matrix at once: the three orders must give the same matches, round by round, from margins that are not thin
        margins = []

        def run(how):
            def dynamics(P):
                x, steps, err = M.iidyn(P, max_iters=M.PROBE_STEPS, summation=how)
                margins.append(M.threshold_margin(x))
                return x, steps, err
            return M.gt_match(fa, fb, da, db, lam=lam, dynamics=dynamics)
        lists = [run(how) for how in ORDERS]
        for m, r in lists[1:]:
            assert np.array_equal(m, lists[0][0]) and [(n, g) for n, _, g in r] == [(n, g) for n, _, g in lists[0][1]], f"matcher scene {i}"
        assert min(margins) > 1e-6, f"matcher scene {i}"
    assert len(lists[0][1]) > 1 and len(M.gt_match(*scenes[7][0], lam=M.BATCH_LAMBDA, max_iters=M.PROBE_STEPS)[1]) == 1


def test_the_matrix_at_the_cap_meets_the_conditions():
    fa, fb, cand = M.big_scene()
    assert cand.shape[0] == M.BIG_N == match.MAX_N
    P, _, _ = M.payoff(fa, fb, cand, M.BIG_LAMBDA)
    check_orders(P, M.BIG_STEPS, "N = 8192")


# -------------------------------------------------------------------------------------------------------- payoff, closed forms
def exact_pair(n=6):
    """integer positions, a scale ratio of 2, no rotation, an integer shift: every transfer error is exactly 0"""
    xy = np.array([[3, 4], [10, 2], [7, 9], [1, 12], [15, 6], [8, 8]][:n], np.float32)
    fa = np.column_stack([xy, np.full(n, 2.0), np.full(n, 0.5)]).astype(np.float32)
    fb = np.column_stack([2 * xy + np.array([5, -3]), np.full(n, 4.0), np.full(n, 0.5)]).astype(np.float32)
    cand = np.stack([np.arange(n), np.arange(n)], axis=1).astype(np.int32)
    return fa, fb, cand


def test_payoff_of_an_exact_similarity_is_one_off_the_exclusions():
    fa, fb, cand = exact_pair()
    P, ge, excl = M.payoff(fa, fb, cand, 1e-3)
    assert np.array_equal(excl, np.eye(6, dtype=bool)) and np.all(ge[~excl] == 0) and np.all(P[~excl] == 1.0) and np.all(P[excl] == 0.0)


def test_payoff_of_one_displaced_target_takes_the_larger_error():
    fa, fb, cand = exact_pair()
    fb[2, 0] += 6.0                                          # candidate 2's target, 6 px off: its own transform moves with it
    lam = 1e-3
    P, ge, _ = M.payoff(fa, fb, cand, lam)
    # T_2 applied to another source misses by 6 px; T_i applied to source 2 misses target 2 by 6 px as well: d^2 = 36 either way
    assert np.all(ge[2, [0, 1, 3, 4, 5]] == 36.0) and np.all(P[2, [0, 1, 3, 4, 5]] == np.exp(-lam * 36.0))
    fb2 = fb.copy()
    fb2[2, 2] = 8.0                                          # and a scale ratio of 4 for candidate 2 alone: the two errors differ
    P2, ge2, _ = M.payoff(fa, fb2, cand, lam)
    Pmin, gemin, _ = M.payoff(fa, fb2, cand, lam, geo="min")
    assert np.all(ge2[2, [0, 1]] > gemin[2, [0, 1]]) and np.all(P2[2, [0, 1]] < Pmin[2, [0, 1]])      # the probe catches min for max
    s0, t0 = fa[0, :2].astype(np.float64), fb2[0, :2].astype(np.float64)
    s2, t2 = fa[2, :2].astype(np.float64), fb2[2, :2].astype(np.float64)
    e_20 = np.sum((t0 - (4.0 * s0 + (t2 - 4.0 * s2))) ** 2)  # T_2 on source 0 against target 0
    e_02 = np.sum((t2 - (2.0 * s2 + (t0 - 2.0 * s0))) ** 2)  # T_0 on source 2 against target 2
    assert ge2[2, 0] == max(e_20, e_02) and gemin[2, 0] == min(e_20, e_02) and P2[2, 0] == np.exp(-lam * max(e_20, e_02))


def test_payoff_exclusions_and_symmetry():
    fa, fb, _, _, _ = M.scene(5, n=20)
    cand = np.array([[0, 0], [0, 1], [1, 1], [2, 1], [3, 3], [4, 5], [5, 4]], np.int32)
    P, _, excl = M.payoff(fa, fb, cand, 1e-8)
    want = np.eye(7, dtype=bool)
    for i, j in ((0, 1), (1, 2), (1, 3), (2, 3)):
        want[i, j] = want[j, i] = True
    assert np.array_equal(excl, want) and np.all(P[excl] == 0) and np.all(P[~excl] > 0) and np.array_equal(P, P.T)


def test_payoff_angles_across_pi_go_through_ang_diff():
    fa, fb, cand = exact_pair(4)
    for a_src, a_tgt, want in ((0.1, 6.2, 0.1 - 6.2 + 2 * np.pi), (6.2, 0.1, 6.2 - 0.1 - 2 * np.pi), (3.2, 0.0, 3.2 - 2 * np.pi), (0.0, 3.2, -3.2 + 2 * np.pi)):
        d = M.ang_diff(np.float32(a_tgt), np.float32(a_src), np.float64)
        assert abs(d) <= np.pi and abs(d - want) < 1e-6
        fa[:, 3], fb[:, 3] = a_src, a_tgt
        P, ge, excl = M.payoff(fa, fb, cand, 1e-3)
        # rotating everything by the same angle about the origin is NOT this scene's transform: the errors are those of a rotation by d
        c, s = np.cos(d), np.sin(d)
        x = 2.0 * (fa[1, 0] * c - fa[1, 1] * s) + (fb[0, 0] - 2.0 * (fa[0, 0] * c - fa[0, 1] * s))
        y = 2.0 * (fa[1, 0] * s + fa[1, 1] * c) + (fb[0, 1] - 2.0 * (fa[0, 0] * s + fa[0, 1] * c))
        e01 = (fb[1, 0] - x) ** 2 + (fb[1, 1] - y) ** 2
        assert ge[0, 1] >= e01 * (1 - 1e-12) and P[0, 1] <= np.exp(-1e-3 * e01 * (1 - 1e-12))


# ------------------------------------------------------------------------------------------------------------------------- kNN
def test_knn_scenes_have_clear_gaps_and_equal_descriptors_tie_to_the_lower_index(golden):
    for s in range(4):
        da, db = golden[f"scene{s}_da"], golden[f"scene{s}_db"]
        idx, d, sd = M.knn(da, db, 3)
        assert np.all((sd[:, 1:4] - sd[:, 0:3]) > 1e-5 * sd[:, 1:4]), "a scene's neighbour distances are too close to call in float32"
        assert np.array_equal(idx[golden[f"scene{s}_truth"], 0], np.flatnonzero(golden[f"scene{s}_truth"]))
    b = np.zeros((5, 4), np.float32)
    b[3] = 1.0
    idx, d, _ = M.knn(np.zeros((2, 4), np.float32), b, 3)
    assert np.array_equal(idx, [[0, 1, 2], [0, 1, 2]]) and np.all(d == 0)
    idx, _, _ = M.knn(np.ones((1, 4), np.float32), b, 8)
    assert np.array_equal(idx, [[3, 0, 1, 2, 4]])            # k clamped to nb


# ------------------------------------------------------------------------------------------------------------------ host logic
def test_removal_loop_keeps_the_swapped_in_candidate():
    """The reference overwrites a removed candidate with the last one and moves on: (0, 3) lands in slot 0 after slot 0 was looked
    at, so it survives although source 0 has won.  A removal that looked again would drop it; the product keeps the reference's list,
    because the matches of later rounds (and with them matches_unfiltered.txt) follow from it."""
    cand = np.array([[0, 0], [1, 1], [2, 2], [0, 3]], np.int32)
    win = np.array([[0, 0]], np.int32)
    got = match.remove_candidates(cand, win)
    assert np.array_equal(got, [[0, 3], [1, 1], [2, 2]])
    assert np.array_equal(got, M.remove_candidates(cand, win))
    correct = M.remove_candidates_all(cand, win)
    assert np.array_equal(correct, [[1, 1], [2, 2]]) and not np.array_equal(got, correct)
    # two removals in a row: the second swap brings (3, 0) forward, which is looked at because it lands in a later slot
    cand = np.array([[0, 0], [1, 1], [0, 2], [3, 0], [0, 4]], np.int32)
    assert np.array_equal(match.remove_candidates(cand, win), M.remove_candidates(cand, win))
    assert np.array_equal(match.remove_candidates(cand, win), [[0, 4], [1, 1], [3, 0]])


def test_round_loop_runs_at_most_max_rounds_plus_one():
    cand = np.stack([np.arange(400), np.arange(400)], axis=1).astype(np.int32)
    first5 = lambda live, cands: [(7, np.arange(5)) for _ in live]
    matches, rounds = match.round_loop([cand], first5, min_group_size=5, max_rounds=20)
    assert len(rounds[0]) == 21 and len(matches[0]) == 105 and rounds[0][0] == (400, 7, 5) and rounds[0][-1][0] == 400 - 100
    matches, rounds = match.round_loop([cand], first5, min_group_size=5, max_rounds=0)
    assert len(rounds[0]) == 1 and len(matches[0]) == 5


def test_round_loop_appends_a_small_last_group_and_stops_on_an_empty_list():
    cand = np.stack([np.arange(40), np.arange(40)], axis=1).astype(np.int32)
    sizes = iter([6, 5, 2, 9])
    matches, rounds = match.round_loop([cand], lambda live, cands: [(1, np.arange(next(sizes)))], min_group_size=5, max_rounds=20)
    assert [r[2] for r in rounds[0]] == [6, 5, 2] and len(matches[0]) == 13      # the group of 2 is appended, then the loop ends
    everything = lambda live, cands: [(3, np.arange(cands[p].shape[0])) for p in live]
    # every candidate wins and the removal loop (which skips the slot it has just refilled) leaves about half each time: the list
    # runs empty well before the rounds run out, and the loop stops there instead of playing a game without strategies
    matches, rounds = match.round_loop([cand, cand[:1]], everything, min_group_size=1, max_rounds=20)
    assert [r[0] for r in rounds[0]] == [40, 20, 10, 5, 2, 1] and [r[0] for r in rounds[1]] == [1]
    assert [len(m) for m in matches] == [78, 1] and all(r[0] == r[2] for r in rounds[0])
    assert match.round_loop([np.zeros((0, 2), np.int32)], everything) == ([[]], [[]])


def test_round_loop_with_the_oracle_dynamics_is_the_oracle_matcher(golden):
    s = 0
    fa, fb, da, db = (golden[f"scene{s}_{k}"] for k in ("fa", "fb", "da", "db"))
    lam = float(golden[f"scene{s}_lambda"])
    want, want_rounds = M.gt_match(fa, fb, da, db, lam=lam, max_iters=M.PROBE_STEPS)

    def run(live, cands):
        out = []
        for p in live:
            x, steps, _ = M.iidyn(M.payoff(fa, fb, cands[p], lam)[0], max_iters=M.PROBE_STEPS)
            out.append((steps, M.group(x)))
        return out
    matches, rounds = match.round_loop([M.candidates(M.knn(da, db, 3)[0])], run)
    assert np.array_equal(np.array(matches[0]), want) and rounds[0] == want_rounds and len(want_rounds) >= 2
    sources = want[:, 0]
    print(f"{want.shape[0]} matches in {len(want_rounds)} rounds, {want.shape[0] - np.unique(sources).size} sources matched twice")


def test_skip_gt_is_the_nndr_list():
    idx = np.array([[4, 1], [2, 0], [3, 3]], np.int32)
    dist = np.array([[1.0, 8.0], [1.0, 4.0], [0.0, 0.0]], np.float32)
    assert np.array_equal(match.nndr_matches(idx, dist, 2, 0.25), [[0, 4]])      # strict: 1 < 0.25 * 4 is false, 0 < 0 too
    assert match.nndr_matches(idx, dist, 1, 0.25).shape == (0, 2)
    assert np.array_equal(match.nndr_matches(idx, dist, 2, 0.25), M.nndr_matches(idx, dist, 2, 0.25))


# ----------------------------------------------------------------------------------------------------------------------- files
def test_feature_file_round_trip_and_bytes(tmp_path):
    f = match.Features(xy=[[1.5, 2.25], [3, 4]], scale=[2, 0.5], angle=[0.25, 6.0], desc=[[1, 2, 3], [4, 5, 6]])
    p = tmp_path / "f.bin"
    match.write_features(p, f)
    by_hand = struct.pack("<II", 2, 3) + struct.pack("<7f", 1.5, 2.25, 2, 0.25, 1, 2, 3) + struct.pack("<7f", 3, 4, 0.5, 6.0, 4, 5, 6)
    assert p.read_bytes() == by_hand
    g = match.read_features(p)
    for k in ("xy", "scale", "angle", "desc"):
        assert np.array_equal(getattr(f, k), getattr(g, k)) and getattr(g, k).dtype == np.float32
    assert np.array_equal(g.table(), [[1.5, 2.25, 2, 0.25], [3, 4, 0.5, 6.0]])
    (tmp_path / "short.bin").write_bytes(by_hand[:-4])
    with pytest.raises(ValueError):
        match.read_features(tmp_path / "short.bin")


def test_match_file_round_trip_and_text(tmp_path):
    a = np.array([[100.5, 200.25], [np.float32(0.1), 3]], np.float32)
    b = np.array([[7, 8], [1234.5678, 1e-3]], np.float32)
    p = tmp_path / "matches_unfiltered.txt"
    match.write_matches(p, a, b)
    lines = p.read_text().split("\n")
    assert lines[0] == "2" and lines[1] == "100.5 200.25 7 8" and lines[3] == ""
    assert lines[2] == "0.100000001490116 3 1234.56774902344 0.00100000004749745"      # float32 widened, 15 significant digits
    ra, rb = match.read_matches(p)
    assert np.array_equal(ra, a) and np.array_equal(rb, b)
    match.write_matches(p, match.MatchResult(np.zeros((0, 2), np.int32), np.zeros((0, 2), np.float32), np.zeros((0, 2), np.float32)))
    assert p.read_text() == "0\n"


# ------------------------------------------------------------------------------------------------------------- argument errors
def test_argument_errors_come_before_any_launch():
    with pytest.raises(ValueError, match="cap"):
        match.iidyn(np.zeros((match.MAX_N + 1, match.MAX_N + 1)))
    with pytest.raises(ValueError, match="non-contiguous"):
        match.iidyn(np.zeros((8, 8)).T[::2, ::2])
    with pytest.raises(ValueError, match="square"):
        match.iidyn(np.zeros((3, 4)))
    with pytest.raises(ValueError, match="start"):
        match.iidyn(np.zeros((3, 3)), x0=np.ones(4))
    with pytest.raises(ValueError, match="k = 9"):
        match.knn_candidates(np.zeros((4, 8), np.float32), np.zeros((4, 8), np.float32), 9)
    with pytest.raises(ValueError, match="cannot be compared"):
        match.knn_candidates(np.zeros((4, 8), np.float32), np.zeros((4, 16), np.float32), 3)
    with pytest.raises(ValueError, match="descriptors of 300"):
        match.knn_candidates(np.zeros((4, 300), np.float32), np.zeros((4, 300), np.float32), 3)
    fa, fb, cand = exact_pair()
    with pytest.raises(ValueError, match="outside"):
        match.payoff_matrix(fa, fb, np.array([[0, 6]], np.int32))
    with pytest.raises(ValueError, match="n x 4"):
        match.payoff_matrix(fa[:, :3], fb, cand)
    with pytest.raises(ValueError):
        match.Features(np.zeros((3, 2)), np.zeros(3), np.zeros(2), np.zeros((3, 8)))
    big = match.Features(np.zeros((3000, 2)), np.ones(3000), np.zeros(3000), np.zeros((3000, 8)))
    with pytest.raises(ValueError, match="cap"):
        match.gt_match(big, big)
    small = match.Features(np.zeros((4, 2)), np.ones(4), np.zeros(4), np.zeros((4, 16)))
    with pytest.raises(ValueError, match="cannot be compared"):
        match.gt_match(big, small)
    assert match.scratch_bytes(16, 6000) > 16 * 6000 * 6000 * 8
    with pytest.raises(ValueError):
        match.scratch_bytes(1, match.MAX_N + 1)


# ------------------------------------------------------------------------------------------- each probe catches its mistake
def test_probes_catch_the_mistakes_they_are_there_for(golden):
    # last-index ties: the clique probes end on other strategies
    for name in ("cliques_3_3", "interleaved_3_3"):
        A, xr = golden[f"special_{name}_A"], golden[f"special_{name}_x"]
        x, _, _ = M.iidyn(A, ties="last")
        assert not np.array_equal(x > 0, xr > 0) or np.abs(x - xr).max() > M.bound(A.shape[0]), name
    # the minimum taken over all x: every random probe moves
    for n, d in ((65, 0.5), (257, 0.05), (257, 1.0), (1025, 0.5)):
        A = M.random_symmetric(n, d, M.random_seed(n, d))
        x, _, _ = M.iidyn(A, max_iters=M.PROBE_STEPS, min_over="all")
        assert np.abs(x - golden[f"random_{n}_{int(round(d * 100))}_x"]).max() > M.bound(n), (n, d)
    # a missing simplexify: on most probes it is rounding (its sum is 1 to a few ulp), but 4 + 4 + 1 stops after ONE step with eight
    # values of 1/8 only because that step's x sums to 1 exactly after the division; without it the dynamics goes on to one clique
    A, xr = golden["special_cliques_4_4_1_A"], golden["special_cliques_4_4_1_x"]
    x, steps, _ = M.iidyn(A, do_simplexify=False)
    assert not np.array_equal(x > 0, xr > 0) and steps != int(golden["special_cliques_4_4_1_steps"])
    # min in place of max in the geometric error: test_payoff_of_one_displaced_target_takes_the_larger_error shows it on its probe;
    # on a scene it moves the matrix the dynamics runs on
    fa, fb, da, db = (golden[f"scene0_{k}"] for k in ("fa", "fb", "da", "db"))
    cand = M.candidates(M.knn(da, db, 3)[0])
    assert np.abs(M.payoff(fa, fb, cand, 1e-3, geo="min")[0] - M.payoff(fa, fb, cand, 1e-3)[0]).max() > 1e-3
