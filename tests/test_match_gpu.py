"""The feature matcher on the GPU (wass_amd/match.py, csrc/match.hip) against the numpy oracle (tests/match_oracle.py) and the
reference's recorded dynamics (tests/golden/match_iidyn.npz).  Every probe matrix used here is held to the conditions of
tests/test_match.py (the three summation orders agree, no population value sits on the group threshold)."""
import os

import numpy as np
import pytest

import match_oracle as M
from wass_amd import match

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "match_iidyn.npz")
FULL_SCENE = 1


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


def features(fa, fb, da, db):
    return (match.Features(fa[:, :2], fa[:, 2], fa[:, 3], da), match.Features(fb[:, :2], fb[:, 2], fb[:, 3], db))


def golden_scene(golden, s):
    return tuple(golden[f"scene{s}_{k}"] for k in ("fa", "fb", "da", "db"))


def check_population(got, want, n, label):
    """within 8 N eps of the reference population, the same group, and every value above the bound positive in both"""
    b = M.bound(n)
    d = np.abs(got - want).max()
    print(f"{label}: |gpu - reference| = {d:.3g}, bound {b:.3g}")
    assert d <= b, label
    assert np.array_equal(M.group(got), M.group(want)), label
    big = (got > b) | (want > b)
    assert np.all(got[big] > 0) and np.all(want[big] > 0), label


# -------------------------------------------------------------------------------------------------------------------- dynamics
@pytest.mark.parametrize("n", M.GPU_SIZES)
def test_iidyn_random_matrices(gpu_ctx, n):
    mats = [M.random_symmetric(n, d, M.random_seed(n, d)) for d in M.DENSITIES]
    res = match.iidyn(mats, max_iters=M.PROBE_STEPS, ctx=gpu_ctx)                # a batch of three
    for d, A, r in zip(M.DENSITIES, mats, res):
        want, steps, _ = M.iidyn(A, max_iters=M.PROBE_STEPS)
        check_population(r.x, want, n, f"N = {n}, density {d}")
        assert np.array_equal(r.group, M.group(want)) and 0 <= r.steps <= M.PROBE_STEPS
    alone = match.iidyn(mats[1], max_iters=M.PROBE_STEPS, ctx=gpu_ctx)
    assert np.array_equal(alone.x, res[1].x) and alone.steps == res[1].steps and alone.err == res[1].err
    start = np.linspace(1.0, 2.0, n)
    started = match.iidyn(mats[1], x0=start, max_iters=25, ctx=gpu_ctx)
    check_population(started.x, M.iidyn(mats[1], x0=start, max_iters=25)[0], n, f"N = {n}, a start of its own")


def test_iidyn_at_the_cap_on_a_matrix_filled_on_the_device(gpu_ctx):
    import torch
    fa, fb, cand = M.big_scene()
    d_A = match.payoff_matrix(fa, fb, cand, M.BIG_LAMBDA, ctx=gpu_ctx, device=True)
    assert tuple(d_A.shape) == (M.BIG_N, M.BIG_N)
    rng = np.random.default_rng(3)
    I, J = rng.integers(0, M.BIG_N, 4096), rng.integers(0, M.BIG_N, 4096)
    I[:64], J[:64] = np.arange(64) * 128, np.arange(64) * 128 + rng.integers(0, 4, 64) // 2          # some on and next to the diagonal
    got = d_A[torch.from_numpy(I).cuda(), torch.from_numpy(J).cuda()].cpu().numpy()
    check_payoff_entries(got, fa, fb, cand, I, J, M.BIG_LAMBDA, "4096 entries at N = 8192")
    r = match.iidyn(d_A, max_iters=M.BIG_STEPS, ctx=gpu_ctx)
    want, _, _ = M.iidyn(d_A.cpu().numpy(), max_iters=M.BIG_STEPS)
    check_population(r.x, want, M.BIG_N, "N = 8192")
    assert r.steps == M.BIG_STEPS


def test_iidyn_cliques_ties_and_degenerate_matrices(gpu_ctx, golden):
    names = list(golden["special_names"])
    res = match.iidyn([golden[f"special_{k}_A"] for k in names], ctx=gpu_ctx)
    for k, r in zip(names, res):
        xr = golden[f"special_{k}_x"]
        assert np.array_equal(r.x > 0, xr > 0), f"{k}: support {r.x} against the reference's {xr}"
        assert np.abs(r.x - xr).max() <= M.bound(xr.size), k
        assert np.array_equal(r.group, M.group(xr)), k
    # exact ties among more strategies than one wave holds: two cliques of 40 and one of 60 with larger payoffs, which wins
    A = M.tie_probe()
    r = match.iidyn(A, max_iters=M.PROBE_STEPS, ctx=gpu_ctx)
    want, _, _ = M.iidyn(A, max_iters=M.PROBE_STEPS)
    assert np.array_equal(r.x > 0, want > 0) and np.array_equal(np.flatnonzero(r.x > 0), np.arange(80, 140))
    assert np.abs(r.x - want).max() <= M.bound(140)


def test_iidyn_one_scene_to_the_end(gpu_ctx, golden):
    fa, fb, da, db = golden_scene(golden, FULL_SCENE)
    cand = M.candidates(M.knn(da, db, 3)[0])
    A = match.payoff_matrix(fa, fb, cand, float(golden[f"scene{FULL_SCENE}_lambda"]), ctx=gpu_ctx)
    r = match.iidyn(A, ctx=gpu_ctx)                           # 50 000 steps at most, toll 1e-20: the defaults of match_group
    xr = golden[f"scene{FULL_SCENE}_full_x"]
    check_population(r.x, xr, xr.size, "a scene run to the end, against the recorded reference")
    assert golden[f"scene{FULL_SCENE}_truth"][cand[r.group, 0]].all() and r.group.size >= 5 and r.steps <= int(golden["max_iters"])


def test_iidyn_inputs(gpu_ctx):
    import torch
    A = M.random_symmetric(65, 0.5, M.random_seed(65, 0.5))
    host = match.iidyn(A, max_iters=40, ctx=gpu_ctx)
    d_A = torch.from_numpy(A).cuda()
    dev = match.iidyn(d_A, max_iters=40, ctx=gpu_ctx)
    both = match.iidyn([d_A, A], max_iters=40, ctx=gpu_ctx)
    for r in (dev, *both):
        assert np.array_equal(r.x, host.x) and r.steps == host.steps and np.array_equal(r.group, host.group)
    assert np.array_equal(d_A.cpu().numpy(), A)               # read in place, left alone
    with pytest.raises(ValueError, match="non-contiguous"):
        match.iidyn(d_A.t()[::2, ::2], ctx=gpu_ctx)
    with pytest.raises(ValueError, match="non-contiguous"):
        match.iidyn(np.asfortranarray(A + np.arange(65)), ctx=gpu_ctx)
    zero = match.iidyn(A, max_iters=0, ctx=gpu_ctx)
    assert zero.steps == 0 and zero.err == np.finfo(np.float64).max and np.abs(zero.x - 1.0 / 65).max() < 1e-15


# ---------------------------------------------------------------------------------------------------------------------- payoff
def check_payoff_entries(got, fa, fb, cand, I, J, lam, label):
    want, ge, excl = M.payoff_entries(fa, fb, cand, I, J, lam)
    exact, _, _ = M.payoff_entries(fa, fb, cand, I, J, lam, dtype=np.longdouble)
    noise = float(np.abs(want.astype(np.longdouble) - exact).max())
    assert np.all(got[excl] == 0.0), label
    assert np.all(got[~excl & (ge == 0)] == 1.0), label
    tol = 2 * np.spacing(want) + 4 * noise
    err = np.abs(got - want)
    print(f"{label}: largest |gpu - oracle| = {err.max():.3g} (tolerance there {tol.flat[err.argmax()]:.3g}, oracle noise {noise:.3g})")
    assert np.all(err <= tol), label


def payoff_case(n, seed):
    """n candidates over a scene of about n / 2 features: true pairs, wrong pairs, shared sources and shared targets"""
    m = max(2, n // 2 + 1)
    fa, fb, _, _, _ = M.scene(seed, n=m)
    rng = np.random.default_rng(seed)
    cand = np.stack([rng.integers(0, m, n), rng.integers(0, m, n)], axis=1).astype(np.int32)
    half = n // 2
    cand[:half, 1] = cand[:half, 0]                          # true partners
    return fa, fb, cand


@pytest.mark.parametrize("n", (1, 3, 65, 257, 1025))
def test_payoff_matrix_against_the_oracle(gpu_ctx, n):
    fa, fb, cand = payoff_case(n, 40 + n)
    for lam in (1e-5, 1e-3):
        got = match.payoff_matrix(fa, fb, cand, lam, ctx=gpu_ctx)
        assert got.shape == (n, n) and np.array_equal(got, got.T) and np.all(np.diag(got) == 0)
        I, J = np.arange(n)[:, None], np.arange(n)[None, :]
        check_payoff_entries(got, fa, fb, cand, I, J, lam, f"payoff N = {n}, lambda {lam}")
    dev = match.payoff_matrix(fa, fb, cand, 1e-3, ctx=gpu_ctx, device=True)
    assert np.array_equal(dev.cpu().numpy(), got)


def test_payoff_exact_transform_and_angles_across_pi(gpu_ctx):
    xy = np.array([[3, 4], [10, 2], [7, 9], [1, 12], [15, 6], [8, 8]], np.float32)
    fa = np.column_stack([xy, np.full(6, 2.0), np.full(6, 0.5)]).astype(np.float32)
    fb = np.column_stack([2 * xy + np.array([5, -3]), np.full(6, 4.0), np.full(6, 0.5)]).astype(np.float32)
    cand = np.stack([np.arange(6), np.arange(6)], axis=1).astype(np.int32)
    got = match.payoff_matrix(fa, fb, cand, 1e-3, ctx=gpu_ctx)
    assert np.array_equal(got, 1.0 - np.eye(6))               # exactly 1 off the diagonal, exactly 0 on it
    I, J = np.arange(6)[:, None], np.arange(6)[None, :]
    for a_src, a_tgt in ((0.1, 6.2), (6.2, 0.1), (3.2, 0.0), (0.0, 3.2), (9.5, -9.5), (-9.5, 9.5)):
        fa[:, 3], fb[:, 3] = a_src, a_tgt
        check_payoff_entries(match.payoff_matrix(fa, fb, cand, 1e-3, ctx=gpu_ctx), fa, fb, cand, I, J, 1e-3, f"angles {a_src} / {a_tgt}")
    fa[0, 3] = np.nan
    with pytest.raises(match._lib.WassError):
        match.payoff_matrix(fa, fb, cand, 1e-3, ctx=gpu_ctx)


# ------------------------------------------------------------------------------------------------------------------------- kNN
@pytest.mark.parametrize("na,nb,d,k,seed", ((1, 1, 1, 3, 8), (3, 2, 64, 3, 23), (65, 257, 64, 3, 712), (300, 1025, 128, 8, 3129)))
def test_knn_candidates(gpu_ctx, na, nb, d, k, seed):
    """the seeds are those whose neighbour distances differ by more than a relative 1e-5 (asserted below): closer ones cannot be
    told apart in float32, whatever the kernel does"""
    import torch
    rng = np.random.default_rng(seed)
    a, b = rng.normal(0, 1, (na, d)).astype(np.float32), rng.normal(0, 1, (nb, d)).astype(np.float32)
    want, _, sd = M.knn(a, b, k)
    kk = min(k, nb)
    if nb > kk:
        assert np.all((sd[:, 1:kk + 1] - sd[:, 0:kk]) > 1e-5 * sd[:, 1:kk + 1]), "the probe's distances are too close to call in float32"
    idx, dist = match.knn_candidates(a, b, k, ctx=gpu_ctx)
    assert idx.shape == (na, kk) and idx.dtype == np.int32 and np.array_equal(idx, want)
    ref = M.dist_f32(a, b, want)
    ulp = np.abs(dist.astype(np.float64) - ref.astype(np.float64)) / np.spacing(ref).astype(np.float64)
    print(f"kNN {na} x {nb} x {d}: distances within {ulp.max():g} float32 ulp of the sequential restatement")
    assert ulp.max() <= 2
    d_idx, d_dist = match.knn_candidates(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), k, ctx=gpu_ctx)
    assert np.array_equal(d_idx.cpu().numpy(), idx) and np.array_equal(d_dist.cpu().numpy(), dist)


def test_knn_equal_descriptors_tie_to_the_lower_index(gpu_ctx):
    b = np.zeros((70, 16), np.float32)
    b[5] = 2.0
    b[66] = 1.0
    idx, dist = match.knn_candidates(np.zeros((67, 16), np.float32), b, 8, ctx=gpu_ctx)
    assert np.array_equal(idx, np.tile([0, 1, 2, 3, 4, 6, 7, 8], (67, 1))) and np.all(dist == 0)
    idx, dist = match.knn_candidates(np.ones((1, 16), np.float32), b, 3, ctx=gpu_ctx)
    assert np.array_equal(idx, [[66, 0, 1]]) and np.array_equal(dist, [[0, 16, 16]])


# ----------------------------------------------------------------------------------------------------------------- the matcher
def oracle_match(fa, fb, da, db, lam):
    return M.gt_match(fa, fb, da, db, lam=lam, max_iters=M.PROBE_STEPS)


@pytest.fixture(scope="module")
def scene_matches(golden):
    """the oracle's match lists of the four scenes, computed once"""
    return [oracle_match(*golden_scene(golden, s), float(golden[f"scene{s}_lambda"])) for s in range(4)]


def test_gt_match_end_to_end(gpu_ctx, golden, scene_matches):
    for s in range(4):
        fa, fb, da, db = golden_scene(golden, s)
        want, want_rounds = scene_matches[s]
        A, B = features(fa, fb, da, db)
        r = match.gt_match(A, B, lam=float(golden[f"scene{s}_lambda"]), max_iters=M.PROBE_STEPS, ctx=gpu_ctx)
        assert np.array_equal(r.matches, want), f"scene {s}"
        assert [(n, g) for n, _, g in r.rounds] == [(n, g) for n, _, g in want_rounds]          # the step counts are not compared
        assert np.array_equal(r.loc_a, fa[want[:, 0], :2]) and np.array_equal(r.loc_b, fb[want[:, 1], :2])
        assert len(r.rounds) <= 21
    skipped = match.gt_match(A, B, skip_gt=True, nndr=0.9, ctx=gpu_ctx)
    idx, _, _ = M.knn(da, db, 3)
    assert np.array_equal(skipped.matches, M.nndr_matches(idx, M.dist_f32(da, db, idx), 3, 0.9)) and skipped.matches.shape[0] > 0
    assert skipped.rounds == []


def test_gt_match_batch_is_the_singles_bit_for_bit(gpu_ctx, golden):
    problems = [features(*p) for p in M.batch_problems(golden_scene(golden, 0))]
    kw = dict(lam=M.BATCH_LAMBDA, max_iters=M.PROBE_STEPS, ctx=gpu_ctx)
    singles = [match.gt_match(a, b, **kw) for a, b in problems]
    assert len({s.rounds[0][0] for s in singles}) == 5                           # five different N
    assert len(singles[3].rounds) == 1 and max(len(s.rounds) for s in singles) > 1     # one ends in round 1
    batch = match.gt_match_batch(problems, **kw)
    order = [4, 2, 0, 3, 1]
    shuffled = match.gt_match_batch([problems[i] for i in order], **kw)
    for i, (s, b) in enumerate(zip(singles, batch)):
        o = shuffled[order.index(i)]
        for r in (b, o):
            assert np.array_equal(r.matches, s.matches) and r.rounds == s.rounds
            assert np.array_equal(r.loc_a, s.loc_a) and np.array_equal(r.loc_b, s.loc_b)
    # the populations themselves, problem by problem, in two batch orders
    mats = [match.payoff_matrix(a.table(), b.table(), match.candidate_list(match.knn_candidates(a.desc, b.desc, 3, gpu_ctx)[0]), M.BATCH_LAMBDA, ctx=gpu_ctx)
            for a, b in problems]
    alone = [match.iidyn(A, max_iters=M.PROBE_STEPS, ctx=gpu_ctx) for A in mats]
    for perm in (list(range(5)), order):
        together = match.iidyn([mats[i] for i in perm], max_iters=M.PROBE_STEPS, ctx=gpu_ctx)
        for i, r in zip(perm, together):
            assert np.array_equal(r.x, alone[i].x) and r.steps == alone[i].steps and r.err == alone[i].err
