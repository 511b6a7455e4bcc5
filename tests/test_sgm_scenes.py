"""The scenes of sgm_scenes.py held to their conditions, on the CPU oracle alone.

test_sgm_select_gpu.py compares the GPU with the oracle bit for bit on these cases; that comparison sees only what the inputs make
happen.  Here every case is shown to make it happen: volumes that are not saturated, maps that are mostly valid (or, with the
left-right check on, well split between its two outcomes), every target index winning, all sub-pixel fractions, exact ties and
uniqueness rejections from far lanes.  These are conditions on inputs, not measurements of the code under test: a case that misses
one is a case to change.  The numpy restatement of the selection (sgm_scenes.select) is held to the oracle's raw map on every case,
and each of its deliberate mistakes must change that map at every D -- so a kernel that made the mistake would fail the GPU file.
"""
import numpy as np
import pytest

import sgm_scenes as sc

_CASES = sc.all_cases()


def _figures(c, p, So, rawo):
    D, minD = c.D, c.min_disp
    INV = (minD - 1) * 16
    region = rawo[:, minD + D:]
    valid = region != INV
    best, minS, ok, _, _ = sc.winners(So, D, p.uniq_ratio)
    ok = ok & (best >= 0)
    return dict(region=region, valid=valid, best=best, minS=minS, ok=ok, saturated=float((minS >= sc.INVALID_COST).mean()),
                valid_share=float(valid.mean()), rejected_share=float((ok & ~valid).mean()))


@pytest.mark.parametrize("c", _CASES, ids=[c.id for c in _CASES])
def test_case_meets_its_conditions(oracle, c):
    right, left, p, disp, st, Co, So, rawo = sc.run_oracle(oracle, c)
    assert right.shape[1] == sc.stair_disparity(c.D, c.min_disp)[1] and right.shape[0] == c.h
    f = _figures(c, p, So, rawo)
    print(f"{c.id}: {right.shape[1]}x{c.h} max_C={st.max_C} max_L={st.max_L} all-saturated={100 * f['saturated']:.2f}% "
          f"valid={100 * f['valid_share']:.1f}% lr-rejected={100 * f['rejected_share']:.1f}%")
    assert st.overflow == 0
    assert f["saturated"] <= 0.10
    # the restatement reproduces the oracle's selection, so what it says about winners and ties below describes the oracle
    np.testing.assert_array_equal(sc.select(So, p), rawo)

    S = So.astype(np.int32)
    best, minS, ok, valid = f["best"], f["minS"], f["ok"], f["valid"]
    if c.family in ("selection", "subpixel", "steady"):                   # left-right check off
        assert c.d12 == sc.LR_OFF and f["valid_share"] >= 0.90
        wins = {t: int(((best == t) & valid).sum()) for t in sc.targets(c.D)}
        print(f"  fewest valid pixels for a target: {min(wins.values())} (d = {min(wins, key=wins.get)})")
        assert min(wins.values()) >= 5, wins
    if c.family == "lrcheck":                                     # left-right check on: both outcomes
        assert f["valid_share"] >= 0.10 and f["rejected_share"] >= 0.10
    if c.scene == "smooth_terrace":
        fr = np.unique(f["region"][valid] & 15)
        print(f"  sub-pixel fractions present: {len(fr)}")
        assert len(fr) == 16
    if c.family == "periodic":
        V = sc.nslots(c.D)
        q = 100 - c.uniq
        real = (minS > 0) & (minS < sc.INVALID_COST)
        ties = int((((S == minS[..., None]).sum(-1) >= 2) & real).sum())
        d = np.arange(c.D)[None, None, :]
        outside = np.abs(d - best[..., None]) > 1
        far = (S * q < (minS * 100)[..., None]) & outside & (d // V != (best // V)[..., None])
        far_rej = int((far.any(-1) & (best >= 0)).sum())
        exact = int((((S * q == (minS * 100)[..., None]) & outside).any(-1) & real).sum())
        print(f"  exact ties with minS > 0: {ties}; rejections by a d in another lane: {far_rej}; pixels with S q == 100 minS: {exact}")
        assert ties >= 10
        if c.uniq >= 1:                                           # at 0 the test S * 100 < minS * 100 rejects nothing, by definition
            assert far_rej >= 10
        if c.uniq in (10, 40):
            assert exact >= 1


class _P:
    def __init__(self, D, min_disp, uniq, d12):
        self.num_disp, self.min_disp, self.uniq_ratio, self.disp12_max_diff = D, min_disp, uniq, d12


_ROWS = [("terrace", 10, sc.LR_OFF), ("terrace", 1, -1), ("smooth_terrace", 1, sc.LR_OFF)] + [("periodic", u, sc.LR_OFF) for u in (0, 10, 99)]
_last = {}


def _volumes(oracle, D):
    """S of the three scenes at D (8 paths, the windows the GPU file uses) and select() of each parameter row, kept for the cases of
    one D, which run one after the other."""
    if _last.get("D") != D:
        _last.clear()
        vols = {}
        for c in (sc.Case("selection", "terrace", D, 20, 8, 5, 1, 10, sc.LR_OFF, 0),
                  sc.Case("subpixel", "smooth_terrace", D, 20, 8, 5, 1, 1, sc.LR_OFF, 0),
                  sc.Case("periodic", "periodic", D, sc.periodic_height(D), 8, 3, 1, 10, sc.LR_OFF, 0)):
            vols[c.scene] = sc.run_oracle(oracle, c)[6]
        _last.update(D=D, vols=vols, good={r: sc.select(vols[r[0]], _P(D, 1, r[1], r[2])) for r in _ROWS})
    return _last["vols"], _last["good"]


@pytest.mark.parametrize("mistake", sc.MISTAKES)
@pytest.mark.parametrize("D", sc.ALL_D)
def test_every_mistake_changes_the_map(oracle, D, mistake):
    """S depends on neither uniq_ratio nor disp12_max_diff, so one volume per scene serves every parameter row of that scene;
    select() without a mistake equals the oracle on the GPU file's cases (test_case_meets_its_conditions)."""
    vols, good = _volumes(oracle, D)
    n = {r: int((sc.select(vols[r[0]], _P(D, 1, r[1], r[2]), mistake=mistake) != good[r]).sum()) for r in _ROWS}
    print(f"D={D} {mistake}: {sum(n.values())} pixels change ({ {k: v for k, v in n.items() if v} })")
    if mistake == "padded" and D % 128 == 0:
        assert sum(n.values()) == 0                               # D fills its 64 lanes: there is no padded slot to count
    else:
        assert sum(n.values()) >= 1
