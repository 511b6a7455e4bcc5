"""The oracle of the DFT stage tests on the CPU (tests/dft_oracle.py): its model is right, its tables reach the kernel instances,
tiles and ragged edges they claim to reach, its probe inputs are exact, and every check the GPU test makes can fail: a model
with one thing broken misses the bound by at least five times."""
import functools

import numpy as np
import pytest

import dft_oracle as D
import filter_oracle as FO
import spectrum_oracle as SO

ids = lambda c: "x".join(str(v) for v in c)


# ---- the references the checks share ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ref3d(case):
    nt, ny, nx = case
    _, view = D.dense_cube_3d(case)
    prep, flag = D.prepare3d(view, *D.dense_windows(nt, ny, nx))
    xw = prep.astype(np.float64)
    ref = np.fft.fftshift(np.abs(np.fft.fftn(xw)) ** 2)
    tol = D.tol_of(ref, D.bound3d_e2(xw))
    for a in (xw, ref, tol):
        a.setflags(write=False)
    return xw, ref, tol


@functools.lru_cache(maxsize=None)
def ref_probes(case):
    cube = D.probe_cube(*case)
    out = []
    for pr in D.probes(*case):
        cells = D.probe_cells(pr, cube)
        xw = np.zeros(case)
        for t, y, x, d in cells:
            xw[t, y, x] = d
        out.append((pr, cells, xw, D.probe_expected(cells, *case), D.probe_bound(cells)))
    return out


@functools.lru_cache(maxsize=None)
def ref_spatial(case):
    rows, cols = case
    _, view = D.dense_frames_spatial(case)
    Hs = D.butterworth_transfer(rows, cols)
    x = np.ascontiguousarray(view[0])
    return x, Hs, FO.spatial_apply(x, Hs), FO.spatial_bound(x)


def _welch_refs(cube, nperseg, rangespan):
    from wass_amd.postproc import spectrum_series
    series = spectrum_series(cube, rangespan).astype(np.float64) * D.WELCH_SCALE
    model = D.staged_welch(series, 10.0, nperseg)
    ref = SO.compute_spectrum(cube, 0.1, nperseg=nperseg, rangespan=rangespan, scale=D.WELCH_SCALE)[1]
    return series, ref, D.welch_tolerance(model, 10.0, nperseg, cube.shape[0])


@functools.lru_cache(maxsize=None)
def ref_welch(case):
    n_samples, nperseg, rangespan = case
    return _welch_refs(SO.make_cube(n_samples, *D.WELCH_GRID, seed=n_samples + nperseg), nperseg, rangespan)


@functools.lru_cache(maxsize=None)
def ref_welch_impulse(case):
    n_samples, nperseg, rangespan = case
    return _welch_refs(D.impulse_cube(n_samples, nperseg), nperseg, rangespan)


@functools.lru_cache(maxsize=None)
def ref_spatial_deltas(case):
    """[(Hs, frame, oracle, bound)] over the injected transfer functions and the delta frames."""
    return [(Hi, fr, FO.spatial_apply(fr, Hi), FO.spatial_bound(fr)) for Hi in D.injected_transfers(*case).values() for fr in D.delta_frames(*case)]


ratio = D.ratio


def tile_ratio(got, ref, bound_norm, kind, raw=False):
    te, n = D.tile_errors(got, ref)
    lim = bound_norm / np.sqrt(n) * (1.0 if raw else D.TILE_MARGIN[kind])
    return ratio(te.max(), lim)


def checks_3d(case, variant=None, dtype=np.float64):
    xw, ref, tol = ref3d(case)
    S = D.staged3d(xw, variant, dtype)
    out = {"element": ratio(np.abs(S - ref), tol), "tile": tile_ratio(S, ref, float(np.linalg.norm(tol)), "3d")}
    out["probe"] = max(ratio(np.abs(D.staged3d(pxw, variant, dtype) - pref), D.tol_of(pref, e2)) for _, _, pxw, pref, e2 in ref_probes(case))
    return out


def checks_spatial(case, variant=None, dtype=np.float64):
    rows, cols = case
    x, Hs, ref, B = ref_spatial(case)
    got = D.staged_spatial(x, Hs, variant, dtype)
    out = {"norm": ratio(np.linalg.norm(got - ref), B), "tile": tile_ratio(got, ref, B, "spatial")}
    worst = max(ratio(np.linalg.norm(D.staged_spatial(fr, Hi, variant, dtype) - want), Bd) for Hi, fr, want, Bd in ref_spatial_deltas(case))
    out["delta"] = worst
    return out


def checks_welch(case, variant=None, dtype=np.float64):
    series, ref, tol = ref_welch(case)
    P = D.staged_welch(series, 10.0, case[1], variant, dtype)["P"]
    out = {"element": ratio(np.abs(P - ref), tol), "peak": ratio(np.abs(P - ref).max(), 1e-5 * ref.max())}
    series, ref, tol = ref_welch_impulse(case)
    out["impulse"] = ratio(np.abs(D.staged_welch(series, 10.0, case[1], variant, dtype)["P"] - ref), tol)
    return out


# ---- the model is right ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", D.CASES_3D, ids=ids)
def test_staged3d_is_fftn(case):
    xw, ref, _ = ref3d(case)
    S = D.staged3d(xw)
    scale = max(float(ref.max()), 1e-300)
    print(f"{case}: max |staged - fftn| / peak = {np.abs(S - ref).max() / scale:.2e}")
    assert np.abs(S - ref).max() <= 1e-11 * scale
    for pr, cells, pxw, pref, e2 in ref_probes(case):
        full = np.fft.fftshift(np.abs(np.fft.fftn(pxw)) ** 2)
        assert np.abs(pref - full).max() <= 1e-12 * max(float(full.max()), 1e-300)
        assert np.abs(D.staged3d(pxw) - pref).max() <= 1e-12 * max(float(full.max()), 1e-300)
    a, b = D.mirror_pairs(*case)
    assert np.array_equal(S.ravel()[a], S.ravel()[b]) and len(a) == case[0] * case[1] * (case[2] - case[2] // 2 - 1)


@pytest.mark.parametrize("case", D.CASES_WELCH, ids=ids)
def test_staged_welch_is_the_oracle(case):
    series, ref, tol = ref_welch(case)
    P = D.staged_welch(series, 10.0, case[1])["P"]
    print(f"{case}: max |staged - oracle| / peak = {np.abs(P - ref).max() / ref.max():.2e}")
    assert P.shape == ref.shape and np.abs(P - ref).max() <= 1e-12 * ref.max()
    one = SO.welch(series[0] - series[0].mean(), 10.0, case[1])[1]
    alone = D.staged_welch(series[:1], 10.0, case[1])["P"]
    assert np.abs(alone - one).max() <= 1e-12 * one.max()


@pytest.mark.parametrize("case", D.CASES_SPATIAL, ids=ids)
def test_staged_spatial_is_the_oracle(case):
    x, Hs, ref, B = ref_spatial(case)
    got = D.staged_spatial(x, Hs)
    print(f"{case}: max |staged - oracle| / max |oracle| = {np.abs(got - ref).max() / np.abs(ref).max():.2e}")
    assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max()
    for name, Hi in D.injected_transfers(*case).items():
        Hu = np.fft.ifftshift(Hi)
        assert np.array_equal(Hu, Hu[(-np.arange(case[0])) % case[0]][:, (-np.arange(case[1])) % case[1]]), "real and even"
        want = FO.spatial_apply(x, Hi)
        assert np.abs(D.staged_spatial(x, Hi) - want).max() <= 1e-12 * max(np.abs(x).max(), 1.0)
        if name == "ones":
            assert np.abs(want - x).max() <= 1e-12 * np.abs(x).max()


# ---- the tables reach what they claim -------------------------------------------------------------------------------------------
def _all_stages():
    out = []
    for c in D.CASES_3D:
        out += [("3d", c, s) for s in D.plan3d(*c)]
    for c in D.CASES_WELCH:
        out += [("welch", c, s) for s in D.plan_welch(D.welch_series_count(c[2]), c[0], c[1])]
    for c in D.CASES_SPATIAL:
        out += [("spatial", c, s) for s in D.plan_spatial(*c, D.SPATIAL_BATCH)]
    return out


def test_tables_reach_every_instance_tile_and_edge():
    stages = _all_stages()
    last = None
    for kind, c, s in stages:
        if (kind, c) != last:
            plan = {"3d": lambda: D.plan3d(*c), "welch": lambda: D.plan_welch(D.welch_series_count(c[2]), c[0], c[1]),
                    "spatial": lambda: D.plan_spatial(*c, D.SPATIAL_BATCH)}[kind]()
            print(f"{kind} {c}: {D.describe(plan)}")
            last = (kind, c)
    # what an instance's callers cannot produce: the Welch estimate of compute_spectrum has an even number of series, so an
    # even number of columns
    impossible = {((False, False), "rN", 1), ((False, False), "rN", 63)}
    for inst in D.INSTANCES:
        mine = [s for _, _, s in stages if s["inst"] == inst]
        assert mine, inst
        assert any(s["grid"][1] > 1 for s in mine), (inst, "tiles in M")
        assert any(s["grid"][0] > 1 for s in mine), (inst, "tiles in N")
        for key, wanted in (("rM", (0, 1, 63)), ("rN", (0, 1, 63)), ("rK", (0, 1, 15))):
            for r in wanted:
                hit = any(s[key] == r for s in mine)
                assert hit != ((inst, key, r) in impossible), (inst, key, r)
        nks = {s["nk"] for s in mine}
        assert 1 in nks and 2 in nks and max(nks) >= 8, (inst, nks)
    assert {c[2] // 2 + 1 for c in D.CASES_3D} >= {63, 64, 65}
    assert any(s["stage"] == "y" and s["batch"] > 1 for kind, _, s in stages if kind == "3d")
    assert any(s["stage"] == "y" and s["batch"] > 1 for kind, _, s in stages if kind == "spatial")
    parities = {"nt": [c[0] for c in D.CASES_3D], "ny": [c[1] for c in D.CASES_3D], "nx": [c[2] for c in D.CASES_3D],
                "nps": [min(c[0], c[1]) for c in D.CASES_WELCH], "rows": [c[0] for c in D.CASES_SPATIAL], "cols": [c[1] for c in D.CASES_SPATIAL]}
    for name, vals in parities.items():
        assert {v % 2 for v in vals} == {0, 1}, name
    # what the issue lists is all there
    assert set(D.CASES_3D) >= {(1, 1, 1), (1, 1, 2), (2, 1, 1), (1, 5, 1), (3, 5, 7), (4, 84, 84), (5, 64, 126), (7, 65, 128), (6, 63, 127),
                               (16, 63, 130), (17, 129, 66), (33, 17, 31), (66, 20, 36), (130, 9, 10)}
    assert set(D.CASES_WELCH) >= {(333, 512, 3), (40, 15, 0), (40, 16, 0), (40, 17, 1), (9, 2, 0), (9, 3, 0), (700, 127, 5), (700, 129, 5)}
    assert set(D.CASES_SPATIAL) >= {(1, 1), (1, 8), (8, 1), (2, 2), (3, 3), (5, 2), (5, 3), (63, 65), (65, 63), (64, 127), (127, 129), (129, 64),
                                    (17, 130)}
    assert D.welch_dims(333, 512) == (333, 167, 1, 167) and D.welch_series_count(0) == 2
    # the largest case stays small
    assert max(np.prod(c) for c in D.CASES_3D) <= 1.2e6


def test_plans_restate_the_launches():
    """Against figures worked out by hand from spec3d_run, wass_spec1d_welch and spat_run."""
    x, y, t = D.plan3d(7, 65, 128)
    assert (x["inst"], x["M"], x["N"], x["K"], x["grid"], x["nk"]) == ((False, True), 65, 455, 128, (8, 2, 1), 8)
    assert (y["inst"], y["M"], y["N"], y["K"], y["grid"], y["nk"]) == ((True, False), 65, 65, 65, (2, 2, 7), 5)
    assert (t["inst"], t["M"], t["N"], t["K"], t["grid"], t["nk"]) == ((True, False), 7, 4225, 7, (67, 1, 1), 1)
    (w,) = D.plan_welch(122, 700, 127)
    assert (w["inst"], w["M"], w["N"], w["K"], w["grid"], w["nk"]) == ((False, False), 64, 122 * 9, 127, (18, 1, 1), 8)
    x, y, yi, xi = D.plan_spatial(127, 129, 2)
    assert (x["M"], x["N"], x["K"], x["grid"]) == (65, 127, 129, (2, 2, 2)) and y == dict(yi, stage="y")
    assert (y["M"], y["N"], y["K"], y["grid"]) == (127, 65, 127, (2, 2, 2))
    assert (xi["inst"], xi["M"], xi["N"], xi["K"], xi["grid"], xi["nk"], xi["rK"]) == ((True, True), 129, 127, 65, (2, 3, 2), 5, 1)


# ---- the probe inputs are exact -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", D.CASES_3D, ids=ids)
def test_probe_inputs_are_exact(case):
    nt, ny, nx = case
    cube = D.probe_cube(*case)
    assert np.array_equal(cube, np.round(cube)) and np.abs(cube).max() <= 6
    total = int(cube.astype(np.int64).sum())
    assert float(cube.astype(np.float64).sum()) == float(total) == float(np.sum(cube[::-1, ::-1, ::-1].astype(np.float64)))
    assert abs(total) < 2 ** 24 and cube.size < 2 ** 24
    prs = D.probes(*case)
    assert 1 <= len(prs) <= 12 and prs[0] == ((nt - 1,), (ny - 1,), (nx - 1,))
    for axis, n in enumerate(case):
        used = {p for pr in prs for p in pr[axis]}
        assert used >= set(D.hot_positions(n)), (axis, used)
        assert all(len(pr[axis]) == min(2, n) for pr in prs[1:])
    for pr, cells, pxw, pref, e2 in ref_probes(case):
        prep, flag = D.prepare3d(cube, *D.probe_windows(pr, *case))
        assert not flag and np.array_equal(prep.astype(np.float64), pxw)           # the general restatement agrees with the sparse one
        hot = {(t, y, x) for t in pr[0] for y in pr[1] for x in pr[2]}
        assert len(hot) <= 8 and {tuple(i) for i in np.argwhere(prep != 0)} <= hot
        assert {c[:3] for c in cells} <= hot
    print(f"{case}: {len(prs)} probes, hot positions t {D.hot_positions(nt)} y {D.hot_positions(ny)} x {D.hot_positions(nx)}")


def test_prepare3d_is_the_oracles_segment():
    """prepare3d (the kernels' float32 preparation, restated) against spectrum_oracle.segments3d (the reference's own numpy
    operations) on a plan's windows: equal up to the cast of the result to float32, the rounding of the float32 subtraction and
    the global mean, which the kernels take from an fp64 sum and numpy from a pairwise float32 one (at most (log2 N + 2) u mean |z|
    apart)."""
    from wass_amd.postproc import spectrum3d_plan
    cube = SO.make_cube(40, 123, 128, seed=9, nan_fraction=0.01)
    p = spectrum3d_plan(cube.shape, 0.1, 0.1)
    n = 0
    for s, (zw, _) in zip(p.starts, SO.segments3d(cube, 0.1, 0.1)):
        seg = cube[s:s + p.nt, p.r0:p.r0 + p.ny, p.c0:p.c0 + p.nx]
        prep, flag = D.prepare3d(seg, p.win_t, p.win_y, p.win_x)
        assert not flag and prep.shape == zw.shape and prep.dtype == np.float32
        win = (p.win_y[:, None] * p.win_x)[None] * p.win_t[:, None, None]
        dmean = (np.log2(seg.size) + 2) * D.U * float(np.nanmean(np.abs(seg)))
        worst = ratio(np.abs(prep - zw), 3 * D.U * np.abs(zw) + dmean * win + 1e-300)
        print(f"segment at {s}: largest difference / allowance = {worst:.3f}")
        assert worst <= 1.0, (s, worst)
        n += 1
    assert n == len(p.starts) >= 2
    bad = cube[:p.nt, p.r0:p.r0 + p.ny, p.c0:p.c0 + p.nx].copy()
    bad[:, 3, 4] = np.nan
    prep, flag = D.prepare3d(bad, p.win_t, p.win_y, p.win_x)
    assert flag and np.isfinite(prep).all() and (prep[:, 3, 4] == 0).all()


def test_hot_positions():
    assert D.hot_positions(1) == [0] and D.hot_positions(2) == [0, 1]
    assert D.hot_positions(130) == [0, 15, 16, 17, 63, 64, 65, 128, 129]
    assert D.hot_positions(17) == [0, 8, 15, 16] and D.hot_positions(64) == [0, 15, 16, 17, 32, 48, 63]


# ---- TILE_MARGIN ----------------------------------------------------------------------------------------------------------------
def test_tile_margin_is_measured():
    """The float32 run of the oracle's own model over the whole table: the worst tile ratio is the recorded one, and that run
    passes every check the GPU result is held to."""
    worst = {"3d": (-1.0, None), "spatial": (-1.0, None)}
    for case in D.CASES_3D:
        xw, ref, tol = ref3d(case)
        S = D.staged3d(xw.astype(np.float32), None, np.float32)
        r = tile_ratio(S, ref, float(np.linalg.norm(tol)), "3d", raw=True)
        worst["3d"] = max(worst["3d"], (r, case))
        assert ratio(np.abs(S - ref), tol) <= 1.0
    for case in D.CASES_SPATIAL:
        x, Hs, ref, B = ref_spatial(case)
        got = D.staged_spatial(x, Hs, None, np.float32)
        r = tile_ratio(got, ref, B, "spatial", raw=True)
        worst["spatial"] = max(worst["spatial"], (r, case))
        assert np.linalg.norm(got - ref) <= B
    print("worst float32 tile ratios:", worst)
    for kind in worst:
        rec, at = D.TILE_MEASURED[kind]
        assert rec / 1.5 <= worst[kind][0] <= rec * 1.5, (kind, worst[kind], at)      # a BLAS may block its sums otherwise
        assert D.TILE_MARGIN[kind] == 8 * rec


# ---- the checks can fail --------------------------------------------------------------------------------------------------------
# A variant that applies to a case misses at least one check of that case by 5 x.  Where it does not miss a given check it is listed
# here, shape by shape, with the check that does catch it: {(kind, variant, case): {check it passes: check that catches it}}.  The
# test holds the table to the printed ratios both ways: an entry that is missing fails, and so does one that is no longer needed.
#   3-D: the dense element-wise bound grows with the segment's l1 norm and the per-tile limit with the norm of that bound, so a
#   16-row band of the x stage (the highest kx, where the smooth input has little) or one k tile out of five to nine can stay
#   inside them; the probes put all their weight on a few cells and catch each of these by 1e5.
#   Welch: the flat 1e-5 of the peak is the existing, underived check; the derived element-wise bound catches what it lets through.
#   Where K % 16 = 1 (nps = 129) the last k tile is one sample of periodic Hann weight 5.9e-4, and the noisy cube leaves it inside
#   the bound; the impulse cube, all of whose first segment is that sample, catches it.  The impulse cube in turn has one bin
#   value, so it cannot see a wrong Nyquist factor or a zeroed band as well as the noisy cube does.
#   spatial: the highest kx again; a delta frame has as much there as anywhere.
BLIND = {
    ('3d', 'zero_band:x', (4, 84, 84)): {'tile': 'probe'},
    ('3d', 'zero_band:x', (5, 64, 126)): {'tile': 'probe'},
    ('3d', 'zero_band:x', (7, 65, 128)): {'tile': 'probe'},
    ('3d', 'twiddle_off:x', (7, 65, 128)): {'tile': 'probe'},
    ('3d', 'drop_k:y', (7, 65, 128)): {'element': 'probe'},
    ('3d', 'zero_band:x', (6, 63, 127)): {'tile': 'probe'},
    ('3d', 'drop_k:x', (16, 63, 130)): {'element': 'probe'},
    ('3d', 'zero_band:x', (16, 63, 130)): {'tile': 'probe'},
    ('3d', 'twiddle_off:x', (16, 63, 130)): {'tile': 'probe'},
    ('3d', 'zero_band:x', (17, 129, 66)): {'tile': 'probe'},
    ('3d', 'drop_k:y', (17, 129, 66)): {'element': 'probe', 'tile': 'probe'},
    ('3d', 'zero_band:x', (3, 5, 125)): {'tile': 'probe'},
    ('welch', 'zero_band:w', (333, 512, 3)): {'peak': 'element', 'impulse': 'element'},
    ('welch', 'twiddle_off:w', (333, 512, 3)): {'peak': 'element', 'impulse': 'element'},
    ('welch', 'nyquist_odd', (333, 512, 3)): {'peak': 'element', 'impulse': 'element'},
    ('welch', 'nyquist_odd', (40, 15, 0)): {'peak': 'impulse'},
    ('welch', 'nyquist_even', (40, 16, 0)): {'peak': 'impulse'},
    ('welch', 'nyquist_odd', (40, 17, 1)): {'peak': 'impulse'},
    ('welch', 'zero_band:w', (700, 127, 5)): {'peak': 'impulse'},
    ('welch', 'nyquist_odd', (700, 127, 5)): {'peak': 'impulse'},
    ('welch', 'drop_k:w', (700, 129, 5)): {'element': 'impulse', 'peak': 'impulse'},
    ('welch', 'zero_band:w', (700, 129, 5)): {'peak': 'impulse'},
    ('welch', 'nyquist_odd', (700, 129, 5)): {'peak': 'impulse'},
    ('welch', 'zero_band:w', (300, 125, 0)): {'peak': 'impulse'},
    ('welch', 'nyquist_odd', (300, 125, 0)): {'peak': 'impulse'},
    ('spatial', 'zero_band:x', (63, 65)): {'norm': 'delta', 'tile': 'delta'},
    ('spatial', 'drop_k:xi', (63, 65)): {'norm': 'delta', 'tile': 'delta'},
    ('spatial', 'zero_band:x', (65, 63)): {'norm': 'delta'},
    ('spatial', 'drop_k:xi', (65, 63)): {'norm': 'delta'},
    ('spatial', 'zero_band:x', (64, 127)): {'norm': 'delta', 'tile': 'delta'},
    ('spatial', 'drop_k:xi', (64, 127)): {'norm': 'delta', 'tile': 'delta'},
    ('spatial', 'zero_band:x', (127, 129)): {'norm': 'delta', 'tile': 'delta'},
    ('spatial', 'twiddle_off:x', (127, 129)): {'norm': 'delta', 'tile': 'delta'},
    ('spatial', 'drop_k:xi', (127, 129)): {'norm': 'delta', 'tile': 'delta'},
    ('spatial', 'zero_band:x', (129, 64)): {'norm': 'delta', 'tile': 'delta'},
    ('spatial', 'drop_k:xi', (129, 64)): {'norm': 'delta', 'tile': 'delta'},
    ('spatial', 'zero_band:x', (17, 130)): {'norm': 'delta', 'tile': 'delta'},
    ('spatial', 'twiddle_off:x', (17, 130)): {'norm': 'delta', 'tile': 'delta'},
    ('spatial', 'drop_k:xi', (17, 130)): {'norm': 'delta', 'tile': 'delta'},
    ('spatial', 'zero_band:x', (5, 226)): {'norm': 'delta', 'tile': 'delta'},
    ('spatial', 'twiddle_off:x', (5, 226)): {'norm': 'delta', 'tile': 'delta'},
    ('spatial', 'drop_k:xi', (5, 226)): {'norm': 'delta', 'tile': 'delta'},
}


def _run_variants(kind, case, variants, checks):
    bad, some = [], False
    for v in variants:
        if not D.applies(v, case, kind):
            continue
        some = True
        r = checks(case, v)
        print(f"{kind} {case} {v}: " + ", ".join(f"{k} {x:.3g}" for k, x in r.items()))
        listed = BLIND.get((kind, v, case), {})
        for k, x in r.items():
            if x < 5.0 and (k not in listed or r[listed[k]] < 5.0):
                bad.append((kind, v, case, k, x))
        bad += [(kind, v, case, k, "listed, but it misses") for k in listed if r[k] >= 5.0]
    assert some or (kind, case) == ("3d", (1, 1, 1)), f"no variant applies to {kind} {case}"
    assert not bad, bad


@pytest.mark.parametrize("case", D.CASES_3D, ids=ids)
def test_variants_miss_3d(case):
    _run_variants("3d", case, D.VARIANTS_3D, checks_3d)


@pytest.mark.parametrize("case", D.CASES_WELCH, ids=ids)
def test_variants_miss_welch(case):
    _run_variants("welch", case, D.VARIANTS_WELCH, checks_welch)


@pytest.mark.parametrize("case", D.CASES_SPATIAL, ids=ids)
def test_variants_miss_spatial(case):
    _run_variants("spatial", case, D.VARIANTS_SPATIAL, checks_spatial)


def test_the_blind_table_names_known_cases():
    cases = {"3d": D.CASES_3D, "welch": D.CASES_WELCH, "spatial": D.CASES_SPATIAL}
    variants = {"3d": D.VARIANTS_3D, "welch": D.VARIANTS_WELCH, "spatial": D.VARIANTS_SPATIAL}
    for kind, v, case in BLIND:
        assert case in cases[kind] and v in variants[kind] and D.applies(v, case, kind), (kind, v, case)


def test_a_variant_that_does_not_apply_changes_nothing():
    for case in D.CASES_3D:
        xw, ref, tol = ref3d(case)
        for v in D.VARIANTS_3D:
            if not D.applies(v, case, "3d"):
                assert np.array_equal(D.staged3d(xw, v), D.staged3d(xw)), (case, v)
    for case in D.CASES_SPATIAL:
        x, Hs, ref, B = ref_spatial(case)
        for v in D.VARIANTS_SPATIAL:
            if not D.applies(v, case, "spatial"):
                assert np.array_equal(D.staged_spatial(x, Hs, v), D.staged_spatial(x, Hs)), (case, v)
    for case in D.CASES_WELCH:
        series, ref, tol = ref_welch(case)
        for v in D.VARIANTS_WELCH:
            if not D.applies(v, case, "welch"):
                # equal up to round-off: the mirror row has the same modulus, not the same bits
                np.testing.assert_allclose(D.staged_welch(series, 10.0, case[1], v)["P"], D.staged_welch(series, 10.0, case[1])["P"], rtol=1e-9)


@pytest.mark.parametrize("kind,case", [("3d", c) for c in D.CASES_3D] + [("welch", c) for c in D.CASES_WELCH] + [("spatial", c) for c in D.CASES_SPATIAL],
                         ids=lambda v: v if isinstance(v, str) else ids(v))
def test_the_unbroken_model_passes(kind, case):
    """fp64 and float32 runs of the unbroken model are inside every bound: the checks do not fail on a right answer."""
    checks = {"3d": checks_3d, "welch": checks_welch, "spatial": checks_spatial}[kind]
    for dt in (np.float64, np.float32):
        r = checks(case, None, dt)
        print(f"{kind} {case} {np.dtype(dt).name}: " + ", ".join(f"{k} {x:.3g}" for k, x in r.items()))
        assert max(r.values()) <= 1.0, (case, dt, r)
