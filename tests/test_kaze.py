"""The KAZE detector without a GPU: the host tables of wass_amd/features.py, the numpy oracle (tests/kaze_oracle.py) against closed
forms and independent code, the conditions every picture of tests/test_kaze_gpu.py is held to, the subsampling against a
transcription of the reference's loops, and the file-level entry with the GPU calls stubbed out."""
import os

import numpy as np
import pytest

import kaze_oracle as KO
import kaze_pictures as P
from wass_amd import features as FE
from wass_amd import match

F = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kaze_pin.npz")


# ---------------------------------------------------------------------------------------------------------------- host tables
def test_levels_and_fed_steps():
    L = FE.kaze_levels()
    es = [1.6 * 2.0 ** (s / 4 + o) for o in range(4) for s in range(4)]
    assert [int(np.rint(F(e))) for e in es] == [2, 2, 2, 3, 3, 4, 5, 5, 6, 8, 9, 11, 13, 15, 18, 22] == L.sigma_size.tolist()
    assert np.array_equal(L.esigma, np.array(es).astype(F)) and len(L.taus[0]) == 0
    worst = 0.0
    for i in range(1, 16):
        T = L.etime[i] - L.etime[i - 1]
        tau, plain = L.taus[i], FE.fed_taus(T, reorder=False)
        assert np.array_equal(np.sort(tau), np.sort(plain))                                          # a permutation ...
        assert np.array_equal(tau, plain) == (len(tau) < 4)                                          # ... the identity only at kappa = 1
        assert np.array_equal(plain, KO.fed_taus_unordered(T)) and np.array_equal(tau, KO.fed_taus(T))
        assert (tau > 0).all() and tau.max() > 0.25                                                  # FED: some steps break the stability limit
        err = abs(float(tau.astype(np.float64).sum()) - float(T)) / float(T)
        worst = max(worst, err)
        assert err <= len(tau) * 2.0 ** -23                                                          # one float32 rounding per step
    print(f"FED steps sum to the stopping time within {worst:.2g} relative; {sum(len(t) for t in L.taus)} steps in all")
    small = FE.kaze_levels(FE.KazeOptions(1e-4, 2, 2))
    assert small.sigma_size.tolist() == [2, 2, 3, 5] and small.octave.tolist() == [0, 0, 1, 1] and small.sublevel.tolist() == [0, 1, 0, 1]


def test_taps_weights_and_sizes():
    for sigma, n in ((1.6, 9), (1.0, 5)):
        t = FE.gaussian_taps(sigma)
        assert len(t) == n and np.array_equal(t, t[::-1]) and abs(float(t.astype(np.float64).sum()) - 1) < 1e-6 and np.array_equal(t, KO.gaussian_taps(sigma))
    n1, wn1 = FE.scharr_weights(1)
    assert abs(n1 - 3 / 32) < 1e-8 and abs(wn1 - 10 / 32) < 1e-7                 # the plain 3 x 3 Scharr, normalised
    assert FE.scharr_weights(5) == KO.scharr_weights(5)
    L = FE.kaze_levels()
    assert np.array_equal(FE.keypoint_size(L, [0, 5, 15], [0, 0, 0], 4), (2 * L.esigma[[0, 5, 15]].astype(np.float64)).astype(F))
    assert FE.keypoint_size(L, [5], [F(0.5)], 4)[0] == F(2 * 1.6 * 2.0 ** (1 + 1.5 / 4))


def test_scratch_bytes_and_argument_errors():
    b = FE.kaze_scratch_bytes(2058, 2456)
    plane = 2058 * 2456 * 4
    assert b == 55 * plane + 2058 * 2456 + (1 << 20) * 28 + 4 * 302 == 1146394344
    assert FE.kaze_scratch_bytes(64, 64, FE.KazeOptions(1e-4, 2, 2)) == (12 + 7) * 64 * 64 * 4 + 64 * 64 + (1 << 20) * 28 + 4 * 302
    with pytest.raises(ValueError, match="image"):
        FE.kaze_scratch_bytes(22, 400)                     # the largest reflect-101 reach is 22 pixels
    FE.kaze_scratch_bytes(23, 23)
    with pytest.raises(ValueError, match="options"):
        FE.kaze_levels(FE.KazeOptions(1e-4, 1, 2))         # 2 levels
    with pytest.raises(ValueError, match="options"):
        FE.kaze_levels(FE.KazeOptions(1e-4, 6, 6))
    with pytest.raises(ValueError, match="options"):
        FE.kaze_levels((1e-4, 4, 4))
    with pytest.raises(ValueError, match="subdivisions"):
        FE.subsample_features(np.zeros((3, 3)), 100, 100, subdivisions=0)


# ------------------------------------------------------------------------------------------------- the oracle against other code
def _texture(h, w, seed):
    return np.random.default_rng(seed).random((h, w)).astype(F)


def test_oracle_gauss_and_scharr_against_scipy():
    from scipy import ndimage, signal
    img = _texture(37, 41, 1)
    for sigma in (1.0, 1.6):
        t = KO.gaussian_taps(sigma).astype(np.float64)
        ref = ndimage.correlate1d(ndimage.correlate1d(img.astype(np.float64), t, axis=1, mode="nearest"), t, axis=0, mode="nearest")
        assert np.abs(KO.gauss(img, KO.gaussian_taps(sigma)) - ref).max() < 4e-7
    for s in (1, 3):
        n, wn = (float(v) for v in KO.scharr_weights(s))
        sm, dv = np.zeros(2 * s + 1), np.zeros(2 * s + 1)
        sm[0], sm[s], sm[-1] = n, wn, n
        dv[0], dv[-1] = -1.0, 1.0
        kx = np.outer(sm, dv)                                   # smoothing down the rows, derivative along x
        for got, k in ((KO.scharr_x(img, s), kx), (KO.scharr_y(img, s), kx.T)):
            assert np.abs(got - ndimage.correlate(img.astype(np.float64), k, mode="mirror")).max() < 4e-7      # mirror = reflect-101
            inner = signal.convolve2d(img.astype(np.float64), k[::-1, ::-1], mode="valid")
            assert np.abs(got[s:-s, s:-s] - inner).max() < 4e-7
    plain = np.array([[-3, 0, 3], [-10, 0, 10], [-3, 0, 3]]) / 32.0
    assert np.abs(KO.scharr_x(img, 1) - ndimage.correlate(img.astype(np.float64), plain, mode="mirror")).max() < 4e-7


def test_oracle_fed_cycle_is_the_heat_equation_on_constant_flow():
    from scipy import ndimage
    L0 = _texture(24, 31, 2)
    taus = KO.fed_taus(F(1.5))
    a, b = L0.copy(), L0.astype(np.float64)
    for tau in taus:
        a = KO.fed_step(a, np.ones_like(a), tau)
        b = b + float(tau) * ndimage.laplace(b, mode="nearest")                # explicit scheme, no flux through the border
    assert np.abs(a - b).max() < 1e-4 * np.abs(b).max() and abs(float(a.astype(np.float64).mean()) - float(L0.astype(np.float64).mean())) < 1e-6
    # ... and the cycle as a whole diffuses for its stopping time: a cosine mode decays by its eigenvalue
    x = np.arange(64)
    mode = np.cos(np.pi * (x + 0.5) * 4 / 64)[None, :].repeat(8, 0).astype(F)
    out = mode.copy()
    for tau in taus:
        out = KO.fed_step(out, np.ones_like(out), tau)
    lam = 2.0 * (1.0 - np.cos(np.pi * 4 / 64))
    expect = np.prod([1.0 - float(t) * lam for t in taus])
    assert np.abs(out - expect * mode).max() < 1e-5 and abs(expect - np.exp(-1.5 * lam)) < 2e-3


def test_oracle_response_of_a_gaussian_blob():
    h, w, sig, A = 65, 65, 6.0, 1.0
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    x, y = x - 32, y - 32
    G = A * np.exp(-(x * x + y * y) / (2 * sig * sig))
    lx, ly = KO.scharr_x(G.astype(F), 1), KO.scharr_y(G.astype(F), 1)
    det = KO.scharr_x(lx, 1) * KO.scharr_y(ly, 1) - KO.scharr_y(lx, 1) ** 2
    exact = G * G * ((x * x / sig ** 4 - 1 / sig ** 2) * (y * y / sig ** 4 - 1 / sig ** 2) - (x * y / sig ** 4) ** 2)
    inner = (slice(12, 53), slice(12, 53))
    err = np.abs(det[inner] - exact[inner]).max() / exact.max()
    print(f"Hessian determinant of a sigma = 6 blob: {err:.3g} of its peak off the closed form")
    assert err < 0.1 and np.unravel_index(np.argmax(det), det.shape) == (32, 32)      # Scharr at step 1 widens the blob by about 2 / sigma^2


def test_oracle_contrast_factor_against_np_histogram():
    for name in ("blobs65x63", "default96x80", "constant"):
        img32 = KO.convert(P.picture(name))
        k, hmax, npoints, hist = KO.contrast(img32)
        g = KO.gauss(img32, KO.gaussian_taps(1.0))
        m = np.sqrt(KO.scharr_x(g, 1) ** 2 + KO.scharr_y(g, 1) ** 2)[1:-1, 1:-1]
        nz = m[m > 0]
        if nz.size == 0:
            assert k == F(0.03) and name == "constant"
            continue
        assert hmax == m.max() and npoints == nz.size
        ref, _ = np.histogram(np.minimum(np.floor(F(300) * (nz / hmax)), 299), bins=300, range=(0, 300))
        assert np.array_equal(hist, ref)
        c = np.cumsum(ref)
        nbins = int(np.argmax(c >= int(F(nz.size) * F(0.7)))) + 1
        assert k == hmax * (F(nbins) / F(300)) and 0 < k < hmax
        assert FE.contrast_factor(hmax, npoints, hist) == k


# ------------------------------------------------------------------------------------------------------ properties of the oracle
def test_isotropic_blobs_are_found_at_their_centres():
    h, w = 128, 160
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    centres = [(40, 40, 3.0), (100, 50, 4.0), (60, 95, 2.5), (125, 85, 5.0)]
    img = 40.0 + sum(180.0 * np.exp(-((x - cx) ** 2 + (y - cy) ** 2) / (2 * s * s)) for cx, cy, s in centres)
    d = KO.detect(np.clip(np.rint(img), 0, 255).astype(np.uint8))
    worst = 0.0
    for cx, cy, s in centres:
        dist = np.hypot(d["kp"][:, 0] - cx, d["kp"][:, 1] - cy)
        worst = max(worst, float(dist.min()))
    print(f"{len(d['kp'])} keypoints; every blob has one within {worst:.3g} px of its centre")
    assert worst < 0.05                                   # symmetry puts the offset at 0; the uint8 rounding of the picture breaks it a little


def test_rotated_picture_gives_rotated_keypoints():
    """np.rot90 maps (x, y) to (y, w - 1 - x); gradients turn with it, so angles move by -pi / 2 (y points down) and the descriptors,
    taken in the keypoint's own frame, stay.  The orientation is quantised (windows start every 0.15 rad, and pi / 2 is no multiple of
    that), so the angle and with it the descriptor follow only to about a window step."""
    img = P.picture("interior")
    h, w = img.shape
    a, b = KO.detect(img), KO.detect(np.ascontiguousarray(np.rot90(img)))
    ka, kb = a["kp"], b["kp"]
    assert len(ka) == len(kb) >= 50
    pos = np.column_stack([ka[:, 1], (w - 1) - ka[:, 0]])
    j = np.array([int(np.argmin(np.hypot(kb[:, 0] - p[0], kb[:, 1] - p[1]))) for p in pos])
    dpos = np.hypot(kb[j, 0] - pos[:, 0], kb[j, 1] - pos[:, 1])
    assert len(set(j.tolist())) == len(j) and dpos.max() < 1e-3 and np.abs(kb[j, 2] - ka[:, 2]).max() < 1e-3 and np.array_equal(kb[j, 3], ka[:, 3])
    dang = np.abs((kb[j, 4] - (ka[:, 4] - np.pi / 2) + np.pi) % (2 * np.pi) - np.pi)
    ddesc = np.linalg.norm(b["descriptors"][j] - a["descriptors"], axis=1)
    print(f"positions within {dpos.max():.3g} px; angles off by median {np.median(dang):.3g}, max {dang.max():.3g} rad; "
          f"descriptors off by median {np.median(ddesc):.3g}, max {ddesc.max():.3g}")
    q = lambda v: float(np.quantile(v, 0.9))
    print(f"nine in ten: angles within {q(dang):.3g} rad, descriptors within {q(ddesc):.3g}; {int((dang > 0.3).sum())} of {len(dang)} angles off by more "
          f"than two window steps")
    assert np.median(dang) < 0.15 and np.median(ddesc) < 0.15
    # nine keypoints in ten follow to two window steps (0.3 rad); a descriptor of unit length turned by a rad moves by about a times
    # its gradient content, below 2 sin(a / 2) times sqrt(2): 0.42 at 0.3 rad.  The rest are keypoints whose two best windows score
    # alike (a blob is nearly isotropic), so that the quantisation picks another one: at most a tenth, and at most 8 here.
    assert q(dang) < 0.3 and q(ddesc) < 0.42 and (dang > 0.3).sum() <= 8
    # and a descriptor is nearer to its own rotated self than to any other keypoint's
    nn = np.array([int(np.argmin(np.linalg.norm(b["descriptors"] - v, axis=1))) for v in a["descriptors"]])
    assert (nn == j).mean() > 0.9


def shifted_pictures(dx=7, dy=5, w=160, h=128):
    """blobs on a flat background that stay 40 pixels from the border, and the same picture moved by whole pixels: the flat frame
    gives both the same gradient histogram (the same k) and keeps the reflected border out of every stencil that matters"""
    rng = np.random.default_rng(5)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.full((h, w), 100.0)
    for _ in range(60):
        cx, cy, s = rng.uniform(40, w - 47), rng.uniform(40, h - 45), rng.uniform(1.5, 4.0)
        a, ex = rng.uniform(40, 110) * rng.choice([-1.0, 1.0]), rng.uniform(0.7, 1.4)
        img += a * np.exp(-(((x - cx) / ex) ** 2 + ((y - cy) * ex) ** 2) / (2 * s * s))
    A = np.clip(np.rint(img), 0, 255).astype(np.uint8)
    assert (A[:12] == 100).all() and (A[-12 - dy:] == 100).all() and (A[:, :12] == 100).all() and (A[:, -12 - dx:] == 100).all()
    return A, np.roll(A, (dy, dx), (0, 1))


def test_shifted_picture_pairs_every_feature_with_its_shifted_self():
    """A picture and its copy moved by (7, 5) pixels through the reference's matcher (tests/match_oracle.py, the numpy restatement
    the GPU matcher is held to): the keypoints move with the picture, the descriptors stay, and the matcher pairs every feature
    with its shifted self.  One exception is in the nature of the detector as specified: the duplicate pass looks at the same level
    and the level below only, so a blob can be found twice, at levels 3 and 5, within a pixel and with nearly the same descriptor;
    the matcher cannot tell such twins apart and may pair each with the other's shifted self, which is the same place.  Twins (another
    keypoint within 1.5 px) must be paired with themselves or their twin, everything else with itself.  The dynamics stop at 5 000
    steps here (the matcher's 50 000 give the same matches on this pair, measured, at ten times the time)."""
    import match_oracle as MO
    dx, dy = 7, 5
    A, B = shifted_pictures(dx, dy)
    a, b = KO.detect(A), KO.detect(B)
    ka, kb = a["kp"], b["kp"]
    assert len(ka) == len(kb) >= 30 and a["ss"]["k"] == b["ss"]["k"]
    moved = kb[:, :2] - np.array([dx, dy], F)
    dpos, ddesc = np.abs(moved - ka[:, :2]).max(), np.abs(a["descriptors"] - b["descriptors"]).max()
    print(f"{len(ka)} keypoints; positions follow the shift within {dpos:.3g} px, descriptors within {ddesc:.3g}")
    assert dpos < 1e-4 and np.array_equal(kb[:, 2:4], ka[:, 2:4]) and np.abs(kb[:, 4] - ka[:, 4]).max() < 1e-5 and ddesc < 1e-5
    m, rounds = MO.gt_match(ka[:, [0, 1, 2, 4]], kb[:, [0, 1, 2, 4]], a["descriptors"], b["descriptors"], max_iters=5000)
    got = set(map(tuple, m.tolist()))
    dist = np.hypot(ka[:, None, 0] - ka[None, :, 0], ka[:, None, 1] - ka[None, :, 1]) + 1e9 * np.eye(len(ka))
    twin = dist.min(1) < 1.5
    own = [(i, i) in got for i in range(len(ka))]
    print(f"{len(m)} matches in {len(rounds)} rounds; {sum(own)} of {len(ka)} features paired with their shifted selves, {int(twin.sum())} twins, "
          f"{len(got) - sum(own)} other matches")
    assert rounds[0][2] == len(ka)                                   # the first group is one pair per feature
    for i in range(len(ka)):
        partners = {j for (s_, j) in m[:len(ka)].tolist() if s_ == i}
        assert partners, i
        if twin[i]:
            assert partners <= {i, int(np.argmin(dist[i]))}, i
        else:
            assert own[i] and partners == {i}, i
    assert sum(own) >= len(ka) - 2                                   # measured: 37 of 38, one pair of twins crossed


# ----------------------------------------------------------------------------------- what the GPU test's pictures are there for
def test_every_picture_has_what_its_test_needs():
    for name in P.NAMES:
        d = P.oracle(name)
        img = P.picture(name)
        assert img.dtype == np.uint8 and img.shape == d["ss"]["Ldet"].shape[1:]
        if name.startswith("blobs") or name in ("default96x80", "interior", "sea", "inside"):
            assert len(d["candidates"]) >= 1 and d["refined"][:, 4].sum() >= 1, name
    assert P.oracle("constant")["ss"]["k"] == F(0.03) and len(P.oracle("constant")["candidates"]) == 0
    assert len(P.oracle("interior")["kp"]) >= 50 and len(P.oracle("sea")["kp"]) >= 50
    assert len(P.oracle("interior")["candidates"]) > len(P.oracle("interior")["kept"])          # the duplicate pass has work
    assert not P.oracle("interior")["refined"][:, 4].all()                                       # and the refinement rejects something
    assert len(set(P.oracle("interior")["kp"][:, 3].tolist())) >= 4                              # several levels, sizes and sample steps


def test_border_probes_sit_one_pixel_inside_and_outside_the_rule():
    free = lambda ss: KO.extrema(ss["Ldet"], [dict(l, esigma=F(0)) for l in ss["levels"]])[0].tolist()
    inside, outside = P.oracle("inside"), P.oracle("outside")
    assert free(inside["ss"]) == [[2, 31, 10]] and free(outside["ss"]) == [[2, 31, 9]]          # the same extremum, one column apart
    assert inside["candidates"].tolist() == [[2, 31, 10]] and outside["candidates"].tolist() == []


def test_orientation_fragility_of_the_compared_pictures():
    for name in P.ORIENTED:
        d = P.oracle(name)
        a, fragile, admissible = KO.orientation(d["kp"], d["ss"]["Lx"], d["ss"]["Ly"], flags=True, admissible=True)
        print(f"{name}: {fragile.sum()} of {len(fragile)} keypoints fragile ({100 * fragile.mean():.1f} %), "
              f"{max([len(set(admissible[q].tolist())) for q in np.flatnonzero(fragile)], default=0)} admissible angles at most")
        assert fragile.mean() <= 0.05 and (~fragile).sum() >= 50
        assert np.array_equal(a, d["kp"][:, 4])
        for q in range(len(a)):                                # the oracle's own choice is admissible; nothing is listed for the others
            assert (a[q] in admissible[q].tolist()) if fragile[q] else len(admissible[q]) == 0, (name, q)


MISTAKES = {"border": dict(border="symmetric"), "extremum": dict(strict=False), "sigma_size": dict(sigma_sq=False),
            "fed_order": dict(fed_reorder=False), "rotation": dict(rotate_sign=-1.0)}


@pytest.mark.parametrize("mistake", sorted(MISTAKES))
def test_probes_are_changed_by_the_mistake_they_catch(mistake):
    kw = MISTAKES[mistake]

    def run(name, **k):
        no, ns = P.options(name)
        return KO.detect(P.picture(name), no, ns, **k)

    if mistake == "border":
        for name in ("blobs33x29", "default96x80", "blobs257x40"):
            good, bad = P.oracle(name)["ss"], run(name, **kw)["ss"]
            assert not np.array_equal(good["Lx"], bad["Lx"]) and not np.array_equal(good["Ldet"][:, 0, :], bad["Ldet"][:, 0, :]), name
    elif mistake == "extremum":
        # a plateau: two equal neighbours are both extrema under >=, neither under >
        ldet = np.zeros((3, 7, 8), F)
        ldet[1, 3, 3] = ldet[1, 3, 4] = F(0.01)
        lv = [dict(l, esigma=F(0)) for l in KO.levels(1, 3)]
        assert len(KO.extrema(ldet, lv)[0]) == 0 and len(KO.extrema(ldet, lv, strict=False)[0]) == 2
        # the constant and single-pixel pictures hold such ties: level 1 repeats level 0 (same Lsmooth, same sigma_size)
        good, bad = P.oracle("pixel"), run("pixel", **kw)
        assert np.array_equal(good["ss"]["Ldet"][0], good["ss"]["Ldet"][1])
        assert len(bad["candidates"]) > len(good["candidates"])
    elif mistake == "sigma_size":
        for name in ("blobs65x63", "default96x80"):
            good, bad = P.oracle(name), run(name, **kw)
            assert not np.array_equal(good["ss"]["Ldet"], bad["ss"]["Ldet"]) and not np.array_equal(good["candidates"], bad["candidates"]), name
    elif mistake == "fed_order":
        for name in ("blobs64x64", "default96x80"):
            good, bad = P.oracle(name)["ss"], run(name, **kw)["ss"]
            assert np.array_equal(good["Lt"][0], bad["Lt"][0]) and not np.array_equal(good["Lt"][1:], bad["Lt"][1:]), name
    else:
        for name in P.ORIENTED:
            good = P.oracle(name)
            bad = KO.descriptors(good["kp"], good["ss"]["Lx"], good["ss"]["Ly"], rotate_sign=-1.0)
            assert np.abs(bad - good["descriptors"]).max() > 0.05, name


# ---------------------------------------------------------------------------------------------------------------- subsampling
def reference_subsample(pts, img_width, img_height, max_features=2000, num_subdivisions=5, min_distance=10.0):
    """FeatureSet.cpp:70-97 and 218-321, loop by loop.  pts: (x, y, response) float32.  std::sort is replaced by a stable sort."""
    pts = [(F(p[0]), F(p[1]), F(p[2])) for p in pts]
    border_width = max(int(img_width / 30.0), 2)
    width, height = F(img_width) / F(num_subdivisions), F(img_height) / F(num_subdivisions)
    areas = []
    for ii in range(num_subdivisions):
        for jj in range(num_subdivisions):
            areas.append({"x": int(F(img_width) / F(num_subdivisions) * F(ii)), "y": int(F(img_height) / F(num_subdivisions) * F(jj)),
                          "w": int(width), "h": int(height), "surfs": []})
    for i, (x, y, r) in enumerate(pts):
        for a in areas:
            if (x > border_width and x < img_width - border_width and y > border_width and y < img_height - border_width and x > a["x"] and y > a["y"]
                    and x < a["x"] + a["w"] and y < a["y"] + a["h"]):
                a["surfs"].append(i)
    points_per_area = int(max_features // len(areas))
    extra = 0
    for a in areas:
        if len(a["surfs"]) < points_per_area:
            extra += points_per_area - len(a["surfs"])
    points_per_area = int(F(points_per_area) + F(extra) / F(len(areas)))
    for a in areas:
        if len(a["surfs"]) < 2:
            continue
        surfs = sorted(a["surfs"], key=lambda i: -pts[i][2])
        last = len(surfs) - 1
        k = 0
        while k <= last:
            k2 = k + 1
            while k2 <= last:
                dx, dy = pts[surfs[k]][0] - pts[surfs[k2]][0], pts[surfs[k]][1] - pts[surfs[k2]][1]
                if float(np.sqrt(dx * dx + dy * dy)) < min_distance:
                    surfs[k2] = surfs[last]
                    last -= 1
                    k2 -= 1
                k2 += 1
            k += 1
        surfs = surfs[:last + 1]
        if len(surfs) > points_per_area:
            surfs = surfs[:points_per_area]
        a["surfs"] = surfs
    out, surf_index, area_index, num_skip, more = [], 0, 0, 0, True
    while more:
        if len(areas[area_index]["surfs"]) > surf_index:
            out.append(areas[area_index]["surfs"][surf_index])
        else:
            num_skip += 1
        if num_skip == len(areas):
            more = False
        area_index += 1
        if area_index == len(areas):
            area_index, num_skip, surf_index = 0, 0, surf_index + 1
    return out


def _cloud(seed, n, w, h, lattice=False):
    rng = np.random.default_rng(seed)
    if lattice:          # whole and half pixels: many points exactly on area and border lines, many at exactly the minimum distance
        xy = np.column_stack([rng.integers(0, 2 * w, n) / 2.0, rng.integers(0, 2 * h, n) / 2.0])
    else:
        xy = np.column_stack([rng.uniform(0, w, n), rng.uniform(0, h, n)])
    resp = rng.integers(1, 40, n) / 1000.0 if lattice else rng.uniform(1e-4, 0.1, n)        # the lattice clouds also tie in response
    return np.column_stack([xy, resp]).astype(F)


@pytest.mark.parametrize("case", ["random", "lattice", "few", "many", "empty_areas", "one_per_area", "odd_size"])
def test_subsampling_is_the_references(case):
    w, h, kw = 300, 200, {}
    if case == "random":
        pts = _cloud(1, 900, w, h)
    elif case == "lattice":
        pts = _cloud(2, 1500, w, h, lattice=True)
        assert (pts[:, 0] == 60).any() and (pts[:, 0] == 10).any() and (pts[:, 1] == 40).any()      # on area lines and on the border line
    elif case == "few":
        pts, kw = _cloud(3, 40, w, h), dict(max_features=2000)
    elif case == "many":
        pts, kw = _cloud(4, 3000, w, h), dict(max_features=100, min_distance=4.0)
    elif case == "empty_areas":
        pts = _cloud(5, 600, w, h)
        pts = pts[(pts[:, 0] < 120) | (pts[:, 1] > 160)]
    elif case == "one_per_area":
        pts = np.array([[30 + 60 * i, 20 + 40 * j, 0.01 * (1 + i + j)] for i in range(5) for j in range(5)] + [[35, 25, 0.5], [151, 101, 0.2]], F)
    else:
        w, h = 257, 131
        pts, kw = _cloud(6, 1200, w, h, lattice=True), dict(subdivisions=3, max_features=333, min_distance=7.5)
    got = FE.subsample_features(pts, w, h, **kw).tolist()
    ref = reference_subsample(pts, w, h, kw.get("max_features", 2000), kw.get("subdivisions", 5), kw.get("min_distance", 10.0))
    assert got == ref and len(set(got)) == len(got)
    if case == "one_per_area":
        # an area with one keypoint keeps it; areas 0 and 12 hold two closer than the minimum distance: the stronger stays and comes first
        assert len(got) == 25 and got[0] == 25 and 0 not in got and 26 in got and 12 not in got
    if case == "many":
        assert len(got) <= 100 + 25
    assert len(FE.subsample_features(np.zeros((0, 3), F), w, h)) == 0


# ---------------------------------------------------------------------------------------------------------------------- files
def _stub(monkeypatch, calls):
    def detect_features(image, max_features=2000, options=None, subdivisions=5, min_distance=10.0, ctx=None):
        calls.append((image.shape, image.dtype, max_features, options, subdivisions, min_distance))
        n = 12
        xy = np.column_stack([np.arange(n) * 3.0 + image[0, 0], np.arange(n) * 2.0])
        return match.Features(xy, np.full(n, 5.0), np.zeros(n), np.eye(n, 64))

    def gt_match(fa, fb, **kw):
        calls.append(kw)
        m = np.column_stack([np.arange(len(fa)), np.arange(len(fb))]).astype(np.int32)
        return match.MatchResult(m, fa.xy[m[:, 0]], fb.xy[m[:, 1]])
    monkeypatch.setattr(FE, "detect_features", detect_features)
    monkeypatch.setattr(FE._match, "gt_match", gt_match)


def test_match_workdir_files_markers_and_exit_codes(tmp_path, monkeypatch, capsys):
    from PIL import Image
    calls = []
    _stub(monkeypatch, calls)
    (tmp_path / "undistorted").mkdir()
    Image.fromarray(np.full((40, 50), 7, np.uint8)).save(tmp_path / "undistorted" / "00000000.png")
    Image.fromarray(np.full((40, 50, 3), 9, np.uint8)).save(tmp_path / "undistorted" / "00000001.png")       # colour is read as grey
    cfg = tmp_path / "cfg.txt"
    cfg.write_text("FEATURE_HESSIAN_THRESHOLD=0.001\nFEATURE_N_OCTAVES=3 # three\nFEATURE_N_LAYERS=2\nNUM_FEATURES_PER_IMAGE=500\nAREA_SUBDIVISION=4\n"
                   "FEATURE_MIN_DISTANCE=6.5\nMATCHER_LAMBDA=0.001\nMATCHER_POPULATION_THRESHOLD=0.6\nMATCHER_MIN_GROUP_SIZE=7\nMATCHER_MAX_ROUNDS=3\n"
                   "MATCHER_SKIP_GT=true\n")
    assert FE.main([str(tmp_path), str(cfg)]) == 0
    assert capsys.readouterr().out.split() == ["[P|10|100]", "[P|20|100]"]
    assert calls[0] == ((40, 50), np.uint8, 500, FE.KazeOptions(0.001, 3, 2), 4, 6.5) and calls[1][0] == (40, 50)
    assert calls[2]["lam"] == 0.001 and calls[2]["pop_threshold"] == 0.6 and calls[2]["min_group_size"] == 7 and calls[2]["max_rounds"] == 3
    assert calls[2]["skip_gt"] is True
    a, b = match.read_matches(tmp_path / "matches_unfiltered.txt")
    assert a.shape == (12, 2) and a[0, 0] == 7 and b[0, 0] == 9 and a[3, 1] == 6
    del calls[:]
    assert FE.match_workdir(tmp_path) == 0 and calls[0][2:] == (2000, FE.KazeOptions(), 5, 10.0) and calls[2]["skip_gt"] is False
    capsys.readouterr()
    assert FE.main([]) == -1 and FE.main([str(tmp_path / "nowhere")]) == -1 and FE.main(["a", "b", "c"]) == -1
    assert FE.match_workdir(tmp_path, tmp_path / "missing.txt") == -1
    (tmp_path / "undistorted" / "00000001.png").unlink()
    assert FE.match_workdir(tmp_path) == -1
    assert "00000001.png" in capsys.readouterr().err


def test_match_workdir_of_featureless_pictures_returns_minus_one(tmp_path, monkeypatch, capsys):
    """A picture without features gives an empty feature set, which the matcher refuses (the real gt_match, before it touches a GPU):
    the reference catches its matcher's exception and returns -1 (wass_match.cpp:363-371), so does match_workdir, with one line on
    stderr, both progress markers and no matches_unfiltered.txt."""
    from PIL import Image
    some = lambda n: match.Features(np.arange(2 * n).reshape(n, 2), np.full(n, 5.0), np.zeros(n), np.eye(n, 64))

    def detect_features(image, max_features=2000, options=None, subdivisions=5, min_distance=10.0, ctx=None):
        if (image == image[0, 0]).all():
            return match.Features(np.zeros((0, 2)), np.zeros(0), np.zeros(0), np.zeros((0, 64)))
        if image.shape[0] < 23:
            raise ValueError(f"image: {image.shape[0]} x {image.shape[1]} is smaller than the largest reflect-101 reach")
        return some(12)
    monkeypatch.setattr(FE, "detect_features", detect_features)
    (tmp_path / "undistorted").mkdir()
    textured = np.arange(40 * 50, dtype=np.uint8).reshape(40, 50)
    for flat in ((0,), (1,), (0, 1)):
        for cam in (0, 1):
            Image.fromarray(np.full((40, 50), 7, np.uint8) if cam in flat else textured).save(tmp_path / "undistorted" / f"{cam:08d}.png")
        assert FE.main([str(tmp_path)]) == -1
        io = capsys.readouterr()
        assert io.out.split() == ["[P|10|100]", "[P|20|100]"]
        assert len(io.err.strip().splitlines()) == 1 and "feature" in io.err and "Traceback" not in io.err
        assert not (tmp_path / "matches_unfiltered.txt").exists()
    # a picture the detector refuses ends the same way, after its own marker
    Image.fromarray(textured[:20]).save(tmp_path / "undistorted" / "00000001.png")
    Image.fromarray(textured).save(tmp_path / "undistorted" / "00000000.png")
    assert FE.match_workdir(tmp_path) == -1
    io = capsys.readouterr()
    assert io.out.split() == ["[P|10|100]", "[P|20|100]"] and len(io.err.strip().splitlines()) == 1 and "00000001.png" in io.err
    assert not (tmp_path / "matches_unfiltered.txt").exists()


def test_oracle_against_opencv_pin():
    """scripts/pin_with_opencv.py records cv2.KAZE on the 'interior' picture where OpenCV exists; until then the parity is unpinned.
    Compared: the number of keypoints, and for the oracle's keypoints their nearest recorded one: position, size (a diameter in both),
    angle (OpenCV's in degrees, its fastAtan2 is 0.3 degrees coarse and a window step is 0.15 rad) and descriptor."""
    if not os.path.exists(GOLDEN):
        pytest.skip("tests/golden/kaze_pin.npz has not been recorded (no OpenCV here): DESIGN.md 8 (27)")
    z = np.load(GOLDEN)
    assert np.array_equal(z["image"], P.picture("interior"))
    d = P.oracle("interior")
    pts, desc = z["keypoints"], z["descriptors"]             # x, y, size, angle (degrees), response, octave, class_id
    j = np.array([int(np.argmin(np.hypot(pts[:, 0] - k[0], pts[:, 1] - k[1]))) for k in d["kp"]])
    dist = np.hypot(pts[j, 0] - d["kp"][:, 0], pts[j, 1] - d["kp"][:, 1])
    near = dist < 0.5
    dsize = np.abs(pts[j, 2] - d["kp"][:, 2])[near] / d["kp"][near, 2]
    dang = np.abs((np.deg2rad(pts[j, 3]) - d["kp"][:, 4] + np.pi) % (2 * np.pi) - np.pi)[near]
    ddesc = np.linalg.norm(desc[j] - d["descriptors"], axis=1)[near]
    print(f"OpenCV {z['opencv_version']}: {len(pts)} keypoints, the oracle {len(d['kp'])}; {np.mean(near) * 100:.0f} % within half a pixel; of those: "
          f"size within {np.median(dsize):.3g} (median, relative), angle {np.median(dang):.3g} rad, descriptor {np.median(ddesc):.3g}; "
          f"nine in ten: {np.quantile(dsize, 0.9):.3g}, {np.quantile(dang, 0.9):.3g}, {np.quantile(ddesc, 0.9):.3g}")
    assert abs(len(pts) - len(d["kp"])) <= 0.1 * len(pts) and np.mean(near) >= 0.9
    assert np.quantile(dsize, 0.9) < 0.05 and np.quantile(dang, 0.9) < 0.3 and np.quantile(ddesc, 0.9) < 0.42
