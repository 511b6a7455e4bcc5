"""The KAZE kernels (csrc/kaze.hip) on synthetic planes whose answer is known by hand (tests/kaze_probes.py), on the stage entries at
the limits their argument checks admit, on the smallest pictures the pipeline takes and on pictures without features.
tests/test_kaze_edges.py holds every probe to the oracle and to the mistake it catches, without a GPU.

A KazePyramid of a constant picture gives the device planes; the probes overwrite Ldet, Lx and Ly.  Where a probe needs its own
esigma, taps, reach, pitch or raw keys the C entry is called through ctx._lib, as KazePyramid itself does.  Extrema, refinement and
every + - x / stage are compared bit for bit; orientation and descriptors with the tolerance of tests/test_kaze_gpu.py: half a
float32 ulp plus four times the oracle's own float32-against-fp64 difference, taken over the probes of the test and printed."""
import ctypes as C

import numpy as np
import pytest

import kaze_oracle as KO
import kaze_probes as KP
from wass_amd import features as FE

pytestmark = pytest.mark.gpu
F = np.float32


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def sync():
    import torch
    torch.cuda.synchronize()


def angle_diff(a, b):
    d = np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))
    return np.minimum(d, 2 * np.pi - d)


_pyramids = {}


def pyramid(ctx, w=KP.WK, h=KP.HK, no=2, ns=2):
    """the pyramid of a constant picture, made once per shape; its planes are the probes' to overwrite"""
    key = (w, h, no, ns)
    if key not in _pyramids:
        _pyramids[key] = FE.KazePyramid(np.full((h, w), 97, np.uint8), FE.KazeOptions(1e-4, no, ns), ctx)
    return _pyramids[key]


def load(pyr, Lx=None, Ly=None, Ldet=None):
    import torch
    for t, a in ((pyr.Lx, Lx), (pyr.Ly, Ly), (pyr.Ldet, Ldet)):
        if a is not None:
            assert tuple(t.shape) == a.shape
            t.copy_(torch.from_numpy(np.ascontiguousarray(a, F)))
    sync()


# ------------------------------------------------------------------------------------------------------------------- extrema
def extrema_dev(ctx, vol, threshold, esigma, cap=4096):
    """wass_kaze_extrema_dev on a volume of its own: (status, count, candidates sorted, their values)"""
    import torch
    N, h, w = vol.shape
    d = dev(vol)
    keys = torch.full((cap,), -7, dtype=torch.int64, device=d.device)
    d_count = torch.zeros(1, dtype=torch.int32, device=d.device)
    es = np.ascontiguousarray(esigma, F)
    assert es.shape == (N,)
    count = C.c_uint32()
    sync()
    rc = ctx._check(ctx._lib.wass_kaze_extrema_dev(ctx._h, d.data_ptr(), h * w, N, h, w, float(F(threshold)), es.ctypes.data, keys.data_ptr(), cap,
                                                   d_count.data_ptr(), C.byref(count)), allow=(FE.CAP_REACHED,))
    k = np.sort(keys[:min(int(count.value), cap)].cpu().numpy())
    assert (keys[min(int(count.value), cap):] == -7).all()                   # nothing is written behind the list
    cand = np.stack([k // (h * w), (k // w) % h, k % w], axis=1).astype(np.int64).reshape(-1, 3)
    return rc, int(count.value), cand, vol[cand[:, 0], cand[:, 1], cand[:, 2]]


@pytest.mark.parametrize("group", ["isolated", "thresholds", "border"])
def test_extrema_of_planted_peaks(gpu_ctx, group):
    cases = {"isolated": KP.isolated_peaks, "thresholds": KP.threshold_probes, "border": KP.border_probes}[group]()
    for name, vol, thr, es, cand, vals in cases:
        rc, count, got, gv = extrema_dev(gpu_ctx, vol, thr, es)
        assert rc == 0 and count == len(cand), name
        assert np.array_equal(got, cand) and np.array_equal(gv, vals), f"{name}: {got.tolist()} for {cand.tolist()}"


def test_extrema_ties_and_nan(gpu_ctx):
    vol, cand = KP.tie_probes()
    rc, count, got, _ = extrema_dev(gpu_ctx, vol, 1e-4, np.zeros(3, F))
    tied = [KP.NEIGHBOURS[(x - 2) // 4] if x < KP.TIE_X(26) else "the NaN" for x in got[:, 2].tolist() if x != KP.TIE_X(26)]
    assert rc == 0 and np.array_equal(got, cand), f"peaks found beside a neighbour that equals them: {tied}"


def test_extrema_beyond_the_cap(gpu_ctx):
    ldet, planted = KP.cap_probe()
    pyr = pyramid(gpu_ctx)
    load(pyr, Ldet=ldet)
    full = {tuple(c) for c in planted.tolist()}
    for cap in (1, 7):
        rc, cand, vals = pyr.candidates(cap)
        assert rc == FE.CAP_REACHED and cand.shape == (cap, 3) and len({tuple(c) for c in cand.tolist()}) == cap
        assert all(tuple(c) in full for c in cand.tolist()) and np.array_equal(vals, ldet[cand[:, 0], cand[:, 1], cand[:, 2]])
        rc, count, got, _ = extrema_dev(gpu_ctx, ldet, 1e-4, pyr.levels.esigma, cap)
        assert rc == FE.CAP_REACHED and count == len(planted) and len(got) == cap and all(tuple(c) in full for c in got.tolist())
    rc, cand, vals = pyr.candidates(len(planted))
    assert rc == 0 and np.array_equal(cand, planted)


# ---------------------------------------------------------------------------------------------------------------- refinement
def refine_dev(ctx, vol, keys):
    import torch
    N, h, w = vol.shape
    d, k = dev(vol), dev(np.asarray(keys, np.int64))
    out = torch.full((len(keys) + 1, 5), -7.0, dtype=torch.float32, device=d.device)
    sync()
    ctx._check(ctx._lib.wass_kaze_refine_dev(ctx._h, d.data_ptr(), h * w, N, h, w, k.data_ptr(), len(keys), out.data_ptr()))
    out = out.cpu().numpy()
    assert (out[-1] == -7).all()
    return out[:-1]


def test_refinement_by_hand_bit_for_bit(gpu_ctx):
    vol, cand, exp, case = KP.refine_probes()
    ref = KO.refine(vol, cand)
    keys = (cand[:, 0] * KP.H9 + cand[:, 1]) * KP.W9 + cand[:, 2]
    names = [c[0] for c in KP.REFINE_CASES]
    for n in (1, 63, 64, 65, 129):
        got = refine_dev(gpu_ctx, vol, keys[:n])
        bad = sorted({names[c] for c in case[:n][(got != ref[:n]).any(axis=1)].tolist()})
        assert np.array_equal(got, ref[:n]), f"n = {n}: {bad}"
    hand = ~np.isnan(exp[:, 0])
    assert np.array_equal(got[hand], exp[hand])
    # and through KazePyramid.refine: the same volume as levels 0 .. 2 of a pyramid of four
    pyr = pyramid(gpu_ctx, KP.W9, KP.H9)
    load(pyr, Ldet=np.concatenate([vol, np.zeros((1, KP.H9, KP.W9), F)]))
    assert np.array_equal(pyr.refine(cand), ref)


def test_refinement_refuses_keys_that_are_no_candidates(gpu_ctx):
    """Every key below fails the kernel's range test before anything is read (k_kaze_refine: x, y, level from the key, then the
    test, then the loads), and the good keys read their own 3 x 3 x 3 cells inside the volume."""
    vol, cand, exp, case = KP.refine_probes()
    keys, rows = KP.raw_keys()
    got = refine_dev(gpu_ctx, vol, keys)
    good = np.array([r is None for r in rows])
    k = keys[good]
    own = np.stack([k // (KP.W9 * KP.H9), (k // KP.W9) % KP.H9, k % KP.W9], axis=1)
    assert np.array_equal(got[good], KO.refine(vol, own))
    want = np.array([[r[0], r[1], 0, 0, 0] for r in rows if r is not None], F)
    assert np.array_equal(got[~good], want), got[~good].tolist()


# --------------------------------------------------------------------------------------------------------------- orientation
def check_angles(name, got, a32, a64, fragile, admissible):
    """every angle within the tolerance of the oracle's, a fragile keypoint's within it of one of its admissible angles"""
    keep = ~fragile
    tol = 0.5 * float(np.spacing(F(2 * np.pi))) + 4.0 * (angle_diff(a32[keep], a64[keep]).max() if keep.any() else 0.0)
    err = angle_diff(got[keep], a32[keep]).max() if keep.any() else 0.0
    ferr = max([angle_diff(admissible[q], got[q]).min() for q in np.flatnonzero(fragile)], default=0.0)
    print(f"{name}: {keep.sum()} keypoints, largest difference {err:.3g} rad, tolerance {tol:.3g} rad; {fragile.sum()} fragile, "
          f"{ferr:.3g} rad off their nearest admissible angle")
    assert (got >= 0).all() and (got < F(2 * np.pi) + 1e-6).all()
    assert err <= tol and ferr <= tol
    return tol


def test_orientation_of_k_hot_planes(gpu_ctx):
    pyr = pyramid(gpu_ctx)
    probes = KP.orientation_khot()
    got, a32, a64, names = [], [], [], []
    for p in probes:
        load(pyr, Lx=p["Lx"], Ly=p["Ly"])
        got.append(pyr.orientation(p["kp"]))
        a32.append(KO.orientation(p["kp"], p["Lx"], p["Ly"]))
        a64.append(KO.orientation(p["kp"], p["Lx"], p["Ly"], np.float64))
        names += [p["name"]] * len(p["kp"])
    got, a32, a64 = np.concatenate(got), np.concatenate(a32), np.concatenate(a64)
    expect = np.concatenate([p["expect"] for p in probes])
    # exact ties are the same ties in float32 on the device and in numpy: every probe is compared, none is set aside as fragile
    tol = 0.5 * float(np.spacing(F(2 * np.pi))) + 4.0 * angle_diff(a32, a64).max()
    err = angle_diff(got, a32)
    print(f"{len(got)} k-hot probes: largest difference {err.max():.3g} rad, tolerance {tol:.3g} rad")
    bad = [f"{names[q]}: {got[q]} for {a32[q]}" for q in np.flatnonzero(err > tol)]
    assert not bad, bad
    zero = expect == 0
    assert zero.sum() == 3 and (got[zero] == 0).all() and not np.signbit(got[zero]).any()


@pytest.mark.parametrize("table", ["edges", "sizes"])
def test_orientation_on_dense_planes(gpu_ctx, table):
    Lx, Ly = KP.dense_planes()
    t = KP.orientation_edge_table() if table == "edges" else KP.orientation_size_table()
    pyr = pyramid(gpu_ctx)
    load(pyr, Lx=Lx, Ly=Ly)
    a32, fragile, adm = KO.orientation(t, Lx, Ly, flags=True, admissible=True)
    a64 = KO.orientation(t, Lx, Ly, np.float64)
    check_angles(table, pyr.orientation(t), a32, a64, fragile, adm)


# ---------------------------------------------------------------------------------------------------------------- descriptors
def desc_tol(d32, d64):
    return 0.5 * float(np.spacing(F(1.0))) + 4.0 * np.abs(d32.astype(np.float64) - d64).max()


@pytest.mark.parametrize("which", [0, 1], ids=["Lx", "Ly"])
def test_descriptor_of_one_hot_pixel(gpu_ctx, which):
    Lx, Ly, table = KP.descriptor_onehot(which)
    pyr = pyramid(gpu_ctx)
    load(pyr, Lx=Lx, Ly=Ly)
    got = pyr.descriptors(table)
    ref, d64 = KO.descriptors(table, Lx, Ly), KO.descriptors(table, Lx, Ly, np.float64)
    tol, err = desc_tol(ref, d64), np.abs(got.astype(np.float64) - ref).max()
    print(f"one hot pixel of {'Lx' if which == 0 else 'Ly'}: largest difference {err:.3g}, tolerance {tol:.3g}")
    for q in range(len(table)):
        assert np.array_equal(got[q] != 0, ref[q] != 0), f"scale {table[q, 2] / 2}, angle {table[q, 4]}: entries {np.flatnonzero(got[q] != 0).tolist()} " \
                                                         f"for {np.flatnonzero(ref[q] != 0).tolist()}"
    assert np.array_equal(np.sign(got), np.sign(ref)) and err <= tol


def test_descriptors_at_the_corners_and_sides(gpu_ctx):
    Lx, Ly = KP.dense_planes()
    t = KP.descriptor_edge_table()
    pyr = pyramid(gpu_ctx)
    load(pyr, Lx=Lx, Ly=Ly)
    got = pyr.descriptors(t)
    ref, d64 = KO.descriptors(t, Lx, Ly), KO.descriptors(t, Lx, Ly, np.float64)
    tol, err = desc_tol(ref, d64), np.abs(got.astype(np.float64) - ref).max()
    print(f"corners and sides at scale 6: largest difference {err:.3g}, tolerance {tol:.3g}")
    assert err <= tol


def test_descriptor_of_zero_planes_is_nan(gpu_ctx):
    zero = np.zeros((KP.NLEV, KP.HK, KP.WK), F)
    pyr = pyramid(gpu_ctx)
    load(pyr, Lx=zero, Ly=zero)
    t = KP.descriptor_edge_table()
    assert np.isnan(KO.descriptors(t, zero, zero)).all() and np.isnan(pyr.descriptors(t)).all()        # 0 / 0, as the reference has it
    assert (pyr.orientation(t[:, :4]) == 0).all()


def test_descriptor_batches(gpu_ctx):
    Lx, Ly = KP.dense_planes()
    t = KP.descriptor_batch_table(65)
    pyr = pyramid(gpu_ctx)
    load(pyr, Lx=Lx, Ly=Ly)
    all65 = pyr.descriptors(t)
    ref, d64 = KO.descriptors(t, Lx, Ly), KO.descriptors(t, Lx, Ly, np.float64)
    # a size below 1 gives scale 0 and with it a Gaussian of width 0: NaN, in the oracle as on the device (no detected keypoint is that small)
    flat = (t[:, 2] / F(2) + F(0.5)).astype(np.int64) == 0
    assert 0 < flat.sum() < 10 and np.isnan(ref[flat]).all() and np.isnan(all65[flat]).all() and np.isfinite(all65[~flat]).all()
    tol, err = desc_tol(ref[~flat], d64[~flat]), np.abs(all65[~flat].astype(np.float64) - ref[~flat]).max()
    print(f"{(~flat).sum()} keypoints: largest difference {err:.3g}, tolerance {tol:.3g}")
    assert err <= tol
    assert np.array_equal(pyr.descriptors(t[:2]), all65[:2], equal_nan=True)
    angles = pyr.orientation(t[:, :4])
    for k in range(65):
        assert np.array_equal(pyr.descriptors(t[k:k + 1])[0], all65[k], equal_nan=True), k
        assert pyr.orientation(t[k:k + 1, :4])[0] == angles[k], k


# -------------------------------------------------------------------------------------------------------------- stage entries
class Stage:
    """the C entries on planes of their own"""

    def __init__(self, ctx):
        self.ctx, self.lib, self.hd = ctx, ctx._lib, ctx._h

    def call(self, fn, *args, allow=()):
        sync()
        return self.ctx._check(getattr(self.lib, fn)(self.hd, *args), allow=allow)

    def gauss(self, src, taps):
        import torch
        h, w = src.shape
        s, tmp, dst = dev(src), torch.zeros((h, w), dtype=torch.float32, device="cuda"), torch.zeros((h, w), dtype=torch.float32, device="cuda")
        t = np.ascontiguousarray(taps, F)
        self.call("wass_kaze_gauss_dev", s.data_ptr(), h, w, t.ctypes.data, len(t), tmp.data_ptr(), dst.data_ptr())
        assert np.array_equal(s.cpu().numpy(), src)
        return dst.cpu().numpy()

    def scharr(self, src, reach):
        import torch
        h, w = src.shape
        n, wn = KO.scharr_weights(reach)
        s, lx, ly = dev(src), torch.zeros((h, w), dtype=torch.float32, device="cuda"), torch.zeros((h, w), dtype=torch.float32, device="cuda")
        self.call("wass_kaze_scharr_dev", s.data_ptr(), h, w, reach, float(n), float(wn), lx.data_ptr(), ly.data_ptr())
        return lx, ly

    def hessian(self, lx, ly, reach, extra):
        """(Ldet, Lxx, Lxy, Lyy or None, Lx and Ly after their scaling) of device planes that are left alone"""
        import torch
        h, w = lx.shape
        n, wn = KO.scharr_weights(reach)
        a, b = lx.clone(), ly.clone()
        out = [torch.zeros((h, w), dtype=torch.float32, device="cuda") for _ in range(4 if extra else 1)]
        ptrs = [o.data_ptr() for o in out] + [None] * (4 - len(out))
        self.call("wass_kaze_hessian_dev", a.data_ptr(), b.data_ptr(), h, w, reach, float(n), float(wn), *ptrs)
        return [o.cpu().numpy() for o in out] + [a.cpu().numpy(), b.cpu().numpy()]


def test_gauss_entry_from_1_to_15_taps(gpu_ctx):
    st = Stage(gpu_ctx)
    for w, h in KP.STAGE_SHAPES:
        src = KP.plane(w, h)
        for taps in KP.tap_sets():
            got, ref = st.gauss(src, taps), KO.gauss(src, taps)
            assert np.array_equal(got, ref), f"{w} x {h}, {len(taps)} taps: {int((got != ref).sum())} values differ"


def test_scharr_and_hessian_entries_at_both_ends_of_the_reach(gpu_ctx):
    st = Stage(gpu_ctx)
    for w, h in KP.STAGE_SHAPES:
        src = KP.plane(w, h, 1)
        for s in (1, min(h, w) - 1):
            lx, ly = st.scharr(src, s)
            rx, ry = KO.scharr_x(src, s), KO.scharr_y(src, s)
            assert np.array_equal(lx.cpu().numpy(), rx) and np.array_equal(ly.cpu().numpy(), ry), f"{w} x {h}, reach {s}"
            ss2 = F(s) * F(s)
            rxx, rxy, ryy = KO.scharr_x(rx, s) * ss2, KO.scharr_y(rx, s) * ss2, KO.scharr_y(ry, s) * ss2
            det, sx, sy = st.hessian(lx, ly, s, False)
            full = st.hessian(lx, ly, s, True)
            for name, got, ref in (("Ldet", det, rxx * ryy - rxy * rxy), ("Ldet with the second derivatives kept", full[0], rxx * ryy - rxy * rxy),
                                   ("Lxx", full[1], rxx), ("Lxy", full[2], rxy), ("Lyy", full[3], ryy), ("Lx scaled", sx, rx * F(s)), ("Ly scaled", sy, ry * F(s)),
                                   ("Lx scaled (kept)", full[4], rx * F(s))):
                assert np.array_equal(got, ref), f"{w} x {h}, reach {s}: {name}"


def test_diffuse_entry_of_0_to_3_steps(gpu_ctx):
    import torch
    st = Stage(gpu_ctx)
    taus = np.array([0.25, 0.6, 0.1], F)
    for w, h in KP.STAGE_SHAPES:
        L0 = KP.plane(w, h, 2)
        flow = np.abs(KP.plane(w, h, 3))
        for n in (0, 1, 2, 3):
            lt, tmp, fl = dev(L0), torch.full((h, w), -7.0, dtype=torch.float32, device="cuda"), dev(flow)
            st.call("wass_kaze_diffuse_dev", lt.data_ptr(), tmp.data_ptr(), fl.data_ptr(), h, w, taus.ctypes.data, n)
            ref = L0
            for t in taus[:n]:
                ref = KO.fed_step(ref, flow, t)
            assert np.array_equal(lt.cpu().numpy(), ref), f"{w} x {h}, {n} steps"
            assert np.array_equal(fl.cpu().numpy(), flow)
            if n == 0:
                assert (tmp == -7).all()


def test_flow_entry_where_k_squared_underflows(gpu_ctx):
    import torch
    st = Stage(gpu_ctx)
    w, h = 129, 7
    lx, ly = KP.plane(w, h, 4), KP.plane(w, h, 5)
    lx[0, :6], ly[0, :6] = [0, 1e-20, 1e-25, 0, 3e-23, 1], [0, 0, 1e-25, 1e-20, 0, 0]
    for k in (0.03, 1e-22, 1e-23):
        a, b, out = dev(lx), dev(ly), torch.zeros((h, w), dtype=torch.float32, device="cuda")
        st.call("wass_kaze_flow_dev", a.data_ptr(), b.data_ptr(), h, w, k, out.data_ptr())
        with np.errstate(all="ignore"):
            ref = KO.flow_g2(lx, ly, k)
        got = out.cpu().numpy()
        assert np.array_equal(got, ref, equal_nan=True), f"k = {k}: {got[0, :6].tolist()} for {ref[0, :6].tolist()}"
    assert np.isnan(ref[0, 0]) and ref[0, 5] == 0


def contrast_dev(st, lx, ly):
    import torch
    h, w = lx.shape
    rec = torch.full((2 + 300,), 5, dtype=torch.int32, device="cuda")          # the entry clears its record itself
    hmax, npoints, hist = C.c_float(), C.c_uint32(), np.zeros(300, np.uint32)
    a, b = dev(lx), dev(ly)
    st.call("wass_kaze_contrast_dev", a.data_ptr(), b.data_ptr(), h, w, rec.data_ptr(), C.byref(hmax), C.byref(npoints), hist.ctypes.data)
    return FE.contrast_factor(F(hmax.value), int(npoints.value), hist), F(hmax.value), int(npoints.value), hist


def test_contrast_entry_on_zero_one_and_edge_moduli(gpu_ctx):
    st = Stage(gpu_ctx)
    w, h = 129, 7
    z = np.zeros((h, w), F)
    one, ring = z.copy(), z.copy()
    one[3, 77] = 0.25
    ring[0, :], ring[-1, :], ring[:, 0], ring[:, -1] = 1, 2, 3, 4
    rng = np.random.default_rng(9)
    cases = [("zero", z, z), ("one modulus", one, z), ("one modulus of Ly", z, one), ("the border ring only", ring, ring),
             ("300 bin edges", KP.bin_edge_plane(h, w), z), ("300 bin edges, scaled", KP.bin_edge_plane(h, w) * F(0.3), z),
             ("random", KP.plane(w, h, 6), KP.plane(w, h, 7)), ("3 x 3", rng.standard_normal((3, 3)).astype(F), rng.standard_normal((3, 3)).astype(F))]
    for name, lx, ly in cases:
        k, hmax, n, hist = contrast_dev(st, lx, ly)
        rk, rhmax, rn, rhist = KO.contrast_of(lx, ly)
        assert (k, hmax, n) == (rk, rhmax, rn) and np.array_equal(hist, rhist), name
    k, hmax, n, hist = contrast_dev(st, z, z)
    assert (k, hmax, n, int(hist.sum())) == (F(0.03), 0, 0, 0)
    k, hmax, n, hist = contrast_dev(st, one, z)
    assert (hmax, n, int(hist[299]), int(hist.sum())) == (F(0.25), 1, 1, 1)


def test_convert_entry_with_a_pitch(gpu_ctx):
    import torch
    st = Stage(gpu_ctx)
    for w, h in KP.STAGE_SHAPES:
        img = np.random.default_rng(w + h).integers(0, 255, (h, w)).astype(np.uint8)
        pitch = w + 13
        base = torch.full((h, pitch), 255, dtype=torch.uint8, device="cuda")
        base[:, :w] = dev(img)
        dst = torch.zeros((h, w), dtype=torch.float32, device="cuda")
        st.call("wass_kaze_convert_dev", base.data_ptr(), pitch, h, w, float(F(1.0 / 255.0)), dst.data_ptr())
        assert np.array_equal(dst.cpu().numpy(), KO.convert(img)), f"{w} x {h}"


# ------------------------------------------------------------------------------------------------------------ small pictures
@pytest.mark.parametrize("shape", KP.SMALL_PICTURES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_smallest_pictures_every_stage(gpu_ctx, shape):
    w, h, no, ns = shape
    ref = KP.small_oracle(w, h, no, ns)
    pyr = FE.KazePyramid(KP.small_picture(w, h), FE.KazeOptions(1e-4, no, ns), gpu_ctx, keep=True)
    ss, rs, ex = FE.kaze_scale_space(pyr), FE.kaze_response(pyr), FE.kaze_extrema(pyr)
    assert ss["hmax"] == ref["ss"]["hmax"] and ss["npoints"] == ref["ss"]["npoints"] and np.array_equal(ss["hist"], ref["ss"]["hist"])
    assert ss["k"] == ref["ss"]["k"]
    for key in ("Lsmooth", "flow", "Lt"):
        assert np.array_equal(ss[key], ref["ss"][key]), key
    for key in ("Lx", "Ly", "Lxx", "Lxy", "Lyy", "Ldet"):
        assert np.array_equal(rs[key], ref["ss"][key]), key
    assert ex["status"] == 0 and np.array_equal(ex["candidates"], ref["candidates"]) and np.array_equal(ex["values"], ref["values"])
    assert np.array_equal(ex["kept"], ref["kept"]) and np.array_equal(ex["refined"], ref["refined"]) and np.array_equal(ex["size"], ref["size_all"])
    if (w, h) == (23, 130):
        kp = FE.kaze_detect(KP.small_picture(w, h), ctx=gpu_ctx)
        assert len(kp) == 3 and np.array_equal(kp.table()[:, :4], ref["kp"][:, :4]) and np.array_equal(kp.response, ref["response"])
        a32, fragile, adm = KO.orientation(ref["kp"], ref["ss"]["Lx"], ref["ss"]["Ly"], flags=True, admissible=True)
        tol = check_angles("23 x 130", kp.angle, a32, KO.orientation(ref["kp"], ref["ss"]["Lx"], ref["ss"]["Ly"], np.float64), fragile, adm)
        # the descriptor at the device's own angle: within the angle's tolerance of the oracle's where the keypoint is not fragile
        table = kp.table()
        d32, d64 = KO.descriptors(table, ref["ss"]["Lx"], ref["ss"]["Ly"]), KO.descriptors(table, ref["ss"]["Lx"], ref["ss"]["Ly"], np.float64)
        assert np.abs(kp.descriptors.astype(np.float64) - d32).max() <= desc_tol(d32, d64)
    else:
        assert len(ref["kp"]) == 0 and len(FE.kaze_detect(KP.small_picture(w, h), FE.KazeOptions(1e-4, no, ns), gpu_ctx)) == 0


def test_pictures_below_the_reach_are_refused(gpu_ctx):
    with pytest.raises(ValueError, match="image"):
        FE.kaze_detect(np.full((70, 5), 9, np.uint8), FE.KazeOptions(1e-4, 2, 2), gpu_ctx)          # 5 x 70
    with pytest.raises(ValueError, match="image"):
        FE.kaze_detect(np.full((5, 70), 9, np.uint8), FE.KazeOptions(1e-4, 2, 2), gpu_ctx)
    with pytest.raises(ValueError, match="image"):
        FE.kaze_detect(np.full((130, 22), 9, np.uint8), ctx=gpu_ctx)                                # 22 x 130


# -------------------------------------------------------------------------------------------------------- featureless pictures
def test_featureless_picture_gives_empty_keypoints_and_features(gpu_ctx):
    flat = np.full((63, 65), 97, np.uint8)
    for opts in (FE.KazeOptions(1e-4, 2, 2), None):
        kp = FE.kaze_detect(flat, opts, gpu_ctx)
        assert len(kp) == 0 and kp.status == 0 and kp.descriptors.shape == (0, 64) and kp.descriptors.dtype == np.float32
        assert kp.x.shape == kp.y.shape == kp.size.shape == kp.angle.shape == kp.response.shape == kp.level.shape == (0,)
        f = FE.detect_features(flat, options=opts, ctx=gpu_ctx)
        assert len(f) == 0 and f.xy.shape == (0, 2) and f.desc.shape == (0, 64) and f.scale.shape == f.angle.shape == (0,)


@pytest.mark.parametrize("flat", [(0,), (1,), (0, 1)], ids=["left", "right", "both"])
def test_match_workdir_of_a_featureless_pair_ends_like_the_reference(gpu_ctx, tmp_path, capsys, flat):
    from PIL import Image
    import kaze_pictures as P
    (tmp_path / "undistorted").mkdir()
    for cam in (0, 1):
        img = np.full((63, 65), 97, np.uint8) if cam in flat else P.picture("blobs65x63")
        Image.fromarray(img).save(tmp_path / "undistorted" / f"{cam:08d}.png")
    (tmp_path / "cfg.txt").write_text("FEATURE_N_OCTAVES=2\nFEATURE_N_LAYERS=2\n")
    assert FE.match_workdir(tmp_path, tmp_path / "cfg.txt", ctx=gpu_ctx) == -1
    io = capsys.readouterr()
    assert io.out.split() == ["[P|10|100]", "[P|20|100]"]
    assert len(io.err.strip().splitlines()) == 1 and "Traceback" not in io.err
    assert not (tmp_path / "matches_unfiltered.txt").exists()
