"""numpy restatement of DESIGN.md, "Spectral products": the conventions, the label maps, every sum in the fold order the kernels of
specprod.hip keep (reduce.h's block_sum and the thread-strided partials before it), the host formulas and the current fit.  Test
infrastructure only: nothing here is imported by the package.  Every + and * below is one fp64 rounding, as on the device.

`broken` names deliberate mistakes (tests/test_specprod.py shows that the probes of the GPU suite tell each from the
specification): f0_in_P, nyquist_in_P, kappa_plus, dir_edge, no_mod, corners, pairwise, sequential, fused, gt_threshold, lt_gate,
tie_high, gate_round0."""
import numpy as np

TWO_PI = 2.0 * np.pi
SUMS = ("Axx", "Axy", "Ayy", "bx", "by", "sw", "sr2")


def spacing(a):
    a = np.asarray(a, np.float64)
    return float((a[-1] - a[0]) / (len(a) - 1)) if len(a) > 1 else 1.0


def dft_axes(nt, ny, nx, du, dt):
    """(kx, ky, f): the bins of np.fft.fftn after fftshift, as angular wavenumbers and as frequencies"""
    def ax(n, d):
        return (np.arange(n) - n // 2) * (1.0 / (n * d))            # np.fft.fftfreq's rounding
    return TWO_PI * ax(nx, du), TWO_PI * ax(ny, du), ax(nt, dt)


def positive_half(f, broken=()):
    """f > df / 2, not f > 0: the reference builds f with np.arange, which may leave its zero bin at a rounding error above zero"""
    f = np.asarray(f, np.float64)
    half = 0.5 * spacing(f)
    if "f0_in_P" in broken:
        return np.flatnonzero(f > -half)
    if "nyquist_in_P" in broken:
        return np.flatnonzero(np.abs(f) > half)
    return np.flatnonzero(f > half)


def kappa(kx, ky, broken=()):
    s = 1.0 if "kappa_plus" in broken else -1.0
    return s * np.asarray(kx, np.float64), s * np.asarray(ky, np.float64)


def label_maps(kx, ky, ndir, dk=None, k_min=0.0, k_max=np.inf, broken=()):
    """(L_dir, L_k, nk, kmod, theta)"""
    kapx, kapy = kappa(kx, ky, broken)
    KX, KY = np.meshgrid(kapx, kapy)
    kmod = np.sqrt(KX * KX + KY * KY)
    theta = np.mod(np.arctan2(KY, KX), TWO_PI)
    used = (kmod != 0) & (kmod >= k_min) & (kmod <= k_max)
    dtheta = TWO_PI / ndir
    q = np.floor(theta / dtheta + (0.0 if "dir_edge" in broken else 0.5))
    if "no_mod" not in broken:
        q = np.mod(q, ndir)
    L_dir = np.where(used, q, -1).astype(np.int32)
    if dk is None:
        dk = max(spacing(kx), spacing(ky))
    L_k = np.floor(kmod / dk + 0.5)
    nk = int(np.floor(min(np.abs(kx).max(), np.abs(ky).max()) / dk)) + 1
    if "corners" in broken:
        nk = int(L_k.max()) + 1
    used = used & (L_k < nk)
    L_k = np.where(used, L_k, -1).astype(np.int32)
    return L_dir, L_k, nk, kmod, theta


# ---- the folds -----------------------------------------------------------------------------------------------------------------
def block_sum(x):
    """reduce.h: for o = 128, 64, .. 1: x[t] += x[t + o] for t < o; x is 256 x anything"""
    x = np.array(x, np.float64)
    o = 128
    while o:
        x[:o] += x[o:2 * o]
        o //= 2
    return x[0]


def strided_fold(vals, broken=()):
    """thread t adds elements t, t + 256, .. in that order from 0.0; then block_sum.  vals: n x anything"""
    vals = np.asarray(vals, np.float64)
    if "pairwise" in broken:
        return vals.sum(axis=0)
    if "sequential" in broken:
        acc = np.zeros(vals.shape[1:])
        for v in vals:
            acc = acc + v
        return acc
    part = np.zeros((256,) + vals.shape[1:])
    for s in range(0, len(vals), 256):
        chunk = vals[s:s + 256]
        part[:len(chunk)] += chunk
    return block_sum(part)


def label_sums(S, P, L, nlab, scale=1.0, broken=()):
    """T[p][b], p over P"""
    S = np.asarray(S, np.float64)
    flat = L.ravel()
    order = np.argsort(flat, kind="stable")              # raster order inside a label
    order = order[flat[order] >= 0]
    bounds = np.searchsorted(flat[order], np.arange(nlab + 1))
    v = S[P].reshape(len(P), -1) * scale
    T = np.zeros((len(P), nlab))
    for b in range(nlab):
        cells = order[bounds[b]:bounds[b + 1]]
        if len(cells):
            T[:, b] = strided_fold(v[:, cells].T, broken)
    return T


def e2_sum(S, P, scale=1.0):
    acc = np.zeros(S.shape[1:])
    for p in P:
        acc = acc + S[p] * scale
    return acc


def peak(S, plist, labels, scale=1.0, broken=()):
    """(value, flat index into the whole cube): the largest bin over the frequencies plist and the cells with a label >= 0"""
    S = np.asarray(S, np.float64)
    cells = S.shape[1] * S.shape[2]
    used = np.flatnonzero(labels.ravel() >= 0)
    if not len(plist) or not len(used):
        return float("nan"), -1
    v = S[plist].reshape(len(plist), -1)[:, used] * scale
    m = v.max()
    at = np.flatnonzero(v.ravel() == m)
    a = at[-1] if "tie_high" in broken else at[0]
    return float(m), int(plist[a // len(used)]) * cells + int(used[a % len(used)])


def check_positive_half(S, P, scale=1.0):
    v = np.asarray(S, np.float64)[P] * scale
    if not (np.isfinite(v) & (v >= 0)).all():
        raise ValueError("the positive half of the spectrum holds a bin that is negative or not finite")


# ---- the products --------------------------------------------------------------------------------------------------------------
def products(S, kx, ky, f, ndir=72, dk=None, k_min=0.0, k_max=np.inf, scale=1.0, broken=()):
    S, kx, ky, f = (np.asarray(a, np.float64) for a in (S, kx, ky, f))
    P = positive_half(f, broken)
    check_positive_half(S, P, scale)
    L_dir, L_k, nk, _, _ = label_maps(kx, ky, ndir, dk, k_min, k_max, broken)
    dkx, dky, df = spacing(kx), spacing(ky), spacing(f)
    dk = max(dkx, dky) if dk is None else dk
    dtheta = TWO_PI / ndir
    T_dir, T_k = label_sums(S, P, L_dir, ndir, scale, broken), label_sums(S, P, L_k, nk, scale, broken)
    E2 = e2_sum(S, P, scale)
    pv, pi = peak(S, P, L_dir, scale, broken)
    out = {"freq": f[P], "T_dir": T_dir, "T_k": T_k, "E2": E2, "peak_value": pv, "peak_index": pi, "L_dir": L_dir, "L_k": L_k, "nk": nk}
    out.update(derive(T_dir, T_k, E2, dkx, dky, df, dk, dtheta))
    return out


def derive(T_dir, T_k, E2, dkx, dky, df, dk, dtheta):
    """the host half: numpy fp64 from the tables"""
    nf, ndir = T_dir.shape
    D = 2.0 * T_dir * dkx * dky / dtheta
    srow = np.zeros(nf)
    for b in range(ndir):
        srow = srow + T_dir[:, b]
    S_f = 2.0 * dkx * dky * srow
    F_fk = 2.0 * T_k * dkx * dky / dk
    S_k = np.zeros(T_k.shape[1])
    for p in range(nf):
        S_k = S_k + F_fk[p] * df
    theta_b = np.arange(ndir) * dtheta
    c, s = np.cos(theta_b), np.sin(theta_b)
    sa, sb, sd = np.zeros(nf), np.zeros(nf), np.zeros(nf)
    for b in range(ndir):
        sa, sb, sd = sa + D[:, b] * c[b], sb + D[:, b] * s[b], sd + D[:, b]
    with np.errstate(invalid="ignore", divide="ignore"):
        a1, b1 = sa / sd, sb / sd
        mean_direction = np.arctan2(b1, a1)
        spread = np.sqrt(2.0 * (1.0 - np.hypot(a1, b1)))
    m0 = 0.0
    for p in range(nf):
        m0 = m0 + S_f[p] * df
    return {"D": D, "S_f": S_f, "F_fk": F_fk, "S_k": S_k, "E_k2": 2.0 * E2 * df, "mean_direction": mean_direction, "spread": spread,
            "m0": float(m0)}


# ---- the current fit -----------------------------------------------------------------------------------------------------------
def sigma0_map(kmod, depth=np.inf, g=9.81):
    return np.sqrt(g * kmod) if np.isinf(depth) else np.sqrt(g * kmod * np.tanh(kmod * depth))


def current_sums(S, pa, pb, labels, omega, kapx, kapy, sig0, U, V, thr, gate, scale=1.0, broken=()):
    """(dict of the seven sums, n): per cell over p ascending; block_sum over groups of 256 cells in raster order; strided_fold"""
    S = np.asarray(S, np.float64)
    ny, nx = S.shape[1:]
    used = labels >= 0
    KX, KY = np.meshgrid(np.asarray(kapx, np.float64), np.asarray(kapy, np.float64))
    uv = KX * U + KY * V
    acc = np.zeros((7, ny, nx))
    n = 0
    for p in range(pa, pb):
        w = S[p] * scale
        if not (np.isfinite(w[used]) & (w[used] >= 0)).all():
            raise ValueError("a bin of the fit is negative or not finite")
        d = omega[p] - sig0
        r = d - uv
        take = used & ((w > thr) if "gt_threshold" in broken else (w >= thr)) & ((np.abs(r) < gate) if "lt_gate" in broken else (np.abs(r) <= gate))
        wkx, wky = w * KX, w * KY
        if "fused" in broken:
            terms = (w * (KX * KX), w * (KX * KY), w * (KY * KY), w * (KX * d), w * (KY * d), w, w * (r * r))
        else:
            terms = (wkx * KX, wkx * KY, wky * KY, wkx * d, wky * d, w, (w * r) * r)
        for q, t in enumerate(terms):
            acc[q] = np.where(take, acc[q] + t, acc[q])
        n += int(take.sum())
    cells = ny * nx
    groups = -(-cells // 256)
    flat = np.zeros((7, groups * 256))
    flat[:, :cells] = acc.reshape(7, cells)
    part = block_sum(flat.reshape(7, groups, 256).transpose(2, 0, 1))        # 7 x groups
    tot = strided_fold(part.T, broken)
    return dict(zip(SUMS, (float(v) for v in tot))), n


def solve(s, n):
    """Cramer's rule: (U, V, singular)"""
    det = s["Axx"] * s["Ayy"] - s["Axy"] * s["Axy"]
    if n < 2 or not det > 0:
        return float("nan"), float("nan"), True
    return (s["bx"] * s["Ayy"] - s["by"] * s["Axy"]) / det, (s["Axx"] * s["by"] - s["Axy"] * s["bx"]) / det, False


def dispersion_current(S, kx, ky, f, depth=np.inf, g=9.81, threshold=0.1, f_min=0.0, f_max=np.inf, k_min=0.0, k_max=np.inf, iterations=3,
                       gate=2.0, scale=1.0, broken=()):
    S, kx, ky, f = (np.asarray(a, np.float64) for a in (S, kx, ky, f))
    P = positive_half(f, broken)
    check_positive_half(S, P, scale)
    labels, _, _, kmod, _ = label_maps(kx, ky, 1, None, k_min, k_max, broken)
    kapx, kapy = kappa(kx, ky, broken)
    sig0 = sigma0_map(kmod, depth, g)
    omega = TWO_PI * f
    domega = TWO_PI * spacing(f)
    Pu = P[(f[P] >= f_min) & (f[P] <= f_max)]
    pa, pb = (int(Pu[0]), int(Pu[-1]) + 1) if len(Pu) else (int(P[0]), int(P[0]))
    smax, _ = peak(S, np.arange(pa, pb), labels, scale)
    thr = threshold * smax
    U = V = 0.0
    trace, singular = [], np.isnan(smax)
    sums, n = dict.fromkeys(SUMS, 0.0), 0
    for m in range(iterations + 1):
        if singular:
            break
        gv = gate * domega if (m > 0 or "gate_round0" in broken) else np.inf
        sums, n = current_sums(S, pa, pb, labels, omega, kapx, kapy, sig0, U, V, thr, gv, scale, broken)
        U, V, singular = solve(sums, n)
        trace.append({"round": m, "U": U, "V": V, "n_bins": n, "singular": singular, **sums})
    if singular:
        U = V = float("nan")
    with np.errstate(invalid="ignore", divide="ignore"):
        rms = float(np.sqrt(np.float64(sums["sr2"]) / np.float64(sums["sw"])))
    return {"U": U, "V": V, "speed": float(np.hypot(U, V)), "direction": float(np.mod(np.arctan2(V, U), TWO_PI)), "n_bins": n, "rms": rms,
            "singular": bool(singular), "trace": trace, "threshold_value": thr, "labels": labels, "sigma0": sig0, "pa": pa, "pb": pb}
