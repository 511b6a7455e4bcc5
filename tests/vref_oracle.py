"""numpy restatement of wass_amd/csrc/vref.hip (variational refinement of the gridded surface), parametrised by dtype:
float32 repeats the kernels' operations one by one, in their order (bits); float64 is the same model for calculus.
Holds the forward model, the hand-derived gradient, the Adam loop, the probe scenes and their condition checkers.
A Scene's `mistake` switches in one of the errors the probes are there to catch (tests only)."""
import dataclasses

import numpy as np

B1, B2 = 0.9, 0.999
MISTAKES = ("convolution", "transposed", "corner_aligned", "no_mask", "eps_in_sqrt", "xy_swapped")


def derivative_of_gaussian_win(N, sigma):
    """the reference's expression (TFVariationalRefinement.py:9-15) with scipy's window written out: fp64"""
    assert N % 2 == 1
    n = np.arange(N, dtype=np.float64) - (N - 1) / 2.0
    g = np.exp(-n ** 2 / (2 * sigma * sigma))[None]
    x = g.T @ g
    return np.gradient(x, axis=1), np.gradient(x, axis=0)


@dataclasses.dataclass
class Scene:
    I0: np.ndarray
    I1: np.ndarray
    Xb: np.ndarray
    Yb: np.ndarray
    mask: np.ndarray
    R: np.ndarray
    T: np.ndarray
    P: tuple
    kx: np.ndarray
    ky: np.ndarray
    dt: type
    mistake: str = ""

    @property
    def shape(self):
        return self.Xb.shape

    @property
    def coarse(self):
        ny, nx = self.shape
        return (nx // 2, ny // 2) if self.mistake == "transposed" else (ny // 2, nx // 2)


def scene(I0, I1, Rp2c, Tp2c, P0cam, P1cam, XX, YY, baseline, mask, dt=np.float32, mistake=""):
    """the constructor's casts: fp64 quotients and matrices, then one cast to dt"""
    kx, ky = derivative_of_gaussian_win(7, 0.8)
    f = lambda a: np.ascontiguousarray(np.asarray(a, np.float64).astype(dt))  # noqa: E731
    return Scene(f(I0), f(I1), f(np.asarray(XX, np.float64) / baseline), f(np.asarray(YY, np.float64) / baseline), f(mask),
                 f(Rp2c).reshape(3, 3), f(Tp2c).reshape(3), (f(P0cam).reshape(3, 4), f(P1cam).reshape(3, 4)), f(kx), f(ky), dt, mistake)


def as_dtype(S, dt):
    d = {k: (v.astype(dt) if isinstance(v, np.ndarray) else v) for k, v in dataclasses.asdict(S).items()}
    d["P"] = tuple(np.asarray(p).astype(dt) for p in S.P)
    d["dt"] = dt
    return Scene(**d)


# ---------------------------------------------------------------------------------------------------------------- forward model
def project(S, Z):
    """u, v, s2 per camera and the node's `ok` (not degenerate)"""
    X, Y, R, T = S.Xb, S.Yb, S.R, S.T
    with np.errstate(all="ignore"):
        c = [((R[r, 0] * X + R[r, 1] * Y) + R[r, 2] * Z) + T[r] for r in range(3)]
        out, ok = [], np.ones(S.shape, bool)
        for P in S.P:
            s = [((P[r, 0] * c[0] + P[r, 1] * c[1]) + P[r, 2] * c[2]) + P[r, 3] for r in range(3)]
            u, v = s[0] / s[2], s[1] / s[2]
            ok &= (s[2] > 0) & np.isfinite(u) & np.isfinite(v)
            out.append((u, v, s[2]))
    return out, ok


def bilinear(I, u, v, dt):
    """tfa's sampler and the derivative of its value with respect to (u, v); u, v finite"""
    H, W = I.shape
    zero, one = dt(0), dt(1)
    fx = np.minimum(np.maximum(zero, np.floor(u)), dt(W - 2))
    fy = np.minimum(np.maximum(zero, np.floor(v)), dt(H - 2))
    rx, ry = u - fx, v - fy
    ax, ay = np.minimum(np.maximum(zero, rx), one), np.minimum(np.maximum(zero, ry), one)
    ix, iy = fx.astype(np.int64), fy.astype(np.int64)
    tl, tr, bl, br = I[iy, ix], I[iy, ix + 1], I[iy + 1, ix], I[iy + 1, ix + 1]
    dtop, dbot = tr - tl, br - bl
    top, bot = ax * dtop + tl, ax * dbot + bl
    val = ay * (bot - top) + top
    gx = np.where((rx >= 0) & (rx <= 1), ay * (dbot - dtop) + dtop, zero)
    gy = np.where((ry >= 0) & (ry <= 1), bot - top, zero)
    return val, gx, gy


def q_vectors(S):
    R = S.R
    return [[(P[r, 0] * R[0, 2] + P[r, 1] * R[1, 2]) + P[r, 2] * R[2, 2] for r in range(3)] for P in S.P]


def sample(S, Z, grad=False):
    """I0s, I1s, (u0, v0, u1, v1) and, with grad, d and gd / cD = d * (dI0 - dI1)"""
    dt = S.dt
    Z = np.asarray(Z, dt)
    cams, ok = project(S, Z)
    mask = np.ones_like(S.mask) if S.mistake == "no_mask" else S.mask
    vals, dI = [], []
    q = q_vectors(S)
    for k, ((u, v, s2), I) in enumerate(zip(cams, (S.I0, S.I1))):
        us, vs, s2s = np.where(ok, u, dt(0)), np.where(ok, v, dt(0)), np.where(ok, s2, dt(1))
        if S.mistake == "xy_swapped":
            val, gy, gx = bilinear(I, vs, us, dt)
        else:
            val, gx, gy = bilinear(I, us, vs, dt)
        vals.append(np.where(ok, val * mask, dt(0)))
        du, dv = (q[k][0] - us * q[k][2]) / s2s, (q[k][1] - vs * q[k][2]) / s2s
        dI.append((gx * du + gy * dv) * mask)
    uv = (cams[0][0], cams[0][1], cams[1][0], cams[1][1])
    if not grad:
        return vals[0], vals[1], uv
    d = (vals[0] - vals[1]) / dt(255)
    return vals[0], vals[1], uv, d, np.where(ok, d * (dI[0] - dI[1]), dt(0))


def correlate(S, A, K):
    """zero-padded cross-correlation, the taps in row-major order"""
    if S.mistake == "convolution":
        K = K[::-1, ::-1]
    ny, nx = A.shape
    pad = np.zeros((ny + 6, nx + 6), S.dt)
    pad[3:3 + ny, 3:3 + nx] = A
    acc = np.zeros((ny, nx), S.dt)
    for a in range(7):
        for b in range(7):
            acc = acc + K[a, b] * pad[a:a + ny, b:b + nx]
    return acc


def zgrad(S, Z):
    Z = np.asarray(Z, S.dt)
    return correlate(S, Z, S.kx), correlate(S, Z, S.ky)


def loss(S, Z):
    """(data, smoothness): the terms in dt, the sums fp64"""
    _, _, _, d, _ = sample(S, Z, grad=True)
    zdx, zdy = zgrad(S, Z)
    n = float(d.size)
    return float((d * d).astype(np.float64).sum()) / n, float((zdx * zdx + zdy * zdy).astype(np.float64).sum()) / n


def axis_tables(n_in, n_out, dt, corner_aligned=False):
    """tf.image.resize's rule per axis: lo, hi, t per output index"""
    d = np.arange(n_out).astype(dt)
    if corner_aligned:
        src = d * (dt(n_in - 1) / dt(max(n_out - 1, 1)))
    else:
        src = (d + dt(0.5)) * (dt(n_in) / dt(n_out)) - dt(0.5)
    fl = np.floor(src)
    lo = np.minimum(np.maximum(fl.astype(np.int64), 0), n_in - 1)
    hi = np.maximum(np.minimum(np.ceil(src).astype(np.int64), n_in - 1), lo)
    return lo, hi, (src - fl).astype(dt)


def _tables(S):
    hc, wc = S.coarse
    ny, nx = S.shape
    ca = S.mistake == "corner_aligned"
    return axis_tables(hc, ny, S.dt, ca), axis_tables(wc, nx, S.dt, ca)


def resize(S, Zc):
    Zc = np.asarray(Zc, S.dt)
    (yl, yh, ty), (xl, xh, tx) = _tables(S)
    tl, tr, bl, br = Zc[np.ix_(yl, xl)], Zc[np.ix_(yl, xh)], Zc[np.ix_(yh, xl)], Zc[np.ix_(yh, xh)]
    top, bot = tl + (tr - tl) * tx[None, :], bl + (br - bl) * tx[None, :]
    return top + (bot - top) * ty[:, None]


def _gather(lo, hi, t, n_in, dt):
    """per coarse index the fine indices that read it (ascending) and their weights, padded with weight 0"""
    n_out = len(lo)
    rows = [[d for d in range(n_out) if lo[d] == c or hi[d] == c] for c in range(n_in)]
    K = max(1, max(len(r) for r in rows))
    idx, w = np.zeros((n_in, K), np.int64), np.zeros((n_in, K), dt)
    for c, r in enumerate(rows):
        assert r == list(range(r[0], r[-1] + 1)) if r else True
        for k, d in enumerate(r):
            idx[c, k] = d
            w[c, k] = (dt(1) - t[d] if lo[d] == c else dt(0)) + (t[d] if hi[d] == c else dt(0))
    return idx, w


def resize_adjoint(S, gZ):
    hc, wc = S.coarse
    (yl, yh, ty), (xl, xh, tx) = _tables(S)
    yi, wy = _gather(yl, yh, ty, hc, S.dt)
    xi, wx = _gather(xl, xh, tx, wc, S.dt)
    row = np.zeros((gZ.shape[0], wc), S.dt)
    for k in range(xi.shape[1]):
        row = row + wx[None, :, k] * gZ[:, xi[:, k]]
    g = np.zeros((hc, wc), S.dt)
    for k in range(yi.shape[1]):
        g = g + wy[:, k, None] * row[yi[:, k], :]
    return g


def gradient(S, Zc, alpha):
    """(gC, gZ): the gradient of data + alpha * smoothness with respect to Zc and to Z = resize(Zc)"""
    dt = S.dt
    Z = resize(S, Zc)
    n = float(Z.size)
    _, _, _, _, gd = sample(S, Z, grad=True)
    gd = gd * dt(2.0 / (255.0 * n))
    zdx, zdy = zgrad(S, Z)
    flip = (lambda K: K) if S.mistake == "convolution" else (lambda K: K[::-1, ::-1])
    gs = (correlate(S, zdx, flip(S.kx)) + correlate(S, zdy, flip(S.ky))) * dt(2.0 * float(alpha) / n)
    gZ = gd + gs
    return resize_adjoint(S, gZ), gZ


def energy(S, Zc, alpha):
    d, s = loss(S, resize(S, Zc))
    return d + float(alpha) * s


def lr_t(lr, t):
    return lr * np.sqrt(1.0 - B2 ** float(t)) / (1.0 - B1 ** float(t))


def adam_step(S, Zc, m, v, g, t, lr=1e-3, eps=1e-7):
    dt = S.dt
    m = m + (g - m) * dt(1.0 - B1)
    v = v + (g * g - v) * dt(1.0 - B2)
    if S.mistake == "eps_in_sqrt":
        return Zc - (m * dt(lr_t(lr, t))) / np.sqrt(v + dt(eps)), m, v
    return Zc - (m * dt(lr_t(lr, t))) / (np.sqrt(v) + dt(eps)), m, v


def optimize(S, Zc, iters, alpha=10.0, lr=1e-3, eps=1e-7, m=None, v=None, step=0):
    """the loop: (Zc, m, v, step) after `iters` more steps"""
    Zc = np.array(Zc, S.dt)
    m = np.zeros_like(Zc) if m is None else np.array(m, S.dt)
    v = np.zeros_like(Zc) if v is None else np.array(v, S.dt)
    for it in range(iters):
        g, _ = gradient(S, Zc, alpha)
        Zc, m, v = adam_step(S, Zc, m, v, g, step + it + 1, lr, eps)
    return Zc, m, v, step + iters


def cv_resize_linear(A, hc, wc):
    """cv.resize(A, (wc, hc), INTER_LINEAR) restated in float32: fx = (float)((d + 0.5) * (in / out) - 0.5) from fp64, s = floor,
    f = fx - s; s < 0: s = 0, f = 0; s >= in - 1: s = in - 1, f = 0; rows of S[s] * (1 - f) + S[s + 1] * f, then the same down."""
    A = np.asarray(A, np.float32)

    def axis(n_in, n_out):
        fx = ((np.arange(n_out) + 0.5) * (n_in / n_out) - 0.5).astype(np.float32)
        s = np.floor(fx).astype(np.int64)
        f = fx - s.astype(np.float32)
        f[s < 0] = 0; s[s < 0] = 0
        f[s >= n_in - 1] = 0; s[s >= n_in - 1] = n_in - 1
        return s, np.minimum(s + 1, n_in - 1), f.astype(np.float32)
    ys, ys1, fy = axis(A.shape[0], hc)
    xs, xs1, fx = axis(A.shape[1], wc)
    rows = A[:, xs] * (np.float32(1) - fx)[None] + A[:, xs1] * fx[None]
    return rows[ys] * (np.float32(1) - fy)[:, None] + rows[ys1] * fy[:, None]


# ---------------------------------------------------------------------------------------------------------------- probe scenes
def texture(h, w, seed, waves=4):
    """a smooth picture in [0, 255]: a few sinusoids, float64"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    t = np.zeros((h, w))
    for _ in range(waves):
        fx, fy = rng.uniform(-0.9, 0.9, 2)
        t += rng.uniform(0.3, 1.0) * np.sin(fx * x + fy * y + rng.uniform(0, 6.28))
    return 127.5 + 120.0 * t / np.abs(t).max()


def mask_of(name, ny, nx):
    if name == "ones":
        return np.ones((ny, nx))
    if name == "zeros":
        return np.zeros((ny, nx))
    return (np.add.outer(np.arange(ny), np.arange(nx)) % 2 == 0).astype(np.float64)


def probe(ny, nx, ih, iw, seed=0, spread=0.7, mask="ones", dt=np.float32, mistake="", uint8=False):
    """A rig looking down the z axis at the grid [-1, 1]^2 from distance 4: the nodes project over the middle `spread` of each
    picture (spread > 1: queries leave the picture on every side).  Heights are expected within +-0.3."""
    rng = np.random.default_rng(1000 + seed)
    XX, YY = np.meshgrid(np.linspace(-1, 1, nx) * 2.0, np.linspace(-1, 1, ny) * 2.0)
    baseline = 2.0
    a = rng.uniform(-0.05, 0.05, 3)
    Rx = np.array([[1, 0, 0], [0, np.cos(a[0]), -np.sin(a[0])], [0, np.sin(a[0]), np.cos(a[0])]])
    Rz = np.array([[np.cos(a[2]), -np.sin(a[2]), 0], [np.sin(a[2]), np.cos(a[2]), 0], [0, 0, 1]])
    R = Rz @ Rx
    T = np.array([0.013, -0.021, 4.0])
    fx, fy = spread * (iw - 1) / 2.0 * 4.0, spread * (ih - 1) / 2.0 * 4.0
    K = np.array([[fx, 0, (iw - 1) / 2.0 + 0.137], [0, fy, (ih - 1) / 2.0 - 0.171], [0, 0, 1.0]])
    P0 = K @ np.hstack([np.eye(3), np.zeros((3, 1))])
    P1 = K @ np.hstack([np.eye(3), np.array([[-0.12], [0.02], [0.01]])])
    I0, I1 = texture(ih, iw, seed), texture(ih, iw, seed + 77)
    if uint8:
        I0, I1 = np.round(I0).astype(np.uint8), np.round(I1).astype(np.uint8)
    return scene(I0, I1, R, T, P0, P1, XX, YY, baseline, mask_of(mask, ny, nx), dt, mistake), dict(
        I0=I0, I1=I1, Rp2c=R, Tp2c=T, P0cam=P0, P1cam=P1, XX=XX, YY=YY, baseline=baseline, mask=mask_of(mask, ny, nx))


def surface(ny, nx, seed, amp=0.2):
    rng = np.random.default_rng(2000 + seed)
    y, x = np.mgrid[0:ny, 0:nx].astype(np.float64)
    return amp * (np.sin(0.7 * x + rng.uniform(0, 6)) * np.cos(0.5 * y + rng.uniform(0, 6))) + rng.uniform(-0.05, 0.05)


# ---- condition checkers: what a probe must satisfy for its comparison to mean something
def distance_to_ties(S, Z):
    """the smallest distance of a query, in either picture and axis, to an integer pixel (which includes both clamps)"""
    cams, ok = project(S, np.asarray(Z, S.dt))
    best = np.inf
    for (u, v, _), I in zip(cams, (S.I0, S.I1)):
        for q, size in ((u, I.shape[1]), (v, I.shape[0])):
            q = q[ok].astype(np.float64)
            inside = (q > 0) & (q < size - 1)
            if inside.any():
                best = min(best, float(np.abs(q[inside] - np.round(q[inside])).min()))
            if (~inside).any():
                best = min(best, float(np.minimum(np.abs(q[~inside]), np.abs(q[~inside] - (size - 1))).min()))
    return best


def all_inside(S, Z):
    cams, ok = project(S, np.asarray(Z, S.dt))
    return bool(ok.all()) and all(((u > 0) & (u < I.shape[1] - 1) & (v > 0) & (v < I.shape[0] - 1)).all()
                                  for (u, v, _), I in zip(cams, (S.I0, S.I1)))


def min_depth(S, Z):
    cams, _ = project(S, np.asarray(Z, S.dt))
    return float(min(np.abs(c[2]).min() for c in cams))


# ---------------------------------------------------------------------------------------------------------------- end to end
def plane_texture(X, Y, waves):
    """an analytic, smooth texture on the plane (plane units): 127.5 + 100 * the mean of sin(kx X + ky Y + phase) over `waves`"""
    t = sum(np.sin(kx * X + ky * Y + ph) for kx, ky, ph in waves) / len(waves)
    return 127.5 + 100.0 * t


def render_plane(Rp2c, Tp2c, Pcam, ih, iw, c0, waves):
    """the picture camera Pcam (3 x 4, from the camera-0 frame) sees of the textured plane z = c0 of the plane frame, by ray-plane
    intersection per pixel centre: s = Pcam [c; 1] is proportional to (u, v, 1), c = Rp2c p + Tp2c"""
    Rp2c, Tp2c, Pcam = np.asarray(Rp2c, np.float64), np.asarray(Tp2c, np.float64).reshape(3), np.asarray(Pcam, np.float64)
    Minv = np.linalg.inv(Pcam[:, :3])
    v, u = np.mgrid[0:ih, 0:iw].astype(np.float64)
    pix = np.stack([u, v, np.ones_like(u)]).reshape(3, -1)
    a = Rp2c.T @ (Minv @ pix)
    b = -Rp2c.T @ (Minv @ Pcam[:, 3] + Tp2c)
    lam = (c0 - b[2]) / a[2]
    p = a * lam + b[:, None]
    return plane_texture(p[0], p[1], waves).reshape(ih, iw)


# Zero padding lets the smoothness term see a constant offset along the border (at the true plane below, smoothness = 4.1e-3 against
# a data loss of 2.1e-5 at the start value): with the reference's alpha = 10 the energy at the truth is HIGHER than at 0.  The
# end-to-end scene therefore runs with a small alpha, so that only a correct data gradient brings the surface to the plane, and
# measures the error inside the mask, which leaves out a margin of three nodes.
E2E = dict(N=24, c0=0.1, iters=120, alpha=1e-4, margin=3, waves=((6.0, 1.2, 0.3), (-1.8, 5.4, 1.1), (3.6, 4.2, 2.0)),
           area=dict(area_center=np.array([-4.0, -30.0]), area_size_x=16.0, area_size_y=16.0))


def e2e_mask(shape):
    m, k = np.zeros(shape, np.float32), E2E["margin"]
    m[k:shape[0] - k, k:shape[1] - k] = 1
    return m


def e2e_scene(gridsetup, ih, iw, dt=np.float32):
    """(Scene, constructor arguments) of the end-to-end test on a set-up dict (Rpl, Tpl, P0cam, P1cam, XX, YY, CAM_BASELINE): the true
    surface is the plane z = E2E['c0'] in plane units, the start value 0"""
    Rp2c = np.asarray(gridsetup["Rpl"], np.float64).T
    Tp2c = (-Rp2c @ np.asarray(gridsetup["Tpl"], np.float64).reshape(3, 1)).reshape(3)
    I0 = render_plane(Rp2c, Tp2c, gridsetup["P0cam"], ih, iw, E2E["c0"], E2E["waves"])
    I1 = render_plane(Rp2c, Tp2c, gridsetup["P1cam"], ih, iw, E2E["c0"], E2E["waves"])
    args = dict(I0=I0.astype(np.float32), I1=I1.astype(np.float32), Rp2c=Rp2c, Tp2c=Tp2c, P0cam=gridsetup["P0cam"], P1cam=gridsetup["P1cam"],
                XX=gridsetup["XX"], YY=gridsetup["YY"], baseline=float(gridsetup["CAM_BASELINE"]), mask=e2e_mask(np.asarray(gridsetup["XX"]).shape))
    return scene(dt=dt, **args), args


def masked_rms(Z, truth, mask):
    e = (np.asarray(Z, np.float64) - truth)[np.asarray(mask) != 0]
    return float(np.sqrt((e * e).mean()))
