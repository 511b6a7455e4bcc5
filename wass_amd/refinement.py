"""Variational refinement of the gridded surface on the GPU: the reference's TFVariationalRefinement
(gridding/wassgridsurface/TFVariationalRefinement.py) without TensorFlow.

    from wass_amd.refinement import VariationalRefinement      # instead of: from TFVariationalRefinement import TFVariationalRefinement

VariationalRefinement(I0, I1, Rp2c, Tp2c, P0cam, P1cam, XX, YY, baseline, mask) takes the reference's constructor arguments and has
its methods: sample_images(Z), compute_Z_gradient(Z), compute_loss(Z), optimize(Zinit, max_iters, alpha).  Every grid node is
projected into both cameras, the two pictures are sampled there, and a half-resolution height field is moved by Adam so that the
samples agree, under a derivative-of-Gaussian smoothness term.  The gradient TensorFlow derived is written out by hand in
csrc/vref.hip (energy_gradient returns it); the whole loop runs on the context's stream without a host round trip.

Differences: the coarse field is (Ny // 2) x (Nx // 2) (the reference transposes the size of a
non-square grid); a Zinit that is not finite is refused; a node behind a camera adds nothing to the data term; Adam,
tf.image.resize and tfa's sampler are restated from their published definitions, not pinned against TensorFlow.

refine_surface(Zi, mask, I0, I1, gridsetup) is what the commented block of the reference's grid() amounts to
(wassgridsurface.py:382-435).  Pictures may be uint8 or float32; every array may be a host array or a device tensor, and a
result comes back on the side its Z came from.

refine_sequence(Zi, I0, I1, gridsetup) is refine_surface for the n frames of a sequence, several frames per kernel launch: the
library's kernels take their frame from blockIdx.z, the set-up the frames share is copied once, and the -Zi / baseline, the
down-sampling and the -Z * baseline run on the device.  Frame i of its result equals refine_surface of frame i bit for bit.
SequenceRefiner is the handle behind it (device tensors in and out), RefineOptions what grid_sequence(refine=...) takes.
"""
from __future__ import annotations

import ctypes as C
import dataclasses

import numpy as np

from .stereo import Context, _Handle, _is_device

ADAM_BETA_1, ADAM_BETA_2 = 0.9, 0.999       # Keras's defaults, compiled into the library


def derivative_of_gaussian_win(N: int, sigma: float = 1.0):
    """The reference's derivative_of_Gaussian_win: np.gradient along x and y of the outer product of
    scipy.signal.windows.gaussian(N, sigma) with itself (exp(-n^2 / (2 sigma^2)), n = 0 .. N-1 about (N-1) / 2), fp64."""
    N = int(N)
    if N < 3 or N % 2 != 1:
        raise ValueError(f"N = {N}: an odd size of at least 3")
    if not sigma > 0:
        raise ValueError("sigma must be positive")
    n = np.arange(N, dtype=np.float64) - (N - 1) / 2.0
    x = np.exp(-n ** 2 / (2 * float(sigma) * float(sigma)))[np.newaxis]
    x = x.T @ x
    return np.gradient(x, axis=1), np.gradient(x, axis=0)


def downsample_linear(Z, hc: int, wc: int) -> np.ndarray:
    """cv.resize(Z, (wc, hc), interpolation=cv.INTER_LINEAR) for a float32 picture, restated in float32 on the host: per axis
    f = (float)((d + 0.5) * (in / out) - 0.5) from fp64, s = floor(f), f -= s; s < 0: s = 0, f = 0; s >= in - 1: s = in - 1, f = 0;
    a row is S[s] * (1 - f) + S[s + 1] * f, and the rows are combined by the same rule."""
    Z = np.asarray(Z, np.float32)
    one = np.float32(1)

    def axis(n_in, n_out):
        f = ((np.arange(n_out) + 0.5) * (n_in / n_out) - 0.5).astype(np.float32)
        s = np.floor(f).astype(np.int64)
        f = f - s.astype(np.float32)
        low, high = s < 0, s >= n_in - 1
        f[low | high] = 0
        s[low] = 0
        s[high] = n_in - 1
        return s, np.minimum(s + 1, n_in - 1), f

    ys, ys1, fy = axis(Z.shape[0], hc)
    xs, xs1, fx = axis(Z.shape[1], wc)
    rows = Z[:, xs] * (one - fx)[np.newaxis] + Z[:, xs1] * fx[np.newaxis]
    return np.ascontiguousarray(rows[ys] * (one - fy)[:, np.newaxis] + rows[ys1] * fy[:, np.newaxis])


# ---- what VariationalRefinement and SequenceRefiner share: tensors on the context's device `dev`, and the set-up both copy there
def _to_dev(a, dtype, dev):
    import torch
    if _is_device(a):
        if a.device != dev:
            raise ValueError(f"a tensor on {a.device}, the context is on {dev}")
        return a.to(dtype).contiguous()
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a))).to(dev).to(dtype).contiguous()


def _new(dev, *shape):
    import torch
    t = torch.empty(shape, dtype=torch.float32, device=dev)
    torch.cuda.synchronize(dev)
    return t


def _matrices(mats, names, flat: bool):
    """Rp2c, Tp2c, P0cam, P1cam as flat fp64 arrays.  A refusal calls them by `names` and gives their size as one number (flat) or
    as rows x columns."""
    out = []
    for name, m, shp in zip(names, mats, ((3, 3), (3,), (3, 4), (3, 4))):
        a = np.ascontiguousarray(np.asarray(m, np.float64))
        size = int(np.prod(shp))
        if a.size != size or not np.isfinite(a).all():
            raise ValueError(f"{name}: {size if flat else ' x '.join(map(str, shp))} finite values expected")
        out.append(a.reshape(-1))
    return out


def _kernels() -> np.ndarray:
    """the two 7 x 7 derivative-of-Gaussian kernels of the smoothness term, float32 [2, 7, 7]"""
    dsx, dsy = derivative_of_gaussian_win(7, sigma=0.8)
    return np.ascontiguousarray(np.stack([dsx, dsy]).astype(np.float32))


def _scaled_grid(XX, YY, baseline, dev):
    """XX / baseline, YY / baseline on the device with the reference's casts: fp64 quotients, then float32"""
    import torch
    return tuple((_to_dev(a, torch.float64, dev) / baseline).to(torch.float32).contiguous() for a in (XX, YY))


@dataclasses.dataclass
class AdamState:
    """The optimiser's state after `step` steps; m, v: (Ny // 2) x (Nx // 2) float32, on the side Zc came from."""
    m: object
    v: object
    step: int = 0


class VariationalRefinement(_Handle):
    def __init__(self, I0, I1, Rp2c, Tp2c, P0cam, P1cam, XX, YY, baseline, mask, ctx: Context | None = None):
        shape = tuple(int(v) for v in XX.shape)
        if len(shape) != 2 or tuple(YY.shape) != shape or tuple(mask.shape) != shape:
            raise ValueError(f"XX, YY and mask must be one Ny x Nx shape, got {tuple(XX.shape)}, {tuple(YY.shape)}, {tuple(mask.shape)}")
        if min(shape) < 2:
            raise ValueError(f"a grid of {shape[0]} x {shape[1]}: at least 2 x 2 nodes")
        for name, I in (("I0", I0), ("I1", I1)):
            if len(I.shape) != 2 or min(int(v) for v in I.shape) < 2:
                raise ValueError(f"{name} of shape {tuple(I.shape)}: a picture of at least 2 x 2 pixels")
        baseline = float(baseline)
        if not np.isfinite(baseline) or baseline == 0:
            raise ValueError("baseline must be finite and not 0")
        mats = _matrices((Rp2c, Tp2c, P0cam, P1cam), ("Rp2c", "Tp2c", "P0cam", "P1cam"), flat=False)
        self.shape = shape
        self.coarse_shape = (shape[0] // 2, shape[1] // 2)
        self.losses = np.zeros((0, 4))
        self.state = None                                        # the AdamState the last optimize() ended with
        self._ctx = ctx if ctx is not None else Context(0)
        import torch
        self._dev = torch.device("cuda", self._ctx.device_id)
        planes = [*_scaled_grid(XX, YY, baseline, self._dev), _to_dev(mask, torch.float32, self._dev),
                  _to_dev(I0, torch.float32, self._dev), _to_dev(I1, torch.float32, self._dev)]
        kernels = _kernels()
        torch.cuda.synchronize(self._dev)
        h = C.c_void_p()
        dp = C.POINTER(C.c_double)
        (ih0, iw0), (ih1, iw1) = planes[3].shape, planes[4].shape
        self._ctx._check(self._ctx._lib.wass_vref_create(
            self._ctx._h, shape[0], shape[1], planes[0].data_ptr(), planes[1].data_ptr(), planes[2].data_ptr(),
            mats[0].ctypes.data_as(dp), mats[1].ctypes.data_as(dp), mats[2].ctypes.data_as(dp), mats[3].ctypes.data_as(dp),
            planes[3].data_ptr(), int(ih0), int(iw0), planes[4].data_ptr(), int(ih1), int(iw1), kernels.ctypes.data, C.byref(h)))
        self._h = h                                              # the library has copied everything it keeps

    def _destroy(self, h):
        self._ctx._lib.wass_vref_destroy(h)

    # ---- plumbing
    def _plane(self, Z, shape, name):
        """Z as a contiguous float32 device tensor of `shape`, finite; and whether the caller's was a device tensor"""
        import torch
        if tuple(int(v) for v in Z.shape) != tuple(shape):
            raise ValueError(f"{name} of shape {tuple(Z.shape)}, expected {tuple(shape)}")
        dev = _is_device(Z)
        if not dev and not np.isfinite(np.asarray(Z)).all():
            raise ValueError(f"{name} holds a value that is not finite")
        d = _to_dev(Z, torch.float32, self._dev)
        if dev and not bool(torch.isfinite(d).all()):
            raise ValueError(f"{name} holds a value that is not finite")
        torch.cuda.synchronize(self._dev)
        return d, dev

    @staticmethod
    def _back(t, dev):
        return t if dev else t.cpu().numpy()

    # ---- the reference's methods
    def sample_images(self, Z):
        """(I0_samp, I1_samp, cam0_p2, cam1_p2): the masked samples, Ny x Nx, and the pixel coordinates, (Ny * Nx) x 2 as (x, y)."""
        import torch
        d, dev = self._plane(Z, self.shape, "Z")
        i0, i1, uv = _new(self._dev, *self.shape), _new(self._dev, *self.shape), _new(self._dev, 4, *self.shape)
        self._ctx._check(self._ctx._lib.wass_vref_sample(self._h, d.data_ptr(), i0.data_ptr(), i1.data_ptr(), uv.data_ptr()))
        p0 = torch.stack([uv[0].reshape(-1), uv[1].reshape(-1)], dim=1)
        p1 = torch.stack([uv[2].reshape(-1), uv[3].reshape(-1)], dim=1)
        return tuple(self._back(t, dev) for t in (i0, i1, p0, p1))

    def compute_Z_gradient(self, Z):
        """(Z_dx, Z_dy): Z correlated with the two 7 x 7 derivative-of-Gaussian kernels (sigma 0.8), zero padding."""
        d, dev = self._plane(Z, self.shape, "Z")
        zdx, zdy = _new(self._dev, *self.shape), _new(self._dev, *self.shape)
        self._ctx._check(self._ctx._lib.wass_vref_zgrad(self._h, d.data_ptr(), zdx.data_ptr(), zdy.data_ptr()))
        return self._back(zdx, dev), self._back(zdy, dev)

    def compute_loss(self, Z):
        """(data_loss, smoothness_loss) as Python floats."""
        d, _ = self._plane(Z, self.shape, "Z")
        a, b = C.c_double(), C.c_double()
        self._ctx._check(self._ctx._lib.wass_vref_loss(self._h, d.data_ptr(), C.byref(a), C.byref(b)))
        return a.value, b.value

    def energy_gradient(self, Zc, alpha=10.0, full=False):
        """The gradient of data_loss + alpha * smoothness_loss of resize(Zc) with respect to the coarse field Zc; with full=True
        also with respect to the full-resolution surface: (gC, gZ)."""
        d, dev = self._plane(Zc, self.coarse_shape, "Zc")
        gc = _new(self._dev, *self.coarse_shape)
        gz = _new(self._dev, *self.shape) if full else None
        self._ctx._check(self._ctx._lib.wass_vref_gradient(self._h, d.data_ptr(), float(alpha), gc.data_ptr(), gz.data_ptr() if full else None))
        return (self._back(gc, dev), self._back(gz, dev)) if full else self._back(gc, dev)

    def adjoint(self, Zdx, Zdy, gd, alpha=10.0):
        """The backward half on given planes (wass_vref_adjoint): (gC, gZ) with gZ = gd + float32(2 alpha / N) * (Zdx and Zdy correlated
        with the flipped kernels) and gC the adjoint of the resize applied to gZ."""
        planes = [self._plane(a, self.shape, n) for a, n in ((Zdx, "Zdx"), (Zdy, "Zdy"), (gd, "gd"))]
        dev = planes[0][1]
        gc, gz = _new(self._dev, *self.coarse_shape), _new(self._dev, *self.shape)
        self._ctx._check(self._ctx._lib.wass_vref_adjoint(self._h, planes[0][0].data_ptr(), planes[1][0].data_ptr(), planes[2][0].data_ptr(),
                                                          float(alpha), gc.data_ptr(), gz.data_ptr()))
        return self._back(gc, dev), self._back(gz, dev)

    def optimize_coarse(self, Zc, iters, alpha=10.0, lr=1e-3, eps=1e-7, report_every=10, state: AdamState | None = None):
        """`iters` Adam steps from the coarse field Zc: (Zc, state, Z) with Z = resize(Zc) * mask.  state: an AdamState to continue
        from (what an earlier call returned); a continued run equals one longer run bit for bit.  The loss trace of this call is
        kept in .losses: rows [steps done, data, smoothness, energy]."""
        import torch
        iters = int(iters)
        if iters < 0:
            raise ValueError("iters must not be negative")
        d, dev = self._plane(Zc, self.coarse_shape, "Zc")
        d = d.clone()                                            # the caller's tensor is not modified
        if state is None:
            m, v, step = torch.zeros_like(d), torch.zeros_like(d), 0
        else:
            m, v, step = self._plane(state.m, self.coarse_shape, "state.m")[0].clone(), self._plane(state.v, self.coarse_shape, "state.v")[0].clone(), int(state.step)
        z = _new(self._dev, *self.shape)
        torch.cuda.synchronize(self._dev)
        every = int(report_every)
        cap = 2 + ((iters + every - 1) // every if every > 0 else 0)
        trace = np.zeros((cap, 4), np.float64)
        n, st = C.c_int(0), C.c_int64(step)
        self._ctx._check(self._ctx._lib.wass_vref_optimize(self._h, d.data_ptr(), m.data_ptr(), v.data_ptr(), C.byref(st), iters, float(alpha),
                                                           float(lr), float(eps), every, trace.ctypes.data, cap, C.byref(n), z.data_ptr()))
        self.losses = trace[:n.value].copy()
        return self._back(d, dev), AdamState(self._back(m, dev), self._back(v, dev), int(st.value)), self._back(z, dev)

    def optimize(self, Zinit, max_iters=400, alpha=10, lr=1e-3, report_every=10):
        """The reference's optimize: Zinit (Ny x Nx) is down-sampled to (Ny // 2) x (Nx // 2) by cv.resize's INTER_LINEAR rule, moved by
        max_iters Adam steps, and the refined full-resolution Z * mask is returned; the loss trace stays in .losses."""
        if tuple(int(v) for v in Zinit.shape) != self.shape:
            raise ValueError(f"Zinit of shape {tuple(Zinit.shape)}, expected {self.shape}")
        dev = _is_device(Zinit)
        host = Zinit.detach().cpu().numpy() if dev else np.asarray(Zinit)
        if not np.isfinite(host).all():
            raise ValueError("Zinit holds a value that is not finite")
        zc = downsample_linear(host, *self.coarse_shape)
        if dev:
            import torch
            zc = torch.from_numpy(zc).to(self._dev)
        _, self.state, z = self.optimize_coarse(zc, max_iters, alpha=alpha, lr=lr, report_every=report_every)
        return z


def _scalar(v) -> float:
    return float(np.ravel(np.asarray(v))[0])


def refine_surface(Zi, mask, I0, I1, gridsetup, ctx: Context | None = None, **kw):
    """What the commented block of the reference's grid() does with a gridded surface Zi (metres, z up, Ny x Nx): the refinement
    runs on -Zi / CAM_BASELINE in the plane's frame with Rp2c = Rpl.T and Tp2c = -Rp2c @ Tpl, and the result comes back as
    -Z * CAM_BASELINE with NaN where mask == 0.  gridsetup: the mapping setup_grid returns (Rpl, Tpl, P0cam, P1cam, XX, YY,
    CAM_BASELINE).  Cells with mask == 0 are set to 0 before the refinement, so a NaN outside the mask is no obstacle.
    kw: max_iters, alpha, lr, report_every of VariationalRefinement.optimize.  Returns a float32 host array."""
    baseline = _scalar(gridsetup["CAM_BASELINE"])
    Rp2c = np.asarray(gridsetup["Rpl"], np.float64).reshape(3, 3).T
    Tp2c = -Rp2c @ np.asarray(gridsetup["Tpl"], np.float64).reshape(3, 1)
    Zi = Zi.detach().cpu().numpy() if _is_device(Zi) else np.asarray(Zi)
    mask = mask.detach().cpu().numpy() if _is_device(mask) else np.asarray(mask)
    inside = mask != 0
    zin = np.where(inside, -Zi.astype(np.float64) / baseline, 0.0).astype(np.float32)
    with VariationalRefinement(I0, I1, Rp2c, Tp2c, gridsetup["P0cam"], gridsetup["P1cam"], gridsetup["XX"], gridsetup["YY"], baseline,
                               inside.astype(np.float32), ctx=ctx) as vr:
        z = vr.optimize(zin, **kw)
    out = (-z.astype(np.float64) * baseline).astype(np.float32)
    out[~inside] = np.nan
    return out


# ---------------------------------------------------------------------------------------------------------------- a sequence
@dataclasses.dataclass
class RefineOptions:
    """The refinement of every frame of a sequence.  max_iters, alpha, lr: the reference's defaults; Adam runs max_iters steps for
    every frame.  With the reference's alpha = 10 and its zero-padded smoothness term a constant offset of the surface costs energy
    along the border of the grid ("Variational refinement", "What the tests found out about the model"): that holds
    for every frame of a sequence.  batch: frames per set of launches -- 4 by default: DESIGN.md, "Variational refinement",
    "Batches", has the measurement: the time per frame stops falling at 4."""
    max_iters: int = 400
    alpha: float = 10.0
    lr: float = 1e-3
    report_every: int = 10
    batch: int = 4


def _plane_to_camera(gridsetup):
    baseline = _scalar(gridsetup["CAM_BASELINE"])
    if not np.isfinite(baseline) or baseline == 0:
        raise ValueError("CAM_BASELINE must be finite and not 0")
    Rp2c = np.asarray(gridsetup["Rpl"], np.float64).reshape(3, 3).T
    Tp2c = -Rp2c @ np.asarray(gridsetup["Tpl"], np.float64).reshape(3, 1)
    return baseline, Rp2c, Tp2c


class SequenceRefiner(_Handle):
    """The handle of a sequence's refinement: XX / b, YY / b, the cameras, the kernels and the axis tables are copied to the device
    once, with room for `batch` frames.  gridsetup: setup_grid's mapping (Rpl, Tpl, P0cam, P1cam, XX, YY, CAM_BASELINE);
    image_shapes: ((ih0, iw0), (ih1, iw1)).  refine() may be called any number of times, with 1 .. batch frames each."""

    def __init__(self, gridsetup, image_shapes, batch: int = 4, ctx: Context | None = None):
        import torch
        self.baseline, Rp2c, Tp2c = _plane_to_camera(gridsetup)
        XX, YY = gridsetup["XX"], gridsetup["YY"]
        self.shape = tuple(int(v) for v in XX.shape)
        if len(self.shape) != 2 or tuple(YY.shape) != self.shape or min(self.shape) < 2:
            raise ValueError(f"XX and YY must be one Ny x Nx shape of at least 2 x 2, got {tuple(XX.shape)}, {tuple(YY.shape)}")
        self.coarse_shape = (self.shape[0] // 2, self.shape[1] // 2)
        self.image_shapes = tuple((int(h), int(w)) for h, w in image_shapes)
        if len(self.image_shapes) != 2 or min(min(s) for s in self.image_shapes) < 2:
            raise ValueError(f"image_shapes {image_shapes}: two pictures of at least 2 x 2 pixels")
        self.batch = int(batch)
        if self.batch < 1:
            raise ValueError("batch must be at least 1")
        mats = _matrices((Rp2c, Tp2c, gridsetup["P0cam"], gridsetup["P1cam"]), ("Rpl", "Tpl", "P0cam", "P1cam"), flat=True)
        self.losses = []                                         # per frame of the last refine(): rows [steps, data, smoothness, energy]
        self._ctx = ctx if ctx is not None else Context(0)
        self._dev = torch.device("cuda", self._ctx.device_id)
        xb, yb = _scaled_grid(XX, YY, self.baseline, self._dev)
        kernels = _kernels()
        torch.cuda.synchronize(self._dev)
        h = C.c_void_p()
        dp = C.POINTER(C.c_double)
        (ih0, iw0), (ih1, iw1) = self.image_shapes
        self._ctx._check(self._ctx._lib.wass_vref_batch_create(
            self._ctx._h, self.batch, self.shape[0], self.shape[1], xb.data_ptr(), yb.data_ptr(), mats[0].ctypes.data_as(dp),
            mats[1].ctypes.data_as(dp), mats[2].ctypes.data_as(dp), mats[3].ctypes.data_as(dp), ih0, iw0, ih1, iw1, kernels.ctypes.data, C.byref(h)))
        self._h = h
        self._n = 0

    def _destroy(self, h):
        self._ctx._lib.wass_vref_batch_destroy(h)

    def _call(self, rc, first_frame=0):
        """a refusal that names a frame becomes a ValueError with the frame's index in the caller's sequence"""
        import re
        from .stereo import WassError
        try:
            self._ctx._check(rc)
        except WassError as e:
            m = re.search(r"frame (\d+)", str(e))
            if e.code == -1 and m:
                k = int(m.group(1))
                raise ValueError(str(e).replace(f"frame {k}", f"frame {k + first_frame}")) from None
            raise

    # ---- the steps of refine(), for callers that want to look in between
    def load(self, Zi, I0, I1, mask=None, first_frame=0):
        """n <= batch frames onto the device: Zi n x Ny x Nx in metres (NaN outside), the pictures n x ih x iw (uint8 or float32),
        mask n x Ny x Nx or Ny x Nx (a node is inside where it is not 0; default: where Zi is not NaN)."""
        import torch
        n = int(Zi.shape[0])
        if tuple(int(v) for v in Zi.shape) != (n,) + self.shape or not 1 <= n <= self.batch:
            raise ValueError(f"Zi of shape {tuple(Zi.shape)}: 1 .. {self.batch} frames of {self.shape} expected")
        for name, I, shp in (("I0", I0, self.image_shapes[0]), ("I1", I1, self.image_shapes[1])):
            if tuple(int(v) for v in I.shape) != (n,) + shp:
                raise ValueError(f"{name} of shape {tuple(I.shape)}, expected {(n,) + shp}")
        keep = [_to_dev(Zi, torch.float32, self._dev), _to_dev(I0, torch.float32, self._dev), _to_dev(I1, torch.float32, self._dev)]
        d_mask = None
        if mask is not None:
            d_mask = _to_dev(mask, torch.float32, self._dev)
            if tuple(d_mask.shape) == self.shape:
                d_mask = d_mask.expand(n, *self.shape).contiguous()
            if tuple(d_mask.shape) != (n,) + self.shape:
                raise ValueError(f"mask of shape {tuple(mask.shape)}, expected {(n,) + self.shape} or {self.shape}")
        torch.cuda.synchronize(self._dev)
        self._n = 0
        self._call(self._ctx._lib.wass_vref_batch_load(self._h, n, keep[0].data_ptr(), d_mask.data_ptr() if d_mask is not None else None,
                                                       keep[1].data_ptr(), keep[2].data_ptr(), self.baseline), first_frame)
        self._n = n

    def set_state(self, Zc, m=None, v=None, step=0):
        """the coarse fields (n x Hc x Wc) and the optimiser's state of the loaded frames; m, v default to zeros"""
        import torch
        shape = (self._n,) + self.coarse_shape
        t = []
        for name, a in (("Zc", Zc), ("m", m), ("v", v)):
            d = torch.zeros(shape, dtype=torch.float32, device=self._dev) if a is None else _to_dev(a, torch.float32, self._dev)
            if tuple(d.shape) != shape:
                raise ValueError(f"{name} of shape {tuple(d.shape)}, expected {shape}")
            t.append(d)
        torch.cuda.synchronize(self._dev)
        self._call(self._ctx._lib.wass_vref_batch_set_state(self._h, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), int(step)))

    def get_state(self):
        """(Zc, m, v, step) of the loaded frames: device tensors n x Hc x Wc"""
        t = [_new(self._dev, self._n, *self.coarse_shape) for _ in range(3)]
        st = C.c_int64(0)
        self._call(self._ctx._lib.wass_vref_batch_get_state(self._h, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), C.byref(st)))
        return t[0], t[1], t[2], int(st.value)

    def optimize(self, iters, alpha=10.0, lr=1e-3, eps=1e-7, report_every=10):
        """`iters` Adam steps of every loaded frame; .losses: per frame the rows [steps done in this call, data, smoothness, energy]"""
        iters, every = int(iters), int(report_every)
        if iters < 0:
            raise ValueError("iters must not be negative")
        cap = 2 + ((iters + every - 1) // every if every > 0 else 0)
        trace = np.zeros((max(self._n, 1), cap, 4), np.float64)
        n = C.c_int(0)
        self._call(self._ctx._lib.wass_vref_batch_optimize(self._h, iters, float(alpha), float(lr), float(eps), every, trace.ctypes.data, cap,
                                                           C.byref(n)))
        self.losses = [trace[f, :n.value].copy() for f in range(self._n)]

    def result(self, out=None, with_plane=False):
        """the refined surfaces in metres, NaN outside the masks (n x Ny x Nx, a device tensor; out: where to put them); with_plane:
        also resize(Zc) * mask in the plane's frame"""
        import torch
        shape = (self._n,) + self.shape
        if out is None:
            out = _new(self._dev, *shape)
        elif not _is_device(out) or tuple(out.shape) != shape or out.dtype != torch.float32 or not out.is_contiguous():
            raise ValueError(f"out: a contiguous float32 device tensor of shape {shape} expected")
        z = _new(self._dev, *shape) if with_plane else None
        torch.cuda.synchronize(self._dev)
        self._call(self._ctx._lib.wass_vref_batch_result(self._h, out.data_ptr(), z.data_ptr() if with_plane else None))
        return (out, z) if with_plane else out

    def refine(self, Zi, I0, I1, options: RefineOptions | None = None, mask=None, out=None, first_frame=0):
        """load, options.max_iters steps, result: device tensors in, a device tensor out; the loss traces stay in .losses.
        first_frame: the index of Zi[0] in the caller's sequence, for the message of a refusal."""
        o = options if options is not None else RefineOptions()
        self.load(Zi, I0, I1, mask, first_frame)
        self.optimize(o.max_iters, alpha=o.alpha, lr=o.lr, report_every=o.report_every)
        return self.result(out)


def refine_sequence(Zi, I0, I1, gridsetup, mask=None, options: RefineOptions | None = None, ctx: Context | None = None, out=None):
    """refine_surface for a sequence.  Zi: n x Ny x Nx in metres, z up, NaN outside (a host array, an np.memmap or a device
    tensor); I0, I1: n x ih x iw, uint8 or float32; mask: n x Ny x Nx or Ny x Nx, a node is inside where it is not 0 (default:
    where Zi is not NaN); out: an n x Ny x Nx float32 host array or memmap (a device tensor when Zi is one) that receives the
    result.  The frames go through the device in sub-batches of options.batch, the last one ragged.  Returns (the refined cube,
    the loss trace of every frame); frame i equals refine_surface(Zi[i], mask_i, I0[i], I1[i], gridsetup) bit for bit."""
    import torch
    o = options if options is not None else RefineOptions()
    n = int(Zi.shape[0])
    if len(Zi.shape) != 3 or n < 1:
        raise ValueError(f"Zi of shape {tuple(Zi.shape)}: n x Ny x Nx expected")
    if int(I0.shape[0]) != n or int(I1.shape[0]) != n:
        raise ValueError("Zi, I0 and I1 must hold the same number of frames")
    dev_in = _is_device(Zi)
    shape = tuple(int(v) for v in Zi.shape)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=Zi.device) if dev_in else np.empty(shape, np.float32)
    elif tuple(out.shape) != shape or _is_device(out) != dev_in or str(out.dtype).split(".")[-1] != "float32":
        raise ValueError(f"out: float32 of shape {shape} on the side of Zi expected")
    per_frame_mask = mask is not None and len(mask.shape) == 3
    nb = max(1, min(int(o.batch), n))
    losses = []
    with SequenceRefiner(gridsetup, (tuple(I0.shape[1:]), tuple(I1.shape[1:])), nb, ctx) as sr:
        d_mask = None if mask is None or per_frame_mask else _to_dev(mask, torch.float32, sr._dev)
        for i0 in range(0, n, nb):
            k = slice(i0, min(n, i0 + nb))
            part = (lambda a: a[k] if _is_device(a) else np.ascontiguousarray(a[k]))
            mk = d_mask if not per_frame_mask else part(mask)
            if dev_in:
                sr.refine(Zi[k], part(I0), part(I1), o, mk, out=out[k], first_frame=i0)
            else:
                out[k] = sr.refine(part(Zi), part(I0), part(I1), o, mk, first_frame=i0).cpu().numpy()
            losses += sr.losses
    return out, losses
