"""The feature detector of wass_match on the GPU: what FeatureSet::detect (src/wass_match/FeatureSet.cpp:176-327) does with
cv::KAZE::create(false, false, threshold, n_octaves, n_sublevels), the reference's own subsampling behind it, and the file-level
step that turns undistorted/0000000{0,1}.png into matches_unfiltered.txt.

The kernels (csrc/kaze.hip) build the non-linear scale space, the Hessian response, find and refine its extrema and compute the
orientation and the M-SURF descriptor of every keypoint; include/wass_gpu.h states their operation order.  The host keeps what is
small and sequential: the level table and FED step sizes, the contrast factor's scan of 300 bins, the duplicate pass over the
sorted candidates, the keypoint's size (the one power of two) and the subsampling.  The algorithm is restated from the published
method and is not pinned against OpenCV.

Host arrays are numpy, device arrays torch tensors passed by raw pointer.  There is no CPU path.
"""
from __future__ import annotations

import ctypes as C
import math
import os
import sys
from dataclasses import dataclass

import numpy as np

from . import _lib
from . import match as _match
from .match import Features, _context, _is_tensor

SOFFSET = 1.6
SDERIVATIVES = 1.0
KCONTRAST_PERCENTILE = 0.7
KCONTRAST_NBINS = 300
TAU_MAX = 0.25
MAX_LEVELS = 32                 # WASS_KAZE_MAX_LEVELS
MAX_CANDIDATES = 1 << 20        # WASS_KAZE_MAX_CANDIDATES: the default cap of the extremum list
CAP_REACHED = 1                 # WASS_KAZE_CAP_REACHED


@dataclass
class KazeOptions:
    threshold: float = 1e-4
    n_octaves: int = 4
    n_sublevels: int = 4


@dataclass
class KazeLevels:
    """per level: esigma, etime float32; sigma_size, octave, sublevel int; taus: the FED step sizes that lead to it (none for level 0)"""
    esigma: np.ndarray
    etime: np.ndarray
    sigma_size: np.ndarray
    octave: np.ndarray
    sublevel: np.ndarray
    taus: list

    def __len__(self):
        return self.esigma.shape[0]


@dataclass
class Keypoints:
    """x, y, size (a diameter), angle (radians in [0, 2 pi)), response float32 n; level int32 n; descriptors float32 n x 64"""
    x: np.ndarray
    y: np.ndarray
    size: np.ndarray
    angle: np.ndarray
    response: np.ndarray
    level: np.ndarray
    descriptors: np.ndarray
    status: int = 0             # CAP_REACHED when the candidate list was cut at its cap

    def __len__(self):
        return self.x.shape[0]

    def table(self) -> np.ndarray:
        """n x 5 float32: x y size level angle, what the orientation and descriptor kernels read"""
        return np.ascontiguousarray(np.column_stack([self.x, self.y, self.size, self.level.astype(np.float32), self.angle]).astype(np.float32))


# ---------------------------------------------------------------------------------------------------------------- host tables
def _check_options(o: KazeOptions) -> KazeOptions:
    o = KazeOptions() if o is None else o
    if not isinstance(o, KazeOptions):
        raise ValueError("options: a KazeOptions")
    if int(o.n_octaves) < 1 or int(o.n_sublevels) < 1:
        raise ValueError(f"options: n_octaves = {o.n_octaves}, n_sublevels = {o.n_sublevels}: at least 1 each")
    n = int(o.n_octaves) * int(o.n_sublevels)
    if n < 3:
        raise ValueError(f"options: {n} levels; the extremum search needs at least 3")
    if n > MAX_LEVELS:
        raise ValueError(f"options: {n} levels; at most {MAX_LEVELS}")
    if not (float(o.threshold) >= 0.0):
        raise ValueError(f"options: threshold = {o.threshold}")
    return o


def _is_prime(n: int) -> bool:
    return n >= 2 and all(n % d for d in range(2, int(math.isqrt(n)) + 1))


def fed_taus(T, tau_max: float = TAU_MAX, reorder: bool = True) -> np.ndarray:
    """The step sizes of one FED cycle of stopping time T (float32), in the kappa-cycle order unless reorder is off"""
    f = np.float32
    T, tm = f(T), f(tau_max)
    n = int(np.ceil(np.sqrt(f(3.0) * T / tm + f(0.25)) - f(0.5) - f(1e-8)) + f(0.5))
    if n <= 0:
        return np.zeros(0, np.float32)
    scale = f(3.0) * T / (tm * f(n * (n + 1)))
    k = np.arange(n, dtype=np.float64)
    h = np.cos(np.pi * (2.0 * k + 1.0) / (4.0 * n + 2.0))
    tauh = (np.float64(scale * tm) / (2.0 * h * h)).astype(np.float32)
    if not reorder or n == 1:
        return tauh
    kappa, prime = n // 2, n + 1
    while not _is_prime(prime):
        prime += 1
    tau, k = np.empty(n, np.float32), 0
    for l in range(n):
        while True:
            index = ((k + 1) * kappa) % prime - 1
            if index < n:
                break
            k += 1
        tau[l] = tauh[index]
        k += 1
    return tau


def kaze_levels(options: KazeOptions | None = None) -> KazeLevels:
    """esigma = soffset 2^(s / n_sublevels + o), etime = esigma^2 / 2, sigma_size = esigma rounded half to even, and the FED steps"""
    o = _check_options(options)
    no, ns = int(o.n_octaves), int(o.n_sublevels)
    octave = np.repeat(np.arange(no, dtype=np.int32), ns)
    sub = np.tile(np.arange(ns, dtype=np.int32), no)
    esigma = (SOFFSET * np.exp2(sub.astype(np.float64) / ns + octave)).astype(np.float32)
    etime = np.float32(0.5) * esigma * esigma
    sigma_size = np.rint(esigma).astype(np.int32)
    taus = [np.zeros(0, np.float32)] + [fed_taus(etime[i] - etime[i - 1]) for i in range(1, no * ns)]
    return KazeLevels(esigma, etime, sigma_size, octave, sub, taus)


def gaussian_taps(sigma: float) -> np.ndarray:
    """ksize = ceil(2 (1 + (sigma - 0.8) / 0.3)) made odd; exp(-x^2 / 2 sigma^2) in fp64, normalised, as float32"""
    ksize = int(math.ceil(2.0 * (1.0 + (sigma - 0.8) / 0.3))) | 1
    x = np.arange(ksize, dtype=np.float64) - (ksize - 1) / 2
    t = np.exp(-x * x / (2.0 * sigma * sigma))
    return (t / t.sum()).astype(np.float32)


def scharr_weights(sigma_size: int):
    """(norm, w * norm) of the scaled Scharr smoothing taps, float32: w = 10 / 3, norm = 1 / (2 sigma_size (w + 2))"""
    f = np.float32
    w = f(10.0) / f(3.0)
    norm = f(1.0) / (f(2.0) * f(sigma_size) * (w + f(2.0)))
    return norm, w * norm


def contrast_factor(hmax, npoints: int, hist) -> np.float32:
    """the bin count at which the running sum of the histogram reaches (int)(npoints * 0.7): k = hmax * (bins / 300); 0.03 if never"""
    f = np.float32
    nthreshold = int(f(npoints) * f(KCONTRAST_PERCENTILE))
    nelements, k = 0, 0
    while nelements < nthreshold and k < KCONTRAST_NBINS:
        nelements += int(hist[k])
        k += 1
    if nelements < nthreshold or npoints == 0:
        return f(0.03)
    return f(hmax) * (f(k) / f(KCONTRAST_NBINS))


def keypoint_size(levels: KazeLevels, level, ds, n_sublevels: int) -> np.ndarray:
    """2 soffset 2^(octave + (sublevel + ds) / n_sublevels), in fp64 from the float32 ds, as float32"""
    level = np.asarray(level, np.int64)
    e = levels.octave[level].astype(np.float64) + (levels.sublevel[level].astype(np.float64) + np.asarray(ds, np.float32).astype(np.float64)) / n_sublevels
    return (2.0 * SOFFSET * np.exp2(e)).astype(np.float32)


def remove_duplicates(cand, values, levels: KazeLevels):
    """The duplicate pass over candidates sorted by (level, y, x).  cand: n x 3 (level, y, x); values: their responses.  The accepted
    list is scanned in order; the first accepted point that is in the same level and closer than esigma drops the candidate, or is
    in the level below and closer than sigma_size: then the candidate takes its place if its response is larger and is dropped
    otherwise.  Returns the indices (into cand) of the accepted list, in its order."""
    cand = np.asarray(cand, np.int64).reshape(-1, 3)
    values = np.asarray(values, np.float32).reshape(-1)
    f = np.float32
    es2 = [f(e) * f(e) for e in levels.esigma]
    ss2 = [f(s) * f(s) for s in levels.sigma_size]
    cell = int(levels.sigma_size.max()) + 1          # no radius is longer than a cell: a hit lies in the 3 x 3 cells around the candidate
    acc, slots = [], {}                              # accepted: [index into cand, level, y, x]; slots: cell -> accepted slots, ascending
    for i, (lev, y, x) in enumerate(cand.tolist()):
        cy, cx = y // cell, x // cell
        near = sorted(s for gy in (cy - 1, cy, cy + 1) for gx in (cx - 1, cx, cx + 1) for s in slots.get((gy, gx), ()))
        hit = -1
        for s_ in near:
            _, l2, y2, x2 = acc[s_]
            if l2 != lev and l2 != lev - 1:
                continue
            d2 = f(x2 - x) * f(x2 - x) + f(y2 - y) * f(y2 - y)
            if d2 < (es2[lev] if l2 == lev else ss2[lev]):
                hit = s_
                break
        if hit < 0:
            slots.setdefault((cy, cx), []).append(len(acc))
            acc.append([i, lev, y, x])
        elif acc[hit][1] == lev - 1 and values[i] > values[acc[hit][0]]:
            _, _, y2, x2 = acc[hit]
            if (y2 // cell, x2 // cell) != (cy, cx):
                slots[(y2 // cell, x2 // cell)].remove(hit)
                lst = slots.setdefault((cy, cx), [])
                lst.append(hit)
                lst.sort()
            acc[hit] = [i, lev, y, x]
    return np.array([a[0] for a in acc], np.int64)


# ------------------------------------------------------------------------------------------------------------------- pictures
def _picture(image, ctx):
    """a contiguous h x w uint8 device tensor of the picture"""
    import torch
    dev = torch.device("cuda", ctx.device_id)
    if _is_tensor(image):
        t = image
        if t.dim() != 2:
            raise ValueError("image: a picture has two dimensions")
        if t.dtype == torch.uint8:
            pass
        elif t.dtype in (torch.float32, torch.float64):
            t = torch.clamp(torch.round(t.to(torch.float64) * 255.0), 0, 255).to(torch.uint8)
        else:
            raise ValueError(f"image: dtype {t.dtype}; uint8, or float in [0, 1]")
        return t.to(dev).contiguous()
    a = np.asarray(image)
    if a.ndim != 2:
        raise ValueError("image: a picture has two dimensions")
    if a.dtype == np.uint8:
        pass
    elif a.dtype in (np.float32, np.float64):
        a = np.clip(np.rint(a.astype(np.float64) * 255.0), 0, 255).astype(np.uint8)
    else:
        raise ValueError(f"image: dtype {a.dtype}; uint8, or float in [0, 1]")
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a if a.flags.writeable else a.copy()).to(dev)     # a picture read through PIL is read-only


def _check_size(h: int, w: int, levels: KazeLevels):
    reach = int(levels.sigma_size.max())
    if min(h, w) <= reach or min(h, w) < 3:
        raise ValueError(f"image: {h} x {w} is smaller than the largest reflect-101 reach of the derivatives ({reach} pixels)")
    if max(h, w) > 32768:
        raise ValueError(f"image: {h} x {w}: at most 32768 rows and columns")


def kaze_scratch_bytes(h: int, w: int, options: KazeOptions | None = None) -> int:
    """An upper bound of the device memory one picture takes in kaze_detect (no GPU needed): Lx, Ly, Ldet of every level, the seven
    planes of the chain, the picture and the candidate list with its records at the cap of 2^20.  A run allocates the list for what
    it finds (65 536 keys first), so it stays below this by up to 29 MB; the sort's and the gather's temporaries (a few times the
    list found) and, with keep=True, three more planes for Lxx, Lxy, Lyy are not in the figure."""
    o = _check_options(options)
    _check_size(int(h), int(w), kaze_levels(o))
    levels = o.n_octaves * o.n_sublevels
    return _lib.scratch_bytes("kaze", (int(h), int(w), levels), f"image: {h} x {w} with {levels} levels")


# -------------------------------------------------------------------------------------------------------------------- pyramid
class KazePyramid:
    """The scale space and the response of one picture on the device: Lx, Ly (scaled) and Ldet of every level.  With keep=True the
    intermediate planes are copied to the host as they are made (Lt, Lsmooth, flow, Lxx, Lxy, Lyy): the stage entries' output."""

    def __init__(self, image, options=None, ctx=None, keep: bool = False, timings: dict | None = None):
        import contextlib
        import time
        import torch

        @contextlib.contextmanager
        def stage(name):
            # every library call ends in a synchronisation, so a host clock around it is the stage's time (scripts/time_kaze.py)
            t0 = time.perf_counter()
            yield
            if timings is not None:
                timings[name] = timings.get(name, 0.0) + (time.perf_counter() - t0)
        self._stage = stage
        self.options = _check_options(options)
        self.levels = kaze_levels(self.options)
        self.ctx = ctx = _context(ctx)
        img = _picture(image, ctx)
        h, w = int(img.shape[0]), int(img.shape[1])
        _check_size(h, w, self.levels)
        self.h, self.w, N = h, w, len(self.levels)
        dev, f32 = img.device, torch.float32
        lib, hd = ctx._lib, ctx._h
        self.Lx, self.Ly, self.Ldet = (torch.empty((N, h, w), dtype=f32, device=dev) for _ in range(3))
        Lt, twin, Lsm, tmp, flow, gx, gy = (torch.empty((h, w), dtype=f32, device=dev) for _ in range(7))
        rec = torch.zeros(2 + KCONTRAST_NBINS, dtype=torch.int32, device=dev)
        extra = [torch.empty((h, w), dtype=f32, device=dev) for _ in range(3)] if keep else [None] * 3
        self.host = {k: [] for k in ("Lt", "Lsmooth", "flow", "Lxx", "Lxy", "Lyy")} if keep else None
        torch.cuda.synchronize(dev)

        def gauss(src, dst, taps):
            t = np.ascontiguousarray(taps, np.float32)
            ctx._check(lib.wass_kaze_gauss_dev(hd, src.data_ptr(), h, w, t.ctypes.data, t.shape[0], tmp.data_ptr(), dst.data_ptr()))

        def scharr(src, s, lx, ly):
            n, wn = scharr_weights(s)
            ctx._check(lib.wass_kaze_scharr_dev(hd, src.data_ptr(), h, w, int(s), float(n), float(wn), lx.data_ptr(), ly.data_ptr()))

        def response(i):
            s = int(self.levels.sigma_size[i])
            scharr(Lsm, s, self.Lx[i], self.Ly[i])
            n, wn = scharr_weights(s)
            ctx._check(lib.wass_kaze_hessian_dev(hd, self.Lx[i].data_ptr(), self.Ly[i].data_ptr(), h, w, s, float(n), float(wn), self.Ldet[i].data_ptr(),
                                                 *[e.data_ptr() if e is not None else None for e in extra]))
            if keep:
                for name, t in (("Lt", Lt), ("Lsmooth", Lsm), ("flow", flow), ("Lxx", extra[0]), ("Lxy", extra[1]), ("Lyy", extra[2])):
                    self.host[name].append(t.cpu().numpy())

        g1 = gaussian_taps(1.0)
        with stage("presmooth"):
            ctx._check(lib.wass_kaze_convert_dev(hd, img.data_ptr(), w, h, w, float(np.float32(1.0 / 255.0)), twin.data_ptr()))
            gauss(twin, Lt, gaussian_taps(SOFFSET))
            gauss(Lt, Lsm, gaussian_taps(SDERIVATIVES))
        # the contrast factor: Gaussian(1) of the picture, plain Scharr, the 70th percentile of the gradient modulus over 300 bins
        with stage("contrast"):
            gauss(twin, flow, g1)
            scharr(flow, 1, gx, gy)
            hmax, npoints, hist = C.c_float(), C.c_uint32(), np.zeros(KCONTRAST_NBINS, np.uint32)
            ctx._check(lib.wass_kaze_contrast_dev(hd, gx.data_ptr(), gy.data_ptr(), h, w, rec.data_ptr(), C.byref(hmax), C.byref(npoints),
                                                  hist.ctypes.data))
            self.hmax, self.npoints, self.hist = np.float32(hmax.value), int(npoints.value), hist
            self.k = contrast_factor(self.hmax, self.npoints, hist)
        flow.zero_()
        torch.cuda.synchronize(dev)
        with stage("response"):
            response(0)
        for i in range(1, N):
            with stage("flow"):
                gauss(Lt, Lsm, gaussian_taps(SDERIVATIVES))
                scharr(Lsm, 1, gx, gy)
                ctx._check(lib.wass_kaze_flow_dev(hd, gx.data_ptr(), gy.data_ptr(), h, w, float(self.k), flow.data_ptr()))
            taus = self.levels.taus[i]
            with stage("diffusion"):
                ctx._check(lib.wass_kaze_diffuse_dev(hd, Lt.data_ptr(), twin.data_ptr(), flow.data_ptr(), h, w, taus.ctypes.data, taus.shape[0]))
            with stage("response"):
                response(i)
        if keep:
            self.host = {k: np.stack(v) for k, v in self.host.items()}

    # -- extrema
    def candidates(self, cap: int = MAX_CANDIDATES):
        """(status, n x 3 int64 (level, y, x) sorted, their responses float32)"""
        import torch
        if not 1 <= int(cap) <= MAX_CANDIDATES:
            raise ValueError(f"cap = {cap}: 1 .. {MAX_CANDIDATES} candidates")
        ctx, h, w, N = self.ctx, self.h, self.w, len(self.levels)
        dev = self.Ldet.device
        # the list is allocated for what is found, at most the cap: where the first call finds more than it holds, a second one follows
        keys = torch.empty(min(int(cap), 1 << 16), dtype=torch.int64, device=dev)
        d_count = torch.zeros(1, dtype=torch.int32, device=dev)
        es = np.ascontiguousarray(self.levels.esigma, np.float32)
        count = C.c_uint32()
        torch.cuda.synchronize(dev)

        def find(buf):
            return ctx._check(ctx._lib.wass_kaze_extrema_dev(ctx._h, self.Ldet.data_ptr(), h * w, N, h, w, float(np.float32(self.options.threshold)),
                                                             es.ctypes.data, buf.data_ptr(), int(buf.shape[0]), d_count.data_ptr(), C.byref(count)),
                              allow=(CAP_REACHED,))
        rc = find(keys)
        if rc == CAP_REACHED and keys.shape[0] < int(cap):
            keys = torch.empty(min(int(cap), int(count.value)), dtype=torch.int64, device=dev)
            torch.cuda.synchronize(dev)
            rc = find(keys)
        n = min(int(count.value), int(keys.shape[0]))
        skeys = torch.sort(keys[:n]).values
        vals = self.Ldet.reshape(-1)[skeys] if n else torch.empty(0, dtype=torch.float32, device=dev)
        k = skeys.cpu().numpy()
        cand = np.stack([k // (h * w), (k // w) % h, k % w], axis=1).astype(np.int64).reshape(-1, 3)
        return rc, cand, vals.cpu().numpy()

    def refine(self, cand):
        """n x 5 float32 (x, y, ds, response, kept) of candidates given as (level, y, x)"""
        import torch
        cand = np.asarray(cand, np.int64).reshape(-1, 3)
        if cand.shape[0] == 0:
            return np.zeros((0, 5), np.float32)
        h, w, N = self.h, self.w, len(self.levels)
        if cand[:, 0].min() < 1 or cand[:, 0].max() > N - 2 or cand[:, 1].min() < 1 or cand[:, 1].max() > h - 2 or cand[:, 2].min() < 1 \
                or cand[:, 2].max() > w - 2:
            raise ValueError("candidates: levels 1 .. N-2 and interior pixels only")
        keys = torch.from_numpy(np.ascontiguousarray((cand[:, 0] * h + cand[:, 1]) * w + cand[:, 2])).to(self.Ldet.device)
        out = torch.empty((cand.shape[0], 5), dtype=torch.float32, device=self.Ldet.device)
        torch.cuda.synchronize(self.Ldet.device)
        self.ctx._check(self.ctx._lib.wass_kaze_refine_dev(self.ctx._h, self.Ldet.data_ptr(), h * w, N, h, w, keys.data_ptr(), cand.shape[0], out.data_ptr()))
        return out.cpu().numpy()

    # -- keypoints
    def _table(self, keypoints, need_angle: bool):
        t = keypoints.table() if isinstance(keypoints, Keypoints) else np.ascontiguousarray(keypoints, np.float32)
        if t.ndim != 2 or t.shape[1] not in (4, 5) or (need_angle and t.shape[1] != 5):
            raise ValueError("keypoints: an n x 5 float32 table (x, y, size, level, angle)" if need_angle else
                             "keypoints: an n x 4 or n x 5 float32 table (x, y, size, level[, angle])")
        if t.shape[1] == 4:
            t = np.ascontiguousarray(np.column_stack([t, np.zeros(t.shape[0], np.float32)]))
        if t.shape[0] and (not np.isfinite(t).all() or t[:, 3].min() < 0 or t[:, 3].max() > len(self.levels) - 1):
            raise ValueError("keypoints: finite values and levels of this scale space only")
        if t.shape[0] and (t[:, 0].min() < 0 or t[:, 0].max() > self.w - 1 or t[:, 1].min() < 0 or t[:, 1].max() > self.h - 1
                           or t[:, 2].min() < 0 or t[:, 2].max() > max(self.h, self.w)):
            raise ValueError("keypoints: positions inside the picture and sizes from 0 to its larger side")
        return t

    def _per_keypoint(self, fn, table, width):
        import torch
        n = table.shape[0]
        if n == 0:
            return np.zeros((0, width) if width > 1 else (0,), np.float32)
        dev = self.Ldet.device
        d_kp = torch.from_numpy(table).to(dev)
        out = torch.empty((n, width) if width > 1 else (n,), dtype=torch.float32, device=dev)
        torch.cuda.synchronize(dev)
        self.ctx._check(fn(self.ctx._h, d_kp.data_ptr(), n, self.Lx.data_ptr(), self.Ly.data_ptr(), self.h * self.w, len(self.levels), self.h, self.w,
                           out.data_ptr()))
        return out.cpu().numpy()

    def orientation(self, keypoints) -> np.ndarray:
        return self._per_keypoint(self.ctx._lib.wass_kaze_orientation_dev, self._table(keypoints, False), 1)

    def descriptors(self, keypoints) -> np.ndarray:
        return self._per_keypoint(self.ctx._lib.wass_kaze_descriptors_dev, self._table(keypoints, True), 64)

    def detect(self, cap: int = MAX_CANDIDATES) -> Keypoints:
        with self._stage("extrema"):
            rc, cand, vals = self.candidates(cap)
        with self._stage("duplicates (host)"):
            kept = cand[remove_duplicates(cand, vals, self.levels)]
        self.counts = (len(cand), len(kept))           # candidates found, accepted by the duplicate pass
        with self._stage("refine"):
            r = self.refine(kept)
        ok = r[:, 4] != 0
        kept, r = kept[ok], r[ok]
        level = kept[:, 0].astype(np.int32)
        size = keypoint_size(self.levels, level, r[:, 2], int(self.options.n_sublevels))
        kp = Keypoints(r[:, 0].copy(), r[:, 1].copy(), size, np.zeros(len(level), np.float32), r[:, 3].copy(), level,
                       np.zeros((len(level), 64), np.float32), int(rc))
        with self._stage("orientation"):
            kp.angle = self.orientation(kp)
        with self._stage("descriptors"):
            kp.descriptors = self.descriptors(kp)
        return kp


def _pyramid(image, options, ctx, keep=False) -> KazePyramid:
    if isinstance(image, KazePyramid):
        if keep and image.host is None:
            raise ValueError("image: this pyramid was built without its intermediate planes")
        return image
    return KazePyramid(image, options, ctx, keep)


# --------------------------------------------------------------------------------------------------------------- stage entries
def kaze_scale_space(image, options=None, ctx=None) -> dict:
    """Lt, Lsmooth, flow (N x h x w float32; flow of level 0 is zero), k, hmax, npoints, hist"""
    p = _pyramid(image, options, ctx, True)
    return {"Lt": p.host["Lt"], "Lsmooth": p.host["Lsmooth"], "flow": p.host["flow"], "k": p.k, "hmax": p.hmax, "npoints": p.npoints, "hist": p.hist}


def kaze_response(image, options=None, ctx=None) -> dict:
    """Lx, Ly (scaled by sigma_size), Lxx, Lxy, Lyy (by its square), Ldet: N x h x w float32 each"""
    p = _pyramid(image, options, ctx, True)
    return {"Lx": p.Lx.cpu().numpy(), "Ly": p.Ly.cpu().numpy(), "Lxx": p.host["Lxx"], "Lxy": p.host["Lxy"], "Lyy": p.host["Lyy"],
            "Ldet": p.Ldet.cpu().numpy()}


def kaze_extrema(image, options=None, ctx=None, cap: int = MAX_CANDIDATES) -> dict:
    """status; candidates (n x 3: level, y, x, sorted) and their values; kept: the accepted list of the duplicate pass (m x 3);
    refined: m x 5 float32 (x, y, ds, response, kept); size: the m diameters"""
    p = _pyramid(image, options, ctx)
    rc, cand, vals = p.candidates(cap)
    kept = cand[remove_duplicates(cand, vals, p.levels)]
    r = p.refine(kept)
    return {"status": int(rc), "candidates": cand, "values": vals, "kept": kept, "refined": r,
            "size": keypoint_size(p.levels, kept[:, 0], r[:, 2], int(p.options.n_sublevels))}


def kaze_orientation(keypoints, image, options=None, ctx=None) -> np.ndarray:
    """the angle of every keypoint of a table (x, y, size, level[, angle]) or a Keypoints, on the scale space of `image`"""
    return _pyramid(image, options, ctx).orientation(keypoints)


def kaze_descriptors(keypoints, image, options=None, ctx=None) -> np.ndarray:
    """the n x 64 descriptors of a table (x, y, size, level, angle) or a Keypoints"""
    return _pyramid(image, options, ctx).descriptors(keypoints)


def kaze_detect(image, options=None, ctx=None, cap: int = MAX_CANDIDATES):
    """cv::KAZE::detectAndCompute of a picture (uint8 host array or device tensor; a float picture in [0, 1] is scaled by 255 and
    rounded, as FeatureSet::detect does), or of a list of pictures: picture i of a list is the single run of picture i."""
    if isinstance(image, (list, tuple)):
        return [kaze_detect(im, options, ctx, cap) for im in image]
    return KazePyramid(image, options, ctx).detect(cap)


# ----------------------------------------------------------------------------------------------------------------- subsampling
def _remove_close(xy: np.ndarray, min_distance: float) -> np.ndarray:
    """FeatureSet.cpp:253-268 on points already sorted: the order of the survivors, swap-with-last removals included"""
    order = np.arange(xy.shape[0])
    last = xy.shape[0] - 1
    k = 0
    while k <= last:
        seg = order[k + 1:last + 1]                      # a view: the swaps below land in `order`
        if seg.shape[0]:
            d = xy[seg] - xy[order[k]]
            f = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]).astype(np.float64) < min_distance     # dist2d: float32, compared as double
            lo, hi = 0, seg.shape[0] - 1
            while lo <= hi:
                nz = np.flatnonzero(f[lo:hi + 1])
                if nz.shape[0] == 0:
                    break
                p = lo + int(nz[0])
                seg[p], f[p] = seg[hi], f[hi]
                hi -= 1
                lo = p
            last = k + 1 + hi
        k += 1
    return order[:last + 1]


def subsample_features(keypoints, width: int, height: int, max_features: int = 2000, subdivisions: int = 5, min_distance: float = 10.0) -> np.ndarray:
    """The subsampling of FeatureSet::detect (FeatureSet.cpp:70-97, 218-321): the indices of the keypoints it keeps, in its output
    order.  keypoints: a Keypoints or an n x 3 array (x, y, response).  std::sort leaves the order of equal responses open; here the
    earlier detection comes first."""
    f = np.float32
    if isinstance(keypoints, Keypoints):
        pts = np.column_stack([keypoints.x, keypoints.y, keypoints.response]).astype(np.float32)
    else:
        pts = np.asarray(keypoints, np.float32).reshape(-1, 3)
    if int(subdivisions) < 1:
        raise ValueError(f"subdivisions = {subdivisions}")
    if pts.shape[0] == 0:
        return np.zeros(0, np.int64)
    W, H, n = int(width), int(height), int(subdivisions)
    border = max(int(W / 30.0), 2)
    aw, ah = int(f(W) / f(n)), int(f(H) / f(n))
    x, y = pts[:, 0], pts[:, 1]
    inside = (x > border) & (x < W - border) & (y > border) & (y < H - border)
    areas = []
    for ii in range(n):
        for jj in range(n):
            ax, ay = int(f(W) / f(n) * f(ii)), int(f(H) / f(n) * f(jj))
            areas.append(np.flatnonzero(inside & (x > ax) & (y > ay) & (x < ax + aw) & (y < ay + ah)))
    na = len(areas)
    per = int(int(max_features) // na)
    extra = sum(per - a.shape[0] for a in areas if a.shape[0] < per)
    per = int(f(per) + f(extra) / f(na))
    for i, a in enumerate(areas):
        if a.shape[0] < 2:
            continue
        a = a[np.argsort(-pts[a, 2], kind="stable")]
        a = a[_remove_close(pts[a, :2], float(min_distance))]
        areas[i] = a[:per] if a.shape[0] > per else a
    out = []
    for s in range(max(a.shape[0] for a in areas)):
        out.extend(int(a[s]) for a in areas if a.shape[0] > s)
    return np.array(out, np.int64)


def detect_features(image, max_features: int = 2000, options=None, subdivisions: int = 5, min_distance: float = 10.0, ctx=None) -> Features:
    """FeatureSet::detect: kaze_detect, then the subsampling.  scale is the keypoint's diameter, angle in [0, 2 pi)."""
    kp = kaze_detect(image, options, ctx)
    if kp.status == CAP_REACHED:
        raise ValueError(f"image: more than {MAX_CANDIDATES} extremum candidates")
    h, w = (int(image.shape[0]), int(image.shape[1]))
    idx = subsample_features(kp, w, h, max_features, subdivisions, min_distance)
    return Features(np.column_stack([kp.x[idx], kp.y[idx]]), kp.size[idx], kp.angle[idx], kp.descriptors[idx].reshape(-1, 64))


# ----------------------------------------------------------------------------------------------------------------------- files
def _bool(v) -> bool:
    return str(v).strip().lower() in ("1", "true", "yes", "on")


def match_workdir(workdir, config=None, ctx=None) -> int:
    """wass_match up to matches_unfiltered.txt (wass_match.cpp:170-250): reads undistorted/0000000{0,1}.png of `workdir`, detects and
    subsamples the features of both, matches them and writes matches_unfiltered.txt; prints [P|10|100] and [P|20|100].  config: a
    KEY=value file with the FEATURE_*, NUM_FEATURES_PER_IMAGE, AREA_SUBDIVISION and MATCHER_* keys.  Returns 0, or -1 with one line on
    stderr: on a missing file, and where the detector or the matcher refuses its input (a picture without features, one smaller than
    the derivatives' reach, options out of range), as the reference catches its extractor's and matcher's exceptions
    (wass_match.cpp:363-371).  matches_unfiltered.txt is written only after the matcher has returned.  epipolar.filter_workdir
    finishes the job."""
    from . import epipolar
    from PIL import Image
    wd = os.fspath(workdir)
    try:
        cfg = epipolar.read_config(config) if config is not None else {}
    except OSError as ex:
        print(f"wass_amd.features: {ex}", file=sys.stderr)
        return -1
    opts = KazeOptions(float(cfg.get("FEATURE_HESSIAN_THRESHOLD", 1e-4)), int(cfg.get("FEATURE_N_OCTAVES", 4)), int(cfg.get("FEATURE_N_LAYERS", 4)))
    feats = []
    for cam, mark in ((0, "[P|10|100]"), (1, "[P|20|100]")):
        path = os.path.join(wd, "undistorted", "%08d.png" % cam)
        try:
            with Image.open(path) as im:
                img = np.asarray(im.convert("L"), np.uint8)
        except OSError:
            print(f"Unable to open undistorted/{cam:08d}.png", file=sys.stderr)
            return -1
        print(mark, flush=True)
        try:
            feats.append(detect_features(img, int(cfg.get("NUM_FEATURES_PER_IMAGE", 2000)), opts, int(cfg.get("AREA_SUBDIVISION", 5)),
                                         float(cfg.get("FEATURE_MIN_DISTANCE", 10.0)), ctx))
        except (ValueError, RuntimeError) as ex:
            print(f"wass_amd.features: undistorted/{cam:08d}.png: {ex}", file=sys.stderr)
            return -1
    try:
        r = _match.gt_match(feats[0], feats[1], lam=float(cfg.get("MATCHER_LAMBDA", 1e-5)),
                            pop_threshold=float(cfg.get("MATCHER_POPULATION_THRESHOLD", 0.7)), min_group_size=int(cfg.get("MATCHER_MIN_GROUP_SIZE", 5)),
                            max_rounds=int(cfg.get("MATCHER_MAX_ROUNDS", 20)), skip_gt=_bool(cfg.get("MATCHER_SKIP_GT", "false")), ctx=ctx)
    except (ValueError, RuntimeError) as ex:
        print(f"wass_amd.features: {len(feats[0])} and {len(feats[1])} features: {ex}", file=sys.stderr)
        return -1
    _match.write_matches(os.path.join(wd, "matches_unfiltered.txt"), r)
    return 0


def main(argv=None) -> int:
    argv = sys.argv[1:] if argv is None else list(argv)
    if not 1 <= len(argv) <= 2:
        print("usage: python -m wass_amd.features WORKDIR [CONFIG]", file=sys.stderr)
        return -1
    if not os.path.isdir(argv[0]):
        print(f"{argv[0]} does not exist, aborting.", file=sys.stderr)
        return -1
    return match_workdir(argv[0], argv[1] if len(argv) > 1 else None)


if __name__ == "__main__":
    sys.exit(main())
