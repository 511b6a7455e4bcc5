"""Drop-in interpolators of the reference's gridding tool (gridding/wassgridsurface), on the GPU.

    from wass_amd.gridding import DCTInterpolator      # instead of: from DCTInterpolator import DCTInterpolator

DCTInterpolator(img_width, img_height, alg_options)(I) returns (Irec float32, ones float32) like the reference's class, with its
option names and defaults (Nfreqs 150, MAX_ITERS 500, TOLERANCE_CHANGE 1e-4, REGULARIZER_ALPHA 8e-7, LEARNING_RATE 5.0).
Differences: the caller's I is not modified (the reference zeroes its NaN cells in place); the start value is a seeded
uniform [0, 1) draw, not torch.rand's stream; a rectangular grid is solved (the reference raises a shape error).

grid_sequence(wass_frames, gridsetup, ...) is the tool's `--action grid` for `--ia DCT` (wassgridsurface.py:235-591) without the
file output: every frame's mesh_cam.xyzC binned, solved (several frames per set of launches), masked, median filtered (mf),
turned into the millimetre cube, with the sequence's zmin / zmax / zmean, the per-point mean and the force_zero_mean pass.
load_camera_mesh(path) is the reference's mesh_cam.xyzC reader (wass_utils.py:22-35).
"""
from __future__ import annotations

import dataclasses
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from .stereo import Context, GridSequence, grid_setup

_DEFAULTS = {"Nfreqs": 150, "MAX_ITERS": 500, "TOLERANCE_CHANGE": 1e-4, "REGULARIZER_ALPHA": 8e-7, "LEARNING_RATE": 5.0}


class DCTInterpolator:
    def __init__(self, img_width, img_height, alg_options=None, ctx: Context | None = None, seed: int = 0):
        self.width, self.height = int(img_width), int(img_height)
        self.options = {k: ((alg_options or {}).get(k) if (alg_options or {}).get(k) is not None else v) for k, v in _DEFAULTS.items()}
        self.Nfreqs = self.options["Nfreqs"]
        self.MAX_ITERS = self.options["MAX_ITERS"]
        self.TOLERANCE_CHANGE = self.options["TOLERANCE_CHANGE"]
        self.REGULARIZER_ALPHA = self.options["REGULARIZER_ALPHA"]
        self.LEARNING_RATE = self.options["LEARNING_RATE"]
        self._ctx = ctx
        self.seed = seed
        self.last_info = None

    def __call__(self, I, verbose=True):
        I = np.asarray(I)
        if I.shape != (self.height, self.width):
            raise ValueError(f"cell map of shape {I.shape}, the interpolator was made for {(self.height, self.width)}")
        if self._ctx is None:
            self._ctx = Context(0)
        Irec, _, info = self._ctx.grid_dct(I, self.options, seed=self.seed)
        self.last_info = info
        if verbose:
            print("DCT interpolator: %d steps%s, data loss %.6g, |x|_1 %.6g, last max delta %.6g"
                  % (info["steps"], " (tolerance reached)" if info["converged"] else "", info["data_loss"], info["reg_loss"], info["fdelta"]))
        return Irec, np.ones((self.height, self.width), np.float32)


def load_camera_mesh(meshfile) -> np.ndarray:
    """mesh_cam.xyzC -> 3 x N float64 points in camera space, with the arithmetic of the reference's reader (wass_utils.py:22-35):
    uint32 N, six doubles of limits (scale xyz, offset xyz), Rinv (3 x 3), Tinv (3), then N uint16 triples; the triples are taken
    to float32, divided by the scales and shifted by the offsets (float64 from there on, numpy's promotion), then Rinv p + Tinv."""
    with open(meshfile, "rb") as f:
        raw = f.read()
    npts = int(np.frombuffer(raw, "<u4", 1)[0])
    head = np.frombuffer(raw, "<f8", 18, offset=4)
    scale, shift = head[0:3].reshape(3, 1), head[3:6].reshape(3, 1)
    Rinv, Tinv = head[6:15].reshape(3, 3), head[15:18].reshape(3, 1)
    q = np.frombuffer(raw, "<u2", 3 * npts, offset=4 + 18 * 8).reshape(npts, 3).T       # 3 x N, a point per column
    pts = q.astype(np.float32) / scale + shift
    return Rinv @ pts + Tinv


def upload_camera_mesh(ctx: Context, pts: np.ndarray):
    """A 3 x N cloud as an N x 1 device mesh (every point valid); an empty cloud becomes one invalid point."""
    n = pts.shape[1]
    if n == 0:
        return ctx.mesh_upload(np.zeros((1, 1), np.uint8), np.zeros((1, 1, 3)))
    return ctx.mesh_upload(np.ones((1, n), np.uint8), np.ascontiguousarray(pts.T).reshape(1, n, 3))


@dataclasses.dataclass
class GridSequenceResult:
    """What the reference hands to its NetCDF writer, frame by frame and at the end."""
    Z: np.ndarray                   # count x height x width float32, millimetres (NaN outside the mask)
    time: np.ndarray                # idx / fps per frame (0 without fps)
    workdir: np.ndarray             # the integer of NNNNNN_wd per frame
    zmin: float
    zmax: float
    zmean: float
    mean_perpoint_mm: np.ndarray    # height x width float64
    dct_info: list                  # per frame: steps, converged, data_loss, reg_loss, fdelta
    empty_frames: list              # indices of the frames whose cloud left no point on the grid
    frame_mean: np.ndarray
    frame_min: np.ndarray
    frame_max: np.ndarray


def _scalar(v) -> float:
    return float(np.ravel(np.asarray(v))[0])


def grid_sequence(wass_frames, gridsetup, mf: int = 0, user_mask=None, alg_options=None, force_zero_mean: bool = False,
                  batch: int = 8, cell: str = "median", ctx: Context | None = None, out=None) -> GridSequenceResult:
    """wassgridsurface --action grid with --ia DCT on the GPU.  wass_frames: the NNNNNN_wd directories in sequence order (each
    holds mesh_cam.xyzC); gridsetup: a mapping with the reference's config.mat keys (Rpl, Tpl, CAM_BASELINE, xmin, xmax, ymin,
    ymax, XX or Nx and Ny, fps) or the path of that file; mf: 0, 3 or 5 (--mf); user_mask: height x width, cells where it is 0
    become NaN; alg_options: the DCT options by the reference's names; batch: frames per DCT solve -- 8 by default: in the
    measurement of DESIGN.md ("The DCT interpolator of row f3") the time per frame stops falling there; cell: "median" or
    "mean", the statistic of a grid cell (grid.hip; the reference's random sub-sampling is not reproduced); out: a
    count x height x width float32 array or np.memmap for the cube (default: a new array)."""
    import torch
    if isinstance(gridsetup, (str, os.PathLike)):
        import scipy.io
        gridsetup = scipy.io.loadmat(os.fspath(gridsetup))
    if "XX" in gridsetup:
        H, W = np.asarray(gridsetup["XX"]).shape
    else:
        W, H = int(_scalar(gridsetup["Nx"])), int(_scalar(gridsetup["Ny"]))
    fps = _scalar(gridsetup["fps"]) if "fps" in gridsetup else 0.0
    gs = grid_setup(gridsetup["Rpl"], gridsetup["Tpl"], _scalar(gridsetup["CAM_BASELINE"]), _scalar(gridsetup["xmin"]),
                    _scalar(gridsetup["xmax"]), _scalar(gridsetup["ymin"]), _scalar(gridsetup["ymax"]), W, H)
    frames = [os.fspath(f) for f in wass_frames]
    count, batch = len(frames), max(1, int(batch))
    if count == 0:
        raise ValueError("no frames")
    if mf not in (0, 3, 5):
        raise ValueError(f"mf = {mf}: 0, 3 or 5 (cv.medianBlur, which the reference calls, takes no other size for float32)")
    if out is None:
        out = np.empty((count, H, W), np.float32)
    elif out.shape != (count, H, W) or out.dtype != np.float32:
        raise ValueError(f"out: a float32 array of shape {(count, H, W)} expected")
    if ctx is None:
        ctx = Context(0)
    dev = torch.device("cuda", ctx.device_id)
    nb_max = min(batch, count)
    d_cells = torch.empty((nb_max, H, W), dtype=torch.float32, device=dev)
    d_grid, d_filt, d_mm = torch.empty_like(d_cells), torch.empty_like(d_cells), torch.empty_like(d_cells)
    d_mask = None
    if user_mask is not None:
        d_mask = torch.from_numpy((np.asarray(user_mask).reshape(H, W) > 0).astype(np.uint8)).to(dev)
    torch.cuda.synchronize(dev)                                  # from here on the buffers are used on the context's stream
    seq = GridSequence(ctx, W, H)
    infos, empty = [], []
    try:
        with ThreadPoolExecutor(max_workers=min(nb_max, 8)) as pool:
            for i0 in range(0, count, batch):
                paths = frames[i0:i0 + batch]
                nb = len(paths)
                clouds = list(pool.map(lambda d: load_camera_mesh(os.path.join(d, "mesh_cam.xyzC")), paths))
                meshes = []
                for k, pts in enumerate(clouds):
                    meshes.append(upload_camera_mesh(ctx, pts))
                    meshes[-1].grid_cells_dev(gs, d_cells[k], cell)
                info, status = ctx.grid_dct_batch_dev(d_cells[:nb], d_grid[:nb], alg_options, d_user_mask=d_mask)
                for m in meshes:                                 # the solve has synchronised: the binning has read them
                    m.close()
                d_zi = d_grid
                if mf:
                    ctx.grid_median_dev(d_grid[:nb], d_filt[:nb], mf, d_mask)
                    d_zi = d_filt
                seq.push_dev(d_zi[:nb], d_mm[:nb])
                out[i0:i0 + nb] = d_mm[:nb].cpu().numpy()
                infos += info
                empty += [i0 + k for k in range(nb) if status[k] != 0]
        st = seq.finish(force_zero_mean)
        if force_zero_mean:
            for i0 in range(0, count, batch):
                nb = min(batch, count - i0)
                d_mm[:nb].copy_(torch.from_numpy(np.ascontiguousarray(out[i0:i0 + nb])))
                torch.cuda.synchronize(dev)
                seq.zero_mean_dev(d_mm[:nb])
                ctx.synchronize()
                out[i0:i0 + nb] = d_mm[:nb].cpu().numpy()
    finally:
        seq.close()
    idx = np.arange(count, dtype=np.float64)
    workdir = np.array([int(os.path.basename(os.path.normpath(f))[:-3]) for f in frames], np.int64)
    return GridSequenceResult(Z=out, time=idx / fps if fps > 0 else np.zeros(count), workdir=workdir, zmin=st["zmin"], zmax=st["zmax"],
                              zmean=st["zmean"], mean_perpoint_mm=st["mean_perpoint_mm"], dct_info=infos, empty_frames=empty,
                              frame_mean=st["frame_mean"], frame_min=st["frame_min"], frame_max=st["frame_max"])
