"""Drop-in interpolators of the reference's gridding tool (gridding/wassgridsurface), on the GPU.

    from wass_amd.gridding import DCTInterpolator      # instead of: from DCTInterpolator import DCTInterpolator

DCTInterpolator(img_width, img_height, alg_options)(I) returns (Irec float32, ones float32) like the reference's class, with its
option names and defaults (Nfreqs 150, MAX_ITERS 500, TOLERANCE_CHANGE 1e-4, REGULARIZER_ALPHA 8e-7, LEARNING_RATE 5.0).
Differences: the caller's I is not modified (the reference zeroes its NaN cells in place); the start value is a seeded
uniform [0, 1) draw, not torch.rand's stream; a rectangular grid is solved (the reference raises a shape error).

grid_sequence(wass_frames, gridsetup, ...) is the tool's `--action grid` for `--ia DCT` (wassgridsurface.py:235-591) without the
file output: every frame's mesh_cam.xyzC binned, solved (several frames per set of launches), masked, median filtered (mf),
turned into the millimetre cube, with the sequence's zmin / zmax / zmean, the per-point mean and the force_zero_mean pass.
With refine=RefineOptions(...) every frame's surface is also refined against its two pictures (wass_amd.refinement), where the
reference's grid() has the call commented out: after the filter, before the statistics.
load_camera_mesh(path) is the reference's mesh_cam.xyzC reader (wass_utils.py:22-35).

linear_nd(points, gridsetup) is `--ia LinearND` (wassgridsurface.py:437-482): the plane through the three cloud points of the
Delaunay triangle that holds a node, without a triangulation being built; grid_sequence(..., algorithm="LinearND") runs it per frame.

setup_grid(wdir, meanplane, baseline, ...) is the tool's `--action setup` (wassgridsurface.py:57-231): the dict of its config.mat
from the first frame of a sequence, with the quantiles of the aligned heights taken on the GPU; generate_gridconfig / read_gridconfig
are `--action generateconfig` and the reader of that file.  `python -m wass_amd.gridding WORKDIR OUTDIR --action ...` runs them
with the reference's option names.  The plots (area_grid.png, grid_projected_cam0.jpg), the JPEG and the NetCDF file stay out.
"""
from __future__ import annotations

import dataclasses
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from .stereo import Context, GridSequence, grid_setup, planes_mean_accumulate, planes_mean_finish

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
    refine_losses: list | None = None   # with refine: per frame the first and the last row [steps, data, smoothness, energy]
    linear_info: list | None = None     # LinearND: per frame {"counts": nodes per flag 0 .. 3, "n_taken": points taken}; None for DCT


def _scalar(v) -> float:
    return float(np.ravel(np.asarray(v))[0])


def _grid_setup_of(gridsetup):
    """(wass_grid_setup, H, W) of a mapping with the reference's config.mat keys or the path of that file"""
    if isinstance(gridsetup, (str, os.PathLike)):
        import scipy.io
        gridsetup = scipy.io.loadmat(os.fspath(gridsetup))
    if "XX" in gridsetup:
        H, W = np.asarray(gridsetup["XX"]).shape
    else:
        W, H = int(_scalar(gridsetup["Nx"])), int(_scalar(gridsetup["Ny"]))
    gs = grid_setup(gridsetup["Rpl"], gridsetup["Tpl"], _scalar(gridsetup["CAM_BASELINE"]), _scalar(gridsetup["xmin"]),
                    _scalar(gridsetup["xmax"]), _scalar(gridsetup["ymin"]), _scalar(gridsetup["ymax"]), W, H)
    return gs, H, W


def linear_nd(points, gridsetup_or_gs, ctx: Context | None = None, return_flags: bool = False, **options):
    """wassgridsurface --ia LinearND (:437-482): the cloud interpolated linearly over its Delaunay triangulation at the nodes of
    XX, YY = meshgrid(linspace(xmin, xmax, W), linspace(ymin, ymax, H)), what scipy.interpolate.LinearNDInterpolator(points[:2].T,
    points[2])(XX, YY) returns, without a triangulation being built (grid_linear.hip, DESIGN.md "LinearND").
    points: a 3 x N array (x, y, z rows, already aligned on the sea plane and in metres, as the reference's mesh_aligned) or a
    tuple of three float64 device tensors; gridsetup_or_gs: a wass_grid_setup (stereo.grid_setup; only the extent and the size are
    read), a mapping with the reference's config.mat keys, or the path of that file.  Points outside the closed extent, with a NaN
    or infinite coordinate, and all but the lowest index of equal (x, y) are not taken.
    Returns the float64 H x W surface; with return_flags also the uint8 H x W flags and the info dict of Context.grid_linear_dev:
      0  the node lies in a triangle whose circumcircle holds no other point, certified by fp64 determinants beyond their rounding
         bounds: the value is the plane through its three points
      1  certainly outside the convex hull: NaN (scipy's fill_value); also everywhere when fewer than three points are taken or
         all are collinear (info["status"] == -6)
      2  a triangle or a hull decision was found but not certified (cocircular points, a node on a hull edge within the
         bound): the value of the triangle found, or NaN.  grid_sequence keeps these values in the cube
      3  the walk reached its step cap: NaN, in the cube too."""
    import torch
    from . import _lib
    gs = gridsetup_or_gs if isinstance(gridsetup_or_gs, _lib.GridSetup) else _grid_setup_of(gridsetup_or_gs)[0]
    if ctx is None:
        ctx = Context(0)
    dev = torch.device("cuda", ctx.device_id)
    if isinstance(points, (tuple, list)) and len(points) == 3 and all(isinstance(t, torch.Tensor) for t in points):
        d_x, d_y, d_z = points
    else:
        pts = np.asarray(points, np.float64)
        if pts.ndim != 2 or pts.shape[0] != 3:
            raise ValueError("points: a 3 x N array expected")
        d_x, d_y, d_z = (torch.from_numpy(np.ascontiguousarray(pts[k])).to(dev) for k in range(3))
    d_out = torch.empty((gs.height, gs.width), dtype=torch.float64, device=dev)
    d_flags = torch.empty((gs.height, gs.width), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)                                  # the tensors are used on the context's stream from here on
    info = ctx.grid_linear_dev(d_x, d_y, d_z, gs, d_out, d_flags, **options)
    out = d_out.cpu().numpy()
    return (out, d_flags.cpu().numpy(), info) if return_flags else out


def _zero_mean_pass(ctx, seq, out, nb_max):
    """--force-zero-mean after seq.finish: the cube goes through seq.zero_mean_dev in slices of nb_max frames"""
    import torch
    count, H, W = out.shape
    dev = torch.device("cuda", ctx.device_id)
    d_mm = torch.empty((nb_max, H, W), dtype=torch.float32, device=dev)
    for i0 in range(0, count, nb_max):
        nb = min(nb_max, count - i0)
        d_mm[:nb].copy_(torch.from_numpy(np.ascontiguousarray(out[i0:i0 + nb])))
        torch.cuda.synchronize(dev)
        seq.zero_mean_dev(d_mm[:nb])
        ctx.synchronize()
        out[i0:i0 + nb] = d_mm[:nb].cpu().numpy()


def _sequence_result(frames, fps, out, st, **more) -> GridSequenceResult:
    count = len(frames)
    idx = np.arange(count, dtype=np.float64)
    workdir = np.array([int(os.path.basename(os.path.normpath(f))[:-3]) for f in frames], np.int64)
    return GridSequenceResult(Z=out, time=idx / fps if fps > 0 else np.zeros(count), workdir=workdir, zmin=st["zmin"], zmax=st["zmax"],
                              zmean=st["zmean"], mean_perpoint_mm=st["mean_perpoint_mm"], frame_mean=st["frame_mean"],
                              frame_min=st["frame_min"], frame_max=st["frame_max"], **more)


def _grid_sequence_linear(frames, gs, H, W, fps, user_mask, force_zero_mean, ctx, out) -> GridSequenceResult:
    """The LinearND branch of grid_sequence: per frame load, upload, Mesh.grid_linear_dev, one rounding to float32, push; it shares
    with the DCT branch the sequence handle's statistics, the zero-mean pass and the result."""
    import torch
    dev = torch.device("cuda", ctx.device_id)
    d_out = torch.empty((H, W), dtype=torch.float64, device=dev)
    d_flags = torch.empty((H, W), dtype=torch.uint8, device=dev)
    d_zi, d_mm = torch.empty((1, H, W), dtype=torch.float32, device=dev), torch.empty((1, H, W), dtype=torch.float32, device=dev)
    d_off = None
    if user_mask is not None:
        d_off = torch.from_numpy(~(np.asarray(user_mask).reshape(H, W) > 0)).to(dev)
    torch.cuda.synchronize(dev)                                  # from here on the buffers are used on the context's stream
    infos, empty = [], []
    seq = GridSequence(ctx, W, H)
    try:
        for i, d in enumerate(frames):
            mesh = upload_camera_mesh(ctx, load_camera_mesh(os.path.join(d, "mesh_cam.xyzC")))
            try:
                info = mesh.grid_linear_dev(gs, d_out, d_flags)  # returns after the stream has run
            finally:
                mesh.close()
            d_zi[0] = d_out.to(torch.float32)                    # the one rounding fp64 -> float32; flag-3 cells are NaN already
            if d_off is not None:
                d_zi[0][d_off] = float("nan")
            torch.cuda.synchronize(dev)
            seq.push_dev(d_zi, d_mm)
            out[i] = d_mm[0].cpu().numpy()
            infos.append({"counts": info["counts"], "n_taken": info["n_taken"]})
            if info["status"] != 0:
                empty.append(i)
        st = seq.finish(force_zero_mean)
        if force_zero_mean:
            _zero_mean_pass(ctx, seq, out, 1)
    finally:
        seq.close()
    return _sequence_result(frames, fps, out, st, dct_info=[], empty_frames=empty, linear_info=infos)


def grid_sequence(wass_frames, gridsetup, mf: int = 0, user_mask=None, alg_options=None, force_zero_mean: bool = False,
                  batch: int = 8, cell: str = "median", ctx: Context | None = None, out=None, refine=None,
                  algorithm: str = "DCT") -> GridSequenceResult:
    """wassgridsurface --action grid with --ia DCT (the default) or --ia LinearND on the GPU.  algorithm="LinearND": every frame
    goes through load, upload and Mesh.grid_linear_dev (linear_nd has the definition and the flags), is rounded once from fp64 to
    float32 and pushed like a DCT frame; the cube keeps the values of flag-2 cells and holds NaN at flag-1 and flag-3 cells.
    linear_info has per frame the nodes per flag and the points taken, dct_info is empty, empty_frames lists the frames with fewer
    than three points (or all collinear).  The reference applies neither the user mask nor --mf in this branch: here user_mask is
    applied (cells to NaN), and mf != 0 or refine raise ValueError.  alg_options, batch and cell are not used.
    What follows describes algorithm="DCT".  wass_frames: the NNNNNN_wd directories in sequence order (each
    holds mesh_cam.xyzC); gridsetup: a mapping with the reference's config.mat keys (Rpl, Tpl, CAM_BASELINE, xmin, xmax, ymin,
    ymax, XX or Nx and Ny, fps) or the path of that file; mf: 0, 3 or 5 (--mf); user_mask: height x width, cells where it is 0
    become NaN; alg_options: the DCT options by the reference's names; batch: frames per DCT solve -- 8 by default: in the
    measurement of DESIGN.md ("The DCT interpolator of row f3") the time per frame stops falling there; cell: "median" or
    "mean", the statistic of a grid cell (grid.hip; the reference's random sub-sampling is not reproduced); out: a
    count x height x width float32 array or np.memmap for the cube (default: a new array); refine: None, or a
    wass_amd.refinement.RefineOptions: every frame's surface is refined against undistorted/00000000.png and 00000001.png of its
    directory (refinement.SequenceRefiner, refine.batch frames per set of launches) after the solve, the user mask and the
    filter, so the cube and every statistic see the refined surface; gridsetup then needs P0cam, P1cam, XX, YY as well, which
    setup_grid writes.  The reference's alpha = 10 holds the surface to 0 along the grid's border (RefineOptions has the pointer)."""
    import torch
    if isinstance(gridsetup, (str, os.PathLike)):
        import scipy.io
        gridsetup = scipy.io.loadmat(os.fspath(gridsetup))
    gs, H, W = _grid_setup_of(gridsetup)
    fps = _scalar(gridsetup["fps"]) if "fps" in gridsetup else 0.0
    frames = [os.fspath(f) for f in wass_frames]
    count, batch = len(frames), max(1, int(batch))
    if count == 0:
        raise ValueError("no frames")
    if mf not in (0, 3, 5):
        raise ValueError(f"mf = {mf}: 0, 3 or 5 (cv.medianBlur, which the reference calls, takes no other size for float32)")
    if algorithm not in ("DCT", "LinearND"):
        raise ValueError(f"algorithm = {algorithm!r}: DCT or LinearND")
    linear = algorithm == "LinearND"
    if linear and (mf != 0 or refine is not None):
        raise ValueError("algorithm LinearND takes neither mf nor refine: the reference's LinearND branch applies no median filter "
                         "and no refinement")
    if out is None:
        out = np.empty((count, H, W), np.float32)
    elif out.shape != (count, H, W) or out.dtype != np.float32:
        raise ValueError(f"out: a float32 array of shape {(count, H, W)} expected")
    pictures = None
    if refine is not None:
        pictures = _refine_inputs(frames, gridsetup, H, W)       # raises before anything touches the device
    if ctx is None:
        ctx = Context(0)
    if linear:
        return _grid_sequence_linear(frames, gs, H, W, fps, user_mask, force_zero_mean, ctx, out)
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
    refiner, traces = None, None
    try:
        if refine is not None:
            from .refinement import SequenceRefiner
            rb = max(1, min(int(refine.batch), nb_max))
            refiner, traces = SequenceRefiner(gridsetup, pictures, rb, ctx), []
            d_ref = torch.empty_like(d_cells)
        with ThreadPoolExecutor(max_workers=min(nb_max, 8)) as pool:
            for i0 in range(0, count, batch):
                paths = frames[i0:i0 + batch]
                nb = len(paths)
                views = pool.map(_load_pictures, paths) if refiner is not None else None      # decoded beside the meshes and the solve
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
                if refiner is not None:
                    views = list(views)
                    for k0 in range(0, nb, refiner.batch):
                        k = slice(k0, min(nb, k0 + refiner.batch))
                        refiner.refine(d_zi[k], np.stack([v[0] for v in views[k]]), np.stack([v[1] for v in views[k]]), refine,
                                       out=d_ref[k], first_frame=i0 + k0)
                        traces += [[t[0].tolist(), t[-1].tolist()] for t in refiner.losses]
                    d_zi = d_ref
                seq.push_dev(d_zi[:nb], d_mm[:nb])
                out[i0:i0 + nb] = d_mm[:nb].cpu().numpy()
                infos += info
                empty += [i0 + k for k in range(nb) if status[k] != 0]
        st = seq.finish(force_zero_mean)
        if force_zero_mean:
            _zero_mean_pass(ctx, seq, out, nb_max)
    finally:
        seq.close()
        if refiner is not None:
            refiner.close()
    return _sequence_result(frames, fps, out, st, dct_info=infos, empty_frames=empty, refine_losses=traces)


REFINE_KEYS = ("Rpl", "Tpl", "CAM_BASELINE", "P0cam", "P1cam", "XX", "YY")
REFINE_PICTURES = ("00000000.png", "00000001.png")


def _load_pictures(framedir):
    """the two undistorted pictures of a frame directory as uint8 grey"""
    from PIL import Image
    out = []
    for name in REFINE_PICTURES:
        with Image.open(os.path.join(framedir, "undistorted", name)) as im:
            out.append(np.asarray(im.convert("L"), np.uint8))
    return out


def _refine_inputs(frames, gridsetup, H, W):
    """What grid_sequence(refine=...) needs beyond the meshes, checked without a device: the keys of gridsetup (ValueError naming
    the missing ones), both pictures of every frame (FileNotFoundError naming the file) and one size per camera over the
    sequence (ValueError naming the first frame that differs).  Returns ((ih0, iw0), (ih1, iw1)); only the headers are read."""
    from PIL import Image
    missing = [k for k in REFINE_KEYS if k not in gridsetup]
    if missing:
        raise ValueError("refine: gridsetup lacks " + ", ".join(missing) + " (setup_grid writes them)")
    for k in ("XX", "YY"):
        if tuple(np.asarray(gridsetup[k]).shape) != (H, W):
            raise ValueError(f"refine: {k} of shape {tuple(np.asarray(gridsetup[k]).shape)}, the grid is {(H, W)}")
    sizes = [None, None]
    for d in frames:
        for cam, name in enumerate(REFINE_PICTURES):
            path = os.path.join(d, "undistorted", name)
            if not os.path.isfile(path):
                raise FileNotFoundError(f"refine: {path} is missing")
            with Image.open(path) as im:
                size = (im.size[1], im.size[0])
            if sizes[cam] is None:
                sizes[cam] = size
            elif size != sizes[cam]:
                raise ValueError(f"refine: {path} of frame {d} is {size[0]} x {size[1]}, the pictures of camera {cam} before it are "
                                 f"{sizes[cam][0]} x {sizes[cam][1]}")
    return tuple(sizes)


# ---------------------------------------------------------------------------------------------------------------- grid set-up
GRIDCONFIG_DEFAULTS = (("area_center_x", "0.0"), ("area_center_y", "-35.0"), ("area_size", "50"), ("N", "1024"))
# every key of the reference's savemat call (wassgridsurface.py:194-231), in its order
CONFIG_MAT_KEYS = ("xmin", "xmax", "ymin", "ymax", "zmin", "zmax", "P0cam", "P1cam", "Hcam0toGrid", "Hcam1toGrid", "Cam0toGrid", "Cam1toGrid",
                   "Hcam0toTexture", "Nx", "Ny", "N", "R", "T", "RTplane", "K0", "K1", "Rpl", "Tpl", "P0plane", "P1plane", "CAM_BASELINE",
                   "scale", "XX", "YY", "KX_ab", "KY_ab", "spec_scale", "x_spacing", "y_spacing", "fps", "timestring")


def generate_gridconfig(outdir) -> str:
    """`--action generateconfig` (:650-661): writes <outdir>/gridconfig.txt with the reference's defaults and returns its path."""
    path = os.path.join(os.fspath(outdir), "gridconfig.txt")
    with open(path, "w") as f:
        f.write("[Area]\n")
        for k, v in GRIDCONFIG_DEFAULTS:
            f.write(f"{k}={v}\n")
    return path


def read_gridconfig(path) -> dict:
    """The [Area] section of a gridconfig.txt: area_center (2 floats), area_size_x, area_size_y, Nx, Ny.  As in the reference
    (:697-718) a pair is taken only when both of its options are there (area_size_x and area_size_y, Nx and Ny); otherwise the
    single option (area_size, N) stands for both."""
    import configparser
    parser = configparser.ConfigParser()
    if not parser.read(os.fspath(path)):
        raise FileNotFoundError(os.fspath(path))
    area = parser["Area"]

    def pair(first, second, single, convert):
        if first in area and second in area:
            return convert(area[first]), convert(area[second])
        both = convert(area[single])
        return both, both

    size_x, size_y = pair("area_size_x", "area_size_y", "area_size", float)
    nx, ny = pair("Nx", "Ny", "N", int)
    return {"area_center": np.array([float(area["area_center_x"]), float(area["area_center_y"])]),
            "area_size_x": size_x, "area_size_y": size_y, "Nx": nx, "Ny": ny}


def mean_plane(planes) -> np.ndarray:
    """np.nanmean(planes, axis=0) of a sequence's planes.txt (:672-678): the path of the file or an n x 4 array."""
    if isinstance(planes, (str, os.PathLike)):
        planes = np.loadtxt(os.fspath(planes))
    planes = np.asarray(planes, np.float64).reshape(-1, 4)
    mean, n = planes_mean_finish(planes_mean_accumulate(planes))
    if n == 0:
        raise ValueError("planes: no row without a NaN")
    return mean


def read_opencv_matrix(path, node: str) -> np.ndarray:
    """The matrix <node> of an OpenCV FileStorage XML file (intrinsics_0000000X.xml has `intr`): rows, cols, dt d (float64) or f
    (float32), the data on one or several lines.  What cv.FileStorage(...).getNode(node).mat() returns for such a node."""
    import re
    with open(os.fspath(path)) as f:
        text = f.read()
    m = re.search(r"<%s(\s[^>]*)?>(.*?)</%s>" % (re.escape(node), re.escape(node)), text, re.S)
    if m is None or "<opencv_storage>" not in text:
        raise ValueError(f"{path}: no node <{node}> in an <opencv_storage>")
    body = m.group(2)

    def field(name):
        f = re.search(r"<%s>(.*?)</%s>" % (name, name), body, re.S)
        if f is None:
            raise ValueError(f"{path}: <{node}> has no <{name}>")
        return f.group(1).strip()

    rows, cols, dt = int(field("rows")), int(field("cols")), field("dt")
    if dt not in ("d", "f"):
        raise ValueError(f"{path}: <{node}> has dt {dt!r}; d or f expected")
    vals = np.array(field("data").split(), np.float64)
    if vals.size != rows * cols:
        raise ValueError(f"{path}: <{node}> holds {vals.size} numbers for {rows} x {cols}")
    return vals.reshape(rows, cols).astype(np.float64 if dt == "d" else np.float32)


def homography_4pt(src, dst) -> np.ndarray:
    """The homography that takes four points onto four points (4 x 2 each), H[2, 2] = 1: what cv.findHomography returns for four
    correspondences (its normalised DLT, no refinement), to rounding.  Both sets are cast to float32 first, as the reference's call
    does, and the system is solved in fp64.  Three collinear points on either side raise ValueError."""
    src = np.asarray(src, np.float32).astype(np.float64)
    dst = np.asarray(dst, np.float32).astype(np.float64)
    if src.shape != (4, 2) or dst.shape != (4, 2):
        raise ValueError("homography_4pt: 4 x 2 points each way expected")
    if not (np.isfinite(src).all() and np.isfinite(dst).all()):
        raise ValueError("homography_4pt: non-finite point")

    def normalise(p, what):
        c = p.mean(axis=0)
        s = np.abs(p - c).mean(axis=0)
        if not (s > 0).all():
            raise ValueError(f"homography_4pt: the {what} points are collinear")
        s = 1.0 / s
        q = (p - c) * s
        for i, j, k in ((0, 1, 2), (0, 1, 3), (0, 2, 3), (1, 2, 3)):
            a, b = q[j] - q[i], q[k] - q[i]
            if abs(a[0] * b[1] - a[1] * b[0]) <= 1e-9:      # twice the triangle's area, in units of the points' own spread
                raise ValueError(f"homography_4pt: three of the {what} points are collinear")
        return q, np.array([[s[0], 0, -c[0] * s[0]], [0, s[1], -c[1] * s[1]], [0, 0, 1.0]])

    p, Tp = normalise(src, "source")
    q, Tq = normalise(dst, "target")
    A = np.zeros((8, 9))
    for i in range(4):
        x, y, u, v = p[i, 0], p[i, 1], q[i, 0], q[i, 1]
        A[2 * i] = [x, y, 1, 0, 0, 0, -u * x, -u * y, -u]
        A[2 * i + 1] = [0, 0, 0, x, y, 1, -v * x, -v * y, -v]
    h = np.linalg.svd(A)[2][-1].reshape(3, 3)
    H = np.linalg.inv(Tq) @ h @ Tp
    if H[2, 2] == 0 or not np.isfinite(H).all():
        raise ValueError("homography_4pt: degenerate correspondences")
    return H / H[2, 2]


def sea_plane_RT(plane):
    """Rpl (3 x 3) and Tpl (3 x 1) of a plane a x + b y + c z + d = 0: the rotation that turns its normal onto the z axis and the
    shift by d along it, what the reference's compute_sea_plane_RT returns.  The library's wass_RT_from_plane holds the arithmetic."""
    from .stereo import RT_from_plane
    rot, shift, _, _ = RT_from_plane([float(v) for v in np.ravel(plane)])
    return rot, shift.reshape(3, 1)


def _four_by_four(m34) -> np.ndarray:
    return np.vstack((np.asarray(m34, np.float64).reshape(3, 4), [0.0, 0.0, 0.0, 1.0]))


def setup_algebra(K0, K1, R, T, P0cam, P1cam, meanplane, baseline, area_center, area_size_x, area_size_y, Nx, Ny, Iw, Ih, z_q02, z_q98,
                  fps=0, timestring="") -> dict:
    """Everything the set-up derives once the files are read and the 2 % / 98 % quantiles of the aligned heights are known: the
    values of the reference's config.mat (CONFIG_MAT_KEYS), from its expressions with its association of the matrix products
    (wassgridsurface.py:82-174), so that the numbers are the reference's.  Raises ValueError where the reference asserts that the
    grid spacings along x and y agree to 1e-2."""
    Nx, Ny = int(Nx), int(Ny)
    intrinsics = (np.asarray(K0), np.asarray(K1))
    projections = (_four_by_four(P0cam), _four_by_four(P1cam))
    Rpl, Tpl = sea_plane_RT(meanplane)
    # plane frame -> camera frame (the inverse of the alignment), pixels -> the square [-1, 1]^2, metres with z up -> plane frame
    cam_from_plane = np.vstack((np.hstack((Rpl.T, -Rpl.T @ Tpl)), [0, 0, 0, 1]))
    unit_from_pixel = np.array([[2.0 / Iw, 0, -1, 0], [0, 2.0 / Ih, -1, 0], [0, 0, 1, 0], [0, 0, 0, 1]], dtype=float)
    per_metre = 1.0 / baseline
    plane_from_grid = np.diag((per_metre, per_metre, -per_metre, 1))
    plane_projection, cam_to_grid = [], []
    for K, P in zip(intrinsics, projections):
        plane_projection.append(unit_from_pixel @ P @ cam_from_plane @ plane_from_grid)
        K44 = np.eye(4)
        K44[:3, :3] = K
        cam_to_grid.append(np.linalg.inv(plane_from_grid) @ np.linalg.inv(cam_from_plane) @ np.linalg.inv(np.linalg.inv(K44) @ P))
    # the extent, and a height range symmetric about 0 that keeps the larger magnitude
    half = (area_size_x / 2, area_size_y / 2)
    lo = [area_center[k] - half[k] for k in (0, 1)]
    hi = [area_center[k] + half[k] for k in (0, 1)]
    zmax, zmin = z_q98 * 1.5, z_q02 * 1.5
    if abs(zmax) > abs(zmin):
        zmin = -zmax
    else:
        zmax = -zmin
    # the four corners of the extent at height 0, where each camera sees them, and the homographies between the two
    corners = np.array([[lo[0], lo[1]], [hi[0], lo[1]], [hi[0], hi[1]], [lo[0], hi[1]]], dtype=float)
    corners_h = np.vstack((corners.T, np.zeros(4), np.ones(4)))
    pixel_from_unit = np.linalg.inv(unit_from_pixel)
    to_grid = []
    for Pp in plane_projection:
        seen = pixel_from_unit @ Pp @ corners_h
        seen /= seen[2, :]
        to_grid.append((seen[:2, :].T, homography_4pt(seen[:2, :].T, corners)))
    to_texture = homography_4pt(to_grid[0][0], np.array([[0, 0], [Nx, 0], [Nx, Ny], [0, Ny]], dtype=np.float32))
    # cell centres and the wavenumber axes of the grid's FFT
    XX, YY = np.meshgrid(np.linspace(lo[0], hi[0], Nx), np.linspace(lo[1], hi[1], Ny))
    dx, dy = XX[0, 1] - XX[0, 0], YY[1, 0] - YY[0, 0]
    if not abs(dx - dy) < 1e-2:
        raise ValueError(f"grid spacing {dx} along x and {dy} along y: they must agree to 1e-2")
    kx = np.arange(-(Nx // 2), Nx // 2, dtype=np.float64) / Nx * (2.0 * np.pi / dx)
    ky = np.arange(-(Ny // 2), Ny // 2, dtype=np.float64) / Ny * (2 * np.pi / dy)
    KX, KY = np.meshgrid(kx, ky)
    out = {"xmin": lo[0], "xmax": hi[0], "ymin": lo[1], "ymax": hi[1], "zmin": zmin, "zmax": zmax,
           "Nx": Nx, "Ny": Ny, "N": max(Nx, Ny), "XX": XX, "YY": YY, "x_spacing": dx, "y_spacing": dy,
           "KX_ab": KX, "KY_ab": KY, "spec_scale": 1.0 / (Nx * Ny),
           "R": np.asarray(R), "T": np.asarray(T), "Rpl": Rpl, "Tpl": Tpl, "RTplane": cam_from_plane,
           "CAM_BASELINE": baseline, "scale": baseline, "fps": fps, "timestring": timestring,
           "Hcam0toTexture": to_texture}
    for cam in (0, 1):
        out.update({f"K{cam}": intrinsics[cam], f"P{cam}cam": projections[cam][0:3, :], f"P{cam}plane": plane_projection[cam],
                    f"Cam{cam}toGrid": cam_to_grid[cam], f"Hcam{cam}toGrid": to_grid[cam][1]})
    return out


class ImageSizeUnknown(ValueError):
    """setup_grid has neither Iw / Ih nor undistorted/00000000.png to read them from"""


def setup_grid(wdir, meanplane, baseline, area_center, area_size_x, area_size_y, Nx, Ny, Iw=None, Ih=None, fps=0, timestring="",
               ctx: Context | None = None, outdir=None) -> dict:
    """wassgridsurface --action setup (:57-231) on the first frame's directory wdir: reads its calibration (intrinsics_0000000X.xml,
    Cam0_poseR/T.txt, P0cam.txt, P1cam.txt) and mesh_cam.xyzC, takes the 2 % and 98 % quantiles of the heights aligned on
    meanplane on the GPU (Mesh.aligned_z_quantiles) and returns the dict of the reference's config.mat (CONFIG_MAT_KEYS), which
    grid_sequence and the wass_amd.postproc functions take.  Two keys more: cam0_rectified, the Ny x Nx uint8 picture of camera 0
    warped onto the grid (None without undistorted/00000000.png), and coverage, the fraction of grid cells that hold a point of
    this frame.  Iw / Ih default to the size of that picture.  outdir: also writes config.mat (the reference's keys only) and
    cam0_rectified.png there."""
    import torch
    wdir = os.fspath(wdir)
    K0 = read_opencv_matrix(os.path.join(wdir, "intrinsics_00000000.xml"), "intr")
    K1 = read_opencv_matrix(os.path.join(wdir, "intrinsics_00000001.xml"), "intr")
    R = np.loadtxt(os.path.join(wdir, "Cam0_poseR.txt"))
    T = np.loadtxt(os.path.join(wdir, "Cam0_poseT.txt"))
    P0cam = np.loadtxt(os.path.join(wdir, "P0cam.txt"))
    P1cam = np.loadtxt(os.path.join(wdir, "P1cam.txt"))
    picture = None
    picfile = os.path.join(wdir, "undistorted", "00000000.png")
    if os.path.exists(picfile):
        from PIL import Image
        with Image.open(picfile) as im:
            picture = np.asarray(im.convert("L"), np.uint8)
        if Iw is None or Ih is None:
            Iw, Ih = picture.shape[1], picture.shape[0]
    if Iw is None or Ih is None:
        raise ImageSizeUnknown(f"{wdir}: no undistorted/00000000.png to take the picture size from; give Iw and Ih")
    if meanplane is None:
        raise ValueError("no mean plane (planes.txt)")
    Nx, Ny = int(Nx), int(Ny)
    Rpl, Tpl = sea_plane_RT(meanplane)
    own_ctx = ctx is None
    if own_ctx:
        ctx = Context(0)
    mesh = None
    try:
        mesh = upload_camera_mesh(ctx, load_camera_mesh(os.path.join(wdir, "mesh_cam.xyzC")))
        (z98, z02), npts = mesh.aligned_z_quantiles(Rpl, Tpl, baseline, [0.98, 0.02])
        if npts == 0:
            raise ValueError(f"{wdir}/mesh_cam.xyzC holds no point")
        res = setup_algebra(K0, K1, R, T, P0cam, P1cam, meanplane, baseline, area_center, area_size_x, area_size_y, Nx, Ny, Iw, Ih,
                            z02, z98, fps, timestring)
        gs = grid_setup(Rpl, Tpl, baseline, res["xmin"], res["xmax"], res["ymin"], res["ymax"], Nx, Ny)
        d_cells = torch.empty((Ny, Nx), dtype=torch.float32, device=torch.device("cuda", ctx.device_id))
        torch.cuda.synchronize(d_cells.device)
        mesh.grid_cells_dev(gs, d_cells, "median")
        ctx.synchronize()
        res["coverage"] = float(torch.isfinite(d_cells).sum().item()) / float(Nx * Ny)
        res["cam0_rectified"] = None if picture is None else ctx.warp_perspective(picture, res["Hcam0toTexture"], Nx, Ny)
    finally:
        if mesh is not None:
            mesh.close()
        if own_ctx:
            ctx.close()
    if outdir is not None:
        import scipy.io
        scipy.io.savemat(os.path.join(os.fspath(outdir), "config.mat"), {k: res[k] for k in CONFIG_MAT_KEYS})
        if res["cam0_rectified"] is not None:
            from PIL import Image
            Image.fromarray(res["cam0_rectified"]).save(os.path.join(os.fspath(outdir), "cam0_rectified.png"))
    return res


def main(argv=None) -> int:
    """python -m wass_amd.gridding WORKDIR OUTDIR --action generateconfig|setup: the option names and exit codes of the reference's
    command line (-1: no output directory, no --gridconfig or file not found, nothing to set up from; -2: no such action here;
    -3: picture size unknown)."""
    import argparse
    import glob
    ap = argparse.ArgumentParser(prog="python -m wass_amd.gridding", description="Grid set-up of a WASS sequence; the quantiles of the "
                                 "first frame's cloud are taken on the GPU.")
    ap.add_argument("workdir", help="sequence directory: the NNNNNN_wd frame directories and planes.txt")
    ap.add_argument("outdir", help="existing directory that receives gridconfig.txt, config.mat and cam0_rectified.png")
    ap.add_argument("--action", choices=("setup", "grid", "generateconfig"), help="generateconfig writes a default gridconfig.txt, "
                    "setup writes config.mat; grid is wass_amd.gridding.grid_sequence, a function")
    ap.add_argument("--gridconfig", help="the [Area] file that setup reads")
    ap.add_argument("-b", "--baseline", type=float, default=1.0, help="distance between the cameras in metres (default 1)")
    ap.add_argument("-f", "--fps", type=float, default=0, help="frame rate stored in config.mat")
    ap.add_argument("-t", "--timestring", default="", help="date and time of the sequence, stored as given")
    ap.add_argument("-Iw", "--image_width", type=float, help="picture width when undistorted/00000000.png is absent")
    ap.add_argument("-Ih", "--image_height", type=float, help="picture height, likewise")
    ap.add_argument("-n", "--num_frames", type=int, default=-1, help="look at the first n frame directories only")
    args = ap.parse_args(argv)

    if args.action == "generateconfig":
        print("wrote", generate_gridconfig(args.outdir))
        return 0
    frames = sorted(glob.glob(os.path.join(args.workdir, "*_wd")))
    if args.num_frames > -1:
        frames = frames[:args.num_frames]
    if not os.path.isdir(args.outdir):
        print(f"{args.outdir}: no such output directory")
        return -1
    if args.action == "grid":
        print("the grid action is a function here: wass_amd.gridding.grid_sequence(frames, 'config.mat') returns the cube; no NetCDF file is written")
        return -2
    if args.action != "setup":
        print("give --action generateconfig or --action setup")
        return -2
    if args.gridconfig is None:
        print("setup needs --gridconfig FILE (generateconfig writes one)")
        return -1
    if not os.path.exists(args.gridconfig):
        print(f"{args.gridconfig}: no such grid configuration file")
        return -1
    planes = os.path.join(args.workdir, "planes.txt")
    if not frames or not os.path.exists(planes):
        print(f"{args.workdir}: setup needs at least one NNNNNN_wd directory and planes.txt")
        return -1
    try:
        res = setup_grid(frames[0], mean_plane(planes), baseline=args.baseline, Iw=args.image_width, Ih=args.image_height, fps=args.fps,
                         timestring=args.timestring, outdir=args.outdir, **read_gridconfig(args.gridconfig))
    except ImageSizeUnknown as e:
        print(e)
        return -3
    except ValueError as e:
        print(e)
        return -1
    print(f"{frames[0]}: heights within {res['zmin']:.2f} .. {res['zmax']:.2f} m, {100.0 * res['coverage']:.1f} % of the "
          f"{res['Nx']} x {res['Ny']} cells hold a point")
    print("wrote", os.path.join(args.outdir, "config.mat"))
    return 0


if __name__ == "__main__":
    import sys
    sys.exit(main())
