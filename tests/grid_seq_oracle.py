"""numpy restatements of the sequence layer of the reference's gridding tool (gridding/wassgridsurface/wassgridsurface.py), written
from its behaviour: the checker of grid_seq.hip, never imported by the product.

  median_blur(z, k, mask)      :359-363  Zi[mask == 0] = 0; cv.medianBlur(Zi, ksize = k); Zi[mask == 0] = NaN.  cv::medianBlur
                                         replicates the border; the median of an odd window is one of its elements, so
                                         np.median over the edge-padded windows is exact in float32.
  sequence_stats(frames, fzm)  :490-494, 528-546  per-frame nanmean / nanmin / nanmax, the fp64 per-point sum in frame order,
                                         Zmin / Zmax / Zmean, Zmean_perpoint = sum / N * 1000, the millimetre slices Zi * 1000.
  zero_mean(cube, mean)        :554-576  float32 chunk minus float64 mean, stored as float32.
"""
import warnings

import numpy as np


def median_blur(z, k, mask=None):
    """z: float32 H x W (or n x H x W, filtered map by map); k: 3 or 5 (0: only the mask); mask: H x W, 0 = outside."""
    z = np.asarray(z, np.float32)
    if z.ndim == 3:
        return np.stack([median_blur(f, k, mask) for f in z])
    z = z.copy()
    if mask is not None:
        z[np.asarray(mask) == 0] = 0
    if k:
        if k not in (3, 5):
            raise ValueError("cv::medianBlur takes 32-bit float for ksize 3 and 5 only")
        r = k // 2
        p = np.pad(z, r, mode="edge")
        win = np.lib.stride_tricks.sliding_window_view(p, (k, k)).reshape(z.shape[0], z.shape[1], k * k)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            z = np.median(win, axis=-1).astype(np.float32)
    if mask is not None:
        z[np.asarray(mask) == 0] = np.nan
    return z


def sequence_stats(frames, force_zero_mean=False):
    """frames: n x H x W float32 metres.  Returns a dict with the reference's end-of-sequence values."""
    frames = np.asarray(frames, np.float32)
    acc = np.zeros(frames.shape[1:], np.float64)
    means, mins, maxs = [], [], []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        for zi in frames:
            acc = acc + zi
            means.append(np.nanmean(zi.astype(np.float64)))      # the exact mean up to fp64 rounding: what the bound is taken against
            mins.append(np.nanmin(zi))
            maxs.append(np.nanmax(zi))
        zmin, zmax, zmean = float(np.amin(np.array(mins))), float(np.amax(np.array(maxs))), float(np.mean(np.array(means)))
    mean_perpoint = acc / float(len(frames)) * 1000
    if force_zero_mean:
        zmean, zmax = 0.0, -zmin
    return {"zmin": zmin, "zmax": zmax, "zmean": zmean, "mean_perpoint_mm": mean_perpoint, "acc": acc,
            "frame_mean": np.array(means, np.float64), "frame_min": np.array(mins, np.float64), "frame_max": np.array(maxs, np.float64),
            "z_mm": frames * np.float32(1000)}


def zero_mean(cube_mm, mean_perpoint_mm):
    """cube_mm: n x H x W float32; mean_perpoint_mm: H x W float64."""
    return (np.asarray(cube_mm, np.float32) - np.asarray(mean_perpoint_mm, np.float64)).astype(np.float32)
