#!/usr/bin/env python3
"""Time wass_amd.postproc.visibility_map at the production size: frames of a 1024 x 1024 grid, du 0.2 m, for a low camera (8 m up,
60 m off the grid: long rays, more than half of the cells occluded) and a high one (30 m up, 20 m off: short rays).  After a
warm-up, the median of --reps calls.

    python scripts/time_visibility.py [--n 1024] [--frames 16] [--reps 5] [--no-host-oracle]

Prints one JSON line per camera:
  dev_ms_per_frame_b1 / _b8 / _b16    a device-resident cube into device tensors, with batch 1, 8 and 16
  host_ms_per_frame_b8                the same from a host array into host arrays (frames, masks and angles cross PCIe)
  occluded_percent, steps             of frame 0 (steps: the longest ray of the oracle, with --no-host-oracle absent)
  oracle_march_s_per_frame            the numpy oracle's march of frame 0 on the host, one thread: the quantity to hold against
                                      the reference's own routine, which takes 1.4 s for ONE 512 x 512 frame on one thread
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import wass_amd  # noqa: E402
from wass_amd import postproc as P  # noqa: E402
import visibility_oracle as VO  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-host-oracle", action="store_true")
    a = ap.parse_args()
    n, du = a.n, 0.2
    XX, YY = VO.make_grid(n, n, du)
    cube = np.stack([VO.make_sea(n, n, du, 16, 1.5, t=0.5 * t) for t in range(a.frames)])
    ctx = wass_amd.Context(0)
    d_cube = torch.from_numpy(cube).cuda()

    def timed(fn):
        fn()
        t = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            fn()
            t.append(time.perf_counter() - t0)
        return 1e3 * float(np.median(t)) / a.frames

    for name, height, back in (("low", 8.0, 60.0), ("high", 30.0, 20.0)):
        cam = VO.camera(XX, YY, "west", height, back)
        res = {"camera": name, "height_m": height, "back_m": back, "grid": n, "frames": a.frames}
        om = torch.empty(cube.shape, dtype=torch.uint8, device="cuda")
        oa = torch.empty(cube.shape, dtype=torch.float32, device="cuda")
        for b in (1, 8, 16):
            res[f"dev_ms_per_frame_b{b}"] = round(timed(lambda: P.visibility_map(d_cube, XX, YY, cam, ctx=ctx, out_occlusion=om, out_angles=oa, batch=b)), 4)
        res["host_ms_per_frame_b8"] = round(timed(lambda: P.visibility_map(cube, XX, YY, cam, ctx=ctx, batch=8)), 4)
        res["occluded_percent"] = round(float(P.visibility_map(cube[:1], XX, YY, cam, ctx=ctx)[2][0]), 3)
        if not a.no_host_oracle:
            zf = VO.heights(cube[0])
            d = VO.rays(XX, YY, zf, cam[:3, 3])
            Zc = zf.astype(np.float64) / VO.spacing(XX, YY)[0]
            t0 = time.perf_counter()
            _, steps = VO.march(Zc, d)
            res["oracle_march_s_per_frame"] = round(time.perf_counter() - t0, 3)
            res["steps"] = steps
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
