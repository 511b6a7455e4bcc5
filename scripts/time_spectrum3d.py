#!/usr/bin/env python3
"""Time wass_amd.postproc.compute_3D_spectrum at the production size: a 1024 x 1024 grid, 1000 frames (Nt 100, 19 segments, a
684-wide window, 4 GB of host cube), du 0.2, dt 0.1.  After a warm-up, the median of --reps calls.

    python scripts/time_spectrum3d.py [--count 1000] [--n 1024] [--reps 5] [--no-baselines]

Prints one JSON line:
  ms_per_call / ms_per_segment     the public function on the host cube (every segment crosses PCIe, S comes back)
  dev_ms_per_call                  the same 19 segments pushed from device memory (wass_spec3d_push_dev) + finish
  h2d_share                        (ms_per_call - dev_ms_per_call) / ms_per_call
  stages_ms_per_segment, tflops    19 device pushes without the finish; f32 TFLOP/s against the real-GEMM flop count of the three
                                   stages with the half spectrum in x (2 products in x, 4 each in y and t)
  numpy_ms_per_call                (a) the fp64 numpy restatement of one segment on the host, times the segment count
  torch_fftn_ms_per_segment        (b) torch.fft.fftn of a complex64 copy of one prepared segment on the same GPU: a yardstick for
                                   the transform alone, not on the product path
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import wass_amd  # noqa: E402
from wass_amd import postproc as P  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--count", type=int, default=1000)
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-baselines", action="store_true")
    a = ap.parse_args()
    du, dt = 0.2, 0.1
    base = np.random.default_rng(0).standard_normal((min(a.count, 100), a.n, a.n), dtype=np.float32) * 300
    cube = np.tile(base, (-(-a.count // base.shape[0]), 1, 1))[:a.count]
    p = P.spectrum3d_plan(cube.shape, du, dt)
    nseg, nxh = len(p.starts), p.nx // 2 + 1
    flop = 2.0 * (2 * nxh * p.nt * p.ny * p.nx + 4 * p.ny * p.ny * nxh * p.nt + 4 * p.nt * p.nt * p.ny * nxh)
    res = {"grid": a.n, "count": a.count, "window": [p.nt, p.ny, p.nx], "segments": nseg, "gflop_per_segment": round(flop / 1e9, 1)}
    med = lambda v: float(np.median(v))
    with wass_amd.Context(0) as ctx:
        P.compute_3D_spectrum(cube, du, dt, ctx=ctx)                    # warm-up: code objects, allocations
        t = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            P.compute_3D_spectrum(cube, du, dt, ctx=ctx)                # returns with S on the host
            t.append((time.perf_counter() - t0) * 1e3)
        res["ms_per_call"], res["ms_all"] = round(med(t), 2), [round(v, 2) for v in t]
        res["ms_per_segment"] = round(med(t) / nseg, 2)
        # the same from device memory: one window's worth of frames resident, pushed nseg times
        d = torch.from_numpy(np.ascontiguousarray(cube[:p.nt + p.shift])).cuda()
        torch.cuda.synchronize()
        with P.Spectrum3D(ctx, p.nt, p.ny, p.nx, p.win_t, p.win_y, p.win_x) as sp:
            def pushes():
                for i in range(nseg):
                    s = (i % 2) * p.shift
                    sp.push_dev(d[s:s + p.nt, p.r0:p.r0 + p.ny, p.c0:p.c0 + p.nx])
            pushes(); sp.finish(p.scale)
            td, ts = [], []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                pushes()
                ctx.synchronize()
                t1 = time.perf_counter()
                sp.finish(p.scale)
                td.append((time.perf_counter() - t0) * 1e3)
                ts.append((t1 - t0) * 1e3)
        res["dev_ms_per_call"] = round(med(td), 2)
        res["h2d_share"] = round((med(t) - med(td)) / med(t), 3)
        res["stages_ms_per_segment"] = round(med(ts) / nseg, 3)
        res["tflops"] = round(flop * nseg / (med(ts) * 1e-3) / 1e12, 2)
    if not a.no_baselines:
        seg = cube[:p.nt, p.r0:p.r0 + p.ny, p.c0:p.c0 + p.nx]
        win = (p.win_y[:, None] * p.win_x)[None] * p.win_t[:, None, None]
        t0 = time.perf_counter()
        z = np.array(seg) * 1.0
        z = np.where(np.isnan(z), np.nanmean(z, axis=0), z)
        zw = (z - np.mean(z)) * win
        S = np.abs(np.fft.fftshift(np.fft.fftn(zw, norm="ortho"))) ** 2
        res["numpy_ms_per_call"] = round((time.perf_counter() - t0) * 1e3 * nseg, 1)
        dz = torch.from_numpy(zw.astype(np.complex64)).cuda()
        torch.fft.fftn(dz); torch.cuda.synchronize()
        tf = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            torch.fft.fftn(dz)
            torch.cuda.synchronize()
            tf.append((time.perf_counter() - t0) * 1e3)
        res["torch_fftn_ms_per_segment"] = round(med(tf), 3)
        del S
    print(json.dumps(res))


if __name__ == "__main__":
    main()
