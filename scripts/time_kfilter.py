#!/usr/bin/env python3
"""Time wass_amd.postproc's dispersion filter at the production size: 1000 frames of a 1024 x 1024 grid (4.2 GB of cube, 14.9 GB of
scratch), du 0.2, dt 0.1, from device and from host memory.  After a warm-up, the median of --reps calls.

    python scripts/time_kfilter.py [--count 1000] [--n 1024] [--reps 5] [--no-baselines] [--log profiles/kfilter_1024.log]

Prints one JSON line and, with --log, appends it to that file:
  dev_ms / host_ms                 Fourier3DFilter.apply on a device tensor / on a host array (the mask set once, outside)
  shell_ms                         set_shell: the maps to the device and k_kf_shell
  stages_ms                        per stage, from the events of set_timing (one timed call, device input): prepare, x, y, t, mul,
                                   t_inv, y_inv, full_close_stage (k_dft_stage<true, true> on the operands of k_dft_close, the
                                   yardstick), close (k_dft_close and the fold of its sums), copy_out
  tflop, tflops                    the work the result needs, counted as the spectrum counts it (real-GEMM flops: 2 products per
                                   real input, 4 per complex one; the closing stage 2, since only the real part is made), over the
                                   six transform stages' time
  torch_rfftn_irfftn_ms            torch.fft.rfftn, a product with the mask and torch.fft.irfftn in complex64 on the same GPU: a
                                   yardstick for the transforms alone (no preparation, no NaN handling, no statistics)
  numpy_s                          the fp64 numpy restatement (rfftn, product, irfftn) on a slab of --slab frames, scaled up to the
                                   cube by frames and by the t transform's n log n
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
    ap.add_argument("--slab", type=int, default=20)
    ap.add_argument("--no-baselines", action="store_true")
    ap.add_argument("--log", default=None)
    a = ap.parse_args()
    du, dt = 0.2, 0.1
    nt, ny, nx = a.count, a.n, a.n
    ch = nx // 2 + 1
    base = np.random.default_rng(0).standard_normal((min(nt, 50), ny, nx), dtype=np.float32) * 0.3
    cube = np.tile(base, (-(-nt // base.shape[0]), 1, 1))[:nt]
    cube[::7, ::5, ::3] = np.nan
    rows, half = float(nt) * ny, float(nt) * ny * ch
    flop = 2.0 * (2 * ch * rows * nx + 4 * ny * half + 4 * nt * half) + 2.0 * (4 * nt * half + 4 * ny * half + 2 * nx * rows * ch)
    res = {"cube": [nt, ny, nx], "scratch_gb": round(P.fourier_filter_scratch_bytes(nt, ny, nx) / 1e9, 2), "tflop": round(flop / 1e12, 2)}
    med = lambda v: float(np.median(v))

    def timed(fn, sync):
        fn()
        sync()
        t = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            fn()
            sync()
            t.append((time.perf_counter() - t0) * 1e3)
        return round(med(t), 2), [round(v, 2) for v in t]

    maps = P.dispersion_mask_maps(nt, ny, nx, du, dt)
    shell = (maps["omega"], maps["kappa_x"], maps["kappa_y"], maps["sigma0"], maps["used"], 0.1, -0.05, 2.0 * maps["domega"], *P.shell_band(maps))
    with wass_amd.Context(0) as ctx, P.Fourier3DFilter(nt, ny, nx, ctx=ctx) as filt:
        res["shell_ms"], _ = timed(lambda: filt.set_shell(*shell), ctx.synchronize)
        res["bins_passing"] = filt.n_pass
        d = torch.from_numpy(cube).cuda()
        dout = torch.empty_like(d)
        torch.cuda.synchronize()
        res["dev_ms"], res["dev_ms_all"] = timed(lambda: filt.apply(d, out=dout), ctx.synchronize)
        filt.set_timing(True)
        filt.apply(d, out=dout)
        st = filt.last_timings()
        filt.set_timing(False)
        res["stages_ms"] = {k: round(v, 2) for k, v in st.items()}
        dft_ms = sum(st[k] for k in ("x", "y", "t", "t_inv", "y_inv", "close"))
        res["transforms_ms"] = round(dft_ms, 2)
        res["tflops"] = round(flop / (dft_ms * 1e-3) / 1e12, 2)
        res["kept"] = round(filt.stats.kept, 4)
        del d, dout
        torch.cuda.empty_cache()
        hout = np.empty_like(cube)
        res["host_ms"], res["host_ms_all"] = timed(lambda: filt.apply(cube, out=hout), ctx.synchronize)
        H = None if a.no_baselines else filt.mask()
    if not a.no_baselines:
        x = torch.from_numpy(np.nan_to_num(cube)).cuda()
        dH = torch.from_numpy(H).cuda()

        def torch_filter():
            X = torch.fft.rfftn(x)
            X *= dH
            return torch.fft.irfftn(X, s=x.shape)
        res["torch_rfftn_irfftn_ms"], _ = timed(torch_filter, torch.cuda.synchronize)
        del x, dH
        torch.cuda.empty_cache()
        s = min(a.slab, nt)
        slab = np.nan_to_num(cube[:s]).astype(np.float64)
        t0 = time.perf_counter()
        y = np.fft.irfftn(np.fft.rfftn(slab) * H[:s], s=slab.shape, axes=(0, 1, 2))
        sec = time.perf_counter() - t0
        del y
        res["numpy_slab_s"] = round(sec, 2)
        res["numpy_s"] = round(sec * (nt / s) * (np.log2(float(nt) * ny * nx) / np.log2(float(s) * ny * nx)), 1)
    line = json.dumps(res)
    print(line)
    if a.log:
        with open(a.log, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
