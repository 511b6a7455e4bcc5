#!/usr/bin/env python3
"""Time wass_amd.postproc's Butterworth filters at the production size: 1000 frames of a 1024 x 1024 grid (4 GB of float32), dt 1 / 12,
du 0.2.  After a warm-up, the median of --reps calls.

    python scripts/time_filters.py [--count 1000] [--n 1024] [--reps 5] [--no-baselines] [--no-host]

Prints one JSON line:
  lowpass_dev_ms, highpass_dev_ms    butterworth_filter on a device-resident cube into a device tensor (8th order, 1 Hz low-pass;
                                     0.05 Hz high-pass with the mean removed)
  *_gbs, *_of_5tbs                   the bytes the kernels move (24 B per sample; 48 with the mean removed: the fp64 result is written,
                                     summed and read again) per second, and as a fraction of 5.0 TB/s
  lowpass_host_ms, highpass_host_ms  the same from a host array into a host array (slabs cross PCIe both ways)
  spatial_dev_ms, spatial_tflops     spatial_lowpass of the same device cube; f32 TFLOP/s against the real-GEMM flop count the result
                                     needs (2 products in each x stage, 4 in each y stage); spatial_tflops_executed counts the 4 the
                                     last x stage runs (k_dft_stage also makes the imaginary part, which is dropped)
  spatial_host_ms                    the same from and to host memory
  scipy_*_ms_scaled, numpy_fft_ms_scaled   baselines on the host: scipy.signal.sosfiltfilt (the numpy oracle where scipy is absent) on
                                     a slab of --base-rows rows in as many threads as OMP_NUM_THREADS says (16 by default), and the fp64
                                     np.fft oracle on --base-frames frames, both SCALED UP to the whole cube
"""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import wass_amd  # noqa: E402
from wass_amd import postproc as P  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--count", type=int, default=1000)
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-baselines", action="store_true")
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--base-rows", type=int, default=16)
    ap.add_argument("--base-frames", type=int, default=32)
    a = ap.parse_args()
    dt, du, n, count = 1.0 / 12.0, 0.2, a.n, a.count
    base = np.random.default_rng(0).standard_normal((min(count, 100), n, n), dtype=np.float32) * 300
    cube = np.tile(base, (-(-count // base.shape[0]), 1, 1))[:count]
    samples = float(count) * n * n
    res = {"grid": n, "count": count}
    med = lambda v: float(np.median(v))

    def timed(fn):
        fn()
        t = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            fn()
            t.append((time.perf_counter() - t0) * 1e3)
        return med(t), [round(v, 2) for v in t]

    with wass_amd.Context(0) as ctx:
        d = torch.from_numpy(cube).cuda()
        out = torch.empty_like(d)
        torch.cuda.synchronize()
        for name, kind, fc, bytes_per in (("lowpass", "lowpass", 1.0, 24.0), ("highpass", "highpass", 0.05, 48.0)):
            ms, every = timed(lambda: P.butterworth_filter(d, dt, cutoff=fc, type=kind, ctx=ctx, out=out))
            res[f"{name}_dev_ms"], res[f"{name}_dev_ms_all"] = round(ms, 2), every
            res[f"{name}_gbs"] = round(bytes_per * samples / (ms * 1e-3) / 1e9, 1)
            res[f"{name}_of_5tbs"] = round(bytes_per * samples / (ms * 1e-3) / 5.0e12, 3)
        res["scratch_gb"] = round(P.sosfiltfilt_scratch_bytes(count, n, n, 27, host=False)[0] / 1e9, 2)
        ch = n // 2 + 1
        flop = 2.0 * (2 * ch * n * n + 4 * n * n * ch + 4 * n * n * ch + 2 * n * n * ch) * count
        flop_run = flop + 2.0 * 2 * n * n * ch * count
        filt = P.Spatial2DButterworth(n, n, du, 2.0 * np.pi / 9.81, 4, ctx=ctx, batch=16)
        ms, every = timed(lambda: filt.apply_batch(d, out=out))
        res["spatial_dev_ms"], res["spatial_dev_ms_all"] = round(ms, 2), every
        res["spatial_tflops"] = round(flop / (ms * 1e-3) / 1e12, 2)
        res["spatial_tflops_executed"] = round(flop_run / (ms * 1e-3) / 1e12, 2)
        del d, out
        torch.cuda.empty_cache()
        if not a.no_host:
            hout = np.empty_like(cube)
            for name, kind, fc in (("lowpass", "lowpass", 1.0), ("highpass", "highpass", 0.05)):
                ms, every = timed(lambda: P.butterworth_filter(cube, dt, cutoff=fc, type=kind, ctx=ctx, out=hout))
                res[f"{name}_host_ms"], res[f"{name}_host_ms_all"] = round(ms, 1), every
            ms, every = timed(lambda: filt.apply_batch(cube, out=hout))
            res["spatial_host_ms"], res["spatial_host_ms_all"] = round(ms, 1), every
        filt.close()
    if not a.no_baselines:
        import filter_oracle as FO
        threads = int(os.environ.get("OMP_NUM_THREADS", "16") or 16)
        try:
            from scipy.signal import sosfiltfilt as host_filter
            res["baseline"] = "scipy.signal.sosfiltfilt"
        except ImportError:
            host_filter = lambda sos, x, axis=0: FO.sosfiltfilt(sos, x)
            res["baseline"] = "numpy oracle"
        res["baseline_threads"], res["baseline_rows"], res["baseline_frames"] = threads, a.base_rows, a.base_frames
        for name, kind, fc in (("lowpass", "lowpass", 1.0), ("highpass", "highpass", 0.05)):
            sos = P.butter_sos(8, fc, kind, 1.0 / dt)
            rows = [np.ascontiguousarray(cube[:, r]) for r in range(a.base_rows)]           # one row of the grid per task, as wasspost
            with ThreadPoolExecutor(threads) as pool:
                t0 = time.perf_counter()
                list(pool.map(lambda x: host_filter(sos, x, axis=0).astype(np.float32), rows))
                ms = (time.perf_counter() - t0) * 1e3
            res[f"scipy_{name}_ms_scaled"] = round(ms * n / a.base_rows, 0)
        Hs = FO.transfer_function(n, n, du, 2.0 * np.pi / 9.81, 4)
        with ThreadPoolExecutor(threads) as pool:
            t0 = time.perf_counter()
            list(pool.map(lambda x: FO.spatial_apply(x, Hs).astype(np.float32), [cube[i] for i in range(a.base_frames)]))
            ms = (time.perf_counter() - t0) * 1e3
        res["numpy_fft_ms_scaled"] = round(ms * count / a.base_frames, 0)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
