#!/usr/bin/env python3
"""Time wass_amd.postproc.wave_statistics at the production size: 1000 frames of a 1024 x 1024 grid (4 GB of float32, millimetres),
dt 1 / 12: a sea of a dozen components around 0.15 Hz with white noise on top, made on the device.  After a warm-up, the median of
--reps calls.

    python scripts/time_wavestats.py [--count 1000] [--n 1024] [--reps 5] [--no-baseline] [--no-host]

Prints one JSON line:
  dev_ms, dev_hist_ms     wave_statistics of the device-resident cube, without and with the pooled histogram (64 bins)
  waves_per_cell          mean number of waves of a series
  bytes_gb, gbs, of_6p2tbs   what the kernels move -- 8 B per sample (the cube is read for the mean and for the scan), 160 B per wave
                          (H_k and T_k written once; H_k read in each of the 16 passes of the descent and, with T_k, in the last), 108 B
                          per cell of results -- per second, and as a fraction of the 6.2 TB/s of a pure read stream
  host_ms                 the same from a host array (the slab crosses PCIe once)
  scratch_gb, rows_per_slab   device scratch of the two forms
  numpy_ms_scaled         the numpy restatement of the tests on --base-rows rows of the grid, SCALED UP to the whole grid
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


def sea(count, n, dt, device):
    g = torch.Generator(device=device).manual_seed(0)
    rng = np.random.default_rng(0)
    y, x = torch.meshgrid(torch.arange(n, device=device, dtype=torch.float32), torch.arange(n, device=device, dtype=torch.float32), indexing="ij")
    z = torch.empty((count, n, n), dtype=torch.float32, device=device)
    comps = [(f, rng.uniform(60.0, 140.0), rng.uniform(0, 2 * np.pi), rng.uniform(0, 2 * np.pi)) for f in rng.uniform(0.11, 0.19, 12)]
    for t in range(count):
        frame = 300.0 + 25.0 * torch.randn((n, n), generator=g, device=device)
        for f, a, th, ph in comps:
            k = 0.2 * (2 * np.pi * f) ** 2 / 9.81
            frame += a * torch.cos(2 * np.pi * f * t * dt - k * (np.cos(th) * x + np.sin(th) * y) + ph)
        z[t] = frame
    return z


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--count", type=int, default=1000)
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--base-rows", type=int, default=1)
    a = ap.parse_args()
    dt, n, count = 1.0 / 12.0, a.n, a.count
    res = {"grid": n, "count": count}

    def timed(fn):
        fn()
        t = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            fn()
            t.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(t)), [round(v, 2) for v in t]

    kw = dict(dt=dt, datascale=1e-3)
    with wass_amd.Context(0) as ctx:
        d = sea(count, n, dt, "cuda")
        torch.cuda.synchronize()
        ms, every = timed(lambda: P.wave_statistics(d, ctx=ctx, **kw))
        res["dev_ms"], res["dev_ms_all"] = round(ms, 2), every
        msh, every = timed(lambda: P.wave_statistics(d, ctx=ctx, hist_bins=64, hist_width=0.05, **kw))
        res["dev_hist_ms"], res["dev_hist_ms_all"] = round(msh, 2), every
        ws = P.wave_statistics(d, ctx=ctx, **kw)
        s = ws.summary()
        res["summary"] = {k: (round(v, 4) if isinstance(v, float) else v) for k, v in s.items()}
        res["waves_per_cell"] = round(s["n_waves"] / max(s["valid_cells"], 1), 1)
        moved = 8.0 * count * n * n + 160.0 * s["n_waves"] + 108.0 * n * n
        res["bytes_gb"] = round(moved / 1e9, 2)
        res["gbs"] = round(moved / (ms * 1e-3) / 1e9, 1)
        res["of_6p2tbs"] = round(moved / (ms * 1e-3) / 6.2e12, 3)
        res["scratch_gb"] = {"device": round(P.wave_statistics_scratch_bytes(count, n, n, host=False)[0] / 1e9, 2),
                             "host": round(P.wave_statistics_scratch_bytes(count, n, n, host=True)[0] / 1e9, 2)}
        res["rows_per_slab"] = {"device": P.wave_statistics_scratch_bytes(count, n, n, host=False)[1],
                                "host": P.wave_statistics_scratch_bytes(count, n, n, host=True)[1]}
        cube = d.cpu().numpy() if not (a.no_host and a.no_baseline) else None
        del d, ws
        torch.cuda.empty_cache()
        if not a.no_host:
            ms, every = timed(lambda: P.wave_statistics(cube, ctx=ctx, **kw))
            res["host_ms"], res["host_ms_all"] = round(ms, 1), every
    if not a.no_baseline:
        import wavestats_oracle as WO
        part = np.ascontiguousarray(cube[:, :a.base_rows])
        t0 = time.perf_counter()
        WO.wave_stats(part, **kw)
        res["numpy_ms_scaled"] = round((time.perf_counter() - t0) * 1e3 * n / a.base_rows, 0)
        res["baseline_rows"] = a.base_rows
    print(json.dumps(res))


if __name__ == "__main__":
    main()
