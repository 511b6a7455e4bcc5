#!/usr/bin/env python3
"""Time the spectral products at the production size: the 3-D spectrum of 1000 frames of a 1024 x 1024 grid is 100 x 684 x 684 fp64
(374 MB; 49 frequencies above zero, 183 MB), 72 directions.  After a warm-up, the median of --reps calls, each a host clock around
a call that ends in a device synchronisation.

    python scripts/time_specprod.py [--count 1000] [--n 1024] [--reps 5] [--no-baseline] [--kernels]

Prints one JSON line:
  products_dev_ms         spectrum_products of the device-resident S: label maps and cell lists on the host, their upload, the kernels,
                          the download of the tables and of E2
  current_dev_ms          dispersion_current of the device-resident S (the peak and four rounds of sums)
  chain_ms                compute_3D_spectrum_dev (19 segments pushed from the device-resident cube, S stays there) + spectrum_products
  half_mb                 the bytes of S the products have to read once: the frequencies above zero
  baseline_spectrum_dev_ms   what a caller did before, at its best: the same 19 segments pushed from the device-resident cube, then
                          Spectrum3D.finish with its download of S
  baseline_spectrum_ms    compute_3D_spectrum from a host copy of the cube (segments uploaded, S downloaded)
  numpy_products_ms       the products with numpy on the host: np.bincount per frequency for the two tables, a sum for E2, an argmax
  oracle_products_ms      the same through tests/specprod_oracle.py, which keeps the device's fold order and is slower for it
  baseline_numpy_ms, baseline_oracle_ms   baseline_spectrum_dev_ms + either; ratio_numpy_over_chain = baseline_numpy_ms / chain_ms
  equal_to_oracle         the products of this size compared with the oracle once, np.array_equal on every field (the suite stops at
                          20 x 129 x 131)
--kernels: only a warm-up and --reps calls of spectrum_products and dispersion_current on a synthetic device S, for a run under
`rocprofv3 --kernel-trace --stats`, which gives the kernels' own times (k_sp_label, k_sp_cells, k_sp_best, k_sp_current, k_sp_fold).
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


def sea(count, n, du, dt, device, current=(0.3, -0.2)):
    """millimetres: a dozen deep-water components around 0.25 Hz riding a current, white noise on top"""
    g = torch.Generator(device=device).manual_seed(0)
    rng = np.random.default_rng(0)
    y, x = torch.meshgrid(torch.arange(n, device=device, dtype=torch.float32) * du, torch.arange(n, device=device, dtype=torch.float32) * du,
                          indexing="ij")
    z = torch.empty((count, n, n), dtype=torch.float32, device=device)
    comps = []
    for f0 in rng.uniform(0.18, 0.35, 12):
        k, th = (2 * np.pi * f0) ** 2 / 9.81, rng.uniform(-0.6, 0.6)
        kx, ky = k * np.cos(th), k * np.sin(th)
        comps.append((kx, ky, np.sqrt(9.81 * k) + kx * current[0] + ky * current[1], rng.uniform(60.0, 140.0), rng.uniform(0, 2 * np.pi)))
    for t in range(count):
        frame = 25.0 * torch.randn((n, n), generator=g, device=device)
        for kx, ky, w, a, ph in comps:
            frame += a * torch.cos(kx * x + ky * y - w * t * dt + ph)
        z[t] = frame
    return z


def numpy_products(S, kx, ky, f, ndir):
    """the plain host way: what a caller would write with numpy"""
    L_dir, L_k, nk, _ = P.spectral_label_maps(kx, ky, ndir)
    p0 = int(np.flatnonzero(f > 0.5 * (f[1] - f[0]))[0])
    ud, uk = L_dir.ravel() >= 0, L_k.ravel() >= 0
    T_dir = np.stack([np.bincount(L_dir.ravel()[ud], weights=S[p].ravel()[ud], minlength=ndir) for p in range(p0, len(f))])
    T_k = np.stack([np.bincount(L_k.ravel()[uk], weights=S[p].ravel()[uk], minlength=nk) for p in range(p0, len(f))])
    return T_dir, T_k, S[p0:].sum(0), int(np.argmax(S[p0:].reshape(len(f) - p0, -1)[:, ud]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--count", type=int, default=1000)
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ndir", type=int, default=72)
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--kernels", action="store_true")
    a = ap.parse_args()
    du, dt = 0.25, 1.0 / 12.0
    res = {"grid": a.n, "count": a.count, "ndir": a.ndir}

    def timed(fn):
        fn()
        t = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            fn()
            t.append((time.perf_counter() - t0) * 1e3)
        return round(float(np.median(t)), 2), [round(v, 2) for v in t]

    with wass_amd.Context(0) as ctx:
        if a.kernels:
            plan = P.spectrum3d_plan((a.count, a.n, a.n), du, dt)
            S = torch.rand((plan.nt, plan.ny, plan.nx), dtype=torch.float64, device="cuda")
            for _ in range(a.reps + 1):
                P.spectrum_products(S, plan.kx, plan.ky, plan.f, ndir=a.ndir, ctx=ctx)
                P.dispersion_current(S, plan.kx, plan.ky, plan.f, threshold=0.5, ctx=ctx)
            print(json.dumps({"kernels_only": True, "shape": list(S.shape), "calls": a.reps + 1}))
            return
        d = sea(a.count, a.n, du, dt, "cuda")
        torch.cuda.synchronize()
        S, kx, ky, f, had_nan = P.compute_3D_spectrum_dev(d, du, dt, datascale=1e-3, ctx=ctx)
        res["shape"] = list(S.shape)
        nf = int((f > 0.5 * (f[1] - f[0])).sum())
        res["nf"], res["half_mb"] = nf, round(nf * S.shape[1] * S.shape[2] * 8 / 1e6, 1)
        scale = float(S.numel())
        res["products_dev_ms"], res["products_dev_ms_all"] = timed(lambda: P.spectrum_products(S, kx, ky, f, ndir=a.ndir, scale=scale, ctx=ctx))
        res["current_dev_ms"], res["current_dev_ms_all"] = timed(lambda: P.dispersion_current(S, kx, ky, f, scale=scale, ctx=ctx))
        res["chain_ms"], res["chain_ms_all"] = timed(
            lambda: P.spectrum_products(P.compute_3D_spectrum_dev(d, du, dt, datascale=1e-3, ctx=ctx)[0], kx, ky, f, ndir=a.ndir, scale=scale, ctx=ctx))
        got = P.spectrum_products(S, kx, ky, f, ndir=a.ndir, scale=scale, ctx=ctx)
        fit = P.dispersion_current(S, kx, ky, f, scale=scale, ctx=ctx)
        res["summary"] = {k: (round(v, 5) if isinstance(v, float) else v) for k, v in got.summary().items()}
        res["current"] = {"U": fit.U, "V": fit.V, "n_bins": [t["n_bins"] for t in fit.trace], "rms": fit.rms}
        res["scratch_mb"] = {k: round(P.spectrum_products_scratch_bytes(*S.shape, nf, a.ndir, len(got.k), host=h)[0] / 1e6, 1)
                             for k, h in (("device", False), ("host", True))}
        if not a.no_baseline:
            import specprod_oracle as O
            plan = P.spectrum3d_plan(d.shape, du, dt)

            def pushed_from_the_device():
                with P.Spectrum3D(ctx, plan.nt, plan.ny, plan.nx, plan.win_t, plan.win_y, plan.win_x) as sp:
                    for s0 in plan.starts:
                        sp.push_dev(d[s0:s0 + plan.nt, plan.r0:plan.r0 + plan.ny, plan.c0:plan.c0 + plan.nx], 1e-3)
                    return sp.finish(plan.scale)[0]
            res["baseline_spectrum_dev_ms"], res["baseline_spectrum_dev_ms_all"] = timed(pushed_from_the_device)
            cube = d.cpu().numpy()
            del d
            torch.cuda.empty_cache()
            res["baseline_spectrum_ms"], res["baseline_spectrum_ms_all"] = timed(lambda: P.compute_3D_spectrum(cube, du, dt, datascale=1e-3, ctx=ctx))
            Sh = P.compute_3D_spectrum(cube, du, dt, datascale=1e-3, ctx=ctx)[0]
            t0 = time.perf_counter()
            numpy_products(Sh, kx, ky, f, a.ndir)
            res["numpy_products_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
            t0 = time.perf_counter()
            ref = O.products(Sh, kx, ky, f, ndir=a.ndir, scale=scale)
            res["oracle_products_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
            res["baseline_numpy_ms"] = round(res["baseline_spectrum_dev_ms"] + res["numpy_products_ms"], 1)
            res["baseline_oracle_ms"] = round(res["baseline_spectrum_dev_ms"] + res["oracle_products_ms"], 1)
            res["ratio_numpy_over_chain"] = round(res["baseline_numpy_ms"] / res["chain_ms"], 2)
            names = ("freq", "D", "S_f", "F_fk", "S_k", "E_k2", "mean_direction", "spread", "T_dir", "T_k", "E2")
            res["equal_to_oracle"] = bool(np.array_equal(S.cpu().numpy(), Sh)) and all(
                np.array_equal(getattr(got, k), ref[k], equal_nan=True) for k in names) and got.m0 == ref["m0"]
            rf = O.dispersion_current(Sh, kx, ky, f, scale=scale)
            res["current_equal_to_oracle"] = bool(fit.U == rf["U"] and fit.V == rf["V"] and fit.n_bins == rf["n_bins"])
    print(json.dumps(res))


if __name__ == "__main__":
    main()
