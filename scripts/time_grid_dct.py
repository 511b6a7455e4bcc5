#!/usr/bin/env python3
"""Time the DCT surface interpolator: wass_grid_dct_dev at 1024 x 1024, Nf 150, all 501 Rprop steps (TOLERANCE_CHANGE 0), after
warm-up, against a torch restatement of the reference loop (autograd + torch.optim.Rprop, DCTInterpolator.py) on the same GPU.

    python scripts/time_grid_dct.py [--n 1024] [--nf 150] [--reps 5] [--batch 1,2,4,8,16]

Prints one JSON line: ms per solve, effective TFLOP/s (2 (2 H W Nf + Nf^2 (H + W)) FLOP per step) and the torch loop's ms.
With --batch also wass_grid_dct_batch_dev on that many distinct maps per call, for every size of the list: "batch" maps the
size to the median ms per call, ms per frame and all repeats.  WASS_GPU_LIB=<another build> times that build's single solve
with the same script (an older build has no batch entry: leave --batch out).
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


def surface(n, seed=0):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:n, 0:n].astype(np.float64) / n
    z = sum(rng.uniform(0.05, 0.3) * np.cos(rng.uniform(3, 30) * 2 * np.pi * (np.cos(t) * xx + np.sin(t) * yy))
            for t in rng.uniform(0, np.pi, 8))
    foot = (np.abs(xx - 0.5) < 0.15 + 0.3 * yy) & (yy > 0.05) & (yy < 0.95) & (rng.random((n, n)) < 0.6)
    return np.where(foot, z, np.nan).astype(np.float32)


def torch_loop(I, nf, iters, lr=5.0, alpha=8e-7):
    """The reference's loop, restated (no tolerance stop: all iters + 1 steps)."""
    n = I.shape[0]
    from scipy.fftpack import dct
    Dc = torch.tensor(dct(np.eye(n), type=3, norm="ortho"), dtype=torch.float, device="cuda", requires_grad=True)
    M = torch.tensor((~np.isnan(I)).astype(np.float32), device="cuda")
    Io = torch.tensor(np.nan_to_num(I, nan=0.0), device="cuda")
    x = torch.rand((nf, nf), device="cuda", requires_grad=True)
    opt = torch.optim.Rprop([x], lr=lr)
    for _ in range(iters + 1):
        def closure():
            opt.zero_grad()
            P = torch.nn.functional.pad(x, (0, n - nf, 0, n - nf), "constant", 0)
            Irec = Dc.T @ P @ Dc
            loss = torch.sum(torch.square(Irec - Io) * M) / torch.sum(M) + alpha * torch.linalg.vector_norm(x, ord=1)
            loss.backward()
            return loss
        opt.step(closure)
    return x.detach()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--nf", type=int, default=150)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--batch", default="", help="comma-separated batch sizes for wass_grid_dct_batch_dev (default: none)")
    a = ap.parse_args()
    n, nf, iters = a.n, a.nf, 500
    zz = surface(n)
    d_zz = torch.tensor(zz, device="cuda")
    d_out = torch.empty_like(d_zz)
    opts = {"Nfreqs": nf, "MAX_ITERS": iters, "TOLERANCE_CHANGE": 0.0}
    res = {"n": n, "nf": nf, "steps": iters + 1}
    with wass_amd.Context(0) as ctx:
        ctx.wait_for_stream(torch.cuda.current_stream().cuda_stream)
        info = ctx.grid_dct_dev(d_zz, d_out, opts)                     # warm-up (allocations, code objects)
        assert info["steps"] == iters + 1
        times = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            ctx.grid_dct_dev(d_zz, d_out, opts)                        # returns when the solve has finished
            times.append((time.perf_counter() - t0) * 1e3)
        batches = [int(b) for b in a.batch.split(",") if b]
        if batches:
            d_all = torch.tensor(np.stack([surface(n, seed=i) for i in range(max(batches))]), device="cuda")
            d_all_out = torch.empty_like(d_all)
            torch.cuda.synchronize()
            res["batch"] = {}
            for nb in batches:
                infos, status = ctx.grid_dct_batch_dev(d_all[:nb], d_all_out[:nb], opts)          # warm-up: the scratch grows
                assert all(i["steps"] == iters + 1 for i in infos) and (status == 0).all()
                tb = []
                for _ in range(a.reps):
                    t0 = time.perf_counter()
                    ctx.grid_dct_batch_dev(d_all[:nb], d_all_out[:nb], opts)
                    tb.append((time.perf_counter() - t0) * 1e3)
                res["batch"][str(nb)] = {"ms_per_call": round(float(np.median(tb)), 3), "ms_per_frame": round(float(np.median(tb)) / nb, 3),
                                         "ms_all": [round(t, 3) for t in tb]}
    flop = 2.0 * (2.0 * n * n * nf + nf * nf * (n + n)) * (iters + 1)
    res["ms_per_solve"] = round(float(np.median(times)), 3)
    res["ms_all"] = [round(t, 3) for t in times]
    res["tflops"] = round(flop / (np.median(times) * 1e-3) / 1e12, 2)
    if not a.no_torch:
        torch_loop(zz, nf, 5)
        torch.cuda.synchronize()
        tt = []
        for _ in range(max(1, a.reps // 2)):
            t0 = time.perf_counter()
            torch_loop(zz, nf, iters)
            torch.cuda.synchronize()
            tt.append((time.perf_counter() - t0) * 1e3)
        res["torch_ms_per_solve"] = round(float(np.median(tt)), 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
