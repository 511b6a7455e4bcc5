#!/usr/bin/env python3
"""Times `polarimetric_prepare` on the GPU for one 2448 x 2048 mosaic (the common polarising sensor): device-resident and from the
host, with the Stokes pictures only and with every output, beside a torch-on-GPU restatement of the staged chain (four upscales, four
remaps through a precomputed map, the element-wise stages; every intermediate picture stored).  Prints ms and the share of the floor
of 14 B per output pixel (1 B of mosaic read, 12 B of S and 1 B of picture written) at 8 TB/s that the fused kernel reaches.  Prints a
table for DESIGN.md.  No speed is promised.

    python scripts/time_prepare_pol.py [--reps 20]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

HBM_BYTES_PER_S = 8.0e12


def best(fn, sync, reps):
    t = []
    for _ in range(reps):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        t.append(time.perf_counter() - t0)
    return min(t)


def staged_torch(torch, mosaic, iu, iv, tab):
    """the staged chain in torch: returns (S [3, H, W], image u8); the map (iu, iv) is given, as a staged program would keep it"""
    F = torch.float32
    m, n = mosaic.shape[0] // 2, mosaic.shape[1] // 2
    quarters = (mosaic[1::2, 1::2], mosaic[0::2, 1::2], mosaic[0::2, 0::2], mosaic[1::2, 0::2])

    def coeffs(size):
        d = torch.arange(2 * size, device=mosaic.device, dtype=F)
        f = (d + 0.5) * 0.5 - 0.5
        s = torch.floor(f)
        a = f - s
        s = s.long()
        edge = (s < 0) | (s >= size - 1)
        a = torch.where(edge, torch.zeros_like(a), a)
        s = s.clamp(0, size - 1)
        return s, (s + 1).clamp(max=size - 1), a

    sx, sx1, ax = coeffs(n)
    sy, sy1, ay = coeffs(m)
    H, W = 2 * m, 2 * n
    wx, wy, a = (iu >> 5), (iv >> 5), ((iv & 31) * 32 + (iu & 31))
    w = tab[a]                                                                  # [H, W, 4]
    und = []
    for q in quarters:
        q = q.to(F) * (1.0 / 255.0)
        h = q[:, sx] * (1 - ax) + q[:, sx1] * ax
        u = h[sy, :] * (1 - ay)[:, None] + h[sy1, :] * ay[:, None]
        acc = None
        for k, (ky, kx) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
            yy, xx = wy + ky, wx + kx
            inside = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
            v = torch.where(inside, u[yy.clamp(0, H - 1), xx.clamp(0, W - 1)], torch.zeros((), device=u.device)) * w[..., k]
            acc = v if acc is None else acc + v
        und.append(acc)
    a0, a45, a90, a135 = und
    k1, k2 = 0.75, 0.25
    I0 = k1 * a0 + k2 * a45 - k2 * a90 + k2 * a135
    I45 = k2 * a0 + k1 * a45 + k2 * a90 - k2 * a135
    I90 = -k2 * a0 + k2 * a45 + k1 * a90 + k2 * a135
    I135 = k2 * a0 - k2 * a45 + k2 * a90 + k1 * a135
    S = torch.stack(((I0 + I45 + I90 + I135) * 0.5, I0 - I90, I45 - I135))
    image = torch.nan_to_num(torch.round(S[0] * 127.0), nan=0.0).clamp(0, 255).to(torch.uint8)
    return S, image


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    import torch
    import prepare_pol_oracle as PP
    import wass_amd
    from wass_amd import postproc as P
    from wass_amd import prepare as W

    cols, rows = 2448, 2048
    mosaic = PP.random_mosaic(rows, cols, 1)
    K, dist = PP.camera(cols, rows), PP.DIST["calibdir"]
    npix = rows * cols
    floor_ms = 1e3 * 14.0 * npix / HBM_BYTES_PER_S
    sync = torch.cuda.synchronize
    out = []
    with wass_amd.Context(0) as ctx:
        d_mosaic = torch.from_numpy(mosaic).cuda()
        fused = {}
        for what, outs in (("Stokes only", ("stokes",)), ("every output", W.PREP_OUTPUTS)):
            run = lambda: W.polarimetric_prepare(d_mosaic, K, dist, outputs=outs, ctx=ctx)
            fused[what] = run()
            t = 1e3 * best(run, sync, a.reps)
            share = f", {100 * floor_ms / t:.0f} % of the {floor_ms:.4f} ms floor of 14 B per pixel" if what == "Stokes only" else ""
            out.append((f"polarimetric_prepare, device-resident, {what}", f"{t:.3f} ms{share}"))
        for what, outs in (("Stokes only", ("stokes",)), ("every output", W.PREP_OUTPUTS)):
            run = lambda: W.polarimetric_prepare(mosaic, K, dist, outputs=outs, ctx=ctx)
            run()
            out.append((f"polarimetric_prepare, from the host, {what}", f"{1e3 * best(run, sync, max(a.reps // 4, 2)):.3f} ms"))
        iu, iv = PP.undistort_map(cols, rows, K, dist)
        d_iu, d_iv = torch.from_numpy(iu).cuda(), torch.from_numpy(iv).cuda()
        tab = torch.from_numpy(np.ascontiguousarray(P.bilinear_table().reshape(1024, 4))).cuda()
        run = lambda: staged_torch(torch, d_mosaic, d_iu, d_iv, tab)
        S, image = run()
        t = 1e3 * best(run, sync, max(a.reps // 4, 2))
        out.append(("the staged chain in torch on the GPU, Stokes only, map given", f"{t:.3f} ms"))
        dS = float((S - fused["Stokes only"].S).abs().max())
        d8 = int((image.int() - fused["Stokes only"].image.int()).abs().max())
        print(f"staged torch against the fused kernel: largest |dS| = {dS:.3e}, largest picture difference = {d8}", file=sys.stderr)
    width = max(len(r[0]) for r in out)
    for name, val in out:
        print(f"| {name.ljust(width)} | {val} |")


if __name__ == "__main__":
    main()
