#!/usr/bin/env python3
"""Times the radiance chain on the GPU: ms per frame of `radiance` for a 1024 x 1024 grid sampled from a 2456 x 2058 picture, and
`bgimage` at 3000 x 1024 x 1024 with a window of 2000 frames, device-resident and from the host; beside them the numpy oracle's
seconds on one thread (tests/radiance_oracle.py, on fewer frames / series and scaled).  Prints a table for DESIGN.md.

    python scripts/time_radiance.py [--frames 16] [--count 3000] [--no-oracle]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def best(fn, sync, reps=3):
    t = []
    for _ in range(reps):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        t.append(time.perf_counter() - t0)
    return min(t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--count", type=int, default=3000)
    ap.add_argument("--no-oracle", action="store_true")
    a = ap.parse_args()
    import torch
    import radiance_oracle as RO
    import wass_amd
    from wass_amd import postproc as P

    H = W = 1024
    Iw, Ih = 2456, 2058
    n = a.frames
    XX, YY = RO.grid(H, W, 0.1)
    Z = RO.heights(n, H, W, 1)
    imgs = np.stack([RO.picture(Ih, Iw, 2, noise=10.0)] * n)
    Pp = RO.pplane(Iw, Ih, XX, YY, "inside")
    sync = torch.cuda.synchronize
    rows = []
    with wass_amd.Context(0) as ctx:
        dZ, dI = torch.from_numpy(Z).cuda(), torch.from_numpy(imgs).cuda()
        out = torch.empty((n, H, W), dtype=torch.float32, device="cuda")
        P.radiance(dI, dZ, XX, YY, Pp, ctx=ctx, out=out)
        t = best(lambda: P.radiance(dI, dZ, XX, YY, Pp, ctx=ctx, out=out), sync)
        rows.append(("radiance, device-resident", f"{1e3 * t / n:.3f} ms per frame"))
        hout = np.empty((n, H, W), np.float32)
        t = best(lambda: P.radiance(imgs, Z, XX, YY, Pp, ctx=ctx, out=hout), sync)
        rows.append(("radiance, from the host", f"{1e3 * t / n:.3f} ms per frame"))
        if not a.no_oracle:
            t0 = time.perf_counter()
            RO.radiance(imgs[:1], Z[:1], XX, YY, Pp)
            rows.append(("radiance, numpy oracle, one thread", f"{time.perf_counter() - t0:.2f} s per frame"))
        del dZ, dI, out
        count = a.count
        x = torch.rand((count, H, W), device="cuda")
        y = torch.empty_like(x)
        P.bgimage(x, 2000, ctx=ctx, out=y)
        t = best(lambda: P.bgimage(x, 2000, ctx=ctx, out=y), sync)
        samples = count * H * W
        rows.append((f"bgimage {count} x 1024 x 1024, size 2000, device-resident",
                     f"{t:.3f} s, {1e3 * t / count:.3f} ms per frame, {12 * samples / t / 1e12:.2f} TB/s at 12 B per sample"))
        hx = x.cpu().numpy()
        del x, y
        torch.cuda.empty_cache()
        hy = np.empty_like(hx)
        t = best(lambda: P.bgimage(hx, 2000, ctx=ctx, out=hy), sync, reps=1)
        rows.append((f"bgimage {count} x 1024 x 1024, size 2000, from the host", f"{t:.2f} s, {1e3 * t / count:.3f} ms per frame"))
        if not a.no_oracle:
            from scipy.ndimage import uniform_filter1d
            t0 = time.perf_counter()
            uniform_filter1d(hx[:, :64], size=2000, axis=0, mode="reflect")
            t = (time.perf_counter() - t0) * (H / 64)
            rows.append(("bgimage, scipy on one thread (64 rows timed, scaled to 1024)", f"{t:.1f} s"))
        I, bg = torch.rand((n, H, W), device="cuda"), torch.rand((n, H, W), device="cuda") * 0.1
        for vats in (False, True):
            P.radiance_threshold(I, bg, use_vats=vats, ctx=ctx)
            t = best(lambda: P.radiance_threshold(I, bg, use_vats=vats, ctx=ctx), sync)
            rows.append((f"radiance_threshold, {'VATS' if vats else 'fixed'}, device-resident", f"{1e3 * t / n:.3f} ms per frame"))
    width = max(len(r[0]) for r in rows)
    for name, val in rows:
        print(f"| {name.ljust(width)} | {val} |")


if __name__ == "__main__":
    main()
