#!/usr/bin/env python3
"""Times the pyramid upsampling on the GPU: `pyr_up` of a count x 1024 x 1024 float32 cube on the device (one level, 1024^2 ->
2048^2: 4 B read and 16 B written per source cell), and `radiance_upscaled` at upscalefactor 2 of a 1024 x 1024 cube beside
`radiance` of a cube that already is 2048 x 2048, both sampled from a 2456 x 2058 picture whose footprint lies inside.  Best of
`--reps` runs after a warm-up of the same shapes, a host clock around the call and a device synchronisation; the two radiance
calls alternate.  Prints a table for DESIGN.md.  Needs a GPU: there is no fall-back.

    python scripts/time_pyramid.py [--count 256] [--frames 16] [--reps 5]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def timed(fn, sync):
    sync()
    t0 = time.perf_counter()
    fn()
    sync()
    return time.perf_counter() - t0


def pyr_up_bytes(count, H, W, elem=4):
    """one level: every source cell read once, four destination cells written"""
    return count * H * W * elem * (1 + 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--count", type=int, default=256, help="frames of the pyr_up cube (256: 1 GiB in, 4 GiB out per call)")
    ap.add_argument("--frames", type=int, default=16, help="frames of the radiance cubes")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import torch
    import pyramid_oracle as PO
    import radiance_oracle as RO
    import wass_amd
    from wass_amd import postproc as P

    H = W = 1024
    Iw, Ih = 2456, 2058
    sync = torch.cuda.synchronize
    rows = []
    with wass_amd.Context(0) as ctx:
        n = a.count
        x = torch.rand((n, H, W), device="cuda")
        y = torch.empty((n, 2 * H, 2 * W), dtype=torch.float32, device="cuda")
        P.pyr_up(x, ctx=ctx, out=y)
        t = min(timed(lambda: P.pyr_up(x, ctx=ctx, out=y), sync) for _ in range(a.reps))
        check = PO.pyr_up(x[:1, :64].cpu().numpy())[0, :126]              # rows that do not see the cut
        assert np.array_equal(y[0, :126].cpu().numpy(), check), "pyr_up does not equal the oracle"
        rows.append((f"pyr_up {n} x 1024 x 1024 float32 -> 2048 x 2048, device-resident",
                     f"{1e3 * t / n:.4f} ms per frame, {pyr_up_bytes(n, H, W) / t / 1e12:.2f} TB/s at 4 B read + 16 B written per source cell"))
        x64 = torch.rand((2, H, W), dtype=torch.float64, device="cuda")
        y64 = torch.empty((2, 2 * H, 2 * W), dtype=torch.float64, device="cuda")
        P.pyr_up(x64, ctx=ctx, out=y64)
        t = min(timed(lambda: P.pyr_up(x64, ctx=ctx, out=y64), sync) for _ in range(a.reps))
        rows.append(("pyr_up 2 x 1024 x 1024 float64 (the grid's XX, YY), device-resident",
                     f"{1e3 * t / 2:.4f} ms per frame, {pyr_up_bytes(2, H, W, 8) / t / 1e12:.2f} TB/s"))
        del x, y, x64, y64
        n = a.frames
        XX, YY = RO.grid(H, W, 0.1)
        XX2, YY2 = RO.grid(2 * H, 2 * W, 0.05)
        Pp = RO.pplane(Iw, Ih, XX, YY, "inside")
        dI = torch.from_numpy(np.stack([RO.picture(Ih, Iw, 2, noise=10.0)] * n)).cuda()
        dZ = torch.from_numpy(RO.heights(n, H, W, 1)).cuda()
        dZ2 = torch.from_numpy(RO.heights(n, 2 * H, 2 * W, 1)).cuda()
        out = torch.empty((n, 2 * H, 2 * W), dtype=torch.float32, device="cuda")
        up = lambda: P.radiance_upscaled(dI, dZ, XX, YY, Pp, 2, ctx=ctx, out=out)
        plain = lambda: P.radiance(dI, dZ2, XX2, YY2, Pp, ctx=ctx, out=out)
        up(); plain()
        tu, tp = [], []
        for _ in range(a.reps):
            tu.append(timed(up, sync))
            tp.append(timed(plain, sync))
        rows.append((f"radiance_upscaled, upscalefactor 2, {n} x 1024 x 1024 -> 2048 x 2048, device-resident", f"{1e3 * min(tu) / n:.3f} ms per frame"))
        rows.append((f"radiance of a cube already {n} x 2048 x 2048, device-resident", f"{1e3 * min(tp) / n:.3f} ms per frame"))
        rows.append(("the upsampling's share of radiance_upscaled (difference of the two)", f"{100 * (min(tu) - min(tp)) / min(tu):.0f} %"))
    width = max(len(r[0]) for r in rows)
    for name, val in rows:
        print(f"| {name.ljust(width)} | {val} |")


if __name__ == "__main__":
    main()
