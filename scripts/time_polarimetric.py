#!/usr/bin/env python3
"""Times `polarimetric_setup` on the GPU: ms per frame for 16 frames of a 1024 x 1024 grid sampled from 2456 x 2058 float32 Stokes
pictures, device-resident and from the host, with the default outputs and with all of them; beside it the numpy oracle's seconds
for one frame on one thread (tests/polarimetric_oracle.py), and `clip_cube` and `zeromean` on the same cube.  Prints a table for
DESIGN.md.  No speed is promised.

    python scripts/time_polarimetric.py [--frames 16] [--no-oracle]
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
    ap.add_argument("--no-oracle", action="store_true")
    a = ap.parse_args()
    import torch
    import polarimetric_oracle as PO
    import radiance_oracle as RO
    import visibility_oracle as VO
    import wass_amd
    from wass_amd import postproc as P

    H = W = 1024
    Iw, Ih = 2456, 2058
    n = a.frames
    XX, YY = RO.grid(H, W, 0.1)
    Z = RO.heights(n, H, W, 1)
    one = PO.stokes_pictures(1, Ih, Iw, 2)
    stokes = np.ascontiguousarray(np.broadcast_to(one, (n, 3, Ih, Iw)))
    Pp = RO.pplane(Iw, Ih, XX, YY, "inside")
    cam = VO.camera(XX, YY, "west", 8.0, 30.0)
    K = PO.intrinsics(Iw, Ih)
    every = P.POL_OUTPUTS
    sync = torch.cuda.synchronize
    rows = []
    with wass_amd.Context(0) as ctx:
        dZ, dS = torch.from_numpy(Z).cuda(), torch.from_numpy(stokes).cuda()
        for what, outs in (("S and the mask", ("S", "occlusion")), ("every output", every)):
            run = lambda: P.polarimetric_setup(dS, dZ, XX, YY, Pp, cam, K, outputs=outs, ctx=ctx)
            run()
            rows.append((f"polarimetric_setup, device-resident, {what}", f"{1e3 * best(run, sync) / n:.3f} ms per frame"))
        del dS
        torch.cuda.empty_cache()
        for what, outs in (("S and the mask", ("S", "occlusion")), ("every output", every)):
            run = lambda: P.polarimetric_setup(stokes, Z, XX, YY, Pp, cam, K, outputs=outs, ctx=ctx)
            rows.append((f"polarimetric_setup, from the host, {what}", f"{1e3 * best(run, sync, reps=2) / n:.3f} ms per frame"))
        run = lambda: P.visibility_map(dZ, XX, YY, cam, angle_limit=85.0, ctx=ctx)
        run()
        rows.append(("of which visibility_map, device-resident", f"{1e3 * best(run, sync) / n:.3f} ms per frame"))
        if not a.no_oracle:
            t0 = time.perf_counter()
            PO.setup(stokes[:1], Z[:1], XX, YY, Pp, cam, K)
            rows.append(("polarimetric_setup, numpy oracle, one thread", f"{time.perf_counter() - t0:.2f} s per frame"))
        out = torch.empty_like(dZ)
        for name, run in (("clip_cube", lambda: P.clip_cube(dZ, -100.0, 100.0, out=out, ctx=ctx)), ("zeromean", lambda: P.zeromean(dZ, out=out, ctx=ctx))):
            run()
            rows.append((f"{name} {n} x 1024 x 1024, device-resident", f"{1e3 * best(run, sync) / n:.3f} ms per frame"))
        hout = np.empty_like(Z)
        for name, run in (("clip_cube", lambda: P.clip_cube(Z, -100.0, 100.0, out=hout, ctx=ctx)), ("zeromean", lambda: P.zeromean(Z, out=hout, ctx=ctx))):
            rows.append((f"{name} {n} x 1024 x 1024, from the host", f"{1e3 * best(run, sync) / n:.3f} ms per frame"))
    width = max(len(r[0]) for r in rows)
    for name, val in rows:
        print(f"| {name.ljust(width)} | {val} |")


if __name__ == "__main__":
    main()
