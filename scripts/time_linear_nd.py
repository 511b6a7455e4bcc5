"""Times the LinearND interpolator (wass_amd.gridding.linear_nd, grid_linear.hip) at the production size: a 1024 x 1024 lattice
and a synthetic cloud of about 4 M points with a hole and a dense corner, milliseconds per frame by stage (bucket, hull, walk)
and the nodes per flag, beside scipy.interpolate.LinearNDInterpolator on the same machine -- on a stated fraction of the cloud
and of the lattice when the whole would take minutes.

    python scripts/time_linear_nd.py [--n 4000000] [--grid 1024] [--reps 5] [--scipy-points 400000] [--scipy-grid 256] [--log FILE]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def synthetic_cloud(n, seed=1):
    """uniform over the unit square with a disc of radius 0.15 about (0.6, 0.4) removed, a tenth of the points in the corner
    [0, 0.05]^2, and a margin of 0.02 that stays empty so that part of the lattice lies outside the hull"""
    rng = np.random.default_rng(seed)
    p = 0.02 + 0.96 * rng.random((int(1.2 * n), 2))
    p = p[(p[:, 0] - 0.6) ** 2 + (p[:, 1] - 0.4) ** 2 > 0.15 ** 2][:n - n // 10]
    p = np.concatenate([p, 0.02 + 0.05 * rng.random((n // 10, 2))])
    z = 0.3 * np.sin(40.0 * p[:, 0]) * np.cos(25.0 * p[:, 1]) + 0.01 * rng.normal(size=p.shape[0])
    return np.ascontiguousarray(np.stack([p[:, 0], p[:, 1], z]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4_000_000)
    ap.add_argument("--grid", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scipy-points", type=int, default=400_000, help="points of the cloud handed to scipy (0: skip scipy)")
    ap.add_argument("--scipy-grid", type=int, default=256, help="side of the lattice scipy evaluates")
    ap.add_argument("--log", default=None)
    args = ap.parse_args()
    import torch
    import wass_amd
    from wass_amd import gridding, stereo

    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    pts = synthetic_cloud(args.n)
    n, G = pts.shape[1], args.grid
    gs = stereo.grid_setup(np.eye(3), np.zeros(3), 1.0, 0.0, 1.0, 0.0, 1.0, G, G)
    say(f"LinearND: {n} points, {G} x {G} lattice, scratch {stereo.linear_scratch_bytes(n, G, G) / 2 ** 20:.0f} MiB, "
        f"device {torch.cuda.get_device_name(0)}")
    with wass_amd.Context(0) as ctx:
        dev = torch.device("cuda", ctx.device_id)
        d = [torch.from_numpy(pts[k]).to(dev) for k in range(3)]
        d_out = torch.empty((G, G), dtype=torch.float64, device=dev)
        d_flags = torch.empty((G, G), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)
        rows = []
        for rep in range(args.reps + 1):                     # the first call grows the scratch and is not counted
            t0 = time.perf_counter()
            info = ctx.grid_linear_dev(d[0], d[1], d[2], gs, d_out, d_flags, timing=True)
            wall = (time.perf_counter() - t0) * 1e3
            if rep:
                rows.append((info["ms_bucket"], info["ms_hull"], info["ms_walk"], wall))
            say(f"  call {rep}: bucket {info['ms_bucket']:.2f} ms, hull {info['ms_hull']:.2f} ms (hand-over and host chain included), "
                f"walk {info['ms_walk']:.2f} ms, call {wall:.2f} ms")
        med = np.median(np.array(rows), axis=0)
        say(f"median of {args.reps}: bucket {med[0]:.2f} ms, hull {med[1]:.2f} ms, walk {med[2]:.2f} ms, whole call {med[3]:.2f} ms per frame")
        say(f"flags 0 / 1 / 2 / 3: {info['counts']}; points taken {info['n_taken']}; acceleration grid {info['accel']}; "
            f"hull {info['hull_vertices']} vertices of {info['hull_candidates']} candidates handed to the host")
        out = d_out.cpu().numpy()
        flags = d_flags.cpu().numpy()
    if args.scipy_points:
        from scipy.interpolate import LinearNDInterpolator
        m, g = min(args.scipy_points, n), args.scipy_grid
        sel = np.random.default_rng(2).choice(n, m, replace=False) if m < n else np.arange(n)
        q = np.linspace(0.0, 1.0, g)
        XX, YY = np.meshgrid(q, q)
        t0 = time.perf_counter()
        f = LinearNDInterpolator(pts[:2, sel].T, pts[2, sel])
        t1 = time.perf_counter()
        ref = f(XX, YY)
        t2 = time.perf_counter()
        say(f"scipy LinearNDInterpolator on {m} of the {n} points ({100.0 * m / n:.0f} %): triangulation {t1 - t0:.1f} s, "
            f"{g} x {g} nodes {t2 - t1:.2f} s ({os.cpu_count()} CPUs seen, Qhull uses one)")
        if m == n and (G - 1) % (g - 1) == 0:
            s = (G - 1) // (g - 1)
            o, fl = out[::s, ::s], flags[::s, ::s]
            decided = fl <= 1
            say(f"  same cloud: NaN pattern equal on the decided nodes: {np.array_equal(np.isnan(o)[decided], np.isnan(ref)[decided])}; "
                f"max |ours - scipy| on flag 0: {np.nanmax(np.abs(o[fl == 0] - ref[fl == 0])):.3g}")
    if args.log:
        with open(args.log, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
