#!/usr/bin/env python3
"""Times the grid set-up on the GPU against the host doing the same thing with numpy, in one run on one machine: a cloud of
`--points` points (4 million) on a 1024 x 1024 grid.

  the quantile entry alone   Mesh.aligned_z_quantiles([0.98, 0.02]) on the resident mesh, and Context.quantiles_dev on a device
                             array of the same heights, against align_on_sea_plane_RT's R @ mesh + T followed by the reference's
                             two np.quantile calls (wassgridsurface.py:87, 122-123)
  setup_grid as a whole      files read, cloud uploaded, quantiles, algebra, coverage, the warped picture; against the host's
                             load_camera_mesh + alignment + quantiles (the rest of setup() is the same numpy on either side)

Median of `--reps` runs after `--warmup` runs of the same shapes, a host clock around calls that end in a device synchronisation;
GPU and host runs alternate.  Prints a table for DESIGN.md and the bytes the selection's passes read.  Needs a GPU: no fall-back.
The rig, its files and the oracle come from the test suite (tests/test_grid_setup.py, tests/grid_setup_oracle.py), as
scripts/soak.py and scripts/cli_throughput.py take theirs from tests/test_cli.py: the script runs from a checkout with tests/.

    python scripts/time_grid_setup.py [--points 4000000] [--reps 25] [--warmup 3]
"""
import argparse
import os
import statistics
import struct
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def write_xyzc(path, pts):
    """3 x N camera-frame points as a mesh_cam.xyzC file (identity Rinv, zero Tinv): what load_camera_mesh reads back"""
    lo, hi = pts.min(axis=1), pts.max(axis=1)
    scale = 65535.0 / (hi - lo)
    q = np.clip(np.rint((pts - lo[:, None]) * scale[:, None]), 0, 65535).astype("<u2")
    with open(path, "wb") as f:
        f.write(struct.pack("<I", pts.shape[1]))
        f.write(np.concatenate([scale, lo, np.eye(3).ravel(), np.zeros(3)]).astype("<f8").tobytes())
        f.write(np.ascontiguousarray(q.T).tobytes())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=4_000_000)
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    import torch
    import grid_setup_oracle as G
    import test_grid_setup as TS
    import wass_amd
    from wass_amd import gridding

    n, N = a.points, 1024
    rng = np.random.default_rng(1)
    Rpl, Tpl = G.sea_plane_RT(TS.PLANE)
    gx, gy = rng.uniform(-27.0, 27.0, n), rng.uniform(-62.0, -8.0, n)
    hz = 0.3 * np.sin(gx * 0.7) + 0.2 * np.cos(gy * 0.5) + rng.normal(0, 0.05, n)
    pts = Rpl.T @ (np.stack([gx, gy, -hz]) / TS.BASELINE - Tpl)
    area = dict(area_center=np.array([0.0, -35.0]), area_size_x=50.0, area_size_y=50.0, Nx=N, Ny=N)
    with tempfile.TemporaryDirectory() as root, wass_amd.Context(0) as ctx:
        wd = os.path.join(root, "000000_wd")
        picture = rng.integers(0, 256, (TS.IH, TS.IW), dtype=np.uint8)
        TS.write_workdir(wd, picture=picture)
        write_xyzc(os.path.join(wd, "mesh_cam.xyzC"), pts)
        cloud = gridding.load_camera_mesh(os.path.join(wd, "mesh_cam.xyzC"))
        mesh = gridding.upload_camera_mesh(ctx, cloud)
        d_z = torch.from_numpy(G.aligned_z(cloud.T, Rpl, Tpl, TS.BASELINE)).cuda()
        torch.cuda.synchronize()

        def host_quantiles():
            al = Rpl @ cloud + Tpl
            al[2, :] *= -1.0
            z = (al * TS.BASELINE)[2, :]
            return np.quantile(z, 0.98), np.quantile(z, 0.02)

        def host_whole():
            gridding.load_camera_mesh(os.path.join(wd, "mesh_cam.xyzC"))
            host_quantiles()

        runs = {"gpu mesh": lambda: mesh.aligned_z_quantiles(Rpl, Tpl, TS.BASELINE, [0.98, 0.02]),
                "gpu array": lambda: ctx.quantiles_dev(d_z, [0.98, 0.02]),
                "host quantiles": host_quantiles,
                "gpu setup_grid": lambda: gridding.setup_grid(wd, TS.PLANE, TS.BASELINE, **area, ctx=ctx),
                "host whole": host_whole}
        got = runs["gpu mesh"]()[0]
        want = G.quantile(G.aligned_z(cloud.T, Rpl, Tpl, TS.BASELINE), [0.98, 0.02])
        assert np.array_equal(got, want) and np.array_equal(runs["gpu array"](), want), "the GPU does not equal the oracle"
        print("difference to the host's BLAS alignment, in metres:", np.abs(np.array(host_quantiles()) - want))
        times = {k: [] for k in runs}
        for rep in range(a.warmup + a.reps):
            for k, fn in runs.items():                       # alternating
                t = timed(fn)
                if rep >= a.warmup:
                    times[k].append(t)
        mesh.close()
    med = {k: statistics.median(v) for k, v in times.items()}
    spread = {k: (min(v), max(v)) for k, v in times.items()}
    per_block, per_launch = wass_amd.stereo.quantiles_launch_shape()
    passes = (1 + 6 * 2) * n * 9                             # pass 0 once, five digit passes and the next-value pass per q: 8 B height + 1 B mask
    align = n * (3 * 8 + 1 + 8)
    rows = [(f"aligned_z_quantiles, 2 quantiles of {n} points, resident mesh", "gpu mesh"),
            ("quantiles_dev, the same heights as a device array", "gpu array"),
            ("host: R @ mesh + T, np.quantile twice", "host quantiles"),
            (f"setup_grid as a whole, {N} x {N} grid", "gpu setup_grid"),
            ("host: load_camera_mesh, alignment, np.quantile twice", "host whole")]
    width = max(len(r[0]) for r in rows)
    for name, k in rows:
        print(f"| {name.ljust(width)} | {1e3 * med[k]:.3f} ms (min {1e3 * spread[k][0]:.3f}, max {1e3 * spread[k][1]:.3f}) |")
    print(f"numpy {np.__version__}, {os.cpu_count()} host CPUs, torch {torch.__version__}, {torch.cuda.get_device_name(0)}")
    print(f"the mesh call reads {(passes + align) / 1e6:.0f} MB in 1 + 13 sweeps and 15 launches: {(passes + align) / med['gpu mesh'] / 1e12:.2f} TB/s "
          f"if that were all; {per_launch // per_block} workgroups of {per_block} elements per sweep")


if __name__ == "__main__":
    main()
