#!/usr/bin/env python3
"""Time the variational refinement: VariationalRefinement.optimize on a 1024 x 1024 grid with two 2456 x 2058 pictures, 400 Adam
steps, after warm-up, against the same model written with torch autograd and torch.optim.Adam on the same GPU (the stand-in for
the reference's TensorFlow loop, as scripts/time_grid_dct.py does for the DCT interpolator).

    python scripts/time_refine.py [--n 1024] [--iw 2456] [--ih 2058] [--iters 400] [--reps 5] [--no-torch]

Prints one JSON line: ms for the whole optimize (down-sampling, 400 steps, the loss trace, the result on the host), ms per
iteration, kernel launches per iteration (three per step; one more per row of the loss trace, one forward pass
after the last step and three checks of the input before the first) and the torch loop's figures.

    python scripts/time_refine.py --batch 1,2,4,8,16 [--parent-lib OTHER/libwassgpu.so] [--reps 5]

times the refinement of a sequence instead (one JSON line again): SequenceRefiner.refine (load, 400 steps, result; device tensors in
and out) per batch size on distinct frames, ms per call and per frame, the median of --reps after a warm-up of every shape;
refine_surface frame by frame (create, host down-sampling, destroy) against refine_sequence on the same host arrays; and, with
--parent-lib, the single entry (optimize_coarse on device tensors) of this build and of that build of the library, alternated in
fresh processes (WASS_GPU_LIB), with the run-to-run spread of the repeated single run.
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import wass_amd  # noqa: E402
from wass_amd import refinement  # noqa: E402


def texture(h, w, seed):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    t = np.zeros((h, w), np.float32)
    for _ in range(4):
        fx, fy = rng.uniform(-0.05, 0.05, 2)
        t += np.float32(rng.uniform(0.3, 1.0)) * np.sin(np.float32(fx) * x + np.float32(fy) * y + np.float32(rng.uniform(0, 6.28)))
    return (127.5 + 120.0 * t / np.abs(t).max()).astype(np.float32)


def rig(n, ih, iw):
    """two cameras 4 units above the grid [-1, 1]^2, looking down; the nodes project over the middle 70 % of the pictures"""
    XX, YY = np.meshgrid(np.linspace(-2, 2, n), np.linspace(-2, 2, n))
    fx, fy = 0.7 * (iw - 1) / 2.0 * 4.0, 0.7 * (ih - 1) / 2.0 * 4.0
    K = np.array([[fx, 0, (iw - 1) / 2.0], [0, fy, (ih - 1) / 2.0], [0, 0, 1.0]])
    P0 = K @ np.hstack([np.eye(3), np.zeros((3, 1))])
    P1 = K @ np.hstack([np.eye(3), np.array([[-0.12], [0.0], [0.0]])])
    yy, xx = np.mgrid[0:n, 0:n] / n
    Z0 = (0.05 * np.sin(9 * xx) * np.cos(7 * yy)).astype(np.float32)
    return dict(I0=texture(ih, iw, 1), I1=texture(ih, iw, 2), Rp2c=np.eye(3), Tp2c=np.array([0.0, 0.0, 4.0]), P0cam=P0, P1cam=P1, XX=XX, YY=YY,
                baseline=2.0, mask=np.ones((n, n), np.float32)), Z0


def torch_loop(a, Z0, iters, alpha=10.0, lr=1e-3):
    """the reference's loop with torch: autograd through resize, projection, a bilinear sampler made of gathers, conv2d; Adam"""
    dev = torch.device("cuda")
    t = lambda v: torch.as_tensor(np.asarray(v, np.float32), device=dev)  # noqa: E731
    n = Z0.shape[0]
    X, Y, mask = t(a["XX"] / a["baseline"]).reshape(-1), t(a["YY"] / a["baseline"]).reshape(-1), t(a["mask"]).reshape(-1)
    R, T, Ps, Is = t(a["Rp2c"]), t(a["Tp2c"]).reshape(3, 1), (t(a["P0cam"]), t(a["P1cam"])), (t(a["I0"]), t(a["I1"]))
    kx, ky = refinement.derivative_of_gaussian_win(7, 0.8)
    kernels = t(np.stack([kx, ky]))[:, None]
    zc = torch.nn.functional.interpolate(t(Z0)[None, None], size=(n // 2, n // 2), mode="bilinear", align_corners=False)[0, 0].clone().requires_grad_(True)
    opt = torch.optim.Adam([zc], lr=lr, eps=1e-7)
    ones = torch.ones((1, n * n), device=dev)

    def energy():
        Z = torch.nn.functional.interpolate(zc[None, None], size=(n, n), mode="bilinear", align_corners=False)[0, 0]
        cam = R @ torch.stack([X, Y, Z.reshape(-1)]) + T
        hom = torch.cat([cam, ones])
        samples = []
        for P, I in zip(Ps, Is):
            s = P @ hom
            u, v = s[0] / s[2], s[1] / s[2]
            H, W = I.shape
            fx, fy = u.detach().floor().clamp(0, W - 2), v.detach().floor().clamp(0, H - 2)
            ax, ay = (u - fx).clamp(0, 1), (v - fy).clamp(0, 1)
            base = (fy * W + fx).long()
            flat = I.reshape(-1)
            tl, tr, bl, br = flat[base], flat[base + 1], flat[base + W], flat[base + W + 1]
            top, bot = ax * (tr - tl) + tl, ax * (br - bl) + bl
            samples.append((ay * (bot - top) + top) * mask)
        data = torch.mean(torch.square((samples[0] - samples[1]) / 255.0))
        slopes = torch.nn.functional.conv2d(Z[None, None], kernels, padding=3)[0]
        return data + alpha * torch.mean(torch.square(slopes[0]) + torch.square(slopes[1]))

    losses = []
    for ii in range(iters):
        opt.zero_grad()
        e = energy()
        e.backward()
        opt.step()
        if ii % 10 == 0:
            with torch.no_grad():
                losses.append(energy())
    torch.cuda.synchronize()
    return zc.detach(), [float(v) for v in losses]


def sequence_frames(n, ih, iw, count):
    """`count` distinct frames on the rig: the set-up mapping, surfaces in metres (z up), uint8 pictures"""
    args, Z0 = rig(n, ih, iw)
    setup = {"Rpl": np.eye(3), "Tpl": -np.asarray(args["Tp2c"], float).reshape(3, 1), "P0cam": args["P0cam"], "P1cam": args["P1cam"],
             "XX": args["XX"], "YY": args["YY"], "CAM_BASELINE": args["baseline"]}
    yy, xx = np.mgrid[0:n, 0:n] / n
    Zi = np.stack([(-0.1 * np.sin(9 * xx + 0.3 * f) * np.cos(7 * yy - 0.2 * f)).astype(np.float32) for f in range(count)])
    I0 = np.stack([np.round(texture(ih, iw, 10 + 2 * f)).astype(np.uint8) for f in range(count)])
    I1 = np.stack([np.round(texture(ih, iw, 11 + 2 * f)).astype(np.uint8) for f in range(count)])
    return setup, Zi, I0, I1


def single_loop(a):
    """the single entry on device tensors, --reps times after a warm-up: what a child process of time_sequence prints"""
    args, Z0 = rig(a.n, a.ih, a.iw)
    with wass_amd.Context(0) as ctx, refinement.VariationalRefinement(ctx=ctx, **args) as vr:
        d_zc = torch.as_tensor(refinement.downsample_linear(Z0, a.n // 2, a.n // 2), device="cuda")
        vr.optimize_coarse(d_zc, a.iters)
        ms = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            vr.optimize_coarse(d_zc, a.iters)
            ms.append((time.perf_counter() - t0) * 1e3)
    print(json.dumps({"ms": ms}))


def time_sequence(a):
    sizes = sorted({int(v) for v in a.batch.split(",")})
    setup, Zi, I0, I1 = sequence_frames(a.n, a.ih, a.iw, max(max(sizes), 4))
    res = {"n": a.n, "picture": [a.ih, a.iw], "iters": a.iters, "reps": a.reps, "batches": {}}
    opts = refinement.RefineOptions(max_iters=a.iters)
    lib = wass_amd._lib.load()
    with wass_amd.Context(0) as ctx:
        dev = torch.device("cuda", ctx.device_id)
        d_Zi, d_I0, d_I1 = (torch.from_numpy(v).to(dev) for v in (Zi, I0, I1))
        d_I0, d_I1 = d_I0.float(), d_I1.float()
        for b in sizes:
            nbytes = ctypes.c_size_t(0)
            lib.wass_vref_batch_scratch_bytes(b, a.n, a.n, a.ih, a.iw, a.ih, a.iw, ctypes.byref(nbytes))
            with refinement.SequenceRefiner(setup, ((a.ih, a.iw), (a.ih, a.iw)), b, ctx) as sr:
                out = torch.empty((b, a.n, a.n), dtype=torch.float32, device=dev)
                sr.refine(d_Zi[:b], d_I0[:b], d_I1[:b], refinement.RefineOptions(max_iters=3), out=out)          # warm-up of this shape
                ms = []
                for _ in range(a.reps):
                    t0 = time.perf_counter()
                    sr.refine(d_Zi[:b], d_I0[:b], d_I1[:b], opts, out=out)
                    ms.append((time.perf_counter() - t0) * 1e3)
                e = [float(sr.losses[b - 1][0][3]), float(sr.losses[b - 1][-1][3])]
            med = float(np.median(ms))
            res["batches"][str(b)] = {"ms_per_call": round(med, 3), "ms_per_frame": round(med / b, 3), "all": [round(t, 3) for t in ms],
                                      "scratch_MiB": round(nbytes.value / 2 ** 20, 1), "energy_first_last_of_last_frame": e}
        # what a user of a sequence sees: host arrays in, host arrays out, 4 frames
        nf = 4
        refinement.refine_surface(Zi[0], np.ones_like(Zi[0]), I0[0], I1[0], setup, ctx=ctx, max_iters=3)
        refinement.refine_sequence(Zi[:nf], I0[:nf], I1[:nf], setup, options=refinement.RefineOptions(max_iters=3), ctx=ctx)
        one, seq = [], []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            for f in range(nf):
                refinement.refine_surface(Zi[f], np.ones_like(Zi[f]), I0[f], I1[f], setup, ctx=ctx, max_iters=a.iters)
            one.append((time.perf_counter() - t0) * 1e3 / nf)
            t0 = time.perf_counter()
            refinement.refine_sequence(Zi[:nf], I0[:nf], I1[:nf], setup, options=opts, ctx=ctx)
            seq.append((time.perf_counter() - t0) * 1e3 / nf)
        res["host_arrays_ms_per_frame"] = {"refine_surface": round(float(np.median(one)), 3), "refine_sequence": round(float(np.median(seq)), 3),
                                           "refine_sequence_batch": opts.batch, "frames": nf}
    # the single entry of this build and of another one, alternated in fresh processes
    if a.parent_lib:
        runs = {"this": [], "parent": []}
        cmd = [sys.executable, os.path.abspath(__file__), "--single-child", "--n", str(a.n), "--iw", str(a.iw), "--ih", str(a.ih), "--iters",
               str(a.iters), "--reps", str(a.reps)]
        for _ in range(3):
            for which in ("this", "parent"):
                env = dict(os.environ)
                env.pop("WASS_GPU_LIB", None)
                if which == "parent":
                    env["WASS_GPU_LIB"] = os.path.abspath(a.parent_lib)
                line = subprocess.run(cmd, env=env, capture_output=True, text=True, check=True, timeout=300).stdout.strip().splitlines()[-1]
                runs[which].append(round(float(np.median(json.loads(line)["ms"])), 3))
        res["single_entry_ms"] = {k: {"medians_of_runs": v, "median": round(float(np.median(v)), 3), "spread": round(max(v) - min(v), 3)}
                                  for k, v in runs.items()}
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", help="comma-separated batch sizes: time the refinement of a sequence instead")
    ap.add_argument("--parent-lib", help="another build of libwassgpu.so whose single entry is timed in alternation")
    ap.add_argument("--single-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--iw", type=int, default=2456)
    ap.add_argument("--ih", type=int, default=2058)
    ap.add_argument("--iters", type=int, default=400)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-torch", action="store_true")
    a = ap.parse_args()
    if a.single_child:
        return single_loop(a)
    if a.batch:
        return time_sequence(a)
    args, Z0 = rig(a.n, a.ih, a.iw)
    res = {"n": a.n, "picture": [a.ih, a.iw], "iters": a.iters}
    with wass_amd.Context(0) as ctx, refinement.VariationalRefinement(ctx=ctx, **args) as vr:
        vr.optimize(Z0, max_iters=3)                                   # warm-up (code objects, allocations)
        whole, loop = [], []
        d_zc = torch.as_tensor(refinement.downsample_linear(Z0, a.n // 2, a.n // 2), device="cuda")
        for _ in range(a.reps):
            t0 = time.perf_counter()
            vr.optimize(Z0, max_iters=a.iters)
            whole.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            vr.optimize_coarse(d_zc, a.iters)                          # device tensors in and out: the loop and its set-up only
            loop.append((time.perf_counter() - t0) * 1e3)
        rows = len(vr.losses)
        res.update(ms_optimize=round(float(np.median(whole)), 3), ms_optimize_all=[round(t, 3) for t in whole],
                   ms_loop=round(float(np.median(loop)), 3), ms_per_iteration=round(float(np.median(loop)) / a.iters, 4),
                   launches_per_iteration=round((3 * a.iters + rows + 4) / a.iters, 3), trace_rows=rows,
                   energy_first_last=[float(vr.losses[0][3]), float(vr.losses[-1][3])])
    if not a.no_torch:
        torch_loop(args, Z0, 3)
        tt = []
        for _ in range(max(1, a.reps // 2)):
            t0 = time.perf_counter()
            _, losses = torch_loop(args, Z0, a.iters)
            tt.append((time.perf_counter() - t0) * 1e3)
        res.update(torch_ms_loop=round(float(np.median(tt)), 3), torch_ms_per_iteration=round(float(np.median(tt)) / a.iters, 4),
                   torch_energy_first_last=[losses[0], losses[-1]], ratio=round(float(np.median(tt)) / float(np.median(loop)), 2))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
