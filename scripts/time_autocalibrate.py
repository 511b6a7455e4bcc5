#!/usr/bin/env python3
"""Times the autocalibration on the GPU at 50 frames x 400 matches (N = 20 000 pooled matches), per stage, in ms.

  essential   epipolar.find_essential over the pooled matches, 1024 hypotheses
  choose      wass_ac_triangulate_dev: the four candidates' points and counts, with upload and download
  linearize   wass_ac_linearize_dev on the points of the bundle adjustment (points already on the device)
  step        wass_ac_step_dev: linearisation, Schur sums, the 12 x 12 solve on the host, back-substitution
  bundle      bundle_adjust as a whole, its iterations, and the time per Levenberg-Marquardt iteration
  after       the host's part after the bundle adjustment: statistics, homography
  whole       autocalibrate from the pooled matches to the result

Median of `--reps` runs after `--warmup` runs of the same shapes, a host clock around calls that end in a device synchronisation.
Prints a table for DESIGN.md.  Needs a GPU: no fall-back.  The scenes come from the test suite's oracle
(tests/epipolar_oracle.py): the script runs from a checkout with tests/.

    python scripts/time_autocalibrate.py [--frames 50] [--matches 400] [--rounds 1024] [--reps 5] [--warmup 2]
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=50)
    ap.add_argument("--matches", type=int, default=400)
    ap.add_argument("--rounds", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    import torch
    import epipolar_oracle as O
    import wass_amd
    from wass_amd import autocalibrate as AC
    from wass_amd import epipolar as EP

    g = O.rig(500)
    K0, K1 = g[0], g[1]
    frames = [O.scene(g, a.matches, 700 + f, noise=0.2)[:2] for f in range(a.frames)]
    p0 = np.concatenate([f[0] for f in frames]).astype(np.float64)
    p1 = np.concatenate([f[1] for f in frames]).astype(np.float64)
    x0, x1 = AC._normalise(p0, K0), AC._normalise(p1, K1)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    t = {k: [] for k in ("essential", "choose", "linearize", "step", "bundle", "after", "whole")}
    with wass_amd.Context(0) as ctx:
        lib, h = ctx._lib, ctx._h
        for rep in range(a.warmup + a.reps):
            dt_e, best = timed(lambda: EP.find_essential(x0, x1, 1.5 / K0[0, 0], a.rounds, None, ctx))
            R4, T4 = AC.pose_candidates(best.E)
            dt_c, (pts4, counts) = timed(lambda: AC.triangulate_candidates(R4, T4, x0, x1, best.mask, ctx))
            k = AC.choose_pose(counts, R4)
            keep = AC.select_points(pts4[k], best.mask)
            P, obs = np.ascontiguousarray(pts4[k][keep]), np.ascontiguousarray(np.concatenate([x0[keep], x1[keep]], axis=1))
            cams = AC.make_cams(np.eye(3), np.zeros(3), R4[k], T4[k])
            n = P.shape[0]
            d_p, d_o = torch.from_numpy(P).cuda(), torch.from_numpy(obs).cuda()
            sums, S, rhs, da, cn, scal = np.zeros(AC.LIN_SUMS), np.zeros(144), np.zeros(12), np.zeros(12), np.zeros(30), np.zeros(4)
            ok = C.c_int(0)
            dt_l, _ = timed(lambda: ctx._check(lib.wass_ac_linearize_dev(h, AC._dp(cams), d_p.data_ptr(), d_o.data_ptr(), n, None, AC._dp(sums))))
            mu = 1e-3 * sums[56]
            dt_s, _ = timed(lambda: ctx._check(lib.wass_ac_step_dev(h, AC._dp(cams), d_p.data_ptr(), d_o.data_ptr(), n, mu, AC._dp(S), AC._dp(rhs),
                                                                    AC._dp(da), None, None, AC._dp(cn), AC._dp(scal), C.byref(ok))))
            dt_b, ba = timed(lambda: AC.bundle_adjust(R4[k], T4[k], P, obs[:, :2], obs[:, 2:], 1000, ctx))

            def after():
                R, T = AC.relative_pose(ba.R0, ba.T0, ba.R1, ba.T1)
                return (AC.structure_error_stats(P, p0[keep], p1[keep], R4[k], T4[k], K0, K1),
                        EP.epipolar_error_stats(AC.fundamental(best.E, K0, K1), p0[keep], p1[keep]),
                        EP.epipolar_error_stats(AC.fundamental(AC.skew(T) @ R, K0, K1), p0[keep], p1[keep]), AC.homography_lsq(p0[keep], p1[keep]))
            dt_a, _ = timed(after)
            dt_w, res = timed(lambda: AC.autocalibrate(p0, p1, x0, x1, K0, K1, a.rounds, ctx))
            if rep >= a.warmup:
                for key, v in zip(t, (dt_e, dt_c, dt_l, dt_s, dt_b, dt_a, dt_w)):
                    t[key].append(v)
        med = {k: 1e3 * statistics.median(v) for k, v in t.items()}
    print(f"N = {p0.shape[0]} pooled matches, {n} points in the bundle adjustment, {ba.iters} iterations, stop reason {ba.reason}, "
          f"|e|^2 {ba.err0:.4g} -> {ba.err1:.4g}; code {res.code}, epipolar error {res.err_before[0]:.4f} -> {res.err_after[0]:.4f} px")
    print("| essential | choose | linearize | step | bundle | per LM iteration | after | whole |   (ms)")
    print("|---|---|---|---|---|---|---|---|")
    print(f"| {med['essential']:.2f} | {med['choose']:.2f} | {med['linearize']:.3f} | {med['step']:.3f} | {med['bundle']:.2f} | "
          f"{med['bundle'] / max(ba.iters, 1):.3f} | {med['after']:.2f} | {med['whole']:.2f} |")
    print(f"numpy {np.__version__}, torch {torch.__version__}, {torch.cuda.get_device_name(0)}, {a.frames} frames x {a.matches} matches, "
          f"rounds = {a.rounds}, {a.reps} runs after {a.warmup}")


if __name__ == "__main__":
    main()
