#!/usr/bin/env python3
"""Times the KAZE detector on the GPU at 2456 x 2058 with the reference's defaults (4 octaves x 4 sublevels) on a synthetic sea
picture (wass_amd.synth), per stage:

  presmooth    uint8 -> float32, Gaussian(1.6), Gaussian(1.0)
  contrast     Gaussian(1.0), Scharr, hmax and the 300-bin histogram, the scan on the host
  flow         per level: Gaussian(1.0) of Lt, Scharr, the PM-G2 conductivity
  diffusion    per level: the FED cycle's explicit steps (166 in all with the defaults)
  response     per level: scaled Scharr, second derivatives and Ldet, Lx and Ly scaled
  extrema      the 3-level search, the sort of the keys, the gather of the responses
  duplicates   the duplicate pass, on the host
  refine, orientation, descriptors

For every stencil stage the bytes it must move (each plane read or written once per kernel that needs it; neighbours come from
cache) and, for the stages that take a millisecond or more, the share of the 8.0 TB/s HBM peak that the time amounts to.  A host
clock around library calls that each end in a device synchronisation: launch, ctypes and synchronisation gaps (tens of
microseconds per call) are inside the figures, so a stage below a millisecond is mostly that overhead and gets no share.  Median,
smallest and largest of `--reps` runs after `--warmup`.  Needs a GPU: no fall-back.

    python scripts/time_kaze.py [--width 2456] [--height 2058] [--reps 9] [--warmup 2]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=2456)
    ap.add_argument("--height", type=int, default=2058)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    import torch
    import wass_amd
    from wass_amd import features as FE
    from wass_amd import synth

    w, h = a.width, a.height
    img = synth.make_pair_torch(w, h, 128, frame_idx=5, device="cuda")[0]
    lv = FE.kaze_levels()
    N = len(lv)
    steps = sum(len(t) for t in lv.taus)
    odd = sum(len(t) & 1 for t in lv.taus)
    P = h * w * 4
    # planes moved: Gaussian = 2 passes x (1 read + 1 write); Scharr 1 + 2; Hessian 2 + 1, then Lx, Ly scaled in place 2 + 2;
    # flow 2 + 1; a step 2 + 1 (and a copy back after an odd number of them); hmax and histogram read 2 each; extrema read every level
    planes = {"presmooth": 0.25 + 1 + 4 + 4, "contrast": 4 + 3 + 4, "flow": (N - 1) * (4 + 3 + 3), "diffusion": 3 * steps + 2 * odd,
              "response": N * (3 + 7), "extrema": N}
    runs = []
    with wass_amd.Context(0) as ctx:
        for r in range(a.warmup + a.reps):
            t = {}
            pyr = FE.KazePyramid(img, None, ctx, timings=t)
            kp = pyr.detect()
            torch.cuda.synchronize()
            if r >= a.warmup:
                runs.append(t)
    names = ["presmooth", "contrast", "flow", "diffusion", "response", "extrema", "duplicates (host)", "refine", "orientation", "descriptors"]
    print(f"{w} x {h}, {N} levels, {steps} FED steps; {pyr.counts[0]} candidates into the duplicate pass, {pyr.counts[1]} accepted, "
          f"{len(kp)} keypoints; scratch bound {FE.kaze_scratch_bytes(h, w) / 1e9:.3f} GB; {a.reps} runs after {a.warmup}")
    print("| stage | ms (median) | min - max | bytes moved | share of 8.0 TB/s |")
    print("|---|---|---|---|---|")
    for n in names + ["all"]:
        v = sorted((sum(t[k] for k in names) if n == "all" else t[n]) * 1e3 for t in runs)
        ms = statistics.median(v)
        spread = f"{v[0]:.2f} - {v[-1]:.2f}"
        if n in planes:
            b = planes[n] * P
            share = f"{b / (ms * 1e-3) / HBM_PEAK * 100:.0f} %" if ms >= 1.0 else ""
            print(f"| {n} | {ms:.2f} | {spread} | {b / 1e9:.2f} GB | {share} |")
        else:
            print(f"| {n} | {ms:.2f} | {spread} | | |")


if __name__ == "__main__":
    main()
