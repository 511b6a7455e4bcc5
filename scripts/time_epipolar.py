#!/usr/bin/env python3
"""Times the essential-matrix filter on the GPU at M = 2000 matches and 1024 hypotheses per pair, per stage and over batches of 1,
2, 4, 8 and 16 pairs, in ms per pair.

  solve     wass_epi_solve5_dev: the five-point problem of every sample, one launch for the batch
  score     wass_epi_score_dev: the 10 240 model slots of every pair against its 2000 matches
  find      wass_epi_find_dev: solve, score, best and mask in one chain, one synchronisation at its end
  filter    epipolar_filter_batch as a whole: sample tables, upload, the chain, recoverPose and the statistics on the host

Median of `--reps` runs after `--warmup` runs of the same shapes, a host clock around calls that end in a device synchronisation.
Prints a table for DESIGN.md.  Needs a GPU: no fall-back.  The scenes come from the test suite's oracle
(tests/epipolar_oracle.py): the script runs from a checkout with tests/.

    python scripts/time_epipolar.py [--matches 2000] [--rounds 1024] [--reps 5] [--warmup 2] [--batches 1,2,4,8,16]
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
    ap.add_argument("--matches", type=int, default=2000)
    ap.add_argument("--rounds", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batches", default="1,2,4,8,16")
    a = ap.parse_args()
    import torch
    import epipolar_oracle as O
    import wass_amd
    from wass_amd import epipolar as EP

    batches = [int(b) for b in a.batches.split(",")]
    M, R = a.matches, a.rounds
    pairs = []
    for p in range(max(batches)):
        g = O.rig(500 + p)
        loc_a, loc_b, _, _, _ = O.scene(g, M, 700 + p, noise=0.2, outliers=0.3)
        pairs.append((loc_a, loc_b, g[0], g[1]))
    table = EP.ransac_samples(M, R)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    rows = []
    with wass_amd.Context(0) as ctx:
        lib, h = ctx._lib, ctx._h
        for B in batches:
            use = pairs[:B]
            pts = [(EP.normalise(la, K0), EP.normalise(lb, K1)) for la, lb, K0, K1 in use]
            ts = [0.5 / ((K0[0, 0] + K0[1, 1]) / 2) for _, _, K0, _ in use]
            d0 = torch.from_numpy(np.stack([x for x, _ in pts])).cuda()
            d1 = torch.from_numpy(np.stack([x for _, x in pts])).cuda()
            d_s = torch.from_numpy(np.stack([table] * B)).cuda()
            d_E = torch.empty((B, R, 10, 9), dtype=torch.float64, device="cuda")
            d_n = torch.empty((B, R), dtype=torch.int32, device="cuda")
            d_c = torch.empty((B, R * 10), dtype=torch.int32, device="cuda")
            d_m = torch.empty((B, M), dtype=torch.uint8, device="cuda")
            d_e = torch.empty((B, M), dtype=torch.float32, device="cuda")
            ms, tt = EP._ints([M] * B), EP._doubles(ts)
            E, idx, cnt = np.zeros((B, 9)), (C.c_int * B)(), (C.c_int * B)()
            t = {"solve": [], "score": [], "find": [], "filter": []}
            for rep in range(a.warmup + a.reps):
                dt_s, _ = timed(lambda: ctx._check(lib.wass_epi_solve5_dev(h, d0.data_ptr(), d1.data_ptr(), 2 * M, d_s.data_ptr(), 5 * R, ms, R, B,
                                                                           d_E.data_ptr(), d_n.data_ptr())))
                dt_c, _ = timed(lambda: ctx._check(lib.wass_epi_score_dev(h, d_E.data_ptr(), R * 10, d_n.data_ptr(), d0.data_ptr(), d1.data_ptr(), 2 * M,
                                                                          ms, tt, B, d_c.data_ptr())))
                dt_f, _ = timed(lambda: ctx._check(lib.wass_epi_find_dev(h, d0.data_ptr(), d1.data_ptr(), 2 * M, d_s.data_ptr(), 5 * R, ms, tt, R, B,
                                                                         E.ctypes.data, idx, cnt, d_m.data_ptr(), d_e.data_ptr(), M)))
                dt_w, res = timed(lambda: EP.epipolar_filter_batch(use, rounds=R, ctx=ctx))
                if rep >= a.warmup:
                    for k, v in zip(t, (dt_s, dt_c, dt_f, dt_w)):
                        t[k].append(v)
            med = {k: 1e3 * statistics.median(v) / B for k, v in t.items()}
            nsol = d_n.cpu().numpy()
            rows.append((B, med))
            print(f"batch {B}: {nsol.mean():.2f} solutions per sample, best counts {list(cnt)[:4]}, kept {[int(r.mask.sum()) for r in res][:4]}", flush=True)
    print("| pairs per batch | solve | score | find (the chain) | epipolar_filter as a whole |   (ms per pair)")
    print("|---|---|---|---|---|")
    for B, med in rows:
        print(f"| {B} | {med['solve']:.3f} | {med['score']:.3f} | {med['find']:.3f} | {med['filter']:.2f} |")
    print(f"numpy {np.__version__}, torch {torch.__version__}, {torch.cuda.get_device_name(0)}, M = {M}, rounds = {R}, {a.reps} runs after {a.warmup}")


if __name__ == "__main__":
    main()
