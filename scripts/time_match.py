#!/usr/bin/env python3
"""Times the feature matcher on the GPU for the reference's default problem: 2000 + 2000 features of dimension 64, 3 candidates each
(N = 6000 strategies), per stage and over batches of 1, 2, 4, 8 and 16 pairs, in ms per pair.

  candidates   knn_candidates, one call per pair
  payoff       the N x N fp64 matrices of the first round, one launch for the batch
  dynamics     iidyn on those matrices (device tensors, read in place for one pair), `--max-iters` steps at most (50 000: the reference's)
  gt_match     gt_match_batch as a whole: candidates, every round's payoff, dynamics and removal loop

Median of `--reps` runs after `--warmup` runs of the same shapes, a host clock around calls that end in a device synchronisation.
The one expectation this is there to confirm or refute: a batch of 16 takes much less than 16 singles, because the dynamics occupies
one compute unit per problem.  Prints a table for DESIGN.md.  Needs a GPU: no fall-back.  The scenes come from the test suite's
oracle (tests/match_oracle.py): the script runs from a checkout with tests/.

    python scripts/time_match.py [--features 2000] [--reps 3] [--warmup 1] [--max-iters 50000] [--batches 1,2,4,8,16]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--features", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--max-iters", type=int, default=50000)
    ap.add_argument("--batches", default="1,2,4,8,16")
    ap.add_argument("--skip-whole", action="store_true", help="leave gt_match as a whole out (it plays up to 21 rounds)")
    a = ap.parse_args()
    import torch
    import match_oracle as M
    import wass_amd
    from wass_amd import match

    batches = [int(b) for b in a.batches.split(",")]
    pairs = []
    for p in range(max(batches)):
        fa, fb, da, db, _ = M.scene(1000 + p, n=a.features)
        pairs.append((match.Features(fa[:, :2], fa[:, 2], fa[:, 3], da), match.Features(fb[:, :2], fb[:, 2], fb[:, 3], db)))

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    rows = []
    with wass_amd.Context(0) as ctx:
        for B in batches:
            use = pairs[:B]
            t = {"candidates": [], "payoff": [], "dynamics": [], "gt_match": []}
            steps = rounds = None
            for rep in range(a.warmup + a.reps):
                dt_k, knn = timed(lambda: [match.knn_candidates(A.desc, Bf.desc, 3, ctx) for A, Bf in use])
                cands = [match.candidate_list(idx) for idx, _ in knn]
                n = cands[0].shape[0]
                d_A = torch.empty((B, n, n), dtype=torch.float64, device="cuda")
                tabs = [(torch.from_numpy(A.table()).cuda(), torch.from_numpy(Bf.table()).cuda(), torch.from_numpy(c).cuda())
                        for (A, Bf), c in zip(use, cands)]

                def payoff():
                    # one launch per pair here (the batched launch is inside gt_match_batch); the kernel time is the same
                    for q, (ta, tb, tc) in enumerate(tabs):
                        ctx._check(ctx._lib.wass_match_payoff_dev(ctx._h, ta.data_ptr(), 0, tb.data_ptr(), 0, tc.data_ptr(), 0, match._ints([n]),
                                                                  match._ints([ta.shape[0]]), match._ints([tb.shape[0]]), 1, 1e-5,
                                                                  d_A[q].data_ptr(), 0))
                dt_p, _ = timed(payoff)
                mats = [d_A[q] for q in range(B)]
                dt_d, dyn = timed(lambda: match.iidyn(mats if B > 1 else mats[0], max_iters=a.max_iters, ctx=ctx))
                steps = [r.steps for r in (dyn if B > 1 else [dyn])]
                del d_A, mats
                if not a.skip_whole:
                    dt_w, res = timed(lambda: match.gt_match_batch(use, max_iters=a.max_iters, ctx=ctx))
                    rounds = [len(r.rounds) for r in res]
                else:
                    dt_w = float("nan")
                if rep >= a.warmup:
                    for k, v in zip(t, (dt_k, dt_p, dt_d, dt_w)):
                        t[k].append(v)
            med = {k: 1e3 * statistics.median(v) / B for k, v in t.items()}
            rows.append((B, n, med, steps, rounds))
            print(f"batch {B}: N = {n}, steps of the first round {steps}, rounds {rounds}", flush=True)
    print("| pairs per batch | candidates | payoff | dynamics | gt_match as a whole |   (ms per pair)")
    print("|---|---|---|---|---|")
    for B, n, med, _, _ in rows:
        print(f"| {B} | {med['candidates']:.2f} | {med['payoff']:.2f} | {med['dynamics']:.1f} | {med['gt_match']:.1f} |")
    print(f"numpy {np.__version__}, torch {torch.__version__}, {torch.cuda.get_device_name(0)}, max_iters {a.max_iters}, {a.reps} runs after {a.warmup}")


if __name__ == "__main__":
    main()
