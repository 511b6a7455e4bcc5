"""Record the reference's own dynamics for tests/test_match.py and tests/test_match_gpu.py:

    python tests/golden/make_golden_match.py <reference checkout>

Compiles the reference's src/wass_match/iidyn.cpp with g++ where it lies (it needs nothing but libc), with a driver of a few lines
written out below, and runs gt_create_population and gt_iidyn (toll 1e-20) on
  * random symmetric matrices (match_oracle.random_symmetric: only the seeds are stored, with a checksum of each matrix),
  * the clique, tie and degenerate matrices,
  * the payoff matrices of four feature scenes (match_oracle.scene, match_oracle.payoff), after 300 steps and to the end.
tests/golden/match_iidyn.npz holds data only: seeds, sizes, the scenes' features, max_iters, and the recorded populations, step
counts and errors.  Nothing of the reference's text, and nothing compiled from it, is kept: the build lives in a temporary directory.
No test runs this file or reads the reference.
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import match_oracle as M  # noqa: E402

DRIVER = r"""
#include <cstdio>
#include <vector>
#include "gt.h"
int main(int argc, char** argv)
{
    FILE* f = fopen(argv[1], "rb");
    int n, iters;
    if (!f || fread(&n, 4, 1, f) != 1 || fread(&iters, 4, 1, f) != 1) return 1;
    std::vector<double> A((size_t)n * n), x(n);
    if (fread(A.data(), 8, A.size(), f) != A.size()) return 1;
    fclose(f);
    double toll = 1E-20;
    gt_create_population(x.data(), n);
    gt_iidyn(A.data(), x.data(), n, &toll, &iters);
    f = fopen(argv[2], "wb");
    fwrite(&iters, 4, 1, f);
    fwrite(&toll, 8, 1, f);
    fwrite(x.data(), 8, x.size(), f);
    fclose(f);
    return 0;
}
"""

RANDOM_SIZES = (3, 65, 257, 1025)
DENSITIES = (0.05, 0.5, 1.0)
RANDOM_STEPS = 300
SCENE_SEEDS = (11, 12, 13, 14)
SCENE_LAMBDA = (1e-5, 1e-3, 1e-5, 1e-3)
SPECIAL = {"cliques_3_3": M.cliques([3, 3]), "cliques_4_4_1": M.cliques([4, 4, 1]), "zeros_5": np.zeros((5, 5)),
           "single": np.zeros((1, 1)), "interleaved_3_3": M.cliques([3, 3], interleave=True)}


def random_seed(n, density):
    return 1000 * n + int(round(density * 100))


def main():
    ref = sys.argv[1]
    src = os.path.join(ref, "src", "wass_match")
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        drv = os.path.join(tmp, "driver.cpp")
        with open(drv, "w") as f:
            f.write(DRIVER)
        exe = os.path.join(tmp, "iidyn_ref")
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-I", src, os.path.join(src, "iidyn.cpp"), drv, "-o", exe])

        def run(A, iters):
            A = np.ascontiguousarray(A, np.float64)
            fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
            with open(fin, "wb") as f:
                f.write(np.array([A.shape[0], iters], "<i4").tobytes())
                f.write(A.tobytes())
            subprocess.check_call([exe, fin, fout])
            raw = open(fout, "rb").read()
            return np.frombuffer(raw, "<f8", A.shape[0], 12).copy(), int(np.frombuffer(raw, "<i4", 1)[0]), float(np.frombuffer(raw, "<f8", 1, 4)[0])

        for n in RANDOM_SIZES:
            for d in DENSITIES:
                A = M.random_symmetric(n, d, random_seed(n, d))
                x, steps, err = run(A, RANDOM_STEPS)
                key = f"random_{n}_{int(round(d * 100))}"
                out[key + "_x"], out[key + "_steps"], out[key + "_err"], out[key + "_sum"] = x, steps, err, A.sum()
                print(key, steps, err)
        for name, A in SPECIAL.items():
            x, steps, err = run(A, M.MAX_ITERS)
            out[f"special_{name}_A"], out[f"special_{name}_x"], out[f"special_{name}_steps"], out[f"special_{name}_err"] = A, x, steps, err
            print(name, steps, x)
        for s, (seed, lam) in enumerate(zip(SCENE_SEEDS, SCENE_LAMBDA)):
            fa, fb, da, db, truth = M.scene(seed)
            idx, _, _ = M.knn(da, db, 3)
            P, _, _ = M.payoff(fa, fb, M.candidates(idx), lam)
            out[f"scene{s}_fa"], out[f"scene{s}_fb"], out[f"scene{s}_da"], out[f"scene{s}_db"], out[f"scene{s}_truth"] = fa, fb, da, db, truth
            out[f"scene{s}_lambda"] = lam
            for tag, iters in (("short", RANDOM_STEPS), ("full", M.MAX_ITERS)):
                x, steps, err = run(P, iters)
                out[f"scene{s}_{tag}_x"], out[f"scene{s}_{tag}_steps"], out[f"scene{s}_{tag}_err"] = x, steps, err
                print("scene", s, tag, steps, err, M.group(x).size)
    out["random_sizes"], out["densities"], out["random_steps"] = np.array(RANDOM_SIZES), np.array(DENSITIES), RANDOM_STEPS
    out["max_iters"], out["special_names"] = M.MAX_ITERS, np.array(sorted(SPECIAL))
    np.savez_compressed(os.path.join(HERE, "match_iidyn.npz"), **out)


if __name__ == "__main__":
    main()
