#!/usr/bin/env python3
"""Generate tests/golden/dct_interp.npz: the reference's DCT interpolator on three small cases.

Run in the build container only (it loads the reference's gridding/wassgridsurface/DCTInterpolator.py by path, which does not
exist on the GPU box), on CPU torch:

    python tests/golden/make_golden_dct.py

Per case: ZZ (the cell map, NaN = no data), x0 (the first torch.rand((Nf, Nf)) after torch.manual_seed(seed): what the
interpolator draws), the options, the reference's Irec and its stop step (read from its printed log).
  one      64 x 64, Nf 16, MAX_ITERS 0 (one Rprop step)
  default  96 x 96, Nf 24, default options, a camera-footprint-shaped mask with holes
  early    64 x 64, Nf 16, TOLERANCE_CHANGE raised so that the tolerance stops it before MAX_ITERS
"""
import contextlib
import importlib.util
import io
import os
import re
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/gridding/wassgridsurface/DCTInterpolator.py"


def _load():
    spec = importlib.util.spec_from_file_location("ref_dct_interpolator", REF)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.DCTInterpolator


def surface(n, seed):
    """A band-limited sea-like surface (a few long-crested waves) over a camera-footprint-shaped mask with holes."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:n, 0:n].astype(np.float64) / n
    z = np.zeros((n, n))
    for _ in range(6):
        k = rng.uniform(2, 9) * 2 * np.pi
        th = rng.uniform(0, np.pi)
        z += rng.uniform(0.05, 0.3) * np.cos(k * (np.cos(th) * xx + np.sin(th) * yy) + rng.uniform(0, 2 * np.pi))
    # trapezoid seen by a camera looking down the y axis: narrow near, wide far
    half = 0.15 + 0.3 * yy
    foot = (np.abs(xx - 0.5) < half) & (yy > 0.08) & (yy < 0.95)
    keep = rng.random((n, n)) < 0.7                       # sparse cells
    holes = np.zeros((n, n), bool)
    for _ in range(4):
        cy, cx, r = rng.uniform(0.2, 0.8), rng.uniform(0.3, 0.7), rng.uniform(0.03, 0.08)
        holes |= (yy - cy) ** 2 + (xx - cx) ** 2 < r * r
    zz = np.where(foot & keep & ~holes, z, np.nan).astype(np.float32)
    return zz


def run(DCTI, zz, opts, seed):
    n = zz.shape[0]
    interp = DCTI(n, n, opts)
    torch.manual_seed(seed)
    x0 = torch.rand((opts["Nfreqs"], opts["Nfreqs"])).numpy().astype(np.float32)
    torch.manual_seed(seed)
    log = io.StringIO()
    with contextlib.redirect_stdout(log), contextlib.redirect_stderr(log):
        Irec, ones = interp(np.copy(zz), verbose=True)
    its = [int(m) for m in re.findall(r"Iteration (\d+)", log.getvalue())]
    stopped = "Reached min tolerance change" in log.getvalue()
    steps = its[-1] + 1 if stopped else opts["MAX_ITERS"] + 1
    assert ones.dtype == np.float32 and Irec.dtype == np.float32
    return x0, Irec, steps, stopped


def main():
    torch.set_num_threads(1)
    DCTI = _load()
    small, big = surface(64, 1), surface(96, 2)
    cases = {
        "one": (small, {"Nfreqs": 16, "MAX_ITERS": 0}, 11),
        "default": (big, {"Nfreqs": 24}, 12),
        "early": (small, {"Nfreqs": 16, "TOLERANCE_CHANGE": 0.05, "LEARNING_RATE": 0.5}, 13),
    }
    out = {"zz_small": small, "zz_big": big}
    for name, (zz, opts, seed) in cases.items():
        full = {"Nfreqs": 150, "MAX_ITERS": 500, "TOLERANCE_CHANGE": 1e-4, "REGULARIZER_ALPHA": 8e-7, "LEARNING_RATE": 5.0}
        full.update(opts)
        x0, Irec, steps, stopped = run(DCTI, zz, full, seed)
        out[f"{name}_x0"] = x0
        out[f"{name}_irec"] = Irec
        out[f"{name}_steps"] = np.int64(steps)
        out[f"{name}_converged"] = np.int64(stopped)
        out[f"{name}_opts"] = np.array([full["Nfreqs"], full["MAX_ITERS"], full["TOLERANCE_CHANGE"], full["REGULARIZER_ALPHA"],
                                        full["LEARNING_RATE"]], np.float64)
        out[f"{name}_zz"] = np.array("zz_small" if zz is small else "zz_big")
        print(f"{name}: {zz.shape} Nf {full['Nfreqs']} steps {steps} stopped {stopped}")
    path = os.path.join(HERE, "dct_interp.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
