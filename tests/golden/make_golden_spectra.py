#!/usr/bin/env python3
"""Generate tests/golden/spectra_*.npz: what the reference's own postproc/wasspost/spectra.py returns for three generated cubes.

    python tests/golden/make_golden_spectra.py <path of the reference checkout>

Run once where the reference, scipy and tqdm are at hand; the tests read the .npz files only.  The cubes are not stored: they
are tests/spectrum_oracle.make_cube with the arguments kept in each file.
  spectra_3d_nx.npz    40 x 120 x 126, du 0.25: the wavenumber axes are as long as the nominal crop (81)
  spectra_3d_nx1.npz   40 x 123 x 130, du 0.1:  one element longer (84, not 83), NaN cells at 1 %
  spectra_1d.npz       700 x 40 x 40, dt 0.1, nperseg 128, rangespan 5, scale 1 / 1000
"""
import contextlib
import importlib.util
import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import spectrum_oracle as SO  # noqa: E402

CASES_3D = {"nx": dict(shape=(40, 120, 126), du=0.25, dt=0.1, seed=3, nan_fraction=0.0, datascale=1.0),
            "nx1": dict(shape=(40, 123, 130), du=0.1, dt=0.08, seed=4, nan_fraction=0.01, datascale=0.001)}
CASE_1D = dict(shape=(700, 40, 40), dt=0.1, seed=5, nperseg=128, rangespan=5, scale=0.001)


def main():
    ref = sys.argv[1]
    spec = importlib.util.spec_from_file_location("ref_spectra", os.path.join(ref, "postproc", "wasspost", "spectra.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    log = io.StringIO()
    for name, c in CASES_3D.items():
        cube = SO.make_cube(*c["shape"], seed=c["seed"], nan_fraction=c["nan_fraction"])
        with contextlib.redirect_stdout(log), contextlib.redirect_stderr(log):
            S, KX, KY, f = mod.compute_3D_spectrum(cube, c["du"], c["dt"], datascale=c["datascale"])
        path = os.path.join(HERE, f"spectra_3d_{name}.npz")
        np.savez_compressed(path, S=S, KX=KX, KY=KY, f=f, shape=np.array(c["shape"]), du=c["du"], dt=c["dt"], seed=c["seed"],
                            nan_fraction=c["nan_fraction"], datascale=c["datascale"])
        print(path, S.shape, os.path.getsize(path), "bytes")
    c = CASE_1D
    cube = SO.make_cube(*c["shape"], seed=c["seed"])
    with contextlib.redirect_stdout(log), contextlib.redirect_stderr(log):
        f, S, ts = mod.compute_spectrum(cube, c["dt"], nperseg=c["nperseg"], rangespan=c["rangespan"], scale=c["scale"])
    path = os.path.join(HERE, "spectra_1d.npz")
    np.savez_compressed(path, f=f, S=S, timeserie=ts, shape=np.array(c["shape"]), dt=c["dt"], seed=c["seed"], nperseg=c["nperseg"],
                        rangespan=c["rangespan"], scale=c["scale"])
    print(path, S.shape, S.dtype, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
