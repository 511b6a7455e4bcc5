#!/usr/bin/env python3
"""Generate tests/golden/filters.npz: what scipy.signal and the reference's Spatial2DButterworth return for small generated inputs.

    python tests/golden/make_golden_filters.py <path of the reference checkout>

Run once where the reference, scipy and tqdm are at hand; the tests read the .npz only.  The inputs are not stored: they are
tests/filter_oracle.series_cube and tests/spectrum_oracle.make_cube with the arguments kept in the file.
  sos_<order>_<type>_<i>   scipy.signal.butter(order, CUTOFFS[i], btype=type, output='sos', fs=12), orders 1 .. 10
  spread_<order>_<type>_<i>   how far scipy's own coefficients move when the cutoff moves by one part in 2^52, per coefficient
  zi_<type>_<i>            scipy.signal.sosfilt_zi of the order-8 sections
  tf_<name>                scipy.signal.sosfiltfilt(sos, cube, axis=0) (float64) of the 600 x 3 x 5 cube, for the four filters of
                           the oracle test, and hp2 of the cube with an offset of 5000 and a drift
  sp_<name>_H, sp_<name>_out   the reference class's transfer function and its apply() on a square and a NON-square surface,
                           given as float64 (on float32 input scipy.fft would compute in single precision)
"""
import importlib.util
import os
import sys

import numpy as np
import scipy.signal

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import filter_oracle as FO  # noqa: E402
import spectrum_oracle as SO  # noqa: E402

FS = 12.0
CUTOFFS = (1.0, 0.3, 0.05, 0.02, 5.9)
TEMPORAL = {"lp0": ("lowpass", 1.0), "lp1": ("lowpass", 0.3), "hp0": ("highpass", 0.05), "hp1": ("highpass", 0.02)}
CUBE = dict(count=600, H=3, W=5, seed=3)
SPATIAL = {"square": dict(rows=48, cols=48, du=0.25, cutoff=0.4, order=4, seed=8),
           "nonsquare": dict(rows=40, cols=56, du=0.2, cutoff=0.64, order=4, seed=9)}


def main():
    ref = sys.argv[1]
    spec = importlib.util.spec_from_file_location("ref_spectra", os.path.join(ref, "postproc", "wasspost", "spectra.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = {"fs": FS, "cutoffs": np.array(CUTOFFS), "cube": np.array([CUBE[k] for k in ("count", "H", "W", "seed")])}
    for order in range(1, 11):
        for bt in ("lowpass", "highpass"):
            for i, fc in enumerate(CUTOFFS):
                b = out[f"sos_{order}_{bt}_{i}"] = scipy.signal.butter(order, fc, btype=bt, output="sos", fs=FS)
                lo = scipy.signal.butter(order, fc * (1 - 2.0 ** -52), btype=bt, output="sos", fs=FS)
                hi = scipy.signal.butter(order, fc * (1 + 2.0 ** -52), btype=bt, output="sos", fs=FS)
                out[f"spread_{order}_{bt}_{i}"] = np.maximum(np.abs(lo - b), np.abs(hi - b))
                if order == 8:
                    out[f"zi_{bt}_{i}"] = scipy.signal.sosfilt_zi(out[f"sos_{order}_{bt}_{i}"])
    cube = FO.series_cube(**CUBE)
    for name, (bt, fc) in TEMPORAL.items():
        sos = scipy.signal.butter(8, fc, btype=bt, output="sos", fs=FS)
        out[f"tf_{name}"] = scipy.signal.sosfiltfilt(sos, cube, axis=0)
    drifting = FO.series_cube(**CUBE, offset=5000.0, drift=0.7)
    out["tf_hp2"] = scipy.signal.sosfiltfilt(scipy.signal.butter(8, 0.05, btype="highpass", output="sos", fs=FS), drifting, axis=0)
    for name, c in SPATIAL.items():
        surf = SO.make_cube(1, c["rows"], c["cols"], seed=c["seed"])[0].astype(np.float64)
        filt = mod.Spatial2DButterworth(c["rows"], c["cols"], c["du"], c["cutoff"], c["order"])
        out[f"sp_{name}_H"] = filt.butterworth_filter
        out[f"sp_{name}_out"] = filt.apply(surf)
        out[f"sp_{name}_args"] = np.array([c["rows"], c["cols"], c["du"], c["cutoff"], c["order"], c["seed"]], np.float64)
    path = os.path.join(HERE, "filters.npz")
    np.savez_compressed(path, **out)
    print(path, len(out), "arrays,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
