"""Writes tests/golden/cube_plans.json: what the *_scratch_bytes functions of wass_amd.postproc answer for a table of
cubes, host and device form.  The functions are pure (no GPU).  Run it on the commit whose plans are to be pinned:

    python tests/golden/make_golden_cube_plans.py

Every entry is {"fn", "kwargs", "result"}; result is [bytes, batch or rows], or {"error": the ValueError's text}.
tests/test_cube_plans.py replays the entries and asserts equality."""
from __future__ import annotations

import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))

PROD = dict(count=1000, H=1024, W=1024)
PIC = dict(Ih=2058, Iw=2456)                    # pictures of 2456 x 2058
BIG = 16384                                     # a 16384 x 16384 frame: 1 GiB of float32
W_MOST = 0x7FFFFF80                             # 0x7fffff00 // W is 0: no slab of even one row can be indexed


def slab_cases(small: dict, below: dict, deep: dict, none: dict, flat: dict, extra: dict):
    """small: the smallest legal cube; below: one below it; deep: so many frames that the cap cuts the slab; none: one row does
    not fit; flat: few frames, so that 0x7fffff00 // W decides; extra: what else the function takes, at production values"""
    prod = dict(PROD, **extra)
    return [small, below, prod, deep, none, dict(prod, slab_rows=1), dict(prod, slab_rows=5000), dict(deep, slab_rows=1),
            dict(flat, H=8, W=1_000_000_000), dict(flat, H=8, W=715_000_000), dict(flat, H=1, W=W_MOST),
            dict(small, slab_rows=-1)]


def batch_cases(small: dict, below: dict, extra: dict, big: int = BIG):
    """the cube is count x H x W; extra: what else the function takes, at production values"""
    prod = dict(PROD, **extra)
    huge = dict(extra, count=64, H=big, W=big)
    return [small, below, prod, dict(huge, batch=32), dict(huge, batch=8), dict(extra, count=2, H=65536, W=32767),
            dict(extra, count=2, H=65536, W=65536), dict(prod, batch=1), dict(prod, batch=5000), dict(prod, count=3, batch=8),
            dict(prod, batch=0), dict(small, batch=-1)]


def table():
    one = dict(count=1, H=1, W=1)
    two = dict(count=1, H=2, W=2)
    pic1 = dict(Ih=1, Iw=1)
    t = []
    t += [("sosfiltfilt_scratch_bytes", k) for k in slab_cases(
        dict(count=4, H=1, W=1, padlen=3), dict(count=3, H=1, W=1, padlen=3), dict(count=4000, H=4096, W=4096, padlen=27),
        dict(count=2_000_000, H=16, W=4096, padlen=27), dict(count=1, padlen=0), dict(padlen=27))]
    t += [("sosfiltfilt_scratch_bytes", dict(one, padlen=0)),
          ("sosfiltfilt_scratch_bytes", dict(count=1, H=0, W=1, padlen=0))]
    t += [("bgimage_scratch_bytes", k) for k in slab_cases(
        dict(one, filtersize=1), dict(one, filtersize=0), dict(count=8000, H=4096, W=4096, filtersize=2000),
        dict(count=2_000_000, H=16, W=4096, filtersize=2000), dict(count=1, filtersize=1), dict(filtersize=2000))]
    t += [("wave_statistics_scratch_bytes", k) for k in slab_cases(
        one, dict(count=1, H=0, W=1), dict(count=4000, H=4096, W=4096, hist_bins=64, hist_width=0.1),
        dict(count=4_000_000, H=16, W=4096), dict(count=1), {})]
    t += [("wave_statistics_scratch_bytes", dict(PROD, hist_bins=4096, hist_width=0.01, crossing="down")),
          ("wave_statistics_scratch_bytes", dict(count=3, H=8, W=1_000_000_000)),
          ("wave_statistics_scratch_bytes", dict(one, hist_bins=2**31 - 1, hist_width=1.0))]
    t += [("visibility_scratch_bytes", k) for k in batch_cases(two, dict(count=1, H=1, W=2), {})]
    t += [("radiance_scratch_bytes", k) for k in batch_cases(dict(one, **pic1), dict(count=0, H=1, W=1, **pic1), PIC)]
    t += [("radiance_scratch_bytes", dict(PROD, Ih=32767, Iw=2456))]
    t += [("radiance_threshold_scratch_bytes", k) for k in batch_cases(one, dict(count=1, H=1, W=0), {})]
    for dtype in ("float32", "float64"):
        for levels in (1, 3):
            t += [("pyr_up_scratch_bytes", k) for k in batch_cases(dict(two, levels=levels, dtype=dtype), dict(count=1, H=1, W=2, levels=levels, dtype=dtype),
                                                                   dict(levels=levels, dtype=dtype), big=BIG >> levels)]
    t += [("pyr_up_scratch_bytes", dict(two, levels=5)), ("pyr_up_scratch_bytes", dict(count=1, H=32768, W=2, levels=2))]
    for factor in (2, 4):
        t += [("radiance_upscaled_scratch_bytes", k) for k in batch_cases(dict(two, upscalefactor=factor, **pic1),
                                                                          dict(count=1, H=1, W=2, upscalefactor=factor, **pic1),
                                                                          dict(PIC, upscalefactor=factor), big=BIG >> factor // 2)]
    t += [("radiance_upscaled_scratch_bytes", dict(count=4, H=BIG, W=BIG, upscalefactor=2, **PIC)),
          ("radiance_upscaled_scratch_bytes", dict(PROD, upscalefactor=1, **PIC))]
    for outputs in (("S", "occlusion"), (), ("S", "occlusion", "angles", "dolp", "normals", "rays_cam")):
        t += [("polarimetric_scratch_bytes", dict(k, outputs=outputs)) for k in batch_cases(dict(two, **pic1), dict(count=1, H=2, W=1, **pic1), PIC)]
    return [(fn, dict(k, host=host)) for fn, k in t for host in (True, False)]


def answer(fn: str, kwargs: dict):
    from wass_amd import postproc
    try:
        return list(getattr(postproc, fn)(**kwargs))
    except ValueError as e:
        return {"error": str(e)}


def main():
    entries = [{"fn": fn, "kwargs": k, "result": answer(fn, k)} for fn, k in table()]
    path = os.path.join(HERE, "cube_plans.json")
    with open(path, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(e) for e in entries) + "\n]\n")
    print(f"{len(entries)} entries -> {path}")


if __name__ == "__main__":
    main()
