"""Writes tests/golden/handle_plans.json: what the pure C planners of the operators that keep their scratch in a handle answer
for a table of sizes: wass_spec3d_scratch_bytes, wass_spatial_filter_scratch_bytes, wass_vref_scratch_bytes and
wass_vref_batch_scratch_bytes, called through _lib.load() (no GPU).  Run it on the commit whose plans are to be pinned:

    python tests/golden/make_golden_handle_plans.py

Every entry is {"fn", "args", "result"}; result is the bytes, or {"error": the planner's return code}.  The planners answer
above the 16 GiB cap too: the cap is applied when a handle is created.  tests/test_handle_plans.py replays the entries and
asserts equality."""
from __future__ import annotations

import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))

SPEC_MAX_AXIS = 8192
VR_MAX_BATCH = 4096
VR_MAX_SIDE = 32768
PIC = (2058, 2456)                              # pictures of 2456 x 2058


def table():
    A = SPEC_MAX_AXIS
    t = []
    # nt, ny, nx: the smallest window and an axis of 0; odd and even axes; the longest axis and one above; the production windows;
    # 16 frames of 1024 x 1024; the largest window there is (far above the cap)
    t += [("wass_spec3d_scratch_bytes", a) for a in (
        (1, 1, 1), (0, 1, 1), (1, 0, 1), (1, 1, 0), (-1, 1, 1),
        (100, 683, 683), (100, 684, 684), (100, 683, 684), (100, 684, 683), (100, 100, 100), (683, 100, 684), (2, 3, 5),
        (A, 1, 1), (1, A, 1), (1, 1, A), (A + 1, 1, 1), (1, A + 1, 1), (1, 1, A + 1),
        (300, 684, 684), (16, 1024, 1024), (A, A, A))]
    # rows, cols, batch: the same, and batches of 1, 16, 65535 and 65536
    t += [("wass_spatial_filter_scratch_bytes", a) for a in (
        (1, 1, 1), (0, 1, 1), (1, 0, 1), (1, 1, 0),
        (683, 683, 16), (684, 684, 16), (683, 684, 16), (684, 683, 16), (100, 100, 16), (3, 5, 2),
        (A, 1, 1), (1, A, 1), (A + 1, 1, 1), (1, A + 1, 1), (A, A, 16),
        (1024, 1024, 16), (1024, 1024, 1), (1024, 1024, 65535), (1024, 1024, 65536),
        (684, 684, 1), (684, 684, 65535), (684, 684, 65536), (A, A, 65535))]
    # ny, nx, ih0, iw0, ih1, iw1: the smallest grid and pictures and one below each; odd and even axes; the largest sides and one
    # above; the production grid with the production pictures
    sizes = ((2, 2, 2, 2, 2, 2), (1, 2, 2, 2, 2, 2), (2, 1, 2, 2, 2, 2), (2, 2, 1, 2, 2, 2), (2, 2, 2, 1, 2, 2), (2, 2, 2, 2, 1, 2),
             (2, 2, 2, 2, 2, 1), (3, 3, 2, 3, 3, 2), (683, 683, 100, 100, 100, 100), (684, 684, 100, 100, 100, 100),
             (683, 684, 100, 683, 684, 100), (100, 100, 683, 684, 684, 683), (6, 70, 9, 11, 11, 9),
             (VR_MAX_SIDE, 2, 2, 2, 2, 2), (VR_MAX_SIDE + 1, 2, 2, 2, 2, 2), (2, VR_MAX_SIDE, 2, 2, 2, 2), (2, VR_MAX_SIDE + 1, 2, 2, 2, 2),
             (2, 2, VR_MAX_SIDE, VR_MAX_SIDE, 2, 2), (2, 2, 2, 2, VR_MAX_SIDE, VR_MAX_SIDE + 1),
             (VR_MAX_SIDE, VR_MAX_SIDE, VR_MAX_SIDE, VR_MAX_SIDE, VR_MAX_SIDE, VR_MAX_SIDE),
             (684, 684) + PIC + PIC, (1024, 1024) + PIC + PIC)
    t += [("wass_vref_scratch_bytes", a) for a in sizes]
    # nb first: batches of 1, 4, the largest and one above it; 0
    t += [("wass_vref_batch_scratch_bytes", (nb,) + a) for a in sizes for nb in (1, 4, VR_MAX_BATCH, VR_MAX_BATCH + 1, 0)]
    return t


def answer(fn: str, args):
    from wass_amd import _lib
    b = C.c_size_t()
    rc = getattr(_lib.load(), fn)(*args, C.byref(b))
    return {"error": rc} if rc else b.value


def main():
    entries = [{"fn": fn, "args": list(a), "result": answer(fn, a)} for fn, a in table()]
    path = os.path.join(HERE, "handle_plans.json")
    with open(path, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(e) for e in entries) + "\n]\n")
    print(f"{len(entries)} entries -> {path}")


if __name__ == "__main__":
    main()
