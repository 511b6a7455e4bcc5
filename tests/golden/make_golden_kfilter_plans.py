"""Writes tests/golden/kfilter_plans.json: what the pure C planner of the dispersion filter, wass_kfilter_scratch_bytes, answers for
a table of sizes, called through _lib.load() (no GPU).  Run it on the commit whose plans are to be pinned:

    python tests/golden/make_golden_kfilter_plans.py

Every entry is {"args", "result"}; result is the bytes, or {"error": the planner's return code}.  The planner answers above the
16 GiB cap too: the cap is applied when a handle is created.  tests/test_kfilter.py replays the entries and asserts equality."""
from __future__ import annotations

import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))

SPEC_MAX_AXIS = 8192


def table():
    A = SPEC_MAX_AXIS
    # nt, ny, nx: the smallest cube and an axis of 0; odd and even axes; thin cubes; the longest axis and one above; the windows of
    # the spectrum; the production cube and the first sizes above the cap; the largest cube there is
    return [(1, 1, 1), (0, 1, 1), (1, 0, 1), (1, 1, 0), (-1, 1, 1), (2, 1, 1), (1, 2, 3), (3, 2, 2), (2, 3, 5), (20, 129, 131),
            (100, 683, 683), (100, 684, 684), (100, 683, 684), (100, 684, 683), (100, 100, 100), (683, 100, 684),
            (A, 1, 1), (1, A, 1), (1, 1, A), (A + 1, 1, 1), (1, A + 1, 1), (1, 1, A + 1),
            (300, 684, 684), (16, 1024, 1024), (1000, 1024, 1024), (1024, 1024, 1024), (1155, 1024, 1024), (1156, 1024, 1024),
            (1200, 1024, 1024), (A, A, A)]


def answer(args):
    from wass_amd import _lib
    b = C.c_size_t()
    rc = _lib.load().wass_kfilter_scratch_bytes(*args, C.byref(b))
    return {"error": rc} if rc else b.value


def main():
    entries = [{"args": list(a), "result": answer(a)} for a in table()]
    path = os.path.join(HERE, "kfilter_plans.json")
    with open(path, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(e) for e in entries) + "\n]\n")
    print(f"{len(entries)} entries -> {path}")


if __name__ == "__main__":
    main()
