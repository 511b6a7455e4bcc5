"""The scratch plans of the operators that keep their scratch in a handle, pinned: wass_spec3d_scratch_bytes,
wass_spatial_filter_scratch_bytes, wass_vref_scratch_bytes and wass_vref_batch_scratch_bytes are pure, and
tests/golden/handle_plans.json holds what they answered before spectrum.hip was moved onto csrc/cube.h (the bytes, or the
error code) for the table of tests/golden/make_golden_handle_plans.py: the smallest legal sizes and one below them, odd and even
axes, the longest axis and one above it, the production windows, batches of 1, 16, 65535 and 65536 (spatial filter) and of 1, 4,
the largest and one above it (refinement), and sizes far above the 16 GiB cap, which only create applies."""
import ctypes as C
import json
import os

from wass_amd import _lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "handle_plans.json")
FUNCTIONS = ("wass_spec3d_scratch_bytes", "wass_spatial_filter_scratch_bytes", "wass_vref_scratch_bytes", "wass_vref_batch_scratch_bytes")


def test_handle_plans_match_golden():
    with open(GOLDEN) as f:
        entries = json.load(f)
    assert {e["fn"] for e in entries} == set(FUNCTIONS)
    lib = _lib.load()
    bad = []
    for e in entries:
        b = C.c_size_t()
        rc = getattr(lib, e["fn"])(*e["args"], C.byref(b))
        got = {"error": rc} if rc else b.value
        if got != e["result"]:
            bad.append((e["fn"], e["args"], e["result"], got))
    assert not bad, f"{len(bad)} of {len(entries)} plans differ, the first: {bad[0]}"
    for fn in FUNCTIONS:                        # every planner has answers of both kinds, and one above 16 GiB
        mine = [e["result"] for e in entries if e["fn"] == fn]
        assert any(isinstance(r, dict) for r in mine) and any(isinstance(r, int) and r > 16 << 30 for r in mine), fn
