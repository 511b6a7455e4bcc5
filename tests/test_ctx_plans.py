"""The scratch plans of the operators that keep their scratch in the context, pinned: wass_ac_scratch_bytes, wass_epi_scratch_bytes
and wass_match_scratch_bytes are pure, and tests/golden/ctx_plans.json holds what they answered before their layouts were stated
as one carve each (the bytes, or the error code) for the table of tests/golden/make_golden_ctx_plans.py: the smallest legal sizes
and one below them, the largest and one above them, and sizes either side of a multiple of 256 bytes of every piece.

Autocalibration and the essential-matrix filter were 256-aligned pieces before, so their plans are equal.  The matcher's context
layout was packed (one round-up to 64 bytes, 64 bytes at the end); it is now five pieces of which each is padded by less than 256
bytes, so its plan may move by alignment padding only: at most 256 * 6 bytes either way."""
import ctypes as C
import json
import os

from wass_amd import _lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ctx_plans.json")
EQUAL = ("wass_ac_scratch_bytes", "wass_epi_scratch_bytes")
MATCH = "wass_match_scratch_bytes"


def _replay():
    with open(GOLDEN) as f:
        entries = json.load(f)
    lib = _lib.load()
    for e in entries:
        b = C.c_size_t()
        rc = getattr(lib, e["fn"])(*e["args"], C.byref(b))
        e["got"] = {"error": rc} if rc else b.value
    return entries


def test_ctx_plans_match_golden():
    entries = _replay()
    assert {e["fn"] for e in entries} == set(EQUAL) | {MATCH}
    bad = [(e["fn"], e["args"], e["result"], e["got"]) for e in entries if e["fn"] in EQUAL and e["got"] != e["result"]]
    assert not bad, f"{len(bad)} plans differ, the first: {bad[0]}"
    for fn in EQUAL + (MATCH,):                 # every planner has answers of both kinds
        mine = [e["result"] for e in entries if e["fn"] == fn]
        assert any(isinstance(r, dict) for r in mine) and any(isinstance(r, int) for r in mine), fn


def test_match_plan_moves_by_padding_only():
    entries = [e for e in _replay() if e["fn"] == MATCH]
    sizes = {}
    for e in entries:
        was, got = e["result"], e["got"]
        if isinstance(was, dict) or isinstance(got, dict):
            assert got == was, (e["args"], was, got)            # the same error code
            continue
        assert abs(got - was) <= 256 * 6, (e["args"], was, got)
        sizes[tuple(e["args"])] = got
    assert len(sizes) > 100
    for (b, n), v in sizes.items():             # monotone in batch and in n_max over the table
        for (b2, n2), v2 in sizes.items():
            if b2 >= b and n2 >= n:
                assert v2 >= v, ((b, n, v), (b2, n2, v2))
