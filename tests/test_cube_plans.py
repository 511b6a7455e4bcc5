"""The scratch plans of the one-shot cube operators, pinned: the *_scratch_bytes functions are pure, and
tests/golden/cube_plans.json holds what they answered before the operators were moved onto csrc/cube.h (bytes and batch or rows,
or the refusal), host and device form, for the table of tests/golden/make_golden_cube_plans.py: the smallest legal cube and one
below it, the production size, cubes that the 16 GiB cap halves or cuts at least twice, cubes that cannot be planned, explicit
batch / slab_rows of 1 and of more than count / H, and widths at which 0x7fffff00 // W decides."""
import json
import os

from wass_amd import postproc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cube_plans.json")
FUNCTIONS = ("sosfiltfilt_scratch_bytes", "bgimage_scratch_bytes", "wave_statistics_scratch_bytes", "visibility_scratch_bytes",
             "radiance_scratch_bytes", "radiance_threshold_scratch_bytes", "pyr_up_scratch_bytes", "radiance_upscaled_scratch_bytes",
             "polarimetric_scratch_bytes")


def test_cube_plans_match_golden():
    with open(GOLDEN) as f:
        entries = json.load(f)
    assert {e["fn"] for e in entries} == set(FUNCTIONS)
    assert {e["kwargs"]["host"] for e in entries} == {True, False}
    bad = []
    for e in entries:
        try:
            got = list(getattr(postproc, e["fn"])(**e["kwargs"]))
        except ValueError as err:
            got = {"error": str(err)}
        if got != e["result"]:
            bad.append((e["fn"], e["kwargs"], e["result"], got))
    assert not bad, f"{len(bad)} of {len(entries)} plans differ, the first: {bad[0]}"
