"""Writes tests/golden/ctx_plans.json: what the pure C planners of the operators that keep their scratch in the context answer for
a table of sizes: wass_ac_scratch_bytes, wass_epi_scratch_bytes and wass_match_scratch_bytes, called through _lib.load() (no GPU).
Run it on the commit whose plans are to be pinned:

    python tests/golden/make_golden_ctx_plans.py

Every entry is {"fn", "args", "result"}; result is the bytes, or {"error": the planner's return code}.
tests/test_ctx_plans.py replays the entries."""
from __future__ import annotations

import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))

AC_MAX_N = 1 << 22
EPI_MAX_ROUNDS = 65536
MATCH_MAX_N = 8192
BATCHES = (0, 1, 2, 15, 16, 17, 31, 32, 33, 64, 1000, 65535, 65536)


def table():
    t = []
    # n: 0 and below, every size up to 80 (3 n, 6 n and AC_LIN n doubles cross multiples of 256 bytes at 32, 16 and below; a
    # workgroup takes 64 points), sizes either side of larger multiples, the largest and one above it
    ns = list(range(-1, 81)) + [127, 128, 129, 255, 256, 257, 1000, 4095, 4096, 4097, 123457, AC_MAX_N - 1, AC_MAX_N, AC_MAX_N + 1]
    t += [("wass_ac_scratch_bytes", (n,)) for n in ns]
    # batch, rounds: 2 b ints and 9 b doubles are 256-aligned at 32 pairs, b rounds ints at 64; no round, the most and one above
    t += [("wass_epi_scratch_bytes", (b, r)) for b in BATCHES for r in (-1, 0, 1, 2, 3, 31, 32, 33, 63, 64, 65, 1000, 1024, EPI_MAX_ROUNDS, EPI_MAX_ROUNDS + 1)]
    # batch, n_max: 4 b ints are 256-aligned at 16 problems, b n doubles at 32 cells; no candidate, the most and one above
    t += [("wass_match_scratch_bytes", (b, n)) for b in BATCHES for n in (0, 1, 2, 3, 4, 5, 6, 31, 32, 33, 100, 1000, MATCH_MAX_N - 1, MATCH_MAX_N, MATCH_MAX_N + 1)]
    return t


def answer(fn: str, args):
    from wass_amd import _lib
    b = C.c_size_t()
    rc = getattr(_lib.load(), fn)(*args, C.byref(b))
    return {"error": rc} if rc else b.value


def main():
    entries = [{"fn": fn, "args": list(a), "result": answer(fn, a)} for fn, a in table()]
    path = os.path.join(HERE, "ctx_plans.json")
    with open(path, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(e) for e in entries) + "\n]\n")
    print(f"{len(entries)} entries -> {path}")


if __name__ == "__main__":
    main()
