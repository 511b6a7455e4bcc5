"""wass::Carve (wass_amd/csrc/scratch.h), the piece-by-piece hand-out every scratch layout of the library is stated with, compiled
with the host compiler alone (the header includes nothing of HIP): tests/native/carve_check.cpp takes a mixed list of sizes,
0 among them, from a Carve without memory and from one over a block of exactly the measured size, and checks that both advance
`used` identically, that every piece is 256-aligned, that consecutive pieces do not overlap and that the last ends inside."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_null_carve_measures_what_a_real_one_hands_out():
    src = os.path.join(HERE, "native", "carve_check.cpp")
    out_dir = os.path.join(HERE, "native", "_build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "carve_check")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", src, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
