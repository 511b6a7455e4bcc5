"""The layouts of the frame tail's memory (wass_amd/csrc/mesh_layout.h: components, plane stages, compaction, inlier buffer,
counters, device record, pinned stage), compiled with the host compiler alone -- the header includes nothing of HIP.
tests/native/mesh_layout_check.cpp carves each over a block of exactly its measured size, for n in {1, 256, 257, 2456 x 2058},
0, 1 and 1800 RANSAC rounds, every 1st and 10th inlier, with and without text, and checks that every piece is 256-aligned, lies
inside measure() and overlaps no other piece of its layout; that the pinned stage holds sizeof(DevState), the largest parameter
block and 1800 x 24 bytes per sample area."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_every_piece_of_every_tail_layout_is_aligned_inside_and_disjoint():
    src = os.path.join(HERE, "native", "mesh_layout_check.cpp")
    out_dir = os.path.join(HERE, "native", "_build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "mesh_layout_check")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", src, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
