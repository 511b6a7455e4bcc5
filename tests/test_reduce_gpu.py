"""wass_amd/csrc/reduce.h, the one statement of the kernels' reductions and scans: tests/native/reduce_check.hip launches every
primitive on a single workgroup (one wave for the wave forms, four waves for the block scan and the tree, 1024 threads for the LDS
scan, block_max twice in one kernel at BY = 1 and 4) and compares bit for bit with host loops that fold in the order the header's
comments state; the doubles are chosen so that a plain left-to-right sum gives other bits (the program checks that first).  A
second test compiles the header alone: it needs nothing of common.h."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(os.path.dirname(HERE), "wass_amd", "csrc", "reduce.h")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
OUT_DIR = os.path.join(HERE, "native", "_build")


@pytest.mark.gpu
def test_every_primitive_folds_in_its_documented_order():
    assert os.path.exists(HIPCC), f"{HIPCC} is missing"
    os.makedirs(OUT_DIR, exist_ok=True)
    exe = os.path.join(OUT_DIR, "reduce_check")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror",
                           os.path.join(HERE, "native", "reduce_check.hip"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


def test_header_stands_alone(tmp_path):
    assert os.path.exists(HIPCC), f"{HIPCC} is missing"
    src = tmp_path / "alone.hip"
    src.write_text(f'#include "{HEADER}"\n'
                   "__global__ void k(double* p) { p[threadIdx.x] = wass::wave_fold(p[threadIdx.x], [](double a, double b) { return a + b; }); }\n")
    out = tmp_path / "alone.s"
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-Wall", "-Werror", "-Wno-unused-command-line-argument", "-S", "--cuda-device-only",
                           str(src),
                           "-o", str(out)])
    assert "ds_bpermute_b32" in out.read_text()
