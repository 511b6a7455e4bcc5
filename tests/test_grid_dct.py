"""DCT surface interpolation (grid_dct.hip), the parts that need no GPU: the numpy oracle against the reference's recorded
output, the basis formula, the ABI structs, and the ISA of the kernels."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import dct_oracle as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "dct_interp.npz")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def golden_cases():
    g = np.load(GOLDEN)
    for name in ("one", "default", "early"):
        o = g[f"{name}_opts"]
        opts = {"Nfreqs": int(o[0]), "MAX_ITERS": int(o[1]), "TOLERANCE_CHANGE": float(o[2]), "REGULARIZER_ALPHA": float(o[3]),
                "LEARNING_RATE": float(o[4])}
        yield name, g[str(g[f"{name}_zz"])], opts, g[f"{name}_x0"], g[f"{name}_irec"], int(g[f"{name}_steps"])


@pytest.mark.parametrize("case", ["one", "default", "early"])
def test_fp32_oracle_reproduces_the_reference(case):
    name, zz, opts, x0, irec, steps = next(c for c in golden_cases() if c[0] == case)
    got, _, nsteps, _, _ = D.interpolate(zz, x0, opts, dtype=np.float32)
    std = float(np.nanstd(zz))
    assert nsteps == steps
    assert np.max(np.abs(got - irec)) <= 1e-5 * std


@pytest.mark.parametrize("n", [16, 96, 150, 1024])
def test_basis_matches_scipy_dct(n):
    from scipy.fftpack import dct
    ref = dct(np.eye(n), type=3, norm="ortho")
    assert np.max(np.abs(D.dct_basis(n) - ref)) <= 1e-13


def test_dct_ctypes_struct_sizes_match_the_compiled_header(tmp_path):
    from wass_amd import _lib
    pairs = [("wass_dct_opts", _lib.DctOpts), ("wass_dct_info", _lib.DctInfo)]
    src = tmp_path / "sizes.c"
    body = "".join(f'printf("%zu\\n", sizeof({c}));' for c, _ in pairs)
    src.write_text(f'#include <stdio.h>\n#include "wass_gpu.h"\nint main(void) {{ {body} return 0; }}\n')
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    sizes = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    for (cname, py), sz in zip(pairs, sizes):
        assert ctypes.sizeof(py) == sz, cname


def test_grid_dct_isa_has_no_wide_buffer_store_with_sgpr_offset(tmp_path):
    """The gfx950 store trap of tests/test_isa_traps.py, on the DCT kernels; they use the f32 MFMA as designed."""
    from wass_amd import build
    out = tmp_path / "grid_dct.s"
    flags = [f for f in build.FLAGS if f != "-fPIC"]
    subprocess.check_call([HIPCC, *flags, "-S", "--cuda-device-only", "-c", os.path.join(ROOT, "wass_amd", "csrc", "grid_dct.hip"), "-o", str(out)],
                          stderr=subprocess.DEVNULL)
    asm = out.read_text()
    assert "global_store_dword" in asm or "buffer_store_dword" in asm
    assert "v_mfma_f32_16x16x4_f32" in asm or "v_mfma_f32_16x16x4f32" in asm
    bad = re.findall(r"buffer_store_dwordx[34]\s+[^\n]*\],\s*s\d+[^\n]*", asm)
    assert not bad, f"{len(bad)} wide buffer stores with an SGPR offset, e.g. {bad[0].strip()}"
