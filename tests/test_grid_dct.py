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


# ---- the helpers of the shape sweep (tests/test_grid_dct_shapes_gpu.py): the probe's closed form and what the case table reaches
# Bound: the closed form and evaluate() use the same f32 bases; the closed form rounds four f32 products and one difference
# (|ir| < |z|, so the difference amplifies nothing), fp64 rounds none of them to f32: <= 4 * 2^-23 relative.
@pytest.mark.parametrize("shape,cell,coef", [
    ((50, 37, 33), (49, 36), (5, 32)), ((50, 37, 33), (0, 0), None), ((17, 33, 17), (16, 32), (16, 16)),
    ((176, 176, 176), (15, 16), (160, 159)), ((330, 322, 321), (329, 321), (320, 320)), ((24, 2300, 20), (16, 2299), (0, 0)),
    ((1, 40, 1), (0, 39), (0, 0)), ((40, 1, 1), (39, 0), None)])
def test_probe_closed_form_matches_fp64(shape, cell, coef):
    H, W, nf = shape
    zz = np.full((H, W), np.nan, np.float32)
    zz[cell] = 0.37
    x = np.zeros((nf, nf), np.float32)
    if coef is not None:
        x[coef] = 0.5
    gr, dlr, _ = D.evaluate(zz, x, 0.0, np.float64)
    g, dl = D.probe_expected(H, W, nf, cell, 0.37, coef)
    assert g.shape == (nf, nf) and g.dtype == np.float32
    assert (np.abs(g - gr) <= 4 * 2.0 ** -23 * np.abs(gr) + 1e-37).all()
    assert abs(dl - dlr) <= 4 * 2.0 ** -23 * dlr


def test_probe_two_cells_add():
    """count = 2 halves cs and the loss: the sum of the two closed forms is the fp64 gradient of the two-cell grid."""
    H, W, nf = 50, 37, 33
    zz = np.full((H, W), np.nan, np.float32)
    zz[0, 0] = zz[H - 1, W - 1] = 0.37
    gr, dlr, _ = D.evaluate(zz, np.zeros((nf, nf), np.float32), 0.0, np.float64)
    a, la = D.probe_expected(H, W, nf, (0, 0), 0.37, count=2)
    b, lb = D.probe_expected(H, W, nf, (H - 1, W - 1), 0.37, count=2)
    assert (np.abs(a + b - gr) <= 8 * 2.0 ** -23 * np.maximum(np.abs(a), np.abs(b)) + 1e-37).all()
    assert abs(la + lb - dlr) <= 1e-6 * dlr


def test_shape_cases_reach_every_launch_plan():
    """The case table covers what it claims: every k_dct_resid<NFT>, two and three passes, nchunk 1 and 8, a shorter last chunk,
    a tpc above 4 that the four waves do not split evenly, waves without a tile, and small, odd and aligned sizes on both axes."""
    plans = {c: D.plan(*c) for c in D.SHAPE_CASES}
    assert len(set(D.SHAPE_CASES)) == len(D.SHAPE_CASES)
    for (H, W, nf), p in plans.items():
        assert 1 <= nf <= min(H, W)
        assert (p["nchunk"] - 1) * p["tpc"] + p["last"] == p["Wp"] // 16 and 1 <= p["last"] <= p["tpc"] and 1 <= p["nchunk"] <= 8
        assert sum(p["nft"]) == p["nfp"] // 16 and all(n == 10 for n in p["nft"][:-1])
    assert {n for p in plans.values() for n in p["nft"]} == set(range(1, 11))
    assert {len(p["nft"]) for p in plans.values()} >= {1, 2, 3}
    assert {p["nchunk"] for p in plans.values()} >= {1, 8}
    assert any(p["tpc"] >= 2 and p["last"] < p["tpc"] for p in plans.values())
    assert any(p["tpc"] > 4 and p["tpc"] % 4 for p in plans.values())
    assert any(p["tpc"] < 4 for p in plans.values())                  # t_end < RESID_WAVES: waves that hold only zeros
    for axis in (0, 1):
        sizes = {c[axis] for c in D.SHAPE_CASES}
        assert any(s < 16 for s in sizes) and 1 in sizes
        assert any(s % 2 and s > 16 for s in sizes)
        assert any(s % 16 == 0 for s in sizes)


def test_plan_matches_the_source():
    """plan() restates constants of grid_dct.hip: fail when they move."""
    src = open(os.path.join(ROOT, "wass_amd", "csrc", "grid_dct.hip")).read()
    for line in ("constexpr int RESID_WAVES = 4;", "constexpr int FT_GROUP = 10;", "int nchunk = (512 + nrb - 1) / nrb;",
                 "if (nchunk > 8) nchunk = 8;", "p.tpc = (nct + nchunk - 1) / nchunk;", "p.nchunk = (nct + p.tpc - 1) / p.tpc;"):
        assert line in src, line


def test_seeded_start_restatement():
    x = D.splitmix_x0(0, 4)
    assert x.dtype == np.float32 and ((x >= 0) & (x < 1)).all() and len(np.unique(x)) == 16
    # splitmix64's first output for state 0 is 0xE220A8397B1DCDAF (the published test vector): its top 24 bits
    assert x[0, 0] == np.float32(0xE220A8 / 16777216.0)
    assert not np.array_equal(D.splitmix_x0(1, 4), x)
