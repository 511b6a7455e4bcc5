"""The sequence layer of the gridding stage, the parts that need no GPU: the mesh_cam.xyzC reader against the reference's own
decoding, the numpy restatements (tests/grid_seq_oracle.py) against scipy and against hand-made cases, and the C ABI."""
import ctypes
import os
import re
import warnings

import numpy as np
import pytest

import grid_seq_oracle as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["wass_grid_dct_batch", "wass_grid_dct_batch_dev", "wass_mesh_grid_cells_dev", "wass_grid_median_dev",
               "wass_grid_seq_create", "wass_grid_seq_push_dev", "wass_grid_seq_finish", "wass_grid_seq_zero_mean_dev",
               "wass_grid_seq_destroy"]


@pytest.mark.parametrize("case", [0, 1])
def test_load_camera_mesh_reproduces_the_reference_decoding(tmp_path, case):
    """tests/golden/xyzc_case*.npz: mesh_cam.xyzC bytes and what the reference's reader made of them -- bit for bit."""
    from wass_amd.gridding import load_camera_mesh
    g = np.load(os.path.join(ROOT, "tests", "golden", f"xyzc_case{case}.npz"))
    f = tmp_path / "mesh_cam.xyzC"
    f.write_bytes(g["xyzc"].tobytes())
    got = load_camera_mesh(str(f))
    want = g["ref_decoded"]
    assert got.dtype == want.dtype and got.shape == want.shape and got.shape[0] == 3 and got.shape[1] > 100
    assert got.tobytes() == np.ascontiguousarray(want).tobytes()


def test_load_camera_mesh_empty_cloud(tmp_path):
    from wass_amd.gridding import load_camera_mesh
    head = np.concatenate([[1.0, 1.0, 1.0, 0.0, 0.0, 0.0], np.eye(3).ravel(), [0.0, 0.0, 0.0]])
    f = tmp_path / "mesh_cam.xyzC"
    f.write_bytes(np.uint32(0).tobytes() + head.astype("<f8").tobytes())
    assert load_camera_mesh(str(f)).shape == (3, 0)


@pytest.mark.parametrize("k", [3, 5])
@pytest.mark.parametrize("shape", [(1, 9), (37, 53), (6, 1), (64, 64)])
def test_median_restatement_equals_scipy(k, shape):
    ndi = pytest.importorskip("scipy.ndimage")
    z = np.random.default_rng(k * 100 + shape[1]).normal(0, 1, shape).astype(np.float32)
    got = S.median_blur(z, k)
    want = ndi.median_filter(z, size=k, mode="nearest")
    assert got.dtype == np.float32
    np.testing.assert_array_equal(got, want)


def test_median_restatement_mask_and_sizes():
    z = np.arange(35, dtype=np.float32).reshape(5, 7)
    m = np.ones((5, 7), np.uint8); m[:, 2] = 0
    got = S.median_blur(z, 3, m)
    assert np.isnan(got[:, 2]).all() and np.isfinite(got[:, [0, 1, 3, 4, 5, 6]]).all()
    # the cell (2, 1): window rows 1..3, columns 0..2 with column 2 zeroed = {7, 8, 0, 14, 15, 0, 21, 22, 0} -> 8
    assert got[2, 1] == 8.0
    # a corner replicates the border: window of (0, 0) = {0, 0, 1, 0, 0, 1, 7, 7, 8} -> 1
    assert S.median_blur(z, 3)[0, 0] == 1.0
    np.testing.assert_array_equal(S.median_blur(z, 0), z)
    for bad in (4, 7):
        with pytest.raises(ValueError):
            S.median_blur(z, bad)
    assert S.median_blur(np.stack([z, z + 1]), 5).shape == (2, 5, 7)


def test_statistics_restatement_on_hand_made_frames():
    a = np.array([[1.0, 2.0, np.nan], [3.0, -4.0, np.nan]], np.float32)          # a masked column
    b = np.array([[0.5, 0.5, np.nan], [0.5, 0.5, np.nan]], np.float32)
    st = S.sequence_stats(np.stack([a, b]))
    assert st["zmin"] == -4.0 and st["zmax"] == 3.0 and st["zmean"] == (0.5 + 0.5) / 2
    np.testing.assert_array_equal(st["frame_mean"], [0.5, 0.5])
    np.testing.assert_array_equal(st["mean_perpoint_mm"], np.array([[750.0, 1250.0, np.nan], [1750.0, -1750.0, np.nan]]))
    np.testing.assert_array_equal(st["z_mm"][0], np.array([[1000, 2000, np.nan], [3000, -4000, np.nan]], np.float32))
    fz = S.sequence_stats(np.stack([a, b]), force_zero_mean=True)
    assert fz["zmean"] == 0.0 and fz["zmax"] == 4.0 and fz["zmin"] == -4.0
    zm = S.zero_mean(st["z_mm"], st["mean_perpoint_mm"])
    assert zm.dtype == np.float32
    np.testing.assert_array_equal(zm[0], np.array([[250, 750, np.nan], [1250, -2250, np.nan]], np.float32))
    # one frame without data: numpy's amin / amax / mean over the per-frame lists are NaN, and so is the per-point mean
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        st = S.sequence_stats(np.stack([a, np.full_like(a, np.nan), b]))
    assert np.isnan(st["zmin"]) and np.isnan(st["zmax"]) and np.isnan(st["zmean"])
    assert np.isnan(st["mean_perpoint_mm"]).all() and np.isnan(st["frame_mean"][1]) and st["frame_min"][0] == -4.0
    # float32 minus float64, rounded once to float32
    c = np.array([[[0.1]]], np.float32) * np.float32(1000)
    m = np.array([[1.0 / 3.0]])
    assert S.zero_mean(c, m)[0, 0, 0] == np.float32(np.float64(c[0, 0, 0]) - m[0, 0])


def test_header_declares_and_library_exports_the_sequence_layer():
    from wass_amd import _lib, build
    src = open(os.path.join(ROOT, "include", "wass_gpu.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = ctypes.CDLL(build.build())
    for n in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % n, src), f"{n} is not declared in wass_gpu.h"
        assert hasattr(lib, n), f"{n} is not exported by libwassgpu.so"
        assert n in _lib.SYMBOLS
    assert "wass_grid_seq_stats" in src
    assert ctypes.sizeof(_lib.GridSeqStats) == 32


def test_grid_seq_stats_size_matches_the_compiled_header(tmp_path):
    import subprocess
    from wass_amd import _lib
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include "wass_gpu.h"\nint main(void) { printf("%zu\\n", sizeof(wass_grid_seq_stats)); return 0; }\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert int(subprocess.check_output([str(exe)])) == ctypes.sizeof(_lib.GridSeqStats)
