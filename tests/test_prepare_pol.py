"""Polarimetric preparation without a GPU: the staged numpy oracle (tests/prepare_pol_oracle.py) against the definitions, its map and
fixed-point sampler against oracle.undistort, the physics of a linear polariser, the float TIFF files and the C boundary."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import polarimetric_oracle as PO  # noqa: E402
import prepare_pol_oracle as PP  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def test_module_imports():
    """The failing-first test: there is no wass_amd.prepare before this feature."""
    from wass_amd import prepare
    assert callable(prepare.polarimetric_prepare) and callable(prepare.write_tiff_f32) and callable(prepare.read_tiff_f32)
    assert callable(prepare.write_polarimetric_outputs)
    assert prepare.PREP_OUTPUTS[0] == "stokes"


@pytest.mark.parametrize("rows,cols", [(2, 2), (6, 8), (5, 3), (7, 10), (9, 9)])
def test_demosaic_indexing(rows, cols):
    I = PP.random_mosaic(rows, cols, 1)
    I0, I45, I90, I135 = PP.demosaic(I)
    m, n = rows // 2, cols // 2
    for q in (I0, I45, I90, I135):
        assert q.shape == (m, n)
    J = I[:2 * m, :2 * n]
    np.testing.assert_array_equal(I0, J[1::2, 1::2])
    np.testing.assert_array_equal(I45, J[0::2, 1::2])
    np.testing.assert_array_equal(I90, J[0::2, 0::2])
    np.testing.assert_array_equal(I135, J[1::2, 0::2])
    for i in range(m):                                  # and by the reference's pointer walk
        for j in range(n):
            assert (I90[i, j], I45[i, j], I135[i, j], I0[i, j]) == (I[2 * i, 2 * j], I[2 * i, 2 * j + 1], I[2 * i + 1, 2 * j], I[2 * i + 1, 2 * j + 1])
    f = PP.to_float(I0)
    assert f.dtype == F
    np.testing.assert_array_equal(f, I0.astype(F) * F(F(1) / F(255)))


@pytest.mark.parametrize("m,n", [(1, 1), (1, 4), (3, 2), (5, 7)])
def test_upscale(m, n):
    q = np.random.default_rng(m * 10 + n).random((m, n)).astype(F)
    u = PP.upscale2(q)
    assert u.shape == (2 * m, 2 * n) and u.dtype == F
    # the first and last row and column are the source's, resized along the other axis alone
    rowsrc = np.stack([PP.upscale2(q[r:r + 1])[0] for r in range(m)])           # [m, 2n]
    colsrc = np.stack([PP.upscale2(q[:, c:c + 1])[:, 0] for c in range(n)], 1)  # [2m, n]
    np.testing.assert_array_equal(u[0], rowsrc[0])
    np.testing.assert_array_equal(u[-1], rowsrc[-1])
    np.testing.assert_array_equal(u[:, 0], colsrc[:, 0])
    np.testing.assert_array_equal(u[:, -1], colsrc[:, -1])
    for c in (u[0, 0], u[0, -1], u[-1, 0], u[-1, -1]):
        assert c in q
    assert u[0, 0] == q[0, 0] and u[-1, -1] == q[-1, -1] and u[0, -1] == q[0, -1] and u[-1, 0] == q[-1, 0]
    # interior: 0.25 / 0.75 blends, along x first
    for X in range(1, 2 * n - 1):
        j = X // 2
        a, b, wa, wb = (j, j + 1, F(0.75), F(0.25)) if X & 1 else (j - 1, j, F(0.25), F(0.75))
        np.testing.assert_array_equal(rowsrc[:, X], q[:, a] * wa + q[:, b] * wb)
    for Y in range(1, 2 * m - 1):
        i = Y // 2
        a, b, wa, wb = (i, i + 1, F(0.75), F(0.25)) if Y & 1 else (i - 1, i, F(0.25), F(0.75))
        np.testing.assert_array_equal(u[Y], rowsrc[a] * wa + rowsrc[b] * wb)
    flat = PP.upscale2(np.full((m, n), F(0.3137255)))
    assert np.all(flat == F(0.3137255))


def test_map_and_fixed_point_sampler_equal_the_undistort_oracle(oracle):
    """The tie: the oracle's map plus the fixed-point bilinear table reproduce oracle.undistort bit for bit."""
    itab = oracle.inter_tab(2)
    for (w, h), name in (((64, 48), "calibdir"), ((64, 48), "barrel"), ((70, 50), "eight"), ((131, 67), "calibdir"), ((258, 10), "calibdir")):
        img = PP.random_mosaic(h, w, 7)
        K, dist = PP.camera(w, h), PP.DIST[name]
        iu, iv = PP.undistort_map(w, h, K, dist)
        np.testing.assert_array_equal(PP.remap_fixed_u8(img, iu, iv, itab), oracle.undistort(img, K, dist), err_msg=f"{w} x {h} {name}")
    # the float sampler is the one polarimetric_setup uses wherever the map is a float32 number of 1/32 pixels
    w, h = 64, 48
    iu, iv = PP.undistort_map(w, h, PP.camera(w, h), PP.DIST["calibdir"])
    pic = np.random.default_rng(3).random((h, w)).astype(F)
    np.testing.assert_array_equal(PP.remap_float(pic, iu, iv), PO.remap_linear_f32(pic, (iu / 32.0).astype(F), (iv / 32.0).astype(F)))


def test_zero_distortion_is_the_identity_map():
    w, h = 70, 50
    iu, iv = PP.undistort_map(w, h, PP.camera(w, h), np.zeros(5))
    y, x = np.mgrid[0:h, 0:w]
    np.testing.assert_array_equal(iu, 32 * x)
    np.testing.assert_array_equal(iv, 32 * y)


@pytest.mark.parametrize("name", ["zero", "calibdir", "barrel"])
def test_mix_enforces_the_constraint(name):
    o = PP.prepare(PP.random_mosaic(48, 64, 11), PP.camera(64, 48), PP.DIST[name])
    I0, I45, I90, I135 = o["I"]
    ulp = np.spacing(np.abs(o["S"][0]))
    ulp = np.maximum(ulp, np.spacing(F(2.0 ** -8)))      # where S0 is 0 (outside the picture) everything is 0
    err = np.abs((I0 + I90).astype(np.float64) - (I45 + I135).astype(np.float64))
    print(f"{name}: largest |I0 + I90 - I45 - I135| = {np.max(err / ulp):.2f} ulp of S0")
    assert np.all(err <= 4 * ulp)
    # before the mix the constraint does not hold: the check can fail
    a0, a45, a90, a135 = o["und"]
    assert np.max(np.abs((a0 + a90) - (a45 + a135))) > 0.1


def test_flat_mosaic():
    for level in (0, 1, 77, 255):
        o = PP.prepare(np.full((20, 30), level, np.uint8), PP.camera(30, 20), PP.DIST["calibdir"])
        S = o["S"]
        assert np.all(S[1] == 0) and np.all(S[2] == 0)
        lit = S[0] > 0
        assert lit.any() == (level > 0)
        assert np.all(o["dolp_f32"][lit] == 0) and np.all(o["dolp"][lit] == 0)


@pytest.mark.parametrize("rho,phi", [(0.6, 0.3), (0.25, 2.0), (0.9, 1.2)])
def test_linear_polariser(rho, phi):
    """A linear polariser of degree rho and angle phi, zero distortion: the index pictures give rho and phi back within the u8
    quantisation bound.  With q = 0.5 / 255 (a u8 sample of I) and g the largest change of an ideal channel over the at most 2 + 2 raw
    pixels between an output pixel and the samples its value is made of, every sample is within delta = q + 4 g of the ideal channel at the
    pixel.  Ideal channels satisfy the constraint, so the mix leaves them alone, and S0 = sum / 2, S1 = a0 - a90, S2 = a45 - a135 are each
    within 2 delta.  With L = rho S0: |dL| <= 2 sqrt(2) delta, so |dolp - rho| <= (2 sqrt(2) + 2 rho) delta / (min S0 - 2 delta), plus q
    for the index; the angle atan2(S1, S2) = pi / 2 - 2 phi is within asin(2 sqrt(2) delta / (rho min S0)), plus one half step of the
    index, 3.1415 / 255, in the decoded angle.  Float32 rounding (1e-6) is far below both."""
    rows, cols = 40, 56
    mosaic, S0 = PP.polariser_mosaic(rows, cols, rho, phi)
    o = PP.prepare(mosaic, PP.camera(cols, rows), np.zeros(5))
    q = 0.5 / 255
    g = 0.1 / 400.0 * (1 + rho) / 2                      # |d S0 / d x|, |d S0 / d y| <= 0.1 / 400 per raw pixel
    delta = q + 4 * g + 1e-6
    s0min = float(S0.min())
    bound_rho = (2 * np.sqrt(2) + 2 * rho) * delta / (s0min - 2 * delta) + q
    bound_ang = np.arcsin(2 * np.sqrt(2) * delta / (rho * s0min)) + 3.1415 / 255
    got_rho = o["dolp"].astype(np.float64) / 255
    ang = (o["aolp"].astype(np.float64) - 127) * (3.1415 / 255) * 2 + 3.1415
    want = (np.pi / 2 - 2 * phi) % (2 * np.pi)
    err_ang = np.abs((ang - want + np.pi) % (2 * np.pi) - np.pi)
    print(f"rho {rho}: largest error {np.max(np.abs(got_rho - rho)):.5f} (bound {bound_rho:.5f}); "
          f"angle: largest error {np.max(err_ang):.5f} rad (bound {bound_ang:.5f})")
    assert np.all(np.abs(got_rho - rho) <= bound_rho)
    assert np.all(err_ang <= bound_ang)
    assert np.all(np.abs(o["S"][0] - S0[:rows, :cols]) <= 2 * delta)


def test_sat_u8():
    v = np.array([np.nan, np.inf, -np.inf, 0.5, 1.5, 2.5, 254.5, 255.5, -0.5, -3.0, 300.0, 126.49999, 126.50001], F)
    np.testing.assert_array_equal(PP.sat_u8(v), [0, 255, 0, 0, 2, 2, 254, 255, 0, 0, 255, 126, 127])


def test_transcendental_pictures_of_the_oracle_stay_clear_of_the_boundaries():
    """The seed of the GPU test: the oracle's own float32 pictures differ from their fp64 evaluation by a few ulps, and at most 1 % of the
    pixels lie within the bound of a rounding boundary."""
    o = PP.prepare(PP.random_mosaic(48, 64, 5), PP.camera(64, 48), PP.DIST["calibdir"], hdr=True)
    for what in ("image", "aolp"):
        o32, o64 = o[what + "_f32"], o[what + "_f64"]
        bound, n = PP.transcendental_bound(o32, o64)
        near = PP.near_boundary(o64, bound)
        print(f"{what}: oracle float32 against fp64: {n:.3e}; pixels near a boundary: {near.mean() * 100:.3f} %")
        assert near.mean() <= 0.01
        ok = np.isfinite(o64)
        assert np.all(np.abs(o32.astype(np.float64) - o64)[ok] <= bound[ok])
        np.testing.assert_array_equal(o[what][~near], PP.sat_u8(o64)[~near])


# ---- files --------------------------------------------------------------------------------------------------------------------------------
def _tricky_picture():
    a = np.random.default_rng(2).standard_normal((7, 5)).astype(F)
    a[0, 0], a[1, 2], a[2, 3], a[3, 1] = np.nan, -0.0, np.inf, -np.inf
    a.view(np.uint32)[4, 4] = 0x7fc12345                  # a NaN with a payload
    a[5, 0] = np.finfo(F).tiny / 4                        # a denormal
    return a


@pytest.mark.parametrize("shape", [(7, 5), (1, 1), (3, 8)])
def test_tiff_round_trip(tmp_path, shape):
    from wass_amd.prepare import read_tiff_f32, write_tiff_f32
    a = _tricky_picture() if shape == (7, 5) else np.random.default_rng(1).random(shape).astype(F)
    p = tmp_path / "a.tiff"
    write_tiff_f32(p, a)
    b = read_tiff_f32(p)
    assert b.dtype == F and b.shape == a.shape
    np.testing.assert_array_equal(b.view(np.uint32), a.view(np.uint32))
    raw = p.read_bytes()
    assert raw[:4] == b"II*\0" and len(raw) == 8 + a.size * 4 + (a.size * 4 & 1) + 2 + 10 * 12 + 4
    with pytest.raises(ValueError):
        (tmp_path / "bad.tiff").write_bytes(b"not a tiff at all")
        read_tiff_f32(tmp_path / "bad.tiff")


def test_tiff_cross_read(tmp_path):
    """An independent reader sees the same picture, and ours reads what an independent writer wrote."""
    from wass_amd.prepare import read_tiff_f32, write_tiff_f32
    a = _tricky_picture()
    p = tmp_path / "a.tiff"
    write_tiff_f32(p, a)
    try:
        import tifffile
    except ImportError:
        tifffile = None
    try:
        from PIL import Image
    except ImportError:
        Image = None
    if tifffile is None and Image is None:
        pytest.skip("no independent TIFF reader (PIL, tifffile) is installed")
    if tifffile is not None:
        np.testing.assert_array_equal(np.asarray(tifffile.imread(str(p)), F).view(np.uint32), a.view(np.uint32))
        tifffile.imwrite(str(tmp_path / "t.tiff"), a)
        np.testing.assert_array_equal(read_tiff_f32(tmp_path / "t.tiff").view(np.uint32), a.view(np.uint32))
    if Image is not None:
        with Image.open(str(p)) as im:
            assert im.mode == "F" and im.size == (a.shape[1], a.shape[0])
            np.testing.assert_array_equal(np.asarray(im, F).view(np.uint32), a.view(np.uint32))
        Image.fromarray(a, mode="F").save(str(tmp_path / "p.tiff"))
        np.testing.assert_array_equal(read_tiff_f32(tmp_path / "p.tiff").view(np.uint32), a.view(np.uint32))


def test_png_writer(tmp_path):
    import struct
    import zlib
    from wass_amd.prepare import write_png_u8
    a = PP.random_mosaic(9, 13, 4)
    p = tmp_path / "a.png"
    write_png_u8(p, a)
    raw = p.read_bytes()
    assert raw[:8] == b"\x89PNG\r\n\x1a\n"
    at, body = 8, b""
    while at < len(raw):
        (n,) = struct.unpack(">I", raw[at:at + 4])
        kind, data = raw[at + 4:at + 8], raw[at + 8:at + 8 + n]
        assert struct.unpack(">I", raw[at + 8 + n:at + 12 + n])[0] == zlib.crc32(kind + data) & 0xffffffff
        if kind == b"IHDR":
            assert struct.unpack(">IIBBBBB", data) == (13, 9, 8, 0, 0, 0, 0)
        if kind == b"IDAT":
            body += data
        at += 12 + n
    rows = np.frombuffer(zlib.decompress(body), np.uint8).reshape(9, 14)
    assert np.all(rows[:, 0] == 0)
    np.testing.assert_array_equal(rows[:, 1:], a)


def test_write_polarimetric_outputs_names(tmp_path):
    from wass_amd.prepare import PolarimetricFrame, read_tiff_f32, write_polarimetric_outputs
    o = PP.prepare(PP.random_mosaic(10, 12, 9), PP.camera(12, 10), PP.DIST["calibdir"])
    frame = PolarimetricFrame(image=o["image"], ranges={}, S=o["S"], channels=o["channels"])
    written = write_polarimetric_outputs(tmp_path / "undistorted", "00000000", frame)
    names = sorted(os.path.basename(p) for p in written)
    assert names == sorted(["00000000.png", "00000000_S0.tiff", "00000000_S1.tiff", "00000000_S2.tiff", "00000000_I0.png",
                            "00000000_I45.png", "00000000_I90.png", "00000000_I135.png"])
    for k in range(3):
        np.testing.assert_array_equal(read_tiff_f32(tmp_path / "undistorted" / f"00000000_S{k}.tiff").view(np.uint32), o["S"][k].view(np.uint32))
    only = write_polarimetric_outputs(tmp_path / "plain", "00000001", PolarimetricFrame(image=o["image"], ranges={}))
    assert [os.path.basename(p) for p in only] == ["00000001.png"]


# ---- the C boundary -----------------------------------------------------------------------------------------------------------------------
def test_symbols_in_header_and_binding():
    from wass_amd import _lib
    header = open(os.path.join(ROOT, "include", "wass_gpu.h")).read()
    for name in ("wass_prepare_pol", "wass_prepare_pol_dev"):
        assert re.search(r"\b%s\s*\(" % name, header)
        assert name in _lib.SYMBOLS
    assert "wass_pol_prep_params" in header and "wass_pol_prep_out" in header
    from wass_amd import build
    lib = ctypes.CDLL(build.build())
    assert hasattr(lib, "wass_prepare_pol") and hasattr(lib, "wass_prepare_pol_dev")


def test_struct_sizes_match_the_header(tmp_path):
    from wass_amd import _lib, prepare
    pairs = [("wass_pol_prep_params", _lib.PolPrepParams), ("wass_pol_prep_out", _lib.PolPrepOut)]
    body = "".join(f'printf("%zu\\n", sizeof({c}));' for c, _ in pairs)
    bits = "".join(f'printf("%d\\n", {b});' for b in ("WASS_PREP_STOKES", "WASS_PREP_DOLP", "WASS_PREP_AOLP", "WASS_PREP_CHANNELS",
                                                     "WASS_PREP_IMAGE_F32", "WASS_PREP_AOLP_F32"))
    src = tmp_path / "sizes.c"
    src.write_text(f'#include <stdio.h>\n#include "wass_gpu.h"\nint main(void) {{ {body} {bits} return 0; }}\n')
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert out[:2] == [ctypes.sizeof(py) for _, py in pairs]
    assert out[2:] == [1 << k for k in range(len(prepare.PREP_OUTPUTS))]


def test_python_argument_errors():
    from wass_amd import prepare
    with pytest.raises(ValueError):
        prepare._prep_outputs(("stokes", "colour"))
    assert prepare._prep_outputs("stokes") == 1 and prepare._prep_outputs(prepare.PREP_OUTPUTS) == 63
    with pytest.raises(ValueError):
        prepare.write_tiff_f32("/nonexistent/x.tiff", np.zeros((2, 2, 2), F))
