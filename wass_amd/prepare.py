"""Polarimetric camera preparation: the `--demosaic` branch of wass_prepare (src/wass_prepare/wass_prepare.cpp:52-85, :103-255) as a
function.  A polarising-filter-array mosaic goes through one fused HIP kernel (wass_amd/csrc/prepare_pol.hip) and comes back as the
float32 Stokes pictures that postproc.polarimetric_setup samples, the u8 stereo input picture and, on request, the DOLP / AOLP index
pictures and the four mixed channel pictures.  The float TIFF and PNG writers name the files as the reference does."""
from __future__ import annotations

import ctypes as C
import os
import struct
import zlib
from dataclasses import dataclass

import numpy as np

from .stereo import Context, _is_device

# bit k of the C entry's `outputs` is PREP_OUTPUTS[k]
PREP_OUTPUTS = ("stokes", "dolp", "aolp", "channels", "image_f32", "aolp_f32")
RANGE_NAMES = ("S0", "S1", "S2", "dolp")


@dataclass
class PolarimetricFrame:
    """What polarimetric_prepare returns, every picture 2m x 2n for a mosaic of rows x cols (m = rows // 2, n = cols // 2).  Pictures
    not named in `outputs` are None."""
    image: object                   # uint8 [2m, 2n]: the stereo input picture, S0 x 127 or the HDR picture x 255, after CLAHE if asked
    ranges: dict                    # {"S0": (min, max), "S1": ..., "S2": ..., "dolp": ...} float32, NaN skipped; dolp NaN unless asked
    S: object = None                # float32 [3, 2m, 2n]: S0, S1, S2
    dolp: object = None             # uint8 [2m, 2n]: the DOLP index, rint(dolp x 255)
    aolp: object = None             # uint8 [2m, 2n]: the AOLP index, rint(aolp x 255 / 3.1415 + 127)
    channels: object = None         # uint8 [4, 2m, 2n]: the mixed I0, I45, I90, I135 x 255
    image_f32: object = None        # float32 [2m, 2n]: `image` before rounding (and before CLAHE)
    aolp_f32: object = None         # float32 [2m, 2n]: `aolp` before rounding


_FIELDS = {"stokes": ("S", lambda H, W: (3, H, W), "float32"), "dolp": ("dolp", lambda H, W: (H, W), "uint8"),
           "aolp": ("aolp", lambda H, W: (H, W), "uint8"), "channels": ("channels", lambda H, W: (4, H, W), "uint8"),
           "image_f32": ("image_f32", lambda H, W: (H, W), "float32"), "aolp_f32": ("aolp_f32", lambda H, W: (H, W), "float32")}


def _prep_outputs(outputs) -> int:
    outputs = (outputs,) if isinstance(outputs, str) else tuple(outputs)
    for name in outputs:
        if name not in PREP_OUTPUTS:
            raise ValueError(f"unknown output {name!r}: choose among {PREP_OUTPUTS}")
    return sum(1 << k for k, name in enumerate(PREP_OUTPUTS) if name in outputs)


def polarimetric_prepare(image, K, dist, hdr: bool = False, outputs=("stokes",), clahe=None, ctx: Context | None = None) -> PolarimetricFrame:
    """wass_prepare --demosaic for one picture.  `image` is the u8 mosaic, rows x cols, macro-pixels [[I90, I45], [I135, I0]], a host
    array (host results) or a device tensor (device tensors); K (3 x 3) applies to the 2m x 2n result, dist holds 0, 4, 5, 8 or 12
    OpenCV distortion coefficients.  Per pixel of the result: the quarter pictures as float32 (u8 / 255), upscaled x2 bilinearly, undistorted
    with Context.undistort's map and postproc.remap_linear_f32's sampler, mixed so that I0 + I90 = I45 + I135, then S0 = (I0 + I45 + I90 +
    I135) / 2, S1 = I0 - I90, S2 = I45 - I135.  `image` of the result is S0 x 127 rounded to u8, or with hdr=True the exposure-weighted HDR
    picture x 255; clahe=(clip_limit, tiles) equalises it as Context.clahe does.  outputs: any of PREP_OUTPUTS."""
    if len(image.shape) != 2:
        raise ValueError("the mosaic must be rows x cols")
    rows, cols = (int(v) for v in image.shape)
    bits = _prep_outputs(outputs)
    K = np.ascontiguousarray(np.asarray(K, np.float64))
    if K.shape != (3, 3):
        raise ValueError("K must be 3 x 3")
    dist = np.ascontiguousarray(np.asarray(dist, np.float64).ravel())
    clip, tiles = (0.0, 0) if clahe is None else (float(clahe[0]), int(clahe[1]))
    if clahe is not None and tiles < 1:
        raise ValueError("clahe = (clip_limit, tiles) with tiles >= 1")
    from ._lib import PolPrepOut, PolPrepParams
    if ctx is None:
        ctx = Context(0)
    H, W = max(rows // 2, 0) * 2, max(cols // 2, 0) * 2
    dev = _is_device(image)
    if dev:
        import torch
        src = image if image.dtype == torch.uint8 and image.stride(1) == 1 and image.stride(0) >= cols else image.to(torch.uint8).contiguous()
        new = lambda shape, dt: torch.empty(shape, dtype=getattr(torch, dt), device=src.device)
        ptr = lambda a: a.data_ptr()
        stride = src.stride(0) if rows > 1 else cols
        entry = ctx._lib.wass_prepare_pol_dev
        torch.cuda.current_stream(src.device).synchronize()
    else:
        src = np.ascontiguousarray(image, np.uint8)
        new = lambda shape, dt: np.empty(shape, getattr(np, dt))
        ptr = lambda a: a.ctypes.data
        stride = cols
        entry = ctx._lib.wass_prepare_pol
    got = {"image": new((H, W), "uint8")}
    for k, name in enumerate(PREP_OUTPUTS):
        if bits >> k & 1:
            field, shape, dt = _FIELDS[name]
            got[field] = new(shape(H, W), dt)
    p = PolPrepParams(int(bool(hdr)), bits, clip, tiles, 0)
    o = PolPrepOut()
    for field, a in got.items():
        setattr(o, field, ptr(a))
    Kc = (C.c_double * 9)(*K.ravel())
    dc = (C.c_double * max(len(dist), 1))(*dist)
    ctx._check(entry(ctx._h, ptr(src), cols, rows, stride, Kc, dc, len(dist), C.byref(p), C.byref(o)))
    r = np.array(o.ranges[:], np.float32)
    ranges = {name: (r[2 * k], r[2 * k + 1]) for k, name in enumerate(RANGE_NAMES)}
    return PolarimetricFrame(ranges=ranges, **got)


# ---- files ------------------------------------------------------------------------------------------------------------------------------
def write_tiff_f32(path, a) -> None:
    """A float32 picture as a baseline little-endian TIFF: one strip, uncompressed, 32 bits per sample, SampleFormat 3 (IEEE float) --
    the structure of cv::imwrite for a CV_32FC1 picture.  The bits are kept (NaN payloads and -0.0 included)."""
    a = np.ascontiguousarray(a, dtype="<f4")
    if a.ndim != 2 or a.size == 0:
        raise ValueError("a float32 picture is h x w")
    h, w = a.shape
    nbytes = a.size * 4
    tags = [(256, 4, w), (257, 4, h), (258, 3, 32), (259, 3, 1), (262, 3, 1), (273, 4, 8), (277, 3, 1), (278, 4, h), (279, 4, nbytes),
            (339, 3, 3)]
    ifd_at = 8 + nbytes + (nbytes & 1)                  # an IFD begins on a word boundary
    with open(path, "wb") as f:
        f.write(struct.pack("<2sHI", b"II", 42, ifd_at))
        f.write(a.tobytes())
        f.write(b"\0" * (nbytes & 1))
        f.write(struct.pack("<H", len(tags)))
        for tag, typ, value in tags:                    # SHORT values sit left-justified in the value field
            f.write(struct.pack("<HHI", tag, typ, 1) + (struct.pack("<HH", value, 0) if typ == 3 else struct.pack("<I", value)))
        f.write(struct.pack("<I", 0))


def read_tiff_f32(path) -> np.ndarray:
    """The float32 picture of a TIFF as write_tiff_f32 and cv::imwrite write it: either byte order, uncompressed, one sample of 32-bit
    IEEE float per pixel, any number of strips."""
    with open(path, "rb") as f:
        data = f.read()
    if len(data) < 8 or data[:2] not in (b"II", b"MM"):
        raise ValueError(f"{path}: not a TIFF")
    e = "<" if data[:2] == b"II" else ">"
    magic, at = struct.unpack(e + "HI", data[2:8])
    if magic != 42:
        raise ValueError(f"{path}: not a classic TIFF")
    size = {1: 1, 2: 1, 3: 2, 4: 4, 16: 8}
    code = {1: "B", 3: "H", 4: "I", 16: "Q"}
    (count,) = struct.unpack(e + "H", data[at:at + 2])
    tags = {}
    for k in range(count):
        tag, typ, n, raw = struct.unpack(e + "HHI4s", data[at + 2 + 12 * k:at + 14 + 12 * k])
        if typ not in code:
            continue
        nb = size[typ] * n
        if nb > 4:
            (where,) = struct.unpack(e + "I", raw)
            raw = data[where:where + nb]
        tags[tag] = struct.unpack(e + code[typ] * n, raw[:nb])
    one = lambda tag, default=None: tags[tag][0] if tag in tags else default
    w, h = one(256), one(257)
    if w is None or h is None or 273 not in tags:
        raise ValueError(f"{path}: no picture")
    if one(259, 1) != 1 or one(258, 1) != 32 or one(277, 1) != 1 or one(339, 1) != 3:
        raise ValueError(f"{path}: not an uncompressed single-channel 32-bit float picture")
    offsets = tags[273]
    counts = tags.get(279) or (w * h * 4,)
    raw = b"".join(data[o:o + n] for o, n in zip(offsets, counts))
    if len(raw) < w * h * 4:
        raise ValueError(f"{path}: truncated")
    return np.frombuffer(raw[:w * h * 4], dtype=e + "f4").astype("=f4", copy=True).reshape(h, w)


def write_png_u8(path, a) -> None:
    """An 8-bit grey picture as a PNG (one IDAT chunk, filter 0 on every row)."""
    a = np.ascontiguousarray(a, np.uint8)
    if a.ndim != 2 or a.size == 0:
        raise ValueError("a grey picture is h x w")
    h, w = a.shape
    rows = np.concatenate((np.zeros((h, 1), np.uint8), a), axis=1).tobytes()

    def chunk(kind: bytes, body: bytes) -> bytes:
        return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body) & 0xffffffff)

    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 0, 0, 0, 0)) + chunk(b"IDAT", zlib.compress(rows, 6)) +
                chunk(b"IEND", b""))


def _host(a) -> np.ndarray:
    return a.cpu().numpy() if _is_device(a) else np.asarray(a)


def write_polarimetric_outputs(outdir, outfile: str, frame: PolarimetricFrame) -> list:
    """The files of wass_prepare --demosaic under the reference's names: <outfile>.png (the stereo input picture) always,
    <outfile>_S0.tiff, _S1.tiff, _S2.tiff where the frame holds S (--save-stokes), <outfile>_I0.png, _I45.png, _I90.png, _I135.png where
    it holds the channels (--save-channels).  Returns the paths written."""
    os.makedirs(outdir, exist_ok=True)
    written = []

    def put(suffix, writer, a):
        path = os.path.join(outdir, outfile + suffix)
        writer(path, _host(a))
        written.append(path)

    if frame.S is not None:
        for k in range(3):
            put(f"_S{k}.tiff", write_tiff_f32, frame.S[k])
    put(".png", write_png_u8, frame.image)
    if frame.channels is not None:
        for k, name in enumerate(("I0", "I45", "I90", "I135")):
            put(f"_{name}.png", write_png_u8, frame.channels[k])
    return written
