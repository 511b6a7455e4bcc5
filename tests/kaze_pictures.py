"""The pictures of the KAZE tests.  tests/test_kaze.py holds each of them to its conditions on the oracle alone (keypoints present,
the share of fragile orientations, what each probe is there to catch); tests/test_kaze_gpu.py compares the device with the oracle
on them.  Sizes are width x height; the stencil kernels launch 64 x 4 tiles."""
import functools

import numpy as np

import kaze_oracle as KO

SMALL = (2, 2)          # octaves x sublevels of the small shapes: sigma_size 2, 2, 3, 5
# one tile; exact tiles; ragged in both directions; several tiles; a wide strip of exact rows
SHAPES = [(33, 29), (64, 64), (65, 63), (130, 67), (257, 40)]
DEFAULT_SHAPE = (96, 80)    # 4 x 4 levels: the 22-pixel taps cross every tile edge and reflect off every border
SEA_SHAPE = (300, 200)
INTERIOR_SHAPE = (160, 128)   # blobs away from the border: no orientation sample falls on a border row, where reflect-101 makes Ly exactly 0
# the pictures whose orientations are compared: at most 5 % of their keypoints are fragile (tests/test_kaze.py)
ORIENTED = ["sea", "interior"]


def blobs(w, h, seed, n=None, noise=3.0, margin=0):
    """bright and dark Gaussian blobs of several sizes on a sloped background, with a little noise: uint8.  margin keeps the blobs'
    centres that far from the border"""
    rng = np.random.default_rng(seed)
    n = max(8, (w * h) // 150) if n is None else n
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    img = 110.0 + 20.0 * x / w - 15.0 * y / h
    for _ in range(n):
        cx, cy, s = rng.uniform(margin, w - margin), rng.uniform(margin, h - margin), rng.uniform(1.5, 5.0)
        a = rng.uniform(40, 110) * rng.choice([-1.0, 1.0])
        ex = rng.uniform(0.7, 1.4)
        img += a * np.exp(-(((x - cx) / ex) ** 2 + ((y - cy) * ex) ** 2) / (2 * s * s))
    img += noise * rng.standard_normal((h, w))
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def sea(w=SEA_SHAPE[0], h=SEA_SHAPE[1], frame=6):
    from wass_amd import synth
    return synth.make_pair(w, h, 32, frame_idx=frame)[0]


def single_pixel(w=64, h=64):
    img = np.full((h, w), 20, np.uint8)
    img[h // 2, w // 2 + 1] = 255
    return img


def step_edge(w=130, h=67):
    """a vertical step at the boundary between the first two tiles (x = 64), and a horizontal one at a row boundary (y = 32)"""
    img = np.full((h, w), 40, np.uint8)
    img[:, 64:] = 200
    img[32:, :] = img[32:, :] // 2 + 30
    return img


def constant(w=65, h=63):
    return np.full((h, w), 97, np.uint8)


def border_blob(x0, w=64, h=64, y0=31, sigma=2.0):
    """one blob centred at column x0: with SMALL its extremum is in level 2, whose border rule keeps x >= 10 (3 esigma = 9.6: rint(0.4) = 0,
    rint(-0.6) = -1)"""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    return np.clip(np.rint(30.0 + 200.0 * np.exp(-((x - x0) ** 2 + (y - y0) ** 2) / (2 * sigma * sigma))), 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def small_pictures():
    """name -> (picture, (octaves, sublevels))"""
    out = {f"blobs{w}x{h}": (blobs(w, h, 100 + i), SMALL) for i, (w, h) in enumerate(SHAPES)}
    out["default96x80"] = (blobs(*DEFAULT_SHAPE, 7, n=40), (4, 4))
    out["pixel"] = (single_pixel(), SMALL)
    out["edge"] = (step_edge(), SMALL)
    out["constant"] = (constant(), SMALL)
    out["inside"] = (border_blob(10), SMALL)
    out["outside"] = (border_blob(9), SMALL)
    out["interior"] = (blobs(*INTERIOR_SHAPE, 11, n=150, noise=2.0, margin=34), (4, 4))
    return out


@functools.lru_cache(maxsize=None)
def oracle(name):
    """the oracle's whole run of a named picture, computed once and shared"""
    if name == "sea":
        return KO.detect(sea())
    img, (no, ns) = small_pictures()[name]
    return KO.detect(img, no, ns)


def picture(name):
    return sea() if name == "sea" else small_pictures()[name][0]


def options(name):
    return (4, 4) if name == "sea" else small_pictures()[name][1]


NAMES = list(small_pictures()) + ["sea"]
