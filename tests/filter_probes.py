"""Inputs for the temporal filter's edge tests (tests/test_filter_edges.py, tests/test_filter_edges_gpu.py): cubes count x H x W
float32 on which a subtly wrong sosfiltfilt shows in the float32 result.  Closed form or seeded; test infrastructure only.

On ordinary data (outputs of 1e2 to 1e3, fp64 noise of 1e-13 to 1e-11) neither a re-associated state update nor a contracted
b0 x + z0 moves a float32 output.  They show where the output IS the fp64 noise (a constant through a high-pass), where the
dynamic range is wide, and, for the padding, wherever 2 x[0] - x[k] is not a float32 number."""
import numpy as np

import filter_oracle as FO

FS = 12.0
H, W = 3, 70                                     # 210 series: a full wave of 64 lanes, full and ragged, and no whole block of 256
# order -> number of sections of k_sos_forward<NS> / k_sos_backward<NS, DEMEAN>: both parities of every NS
ORDERS = (1, 2, 3, 5, 6, 8, 9, 10, 11, 12)
BANDS = {"lp1.0": ("lowpass", 1.0), "hp0.05": ("highpass", 0.05)}


def levels(count, H, W):
    """every cell constant in time at its own level: through a high-pass the output is the recurrence's fp64 noise"""
    cell = np.arange(H * W, dtype=np.float64).reshape(1, H, W)
    return np.broadcast_to((1000.0 + 0.37 * cell).astype(np.float32), (count, H, W)).copy()


def levels_plus_ripple(count, H, W, seed=1):
    """the levels plus a thousandth of series_cube: the float32 padding is no longer exact, the output still small"""
    return (levels(count, H, W).astype(np.float64) + 1e-3 * FO.series_cube(count, H, W, seed=seed).astype(np.float64)).astype(np.float32)


def wide(count, H, W, seed=1):
    """values from 1e-3 to 1e7 with both signs (radiance_oracle.wide_series): the order of the fp64 updates shows"""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((count, H, W)) * 10.0 ** rng.uniform(-3, 7, (count, H, W))).astype(np.float32)


def subnormal(count, H, W, seed=1):
    """float32 values between 1e-45 and 1e-38 with both signs: the float32 padding 2 x0 - x[k] and the output cast land on
    subnormals (a flushing float32 mode would return zeros)"""
    rng = np.random.default_rng(seed)
    v = rng.choice([-1.0, 1.0], (count, H, W)) * 10.0 ** rng.uniform(-45, -38, (count, H, W))
    x = v.astype(np.float32)
    assert (np.abs(x) < np.finfo(np.float32).tiny).all() and (x != 0).mean() > 0.8
    return x


def infinite(count, H, W, seed=1):
    """series_cube with one +inf in one series and one -inf in another (inside, so that the padding and the recurrence both meet
    them); the oracle decides what comes out"""
    x = FO.series_cube(count, H, W, seed=seed)
    x[count // 2, 0, 1 % W] = np.inf
    x[1, H - 1, W - 1] = -np.inf
    return x


PROBES = {"series": lambda c, h, w, seed: FO.series_cube(c, h, w, seed=seed, offset=40.0),
          "levels": lambda c, h, w, seed: levels(c, h, w),
          "levels_plus_ripple": levels_plus_ripple, "wide": wide, "subnormal": subnormal, "infinite": infinite}


# wide is the probe that tells a re-associated update at the ODD orders, where the first section is of first order: its z1 is 0, so
# there the two associations are the same sum, and a constant never reaches the sections behind it.  What is left are float32
# roundings that fall on the other side of a tie, about one element in 1e5: 2400 series, and a seed per order chosen on the CPU so
# that at least one does (tests/test_filter_edges.py asserts it).  At order 1 there is no second section and nothing to tell.
WIDE_HW = (8, 300)
WIDE_SEEDS = {3: 3, 5: 3, 7: 1, 9: 3, 11: 3}


def probe_count(padlen):
    """padlen + 1 frames are the fewest scipy takes; 8 more put one whole block of FILT_U = 8 steps into the middle run"""
    return padlen + 1 + 8


def probe(name, order, H=H, W=W):
    """the probe `name` for a filter of `order`: probe_count(default padlen) frames, seeded by the order"""
    ns = (order + 1) // 2
    pad = 3 * (2 * ns + 1 - order % 2)
    if name == "wide":
        return wide(probe_count(pad), *WIDE_HW, WIDE_SEEDS.get(order, 3))
    return PROBES[name](probe_count(pad), H, W, 100 + order)


def rounded(o64):
    """what the kernel must return: the fp64 oracle rounded to float32 (overflow to inf is the cast's own)"""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(o64).astype(np.float32)
