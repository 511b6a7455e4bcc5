"""Hand-built series for the wave-by-wave statistics: name -> (cube [count, 1, W] float32, keyword arguments of wave_statistics).
Every cube holds the series and its negative side by side, so that two neighbouring lanes close their waves at different times.
tests/test_wavestats.py shows on the CPU which mistake each probe catches; tests/test_wavestats_gpu.py runs them on the GPU."""
import numpy as np

DT = 0.5


def waves(crests, troughs, fills, first=-1.0, last=1.0):
    """first (< 0), then per wave: its crest, `fill` samples of half the crest, its trough (as a positive depth), then last (> 0).
    The up-crossings lie before every crest and before `last`: len(crests) waves of 2 + fill samples, heights crest + trough."""
    s = [first]
    for a, b, n in zip(crests, troughs, fills):
        s += [a] + [a / 2.0] * n + [-b]
    return s + [last]


def _cube(series):
    s = np.asarray(series, np.float32)
    assert np.array_equal(s.astype(np.float64), np.asarray(series, np.float64)), "the probe's values must be float32 numbers"
    return np.ascontiguousarray(np.stack([s, -s], axis=1)[:, None, :])


def random_cube(count, H, W, seed, noise=0.3):
    """a few sinusoids per cell with the phase running over the grid, and white noise on top: waves of many heights"""
    rng = np.random.default_rng(seed)
    t = np.arange(count)[:, None, None]
    y, x = np.arange(H)[None, :, None], np.arange(W)[None, None, :]
    z = np.zeros((count, H, W))
    for f, a in ((0.031, 1.0), (0.047, 0.6), (0.11, 0.25)):
        z += a * np.sin(2 * np.pi * f * t + 0.37 * x + 0.91 * y + rng.uniform(0, 2 * np.pi))
    return (z + noise * rng.standard_normal((count, H, W)) + 0.125).astype(np.float32)


def probes():
    raw = dict(dt=DT, demean=False)
    p = {}
    # no crossing, one crossing
    p["all_positive"] = (_cube([1, 2, 3, 2, 1]), raw)
    p["one_step"] = (_cube([-1, 1]), raw)
    p["one_crossing"] = (_cube([-2, -1, 3, 1, 2]), raw)
    # Nw = 1, 2, 3, 4, 7 (n13 = 1, 1, 1, 2, 3): distinct heights, crests rising so that a span one sample too long shows
    for nw in (1, 2, 3, 4, 7):
        crests = [1.0 + 0.5 * k for k in range(nw)]
        troughs = [2.0, 0.25, 3.0, 0.5, 1.0, 4.0, 0.75][:nw]
        fills = [(3 * k) % 4 for k in range(nw)]
        p[f"nw{nw}"] = (_cube(waves(crests, troughs, fills, last=8.0)), raw)
        p[f"nw{nw}_demean"] = (_cube(waves(crests, troughs, fills, last=8.0)), dict(dt=DT))
    # the most waves a series can hold: count // 2 crossings
    for count in (8, 9, 16, 17):
        p[f"alternating{count}"] = (_cube([(-1.0) ** (k + 1) for k in range(count)]), raw)
        p[f"alternating{count}_demean"] = (_cube([(-1.0) ** (k + 1) for k in range(count)]), dict(dt=DT))
    # exact zeros: < 0 and >= 0 decide
    p["zero_touch"] = (_cube([-1, 0, -1]), raw)
    p["zeros"] = (_cube([0, 0, 0]), raw)
    p["zero_ramp"] = (_cube([-1, 0, 1]), raw)
    p["zeros_waves"] = (_cube([-1, 0, 1, -1, 0, 1, -2, 3, -1, 0, 0, -3, 0]), raw)
    # four waves, n13 = 2: heights 3, 5, 3, 3 with periods 2, 3, 4, 5 samples: the third is waves 1 and 0, not 1 and 3
    p["tie_cut"] = (_cube(waves([2, 4, 1, 1.5], [1, 1, 2, 1.5], [0, 1, 2, 3])), raw)
    # the highest wave twice, periods 3 and 5 samples: t_hmax is the first one's
    p["hmax_twice"] = (_cube(waves([1, 4, 2, 3], [1, 1, 1, 2], [0, 1, 2, 3])), raw)
    # seven waves, the third = heights 1, 1, 2^53 in time order: (1 + 1) + 2^53 is not (2^53 + 1) + 1
    big = 2.0 ** 52
    p["sum_order"] = (_cube(waves([0.25, 0.5, 0.25, 0.5, 0.25, 0.25, big], [0.25, 0.5, 0.25, 0.5, 0.25, 0.25, big], [0, 1, 0, 2, 1, 0, 1])), raw)
    # 2^60 + 100 is 2^60 in fp64, 2^60 + 200 is not: a sum by halves gives another mean
    p["big_small"] = (_cube([2.0 ** 60, 100, 100, 100, -2.0 ** 60, 100, 100, 100]), dict(dt=DT))
    # constant, subnormal and 1e30-sized
    p["constant"] = (_cube([0.75] * 9), dict(dt=DT))
    p["constant_raw"] = (_cube([-0.75] * 9), raw)
    shape = np.asarray(waves([4, 6, 2], [1, 4, 2], [1, 0, 2], first=-2.0, last=7.0), np.float32)
    for name, unit in (("subnormal", np.float32(1e-45)), ("huge", np.float32(1e30))):
        p[name] = (_cube((unit * shape).astype(np.float64)), raw)
        p[name + "_demean"] = (p[name][0], dict(dt=DT))
    # many equal heights at and around the cut: samples on a grid of 1 / 4
    q = np.round(random_cube(257, 1, 65, seed=5, noise=0.5) * 4.0) / 4.0
    p["quantised"] = (q.astype(np.float32), raw)
    # unstructured values, where a fused multiply-add or another order of operations shows in the last bit
    p["random"] = (random_cube(64, 1, 33, seed=6), dict(dt=0.3, datascale=1e-3))
    # crossings at samples 0, 2 and 4: tau keeps every bit of eta[i] / (eta[i] - eta[i+1]) while i is small
    mag = np.random.default_rng(12).uniform(0.1, 1.0, (6, 1, 64))
    p["early_crossings"] = ((mag * np.array([-1, 1, -1, 1, -1, 1]).reshape(6, 1, 1)).astype(np.float32), dict(dt=0.3, demean=False))
    return p
