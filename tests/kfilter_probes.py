"""The probes of the dispersion filter: small inputs, exact in binary where a comparison decides, each there to catch ONE way of
getting the filter wrong (kfilter_oracle.VARIANTS).  tests/test_kfilter.py holds every probe against the broken model it is there
to catch (the model's answer must move by at least 5 tolerances); tests/test_kfilter_gpu.py runs the probes on the device.

The shell probes use maps that are exact in binary, which wass_kfilter_set_shell takes as given: omega[p] = p - nt // 2 (so
domega = 1 and G is the width in bins), kappa = minus the bin number, sigma0 = |kappa_x| + |kappa_y| / 2, a 'dispersion relation'
without a square root.  cos(2 pi (mx x / nx + my y / ny - mf t / nt)) travels towards kappa = (mx, my) at omega = mf."""
from dataclasses import dataclass, field

import numpy as np

import dft_oracle as DO
import kfilter_oracle as KO


@dataclass
class Probe:
    name: str
    catches: tuple                  # the variants of kfilter_oracle this probe is there for
    cube: np.ndarray
    H: np.ndarray = None            # an explicit half mask, or
    shell: dict = None              # U, V, G, f_lo, f_hi, complement for exact_maps(shape)
    restore_mean: bool = True
    keep_nan: bool = True
    expect: str = ""                # what the right answer is, in words
    extra: dict = field(default_factory=dict)


def wave(shape, mf, my, mx, amp=1.0, offset=0.0):
    t, y, x = np.indices(shape)
    nt, ny, nx = shape
    # the phase in whole turns times an exact integer modulus: no drift of the argument
    ph = (mx * x * (nt * ny) + my * y * (nt * nx) - mf * t * (ny * nx)) % (nt * ny * nx)
    return (offset + amp * np.cos(2.0 * np.pi * ph / float(nt * ny * nx))).astype(np.float32)


def exact_maps(shape, variant=None):
    nt, ny, nx = shape
    sgn = 1.0 if variant == "kappa_sign" else -1.0
    bx, by = (np.arange(nx) - nx // 2).astype(np.float64), (np.arange(ny) - ny // 2).astype(np.float64)
    KX, KY = np.meshgrid(bx, by)
    return {"omega": (np.arange(nt) - nt // 2).astype(np.float64), "kappa_x": sgn * bx, "kappa_y": sgn * by,
            "sigma0": np.abs(KX) + 0.5 * np.abs(KY), "used": ((KX != 0) | (KY != 0)).astype(np.uint8)}


def shell_args(probe, variant=None):
    """(omega, kappa_x, kappa_y, sigma0, used, U, V, G, f_lo, f_hi, complement) as set_shell takes them"""
    m = exact_maps(probe.cube.shape, variant)
    s = probe.shell
    return (m["omega"], m["kappa_x"], m["kappa_y"], m["sigma0"], m["used"], s.get("U", 0.0), s.get("V", 0.0), s["G"], s.get("f_lo", -np.inf),
            s.get("f_hi", np.inf), s.get("complement", False))


def mask_of(probe, variant=None):
    if probe.H is not None:
        return probe.H
    return KO.half(KO.shell_mask(*shell_args(probe, variant), variant=variant))


def model(probe, variant=None):
    """{'out', 'tol', ...}: the fp64 oracle's answer to the probe, broken as `variant` says, and the tolerance of the right answer"""
    H = mask_of(probe, variant)
    r = KO.filter_cube(probe.cube, H, probe.restore_mean, probe.keep_nan, variant=variant)
    r["H"] = H
    r["tol"] = KO.out_tolerance(r["out"], KO.bound(r["p"], mask_of(probe)), probe.restore_mean)
    return r


def miss(got, ref_out, tol):
    """max |got - ref| / (5 tol) over the cube; infinite where one is NaN and the other is not, or where tol is 0 and they differ"""
    a, b = np.asarray(got, np.float64), np.asarray(ref_out, np.float64)
    if (np.isnan(a) != np.isnan(b)).any():
        return np.inf
    d = np.abs(np.nan_to_num(a) - np.nan_to_num(b))
    return DO.ratio(d, 5.0 * np.broadcast_to(tol, d.shape))


def _ints(shape):
    return DO.probe_cube(*shape)


def probes():
    out = []
    # a wave on the shell: energy at (+mf, kappa) and at its mirror image; without the mirror rule the half at -mf is dropped
    s = (8, 6, 10)
    out.append(Probe("shell_wave", ("no_mirror",), wave(s, 3, 2, 2, offset=7.0), shell={"G": 0.5}, expect="the wave passes whole"))
    # with a current (1/2, 1/2) the wave towards (2, 2) sits at omega = 3 + 2: kappa with the sign of k looks for it at 3 - 2
    s = (12, 6, 10)
    out.append(Probe("current_wave", ("kappa_sign",), wave(s, 5, 2, 2), shell={"U": 0.5, "V": 0.5, "G": 1.0}, expect="the wave passes whole"))
    # the bin of the wave lies at |r| == G exactly
    out.append(Probe("gate_edge", ("gate_lt",), wave(s, 4, 2, 2), shell={"G": 1.0}, expect="the wave passes whole: |r| = G is inside"))
    # all ones: the identity, which every weight rule but the right one breaks.  Even nx: the Nyquist column stands alone
    s = (3, 4, 6)
    ones = lambda sh: np.ones((sh[0], sh[1], sh[2] // 2 + 1), np.float32)
    out.append(Probe("identity_even", ("w_none", "w_all", "nyquist_doubled", "no_inv"), _ints(s) + np.float32(3), H=ones(s), expect="out = input"))
    s = (4, 3, 5)
    out.append(Probe("identity_odd", ("w_none", "w_all", "no_inv"), _ints(s) - np.float32(2), H=ones(s), expect="out = input"))
    # nothing passes: the mean alone comes back
    out.append(Probe("mean_only", ("no_mean",), _ints(s) + np.float32(40), H=0 * ones(s), expect="out = (float) m_c"))
    c = _ints((5, 4, 6)) + np.float32(1)
    c[1, 2, 3] = c[4, 0, 0] = np.nan
    c[:, 3, 5] = np.nan
    out.append(Probe("nan_back", ("no_nan",), c, H=ones(c.shape), expect="NaN where the input has NaN"))
    # the last k tile of the closing stage: ch = 19, the wave sits in column kx = 18
    s = (2, 3, 37)
    out.append(Probe("last_k_tile", ("close_drop_k",), wave(s, 0, 1, 18) + wave(s, 1, 0, 17), H=ones(s), expect="out = input"))
    return out
