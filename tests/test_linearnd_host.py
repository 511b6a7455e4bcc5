"""The walk of grid_linear.hip compiled for the CPU (tests/native/linearnd_host.hip: the same source, its buckets filled in
reverse index order) against the numpy oracle, bit for bit, with the host's address and undefined-behaviour sanitizers on: every
index into the buckets, the rings and the chords of the circles is checked before the kernel runs them on a GPU.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

import linearnd_oracle as L
from test_linearnd import N, oracle_scene

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def host_walk(tmp_path_factory):
    from wass_amd import build
    build.build()
    out_dir = os.path.join(HERE, "native", "_build")
    os.makedirs(out_dir, exist_ok=True)
    exe, lib = os.path.join(out_dir, "linearnd_host"), os.path.join(ROOT, "wass_amd")
    subprocess.check_call([build.HIPCC, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fno-gpu-rdc",
                           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                           os.path.join(HERE, "native", "linearnd_host.hip"), "-o", exe, "-L" + lib, "-lwassgpu", "-Wl,-rpath," + lib])
    tmp = tmp_path_factory.mktemp("linearnd_host")

    def run(x, y, z, ext, W, H, accel, max_steps=L.DEFAULT_STEPS):
        src, dst = str(tmp / "in.bin"), str(tmp / "out.bin")
        with open(src, "wb") as f:
            np.array([len(x), W, H, accel[0], accel[1], max_steps], np.int64).tofile(f)
            np.array(ext, np.float64).tofile(f)
            for v in (x, y, z):
                np.ascontiguousarray(v, np.float64).tofile(f)
        r = subprocess.run([exe, src, dst], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-4000:]
        raw = open(dst, "rb").read()
        return (np.frombuffer(raw, np.float64, W * H).reshape(H, W), np.frombuffer(raw, np.uint8, W * H, offset=8 * W * H).reshape(H, W))
    return run


def same(got, ref):
    out, flags = got
    assert np.array_equal(flags, ref[1])
    m = flags == 0
    assert np.array_equal(out[m], ref[0][m]) and np.isnan(out[(flags == 1) | (flags == 3)]).all()


@pytest.mark.parametrize("kind", L.SCENES)
def test_host_walk_equals_the_oracle(host_walk, kind):
    x, y, z, *ref = oracle_scene(kind)
    for accel in ((51, 51), (1, 1), (7, 13), (200, 200)):
        same(host_walk(x, y, z, L.UNIT, N, N, accel), ref)


def test_host_walk_duplicates_border_cap(host_walk):
    x, y, z = L.scene("uniform", seed=3, n=300)
    x, y, z = np.r_[x, x[:150]], np.r_[y, y[:150]], np.r_[z, z[:150] + 1.0]
    same(host_walk(x, y, z, L.UNIT, 9, 7, (3, 3)), L.interpolate(x, y, z, *L.UNIT, 9, 7))
    x, y, z = L.scene("uniform", seed=5, n=200)
    x[:40], y[40:80] = np.repeat([0.0, 1.0], 20), np.repeat([0.0, 1.0], 20)
    x[80:82], y[82:84] = [np.nextafter(0.0, -1.0), np.nan], [np.nextafter(1.0, 2.0), np.inf]
    same(host_walk(x, y, z, L.UNIT, 9, 7, (10, 10)), L.interpolate(x, y, z, *L.UNIT, 9, 7))
    x, y, z, *_ = oracle_scene("hole")
    same(host_walk(x, y, z, L.UNIT, N, N, (51, 51), max_steps=2), L.interpolate(x, y, z, *L.UNIT, N, N, max_steps=2))
    xs, ys, zs = L.square_lattice(6)
    ext = (-0.75, 5.75, -0.75, 5.75)
    got = host_walk(xs, ys, zs, ext, 14, 14, (4, 4))
    assert np.array_equal(got[1], L.interpolate(xs, ys, zs, *ext, 14, 14)[1])
