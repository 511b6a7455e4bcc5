"""Record the reference's own visibility computation for tests/test_visibility.py:

    python tests/golden/make_golden_visibility.py <reference checkout>

For three small NaN-free seas it calls the reference's compute_slope_and_normals and compute_occlusion_mask
(postproc/wasspost/geometry.py) the way wasspost's visibilitymap does (wasspost.py:561-587): rays from the camera through every
cell, normalised with np.linalg.norm; the incident angle from np.linalg.vecdot of the normals and the reversed rays; the mask on
the surface divided by dx.  visibility.npz holds, per case, the frame (float32 millimetres), du, the camera, the packed mask
(before the 88 degree rule) and the float32 angles.  numpy >= 2 is needed (np.linalg.vecdot, np.acos)."""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import visibility_oracle as VO  # noqa: E402

CASES = {"a": dict(H=96, W=120, du=0.25, seed=1, amp=1.0, side="west", height=4.0, back=25.0),
         "b": dict(H=80, W=64, du=0.2, seed=2, amp=1.2, side="north", height=5.0, back=30.0),
         "c": dict(H=64, W=64, du=0.5, seed=3, amp=2.0, side="east", height=8.0, back=50.0)}


def main(ref):
    spec = importlib.util.spec_from_file_location("ref_geometry", os.path.join(ref, "postproc", "wasspost", "geometry.py"))
    geometry = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(geometry)
    out = {"names": np.array(sorted(CASES))}
    for name, c in sorted(CASES.items()):
        XX, YY = VO.make_grid(c["H"], c["W"], c["du"])
        Z = VO.make_sea(c["H"], c["W"], c["du"], c["seed"], c["amp"])
        origin = VO.camera(XX, YY, c["side"], c["height"], c["back"])[:3, 3]
        zf = VO.heights(Z)
        dx = XX[0, 1] - XX[0, 0]
        cells = np.stack((XX.ravel(), YY.ravel(), zf.ravel()))                      # 3 x N, fp64
        ray = cells - origin[:, None]
        ray = ray / np.linalg.norm(ray, axis=0)
        _, normals = geometry.compute_slope_and_normals(XX, YY, zf)
        ang = np.rad2deg(np.acos(np.linalg.vecdot(normals.reshape(-1, 3), (-ray).T))).reshape(XX.shape)
        field = np.transpose((-ray).reshape(3, *XX.shape), (1, 2, 0))
        mask = geometry.compute_occlusion_mask(zf / dx, field, invert_y_axis=False)
        assert (zf / dx).dtype == np.float64 and mask.dtype == np.uint8
        print(f"case {name}: {c['H']} x {c['W']}, {100.0 * mask.mean():.1f} % occluded by the march, "
              f"{100.0 * np.mean((mask > 0) | (ang >= 88)):.1f} % with the 88 degree rule, angles {ang.min():.2f} .. {ang.max():.2f}")
        out[f"{name}_Z"] = Z
        out[f"{name}_du"] = np.float64(c["du"])
        out[f"{name}_origin"] = origin
        out[f"{name}_mask"] = np.packbits(mask)
        out[f"{name}_angles"] = ang.astype(np.float32)
    np.savez_compressed(os.path.join(HERE, "visibility.npz"), **out)


if __name__ == "__main__":
    main(sys.argv[1])
