"""Record the reference's own geometry of wasspost polarimetric_setup for tests/test_polarimetric.py:

    python tests/golden/make_golden_polarimetric.py <reference checkout>

For two small NaN-free seas it evaluates, with the reference's numpy expressions (wasspost.py:680-737), the projection of the
homogeneous cell coordinates by one matrix product, the float32 maps, the camera-frame rays inv(K) @ p2d normalised with
np.linalg.norm, and, by calling the reference's compute_slope_and_normals and compute_occlusion_mask
(postproc/wasspost/geometry.py), the normals, the incident angles and the occlusion mask with the 85 degree rule.
polarimetric.npz holds, per case, the inputs (frame in float32 millimetres, du, the matrices, the picture's size) and those
arrays.  The heights are Z * float32(1e-3), as in make_golden_visibility.py.  cv2 is absent, so the remap has no golden.
numpy >= 2 is needed (np.linalg.vecdot, np.acos)."""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import polarimetric_oracle as PO  # noqa: E402
import radiance_oracle as RO  # noqa: E402
import visibility_oracle as VO  # noqa: E402

IW, IH = 320, 240
CASES = {"a": dict(H=96, W=120, du=0.25, seed=21, amp=1.0, side="west", height=4.0, back=25.0),
         "c": dict(H=64, W=64, du=0.5, seed=23, amp=2.0, side="east", height=8.0, back=50.0)}


def main(ref):
    spec = importlib.util.spec_from_file_location("ref_geometry", os.path.join(ref, "postproc", "wasspost", "geometry.py"))
    geometry = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(geometry)
    out = {"names": np.array(sorted(CASES)), "picture": np.array([IW, IH])}
    for name, c in sorted(CASES.items()):
        XX, YY = VO.make_grid(c["H"], c["W"], c["du"])
        Z = VO.make_sea(c["H"], c["W"], c["du"], c["seed"], c["amp"])
        cam = VO.camera(XX, YY, c["side"], c["height"], c["back"])
        Pplane = RO.pplane(IW, IH, XX, YY, "inside")
        K = PO.intrinsics(IW, IH)
        zf = VO.heights(Z)
        dx = XX[0, 1] - XX[0, 0]
        to_norm = np.array([[2.0 / IW, 0, -1, 0], [0, 2.0 / IH, -1, 0], [0, 0, 1, 0], [0, 0, 0, 1]], dtype=float)
        Pcam = np.linalg.inv(to_norm) @ Pplane
        p3d = np.stack((XX.ravel(), YY.ravel(), zf.ravel().astype(np.float64), np.ones(zf.size)))
        p2d = Pcam @ p3d
        p2d = p2d[:3, :] / p2d[2, :]
        mapx = p2d[0].reshape(zf.shape).astype(np.float32)
        mapy = p2d[1].reshape(zf.shape).astype(np.float32)
        q = np.linalg.inv(K) @ p2d
        ray_z = q / np.linalg.norm(q, axis=0)
        ray_g = p3d - cam[:, -1:]
        ray_g = ray_g[:3]
        ray_g = ray_g / np.linalg.norm(ray_g, axis=0)
        _, nfield = geometry.compute_slope_and_normals(XX, YY, zf)
        ang = np.rad2deg(np.acos(np.linalg.vecdot(nfield.reshape(-1, 3), (-ray_g).T))).reshape(XX.shape)
        field = np.transpose((-ray_g).reshape(3, *XX.shape), (1, 2, 0))
        mask = geometry.compute_occlusion_mask(zf / dx, field)
        march = int(mask.sum())
        mask[ang >= 85] = 1
        print(f"case {name}: {c['H']} x {c['W']}, {march} cells occluded by the march, {int(mask.sum())} with the 85 degree rule, "
              f"angles {ang.min():.2f} .. {ang.max():.2f}, maps x {mapx.min():.1f} .. {mapx.max():.1f}, y {mapy.min():.1f} .. {mapy.max():.1f}")
        out[f"{name}_Z"] = Z
        out[f"{name}_du"] = np.float64(c["du"])
        out[f"{name}_cam"] = cam
        out[f"{name}_Pplane"] = Pplane
        out[f"{name}_K"] = K
        out[f"{name}_mapx"] = mapx
        out[f"{name}_mapy"] = mapy
        out[f"{name}_rays_cam"] = ray_z
        out[f"{name}_normals"] = nfield
        out[f"{name}_angles"] = ang.astype(np.float32)
        out[f"{name}_mask"] = np.packbits(mask)
    np.savez_compressed(os.path.join(HERE, "polarimetric.npz"), **out)


if __name__ == "__main__":
    main(sys.argv[1])
