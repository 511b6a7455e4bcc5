"""Scenes for the batched variational refinement (tests/test_vref_batch_gpu.py): several DISTINCT frames on one rig, made from the
pieces of tests/vref_oracle.py.  The rig is vref_oracle.probe's; camera 0 and camera 1 may have pictures of different sizes (each
camera's matrix comes from the probe of its own picture size; the pose depends on the seed only).  A frame has its own two
pictures, its own mask and its own coarse start field."""
import numpy as np

import vref_oracle as V
from wass_amd import refinement

MASKS = ("ones", "checkerboard", "zeros")


class Frames:
    """gridsetup: what SequenceRefiner / refine_sequence take; single(f): the constructor arguments of VariationalRefinement for
    frame f (the same fp64 Rp2c, Tp2c the sequence layer derives from gridsetup); scene(f): the oracle's Scene of frame f."""

    def __init__(self, ny, nx, n, seed, pics=((5, 7), (64, 48)), masks=MASKS, baseline=2.0):
        _, a0 = V.probe(ny, nx, *pics[0], seed=seed)
        _, a1 = V.probe(ny, nx, *pics[1], seed=seed)
        assert np.array_equal(a0["Rp2c"], a1["Rp2c"]) and np.array_equal(a0["Tp2c"], a1["Tp2c"])
        R, T = a0["Rp2c"], a0["Tp2c"]
        self.shape, self.coarse, self.n, self.pics = (ny, nx), (ny // 2, nx // 2), n, pics
        self.gridsetup = {"Rpl": R.T, "Tpl": (-R.T @ T).reshape(3, 1), "P0cam": a0["P0cam"], "P1cam": a1["P1cam"], "XX": a0["XX"], "YY": a0["YY"],
                          "CAM_BASELINE": np.array([[baseline]])}
        self.baseline, self.Rp2c, self.Tp2c = refinement._plane_to_camera(self.gridsetup)
        self.I0 = np.stack([V.texture(*pics[0], 100 * seed + f).astype(np.float32) for f in range(n)])
        self.I1 = np.stack([V.texture(*pics[1], 100 * seed + 50 + f).astype(np.float32) for f in range(n)])
        self.mask = np.stack([V.mask_of(masks[f % len(masks)], ny, nx).astype(np.float32) for f in range(n)])
        self.Zc0 = np.stack([V.surface(ny // 2, nx // 2, seed + f, amp=0.05).astype(np.float32) for f in range(n)])
        assert len({a.tobytes() for a in self.I0}) == n and len({a.tobytes() for a in self.I1}) == n and len({a.tobytes() for a in self.Zc0}) == n

    def single(self, f):
        return dict(I0=self.I0[f], I1=self.I1[f], Rp2c=self.Rp2c, Tp2c=self.Tp2c, P0cam=self.gridsetup["P0cam"], P1cam=self.gridsetup["P1cam"],
                    XX=self.gridsetup["XX"], YY=self.gridsetup["YY"], baseline=self.baseline, mask=self.mask[f])

    def scene(self, f):
        return V.scene(**self.single(f))

    def surfaces(self, seed=0):
        """gridded surfaces in metres, z up, per frame, NaN outside an ellipse (its own per frame), and the masks that go with them"""
        ny, nx = self.shape
        yy, xx = np.mgrid[0:ny, 0:nx]
        Zi, mask = [], []
        for f in range(self.n):
            inside = ((xx - (nx - 1) / 2.0 - 0.3 * f) ** 2 / (0.45 * nx) ** 2 + (yy - (ny - 1) / 2.0) ** 2 / (0.4 * ny + 0.2 * f) ** 2) < 1
            z = (V.surface(ny, nx, seed + 31 * f, amp=0.1) * self.baseline).astype(np.float32)
            z[~inside] = np.nan
            Zi.append(z); mask.append(inside.astype(np.float32))
        return np.stack(Zi), np.stack(mask)


def scratch_bytes(nb, ny, nx, ih0, iw0, ih1, iw1):
    """wass_vref_batch_scratch_bytes from the layout, every part rounded up to 256 bytes.
    shared: XX / b, YY / b (a plane each), the flag (256), the tables: lo, hi, t per fine index (12 bytes) and r0, r1, s, s1, f per
            coarse index (20 bytes), both axes
    frame:  mask, zin, Zdx, Zdy, gd, gZ (six planes), the two pictures, Zc, m, v (three coarse planes), two doubles per 64 x 16 tile"""
    up = lambda b: (b + 255) // 256 * 256                                    # noqa: E731
    hc, wc = ny // 2, nx // 2
    shared = 2 * up(ny * nx * 4) + 256 + up((ny + nx) * 12 + (hc + wc) * 20)
    tiles = ((nx + 63) // 64) * ((ny + 15) // 16)
    frame = 6 * up(ny * nx * 4) + up(ih0 * iw0 * 4) + up(ih1 * iw1 * 4) + 3 * up(hc * wc * 4) + up(tiles * 16)
    return shared + nb * frame, shared, frame
