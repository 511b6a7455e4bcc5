"""Drop-in interpolators of the reference's gridding tool (gridding/wassgridsurface), on the GPU.

    from wass_amd.gridding import DCTInterpolator      # instead of: from DCTInterpolator import DCTInterpolator

DCTInterpolator(img_width, img_height, alg_options)(I) returns (Irec float32, ones float32) like the reference's class, with its
option names and defaults (Nfreqs 150, MAX_ITERS 500, TOLERANCE_CHANGE 1e-4, REGULARIZER_ALPHA 8e-7, LEARNING_RATE 5.0).
Differences: the caller's I is not modified (the reference zeroes its NaN cells in place); the start value is a seeded
uniform [0, 1) draw, not torch.rand's stream; a rectangular grid is solved (the reference raises a shape error).
"""
from __future__ import annotations

import numpy as np

from .stereo import Context

_DEFAULTS = {"Nfreqs": 150, "MAX_ITERS": 500, "TOLERANCE_CHANGE": 1e-4, "REGULARIZER_ALPHA": 8e-7, "LEARNING_RATE": 5.0}


class DCTInterpolator:
    def __init__(self, img_width, img_height, alg_options=None, ctx: Context | None = None, seed: int = 0):
        self.width, self.height = int(img_width), int(img_height)
        self.options = {k: ((alg_options or {}).get(k) if (alg_options or {}).get(k) is not None else v) for k, v in _DEFAULTS.items()}
        self.Nfreqs = self.options["Nfreqs"]
        self.MAX_ITERS = self.options["MAX_ITERS"]
        self.TOLERANCE_CHANGE = self.options["TOLERANCE_CHANGE"]
        self.REGULARIZER_ALPHA = self.options["REGULARIZER_ALPHA"]
        self.LEARNING_RATE = self.options["LEARNING_RATE"]
        self._ctx = ctx
        self.seed = seed
        self.last_info = None

    def __call__(self, I, verbose=True):
        I = np.asarray(I)
        if I.shape != (self.height, self.width):
            raise ValueError(f"cell map of shape {I.shape}, the interpolator was made for {(self.height, self.width)}")
        if self._ctx is None:
            self._ctx = Context(0)
        Irec, _, info = self._ctx.grid_dct(I, self.options, seed=self.seed)
        self.last_info = info
        if verbose:
            print("DCT interpolator: %d steps%s, data loss %.6g, |x|_1 %.6g, last max delta %.6g"
                  % (info["steps"], " (tolerance reached)" if info["converged"] else "", info["data_loss"], info["reg_loss"], info["fdelta"]))
        return Irec, np.ones((self.height, self.width), np.float32)
