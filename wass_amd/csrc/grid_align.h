// grid_align.h -- the alignment of a camera-space point on the sequence's mean sea plane, stated once for every gridder
// (grid.hip bins the result by cell, grid_linear.hip interpolates it): mesh_aligned = (Rpl @ p + Tpl, z negated) * CAM_BASELINE
// (wassgridsurface.py:318, wass_utils.py:54-61), in this order of operations.
#pragma once
#include "common.h"

namespace wass {

struct GridDev {
    double R[9], T[3], baseline, xmin, ymin, xext, yext, wm1, hm1;      // xext = xmax - xmin, wm1 = W - 1
    int gw, gh;
};

__device__ __forceinline__ void grid_align(const GridDev& g, double x, double y, double z, double& ax, double& ay, double& az)
{
    ax = (g.R[0] * x + g.R[1] * y + g.R[2] * z + g.T[0]) * g.baseline;
    ay = (g.R[3] * x + g.R[4] * y + g.R[5] * z + g.T[1]) * g.baseline;
    az = -(g.R[6] * x + g.R[7] * y + g.R[8] * z + g.T[2]) * g.baseline;
}

// grid.hip: the one-workgroup exclusive scan of per-cell counts (cnt[0 .. ng) -> off[0 .. ng)), enqueued on s
void grid_scan_enqueue(const unsigned int* cnt, size_t ng, unsigned int* off, hipStream_t s);

}  // namespace wass
