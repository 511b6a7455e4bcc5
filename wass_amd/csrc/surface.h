// surface.h -- what visibility.hip and polarimetric.hip both need of a gridded surface: the slope of a float32 frame as numpy's
// gradient gives it, and the unit normal compute_slope_and_normals (geometry.py) builds from it.  One definition, so that the
// two files compute the same bits.
#pragma once
#include <hip/hip_runtime.h>

namespace wass {

// np.gradient of a float32 line with spacing d: the difference in float32, the quotient rounded to float32
__device__ __forceinline__ double vis_slope(float lo, float here, float hi, bool first, bool last, double d)
{
    if (first) return (double)(float)((double)(hi - here) / d);
    if (last) return (double)(float)((double)(here - lo) / d);
    return (double)(float)((double)(hi - lo) / (2.0 * d));
}

// the frame's cell (i, j) and its four neighbours in metres (p points at the cell, rows sy elements apart), then
// zf = p[0] * scale and n = (-sx, -sy, 1) / sqrt((sx^2 + sy^2) + 1) in fp64
__device__ __forceinline__ float surface_normal(const float* __restrict__ p, long long sy, int i, int j, int H, int W, float scale, double dx,
                                                double dy, double& n0, double& n1, double& n2)
{
    const float zf = p[0] * scale;
    const float zl = j > 0 ? p[-1] * scale : zf, zr = j < W - 1 ? p[1] * scale : zf;
    const float zu = i > 0 ? p[-sy] * scale : zf, zd = i < H - 1 ? p[sy] * scale : zf;
    const double sx = vis_slope(zl, zf, zr, j == 0, j == W - 1, dx);
    const double sy_ = vis_slope(zu, zf, zd, i == 0, i == H - 1, dy);
    const double nn = sqrt((sx * sx + sy_ * sy_) + 1.0);
    n0 = -(sx / nn);
    n1 = -(sy_ / nn);
    n2 = 1.0 / nn;
    return zf;
}

}  // namespace wass
