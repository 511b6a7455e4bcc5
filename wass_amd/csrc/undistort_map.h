// undistort_map.h -- where cv::undistort reads a destination pixel: the distortion polynomial of initUndistortRectifyMap in fp64 and
// the 1/32-pixel quantisation (round to nearest even), shared by k_undistort (rectify.hip) and k_prepare_pol (prepare_pol.hip).
#pragma once

#include <hip/hip_runtime.h>

namespace wass {

struct Dist12 { double k[12]; };     // k1 k2 p1 p2 k3 k4 k5 k6 s1 s2 s3 s4, zero where the model is shorter

// (x, y): the pixel's normalised coordinates from the per-camera tables; (iu, iv): the source position in 1/32 pixel
__device__ __forceinline__ void undistort_map(double x, double y, const Dist12& D, double fx, double fy, double u0, double v0, int& iu, int& iv)
{
    const double* k = D.k;
    const double x2 = x * x, y2 = y * y;
    const double r2 = x2 + y2, _2xy = 2 * x * y;
    const double kr = (1 + ((k[4] * r2 + k[1]) * r2 + k[0]) * r2) / (1 + ((k[7] * r2 + k[6]) * r2 + k[5]) * r2);
    const double xd = (x * kr + k[2] * _2xy + k[3] * (r2 + 2 * x2) + k[8] * r2 + k[9] * r2 * r2);
    const double yd = (y * kr + k[2] * (r2 + 2 * y2) + k[3] * _2xy + k[10] * r2 + k[11] * r2 * r2);
    const double u = fx * xd + u0, v = fy * yd + v0;
    iu = __double2int_rn(fmax(-2147483648.0, fmin(2147483647.0, u * 32)));
    iv = __double2int_rn(fmax(-2147483648.0, fmin(2147483647.0, v * 32)));
}

}  // namespace wass
