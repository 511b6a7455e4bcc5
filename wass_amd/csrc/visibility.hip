// visibility.hip -- wasspost's `visibilitymap` (postproc/wasspost/wasspost.py:495-621, geometry.py:5-100) as an array function:
// for every frame of a count x H x W float32 cube and every cell, is the cell hidden from the camera by the surface itself, and
// under which incident angle does the camera see it.
//
// Per frame (zf = the float32 heights in metres, Z * (float)datascale):
//   k_vis_prepass   one lane per cell: the surface in cell units Zc = (double)zf / dx as an fp64 plane (so that the march does not
//                   divide), the frame's largest finite Zc, the normal from numpy's gradient of a FLOAT32 array (the difference
//                   and the slope are rounded to float32, as np.gradient does for a float32 input), the unit ray towards the
//                   camera, the incident angle, the angle-limit rule as the mask's first value, and the count of finite cells
//                   that are not below the camera
//   k_vis_march     one lane per cell, a wave = 64 consecutive cells of a row, frames in blockIdx.z: the ray is recomputed with
//                   the very same operations and marched one cell of its dominant axis per step
// All of it fp64 in numpy's own order of operations; the library is built with -ffp-contract=off and without fast-math, so the
// ray, the step and the accumulated position p = p + step are numpy's bits and the mask is exact, not close.  The march reads
// heights with plain global loads (a 1024 x 1024 plane is 8 MiB), VIS_U steps' loads issued before the first comparison: the
// addresses do not depend on the heights, only the end of the ray does.  A ray is dropped, not occluded, when it leaves the
// grid or rises above the frame's maximum (p2 only grows); NaN fails every comparison, so a NaN cell never occludes and its
// own ray is dropped at once.  The loop is bounded by max(H, W) steps whatever the input.
// The only atomics are integer ones (a maximum of order-preserving keys, reduce.h's, and counts): the same input gives the same bits.
// Host side: vis_plan keeps the byte formula; the batch rule, the scratch, the staging of a host batch and the end of a call are
// cube.h's.
#include "common.h"
#include "cube.h"
#include "surface.h"     // vis_slope: shared with polarimetric.hip

namespace wass {

constexpr size_t VIS_SCRATCH_CAP = (size_t)16 << 30;    // bytes one call may allocate
constexpr int VIS_MAX_BATCH = 1024;                     // frames per launch (blockIdx.z)
constexpr int VIS_DEFAULT_BATCH = 8;
constexpr int VIS_U = 4;                                // steps whose heights are loaded ahead of the comparisons
constexpr int VIS_BX = 64, VIS_BY = 4;                  // a block: 4 waves, each 64 cells of one row

// the frame's largest height from its key (reduce.h's order_key); key 0, nothing seen, stands for minus infinity
__device__ __forceinline__ double vis_top(unsigned long long k) { return k ? order_unkey(k) : -INFINITY; }

// d = -(r / |r|), r = cell - camera: the unit direction from the cell to the camera, numpy's operations in numpy's order
__device__ __forceinline__ void vis_ray(double x, double y, double z, double o0, double o1, double o2, double& d0, double& d1, double& d2)
{
    const double r0 = x - o0, r1 = y - o1, r2 = z - o2;
    const double n = sqrt((r0 * r0 + r1 * r1) + r2 * r2);
    d0 = -(r0 / n);
    d1 = -(r1 / n);
    d2 = -(r2 / n);
}

// compute_occlusion_mask's loop for one ray: from (j, i, z0) in steps of (s0, s1, s2) over the H x W surface Zc (cell units).
// true = some cell under the ray is at least as high as the ray.  At most nmax steps.
__device__ __forceinline__ bool vis_march(const double* __restrict__ Zc, int H, int W, int i, int j, double z0, double s0, double s1, double s2,
                                          double maxz, int nmax)
{
    const double dH = (double)H, dW = (double)W;
    double p0 = (double)j, p1 = (double)i, p2 = z0;
    for (int k = 0; k < nmax; k += VIS_U) {
        double at[VIS_U], z[VIS_U];
        bool in[VIS_U];
#pragma unroll
        for (int u = 0; u < VIS_U; ++u) {
            p0 += s0;                                   // the accumulated sum, not k * step
            p1 += s1;
            p2 += s2;
            const double rj = rint(p0), ri = rint(p1);  // half to even; -0 passes as 0; NaN fails
            in[u] = k + u < nmax && ri >= 0.0 && ri < dH && rj >= 0.0 && rj < dW && p2 <= maxz;
            at[u] = p2;
            z[u] = in[u] ? Zc[(size_t)(int)ri * (size_t)W + (size_t)(int)rj] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < VIS_U; ++u) {
            if (!in[u]) return false;
            if (z[u] >= at[u]) return true;
        }
    }
    return false;
}

struct VisGeom {
    const double* XX;              // H x W
    const double* YY;
    double o0, o1, o2;             // the camera in grid coordinates
    double dx, dy;
    double limit;                  // cells with an angle >= limit are occluded too ...
    int use_limit;                 // ... if this is set
    float scale;                   // (float)datascale
};

__global__ void __launch_bounds__(VIS_BX * VIS_BY) k_vis_prepass(const float* __restrict__ Z, long long st, long long sy, int H, int W, const VisGeom g,
                                                                 double* __restrict__ Zc, unsigned char* __restrict__ mask,
                                                                 float* __restrict__ ang, unsigned long long* __restrict__ keys,
                                                                 unsigned long long* __restrict__ notup)
{
    const int j = blockIdx.x * VIS_BX + threadIdx.x, i = blockIdx.y * VIS_BY + threadIdx.y;
    const size_t f = blockIdx.z, HW = (size_t)H * W;
    unsigned long long key = 0;
    bool up = false;
    if (i < H && j < W) {
        const float* __restrict__ p = Z + (long long)f * st + (long long)i * sy + j;
        const float s = g.scale;
        const float zf = p[0] * s;
        const float zl = j > 0 ? p[-1] * s : zf, zr = j < W - 1 ? p[1] * s : zf;
        const float zu = i > 0 ? p[-sy] * s : zf, zd = i < H - 1 ? p[sy] * s : zf;
        const size_t c = (size_t)i * W + j;
        const double zc = (double)zf / g.dx;
        Zc[f * HW + c] = zc;
        if (fabs(zc) <= 1.7976931348623157e308) key = order_key(zc);      // finite
        const double sx = vis_slope(zl, zf, zr, j == 0, j == W - 1, g.dx);
        const double sy_ = vis_slope(zu, zf, zd, i == 0, i == H - 1, g.dy);
        const double nn = sqrt((sx * sx + sy_ * sy_) + 1.0);
        const double n0 = -(sx / nn), n1 = -(sy_ / nn), n2 = 1.0 / nn;
        double d0, d1, d2;
        vis_ray(g.XX[c], g.YY[c], (double)zf, g.o0, g.o1, g.o2, d0, d1, d2);
        const double a = acos((n0 * d0 + n1 * d1) + n2 * d2) * (180.0 / 3.14159265358979323846);
        ang[f * HW + c] = (float)a;
        up = d2 <= 0.0;                                                  // false for a NaN cell
        mask[f * HW + c] = (g.use_limit && a >= g.limit && !up) ? 1 : 0;
    }
    const unsigned long long wave_up = __ballot(up);
    if (wave_up && threadIdx.x == 0) atomicAdd(notup, (unsigned long long)__popcll(wave_up));
    block_max<VIS_BY>(key, keys + f);
}

__global__ void __launch_bounds__(VIS_BX * VIS_BY) k_vis_march(const float* __restrict__ Z, long long st, long long sy, int H, int W, const VisGeom g,
                                                               const double* __restrict__ Zc, const unsigned long long* __restrict__ keys,
                                                               int nmax, unsigned char* __restrict__ mask, unsigned* __restrict__ counts)
{
    const int j = blockIdx.x * VIS_BX + threadIdx.x, i = blockIdx.y * VIS_BY + threadIdx.y;
    const size_t f = blockIdx.z, HW = (size_t)H * W;
    bool occluded = false;
    if (i < H && j < W) {
        const size_t c = (size_t)i * W + j;
        const double* __restrict__ plane = Zc + f * HW;
        occluded = mask[f * HW + c] != 0;
        const float zf = Z[(long long)f * st + (long long)i * sy + j] * g.scale;
        if (!occluded && zf == zf) {
            double d0, d1, d2;
            vis_ray(g.XX[c], g.YY[c], (double)zf, g.o0, g.o1, g.o2, d0, d1, d2);
            if (d2 > 0.0) {
                const double a0 = fabs(d0), a1 = fabs(d1);
                const double m = a0 > a1 ? a0 : a1;     // 0 under the camera: the step is not a number and the ray is dropped
                occluded = vis_march(plane, H, W, i, j, plane[c], d0 / m, d1 / m, d2 / m, vis_top(keys[f]), nmax);
                if (occluded) mask[f * HW + c] = 1;
            }
        }
    }
    const unsigned long long wave = __ballot(occluded);
    if (wave && threadIdx.x == 0) atomicAdd(counts + f, (unsigned)__popcll(wave));
}

// ---- compute_occlusion_mask with an explicit ray field: one H x W fp64 surface in cell units, H x W x 3 fp64 rays ---------------
__global__ void __launch_bounds__(VIS_BX * VIS_BY) k_occ_prepass(const double* __restrict__ ZZ, const double* __restrict__ rays, int H, int W,
                                                                 unsigned long long* __restrict__ key, unsigned long long* __restrict__ notup)
{
    const int j = blockIdx.x * VIS_BX + threadIdx.x, i = blockIdx.y * VIS_BY + threadIdx.y;
    unsigned long long k = 0;
    bool bad = false;
    if (i < H && j < W) {
        const size_t c = (size_t)i * W + j;
        const double z = ZZ[c];
        if (fabs(z) <= 1.7976931348623157e308) k = order_key(z);
        bad = !(rays[3 * c + 2] > 0.0);                 // "rays must go upward"
    }
    const unsigned long long wave_bad = __ballot(bad);
    if (wave_bad && threadIdx.x == 0) atomicAdd(notup, (unsigned long long)__popcll(wave_bad));
    block_max<VIS_BY>(k, key);
}

__global__ void __launch_bounds__(VIS_BX * VIS_BY) k_occ_march(const double* __restrict__ ZZ, const double* __restrict__ rays, int H, int W,
                                                               int invert_y, const unsigned long long* __restrict__ key, int nmax,
                                                               unsigned char* __restrict__ mask)
{
    const int j = blockIdx.x * VIS_BX + threadIdx.x, i = blockIdx.y * VIS_BY + threadIdx.y;
    if (i >= H || j >= W) return;
    const size_t c = (size_t)i * W + j;
    const double r0 = rays[3 * c], r1 = rays[3 * c + 1], r2 = rays[3 * c + 2];
    bool occluded = false;
    if (r2 > 0.0) {
        const double a0 = fabs(r0), a1 = fabs(r1);
        const double m = a0 > a1 ? a0 : a1;
        const double s1 = r1 / m;
        occluded = vis_march(ZZ, H, W, i, j, ZZ[c], r0 / m, invert_y ? -s1 : s1, r2 / m, vis_top(*key), nmax);
    }
    mask[c] = occluded ? 1 : 0;
}

struct VisPlan {
    int batch = 0;                 // frames per launch
    size_t head_bytes = 0, grid_bytes = 0, zc_bytes = 0, stage_bytes = 0, mask_bytes = 0, ang_bytes = 0, total = 0;
};

// 0, or why the problem cannot be planned.  Scratch: keys (8 B), counts (4 B) per frame of the cube and the not-upward count; the
// fp64 plane per frame of a batch; for a host cube also XX and YY and, per frame of a batch, the staged frame, its mask and angles.
static int vis_plan(int count, int H, int W, int batch, bool host, VisPlan& p)
{
    if (count < 1 || H < 2 || W < 2 || batch < 0 || H > 65536 || W > 65536) return WASS_ERR_INVALID_ARG;
    const size_t HW = (size_t)H * W;
    if (HW > 0x7fffff00u) return WASS_ERR_UNSUPPORTED;
    p.head_bytes = align256((size_t)count * 8) + align256((size_t)count * 4) + 256;
    p.grid_bytes = host ? 2 * align256(HW * 8) : 0;
    p.batch = fit_batch(batch, VIS_DEFAULT_BATCH, VIS_MAX_BATCH, count, VIS_SCRATCH_CAP, [&](int b) {
        p.zc_bytes = align256((size_t)b * HW * 8);
        p.stage_bytes = host ? align256((size_t)b * HW * 4) : 0;
        p.mask_bytes = host ? align256((size_t)b * HW) : 0;
        p.ang_bytes = host ? align256((size_t)b * HW * 4) : 0;
        return p.total = p.head_bytes + p.grid_bytes + p.zc_bytes + p.stage_bytes + p.mask_bytes + p.ang_bytes;
    });
    return p.batch ? WASS_OK : WASS_ERR_NO_MEMORY;
}

static int vis_run(wass_ctx* c, bool host, const float* in, size_t st, size_t sy, int count, int H, int W, const double* XX, const double* YY,
                   const double* origin, double datascale, double angle_limit, int batch, unsigned char* mask, float* angles,
                   unsigned long long* occluded, unsigned long long* not_upward)
{
    if (!c) return WASS_ERR_INVALID_ARG;
    if (!in || !XX || !YY || !origin || !mask || !angles) return set_err(c, WASS_ERR_INVALID_ARG, "null argument");
    VisPlan p;
    int rc = vis_plan(count, H, W, batch, host, p);
    if (rc) return set_err(c, rc, "cannot plan the visibility map of a %d x %d x %d cube (H, W from 2 to 65536) under the scratch cap of %zu bytes",
                           count, H, W, VIS_SCRATCH_CAP);
    if (sy < (size_t)W || (count > 1 && st < (size_t)W)) return set_err(c, WASS_ERR_INVALID_ARG, "bad strides");
    WASS_HIP(c, hipSetDevice(c->device));
    hipStream_t s = c->ts();
    double x01[2], y01[2];
    if (host) {
        x01[0] = XX[0]; x01[1] = XX[1]; y01[0] = YY[0]; y01[1] = YY[W];
    } else {
        WASS_HIP(c, hipMemcpy(x01, XX, 16, hipMemcpyDeviceToHost));
        WASS_HIP(c, hipMemcpy(&y01[0], YY, 8, hipMemcpyDeviceToHost));
        WASS_HIP(c, hipMemcpy(&y01[1], YY + W, 8, hipMemcpyDeviceToHost));
    }
    VisGeom g;
    g.dx = x01[1] - x01[0];
    g.dy = y01[1] - y01[0];
    if (!(g.dx > 0.0) || !(g.dy > 0.0)) return set_err(c, WASS_ERR_INVALID_ARG, "the grid spacing must be positive (dx = %g, dy = %g)", g.dx, g.dy);
    g.o0 = origin[0]; g.o1 = origin[1]; g.o2 = origin[2];
    g.use_limit = angle_limit >= 0.0 && angle_limit <= 1.7976931348623157e308;
    g.limit = angle_limit;
    g.scale = (float)datascale;
    const size_t HW = (size_t)H * W;
    Arena mem;
    if ((rc = mem.reserve(c, p.total, "the visibility scratch"))) return rc;
    unsigned long long* keys = mem.take<unsigned long long>((size_t)count * 8);
    unsigned* counts = mem.take<unsigned>((size_t)count * 4);
    unsigned long long* notup = mem.take<unsigned long long>(256);
    double* dXX = mem.take<double>(p.grid_bytes / 2);
    double* dYY = mem.take<double>(p.grid_bytes / 2);
    double* Zc = mem.take<double>(p.zc_bytes);
    float* stage = mem.take<float>(p.stage_bytes);
    unsigned char* dmask = mem.take<unsigned char>(p.mask_bytes);
    float* dang = mem.take<float>(p.ang_bytes);
    hipError_t e = hipMemsetAsync(keys, 0, p.head_bytes, s);   // the head: keys, counts and the not-upward count
    if (e == hipSuccess && host) {
        e = hipMemcpyAsync(dXX, XX, HW * 8, hipMemcpyHostToDevice, s);
        if (e == hipSuccess) e = hipMemcpyAsync(dYY, YY, HW * 8, hipMemcpyHostToDevice, s);
        g.XX = dXX; g.YY = dYY;
    } else {
        g.XX = XX; g.YY = YY;
    }
    const int nmax = H > W ? H : W;
    const dim3 block(VIS_BX, VIS_BY);
    for (int t0 = 0; t0 < count && e == hipSuccess; t0 += p.batch) {
        const int nb = count - t0 < p.batch ? count - t0 : p.batch;
        const dim3 grid((W + VIS_BX - 1) / VIS_BX, (H + VIS_BY - 1) / VIS_BY, nb);
        const float* zin = in + (size_t)t0 * st;
        long long zst = (long long)st, zsy = (long long)sy;
        unsigned char* m = mask + (size_t)t0 * HW;
        float* a = angles + (size_t)t0 * HW;
        if (host) {
            e = upload_rows(stage, zin, 4, nb, 0, H, W, st, sy, s);
            if (e != hipSuccess) break;
            zin = stage; zst = (long long)HW; zsy = W; m = dmask; a = dang;
        }
        hipLaunchKernelGGL(k_vis_prepass, grid, block, 0, s, zin, zst, zsy, H, W, g, Zc, m, a, keys + t0, notup);
        hipLaunchKernelGGL(k_vis_march, grid, block, 0, s, zin, zst, zsy, H, W, g, (const double*)Zc, (const unsigned long long*)(keys + t0), nmax, m,
                           counts + t0);
        e = hipGetLastError();
        if (e == hipSuccess && host) {
            e = hipMemcpyAsync(mask + (size_t)t0 * HW, dmask, (size_t)nb * HW, hipMemcpyDeviceToHost, s);
            if (e == hipSuccess) e = hipMemcpyAsync(angles + (size_t)t0 * HW, dang, (size_t)nb * HW * 4, hipMemcpyDeviceToHost, s);
        }
    }
    rc = finish(c, WASS_OK, e, s, "visibility map");
    if (!rc) {
        std::vector<unsigned> n((size_t)count);
        unsigned long long up = 0;
        e = hipMemcpy(n.data(), counts, (size_t)count * 4, hipMemcpyDeviceToHost);
        if (e == hipSuccess) e = hipMemcpy(&up, notup, 8, hipMemcpyDeviceToHost);
        if (e != hipSuccess) rc = set_err(c, WASS_ERR_DEVICE, "visibility map: %s", hipGetErrorString(e));
        else {
            if (occluded) for (int t = 0; t < count; ++t) occluded[t] = n[(size_t)t];
            if (not_upward) *not_upward = up;
        }
    }
    return rc;
}

static int occ_run(wass_ctx* c, bool host, const double* ZZ, const double* rays, int H, int W, int invert_y, unsigned char* mask,
                   unsigned long long* not_upward)
{
    if (!c) return WASS_ERR_INVALID_ARG;
    if (!ZZ || !rays || !mask) return set_err(c, WASS_ERR_INVALID_ARG, "null argument");
    if (H < 1 || W < 1 || H > 65536 || W > 65536 || (size_t)H * W > 0x7fffff00u) return set_err(c, WASS_ERR_INVALID_ARG, "a %d x %d surface", H, W);
    WASS_HIP(c, hipSetDevice(c->device));
    hipStream_t s = c->ts();
    const size_t HW = (size_t)H * W;
    Arena mem;
    int rc = mem.reserve(c, 256 + (host ? align256(HW * 8) + align256(HW * 24) + align256(HW) : 0), "the occlusion scratch");
    if (rc) return rc;
    unsigned long long* key = mem.take<unsigned long long>(256);
    unsigned long long* notup = key + 1;
    const double* dZ = ZZ;
    const double* dR = rays;
    unsigned char* dM = mask;
    hipError_t e = hipMemsetAsync(key, 0, 256, s);
    if (host) {
        double* z = mem.take<double>(HW * 8);
        double* r = mem.take<double>(HW * 24);
        dM = mem.take<unsigned char>(HW);
        if (e == hipSuccess) e = hipMemcpyAsync(z, ZZ, HW * 8, hipMemcpyHostToDevice, s);
        if (e == hipSuccess) e = hipMemcpyAsync(r, rays, HW * 24, hipMemcpyHostToDevice, s);
        dZ = z; dR = r;
    }
    if (e == hipSuccess) {
        const dim3 block(VIS_BX, VIS_BY), grid((W + VIS_BX - 1) / VIS_BX, (H + VIS_BY - 1) / VIS_BY);
        hipLaunchKernelGGL(k_occ_prepass, grid, block, 0, s, dZ, dR, H, W, key, notup);
        hipLaunchKernelGGL(k_occ_march, grid, block, 0, s, dZ, dR, H, W, invert_y, (const unsigned long long*)key, H > W ? H : W, dM);
        e = hipGetLastError();
        if (e == hipSuccess && host) e = hipMemcpyAsync(mask, dM, HW, hipMemcpyDeviceToHost, s);
    }
    rc = finish(c, WASS_OK, e, s, "occlusion mask");
    if (!rc && not_upward) {
        e = hipMemcpy(not_upward, notup, 8, hipMemcpyDeviceToHost);
        if (e != hipSuccess) rc = set_err(c, WASS_ERR_DEVICE, "occlusion mask: %s", hipGetErrorString(e));
    }
    return rc;
}

}  // namespace wass

using namespace wass;

extern "C" int wass_visibility_scratch_bytes(int count, int H, int W, int batch, int host, size_t* bytes, int* batch_used)
{
    if (!bytes) return WASS_ERR_INVALID_ARG;
    VisPlan p;
    const int rc = vis_plan(count, H, W, batch, host != 0, p);
    if (rc) return rc;
    *bytes = p.total;
    if (batch_used) *batch_used = p.batch;
    return WASS_OK;
}

extern "C" int wass_visibility(wass_ctx* c, const float* in, size_t stride_t, size_t stride_y, int count, int H, int W, const double* XX,
                               const double* YY, const double origin[3], double datascale, double angle_limit, int batch, uint8_t* mask,
                               float* angles, uint64_t* occluded, uint64_t* not_upward)
{
    return vis_run(c, true, in, stride_t, stride_y, count, H, W, XX, YY, origin, datascale, angle_limit, batch, mask, angles,
                   (unsigned long long*)occluded, (unsigned long long*)not_upward);
}

extern "C" int wass_visibility_dev(wass_ctx* c, const float* d_in, size_t stride_t, size_t stride_y, int count, int H, int W, const double* d_XX,
                                   const double* d_YY, const double origin[3], double datascale, double angle_limit, int batch, uint8_t* d_mask,
                                   float* d_angles, uint64_t* occluded, uint64_t* not_upward)
{
    return vis_run(c, false, d_in, stride_t, stride_y, count, H, W, d_XX, d_YY, origin, datascale, angle_limit, batch, d_mask, d_angles,
                   (unsigned long long*)occluded, (unsigned long long*)not_upward);
}

extern "C" int wass_occlusion_rays(wass_ctx* c, const double* ZZ, const double* rays, int H, int W, int invert_y_axis, uint8_t* mask,
                                   uint64_t* not_upward)
{
    return occ_run(c, true, ZZ, rays, H, W, invert_y_axis, mask, (unsigned long long*)not_upward);
}

extern "C" int wass_occlusion_rays_dev(wass_ctx* c, const double* d_ZZ, const double* d_rays, int H, int W, int invert_y_axis, uint8_t* d_mask,
                                       uint64_t* not_upward)
{
    return occ_run(c, false, d_ZZ, d_rays, H, W, invert_y_axis, d_mask, (unsigned long long*)not_upward);
}
