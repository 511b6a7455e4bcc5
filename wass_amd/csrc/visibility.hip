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
// The only atomics are integer ones (a maximum of order-preserving keys, counts): the same input gives the same bits.
#include "common.h"
#include "surface.h"     // vis_slope: shared with polarimetric.hip

namespace wass {

constexpr size_t VIS_SCRATCH_CAP = (size_t)16 << 30;    // bytes one call may allocate
constexpr int VIS_MAX_BATCH = 1024;                     // frames per launch (blockIdx.z)
constexpr int VIS_DEFAULT_BATCH = 8;
constexpr int VIS_U = 4;                                // steps whose heights are loaded ahead of the comparisons
constexpr int VIS_BX = 64, VIS_BY = 4;                  // a block: 4 waves, each 64 cells of one row

// an unsigned key that orders like the double it was made from; no finite value has key 0, which stands for "nothing seen"
__device__ __forceinline__ unsigned long long vis_key(double v)
{
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

__device__ __forceinline__ double vis_unkey(unsigned long long k)
{
    if (!k) return -INFINITY;
    return __longlong_as_double((long long)((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k));
}

__device__ __forceinline__ unsigned long long vis_wave_max(unsigned long long k)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long other = __shfl_xor(k, o, 64);
        k = other > k ? other : k;
    }
    return k;
}

// the block's largest key to *dst; every thread of the block calls it
__device__ __forceinline__ void vis_block_max(unsigned long long k, unsigned long long* dst)
{
    __shared__ unsigned long long part[VIS_BY];
    k = vis_wave_max(k);
    if (threadIdx.x == 0) part[threadIdx.y] = k;
    __syncthreads();
    if (threadIdx.x == 0 && threadIdx.y == 0) {
#pragma unroll
        for (int w = 1; w < VIS_BY; ++w) k = part[w] > k ? part[w] : k;
        if (k) atomicMax(dst, k);
    }
}

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
        if (fabs(zc) <= 1.7976931348623157e308) key = vis_key(zc);      // finite
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
    vis_block_max(key, keys + f);
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
                occluded = vis_march(plane, H, W, i, j, plane[c], d0 / m, d1 / m, d2 / m, vis_unkey(keys[f]), nmax);
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
        if (fabs(z) <= 1.7976931348623157e308) k = vis_key(z);
        bad = !(rays[3 * c + 2] > 0.0);                 // "rays must go upward"
    }
    const unsigned long long wave_bad = __ballot(bad);
    if (wave_bad && threadIdx.x == 0) atomicAdd(notup, (unsigned long long)__popcll(wave_bad));
    vis_block_max(k, key);
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
        occluded = vis_march(ZZ, H, W, i, j, ZZ[c], r0 / m, invert_y ? -s1 : s1, r2 / m, vis_unkey(*key), nmax);
    }
    mask[c] = occluded ? 1 : 0;
}

static size_t vis_align(size_t v) { return (v + 255) & ~(size_t)255; }

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
    int b = batch ? batch : VIS_DEFAULT_BATCH;
    if (b > count) b = count;
    if (b > VIS_MAX_BATCH) b = VIS_MAX_BATCH;
    p.head_bytes = vis_align((size_t)count * 8) + vis_align((size_t)count * 4) + 256;
    p.grid_bytes = host ? 2 * vis_align(HW * 8) : 0;
    for (;; b /= 2) {
        if (b < 1) return WASS_ERR_NO_MEMORY;
        p.zc_bytes = vis_align((size_t)b * HW * 8);
        p.stage_bytes = host ? vis_align((size_t)b * HW * 4) : 0;
        p.mask_bytes = host ? vis_align((size_t)b * HW) : 0;
        p.ang_bytes = host ? vis_align((size_t)b * HW * 4) : 0;
        p.total = p.head_bytes + p.grid_bytes + p.zc_bytes + p.stage_bytes + p.mask_bytes + p.ang_bytes;
        if (p.total <= VIS_SCRATCH_CAP) break;
    }
    p.batch = b;
    return WASS_OK;
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
    char* mem = nullptr;
    if (hipMalloc((void**)&mem, p.total) != hipSuccess) return set_err(c, WASS_ERR_NO_MEMORY, "hipMalloc(%zu) for the visibility scratch failed", p.total);
    char* q = mem;
    unsigned long long* keys = (unsigned long long*)q;      q += vis_align((size_t)count * 8);
    unsigned* counts = (unsigned*)q;                        q += vis_align((size_t)count * 4);
    unsigned long long* notup = (unsigned long long*)q;     q += 256;
    double* dXX = (double*)q;                               q += p.grid_bytes / 2;
    double* dYY = (double*)q;                               q += p.grid_bytes / 2;
    double* Zc = (double*)q;                                q += p.zc_bytes;
    float* stage = (float*)q;                               q += p.stage_bytes;
    unsigned char* dmask = (unsigned char*)q;               q += p.mask_bytes;
    float* dang = (float*)q;
    hipError_t e = hipMemsetAsync(mem, 0, p.head_bytes, s);
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
            for (int t = 0; t < nb && e == hipSuccess; ++t)
                e = hipMemcpy2DAsync(stage + t * HW, (size_t)W * 4, zin + t * st, sy * 4, (size_t)W * 4, H, hipMemcpyHostToDevice, s);
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
    if (e != hipSuccess) rc = set_err(c, WASS_ERR_DEVICE, "visibility map: %s", hipGetErrorString(e));
    e = hipStreamSynchronize(s);                            // the scratch is freed below
    if (!rc && e != hipSuccess) rc = set_err(c, WASS_ERR_DEVICE, "visibility map: %s", hipGetErrorString(e));
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
    (void)hipFree(mem);
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
    const size_t total = 256 + (host ? vis_align(HW * 8) + vis_align(HW * 24) + vis_align(HW) : 0);
    char* mem = nullptr;
    if (hipMalloc((void**)&mem, total) != hipSuccess) return set_err(c, WASS_ERR_NO_MEMORY, "hipMalloc(%zu) for the occlusion scratch failed", total);
    unsigned long long* key = (unsigned long long*)mem;
    unsigned long long* notup = key + 1;
    const double* dZ = ZZ;
    const double* dR = rays;
    unsigned char* dM = mask;
    hipError_t e = hipMemsetAsync(mem, 0, 256, s);
    if (host) {
        double* z = (double*)(mem + 256);
        double* r = (double*)(mem + 256 + vis_align(HW * 8));
        dM = (unsigned char*)(mem + 256 + vis_align(HW * 8) + vis_align(HW * 24));
        if (e == hipSuccess) e = hipMemcpyAsync(z, ZZ, HW * 8, hipMemcpyHostToDevice, s);
        if (e == hipSuccess) e = hipMemcpyAsync(r, rays, HW * 24, hipMemcpyHostToDevice, s);
        dZ = z; dR = r;
    }
    int rc = WASS_OK;
    if (e == hipSuccess) {
        const dim3 block(VIS_BX, VIS_BY), grid((W + VIS_BX - 1) / VIS_BX, (H + VIS_BY - 1) / VIS_BY);
        hipLaunchKernelGGL(k_occ_prepass, grid, block, 0, s, dZ, dR, H, W, key, notup);
        hipLaunchKernelGGL(k_occ_march, grid, block, 0, s, dZ, dR, H, W, invert_y, (const unsigned long long*)key, H > W ? H : W, dM);
        e = hipGetLastError();
        if (e == hipSuccess && host) e = hipMemcpyAsync(mask, dM, HW, hipMemcpyDeviceToHost, s);
    }
    if (e != hipSuccess) rc = set_err(c, WASS_ERR_DEVICE, "occlusion mask: %s", hipGetErrorString(e));
    e = hipStreamSynchronize(s);
    if (!rc && e != hipSuccess) rc = set_err(c, WASS_ERR_DEVICE, "occlusion mask: %s", hipGetErrorString(e));
    if (!rc && not_upward) {
        e = hipMemcpy(not_upward, notup, 8, hipMemcpyDeviceToHost);
        if (e != hipSuccess) rc = set_err(c, WASS_ERR_DEVICE, "occlusion mask: %s", hipGetErrorString(e));
    }
    (void)hipFree(mem);
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
