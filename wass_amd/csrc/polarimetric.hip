// polarimetric.hip -- wasspost's `polarimetric_setup` (postproc/wasspost/wasspost.py:627-805), `clip` and `zeromean` as array
// functions.
//
//   k_remap_linear_f32  cv::remap(CV_32FC1, CV_32FC1 maps, INTER_LINEAR, BORDER_CONSTANT 0) restated as radiance.hip restates the
//                       Lanczos4 one: coordinates quantised to 1/32 pixel (float product, round half to even), the window of 2 x 2
//                       taps at (sat16(X >> 5), sat16(Y >> 5)), the four float32 weights of phase (Y & 31) * 32 + (X & 31) from
//                       a 1024 x 2 x 2 table, ((v00 w00 + v01 w01) + v10 w10) + v11 w11 in float32 without contraction, each tap
//                       outside the picture replaced by 0.  OpenCV is absent here: written from knowledge of OpenCV 4.5.5's
//                       imgwarp.cpp, PARITY UNPINNED (neither the order of the sum nor whether a build contracts it is pinned),
//                       bit-exact against the numpy restatement of tests/polarimetric_oracle.py.
//   k_pol_sample        one lane per cell, frames in blockIdx.z: zf = Z * (float)datascale, the projection of k_radiance, the
//                       camera-frame ray q / |q| with q = ((Ki0 u + Ki1 v) + Ki2), the three Stokes samples at
//                       ((float)u, (float)v), NaN where the mask (wass_visibility_dev made it) is 1, DOLP = sqrt(S1^2 + S2^2) / S0
//                       in float32 (root and quotient formed in fp64 and rounded again: the correctly rounded float32 results),
//                       the normal of surface.h.  No map array exists.
//   k_pol_acc           one lane per cell walks the frames of a launch in order and adds, in fp64, nan_to_num(S), the normal,
//                       zf and 1 - mask to the accumulators: numpy's sequential adds, no atomics, the same bits on every run
//   k_pol_finish        Savg / valid, Navg / |Navg|, Zavg / total_frames
//   k_clip              np.clip in float32 (NaN kept) and the range of what is not NaN (integer atomics on ordered keys)
//   k_zeromean          per cell the fp64 sum over the frames in order, / count, out = (float)((double)z - mean)
// Host side: pol_plan keeps the byte formula; the batch and slab rules, the scratch, the staging of a host batch or slab and the
// end of a call are cube.h's.
#include "common.h"
#include "cube.h"
#include "surface.h"

#include <cfloat>
#include <cmath>
#include <vector>

namespace wass {

constexpr size_t POL_SCRATCH_CAP = (size_t)16 << 30;    // bytes one call may allocate
constexpr int POL_MAX_BATCH = 1024;                     // frames per launch (blockIdx.z)
constexpr int POL_DEFAULT_BATCH = 8;
constexpr int POL_BX = 64, POL_BY = 4;                  // a block: 4 waves, each 64 cells of one row
constexpr int POL_BITS = 5, POL_TAB = 1 << POL_BITS, POL_TAB2 = POL_TAB * POL_TAB;
constexpr int POL_U = 8;                                // frames loaded ahead of the fp64 chain of k_zeromean

// ---------------------------------------------------------------- the bilinear table (imgwarp.cpp interpolateLinear, initInterTab2D)
// tab[((fy * 32 + fx) * 2 + ky) * 2 + kx] = ty[ky] * tx[kx], t = (1 - f / 32, f / 32): every value a multiple of 1 / 1024, exact
static void build_bilinear_tab(float* tab)
{
    const float scale = 1.f / POL_TAB;
    for (int fy = 0; fy < POL_TAB; ++fy)
        for (int fx = 0; fx < POL_TAB; ++fx) {
            const float ty[2] = { 1.f - fy * scale, fy * scale }, tx[2] = { 1.f - fx * scale, fx * scale };
            float* w = tab + (size_t)(fy * POL_TAB + fx) * 4;
            for (int ky = 0; ky < 2; ++ky)
                for (int kx = 0; kx < 2; ++kx) w[ky * 2 + kx] = ty[ky] * tx[kx];
        }
}

constexpr size_t BILINEAR_TAB_BYTES = (size_t)POL_TAB2 * 4 * sizeof(float);     // 16 KiB

int ensure_bilinear_tab(wass_ctx* c)
{
    if (c->bilinear_tab_ready) return WASS_OK;
    int rc = ensure(c, c->bilinear_tab, BILINEAR_TAB_BYTES);
    if (rc) return rc;
    std::vector<float> tab((size_t)POL_TAB2 * 4);
    build_bilinear_tab(tab.data());
    WASS_HIP(c, hipMemcpy(c->bilinear_tab.p, tab.data(), BILINEAR_TAB_BYTES, hipMemcpyHostToDevice));
    c->bilinear_tab_ready = true;
    return WASS_OK;
}

// ---------------------------------------------------------------- the sampler
__device__ __forceinline__ int pol_sat_s16(int v) { return v < -32768 ? -32768 : v > 32767 ? 32767 : v; }

// q = cvRound(m * 32) where that is defined: the float product is finite and inside the int32 range
__device__ __forceinline__ bool pol_quant(float m, int& q)
{
    const float p = m * (float)POL_TAB;
    if (!(fabsf(p) < 2147483648.f)) return false;       // NaN, infinite or out of range
    q = __float2int_rn(p);
    return true;
}

// where the map (mx, my) points: the window's origin and the four weights; false = the sample is 0
struct PolTap { int sx, sy; float4 w; };

__device__ __forceinline__ bool pol_tap(float mx, float my, const float4* __restrict__ tab, PolTap& t)
{
    int X, Y;
    if (!pol_quant(mx, X) || !pol_quant(my, Y)) return false;
    t.sx = pol_sat_s16(X >> POL_BITS);
    t.sy = pol_sat_s16(Y >> POL_BITS);
    t.w = tab[(Y & (POL_TAB - 1)) * POL_TAB + (X & (POL_TAB - 1))];
    return true;
}

// remapBilinear (imgwarp.cpp) for one float32 channel, BORDER_CONSTANT 0.  sw, sh < 32767, so sx + 1 and sy + 1 cannot overflow.
__device__ __forceinline__ float sample_linear(const float* __restrict__ src, int sw, int sh, size_t ss, const PolTap& t)
{
    const int sx = t.sx, sy = t.sy;
    float v00, v01, v10, v11;
    if ((unsigned)sx < (unsigned)(sw - 1) && (unsigned)sy < (unsigned)(sh - 1)) {
        const float* s = src + (size_t)sy * ss + sx;
        v00 = s[0]; v01 = s[1]; v10 = s[ss]; v11 = s[ss + 1];
    } else {
        if (sx >= sw || sx + 2 <= 0 || sy >= sh || sy + 2 <= 0) return 0.f;
        const bool x0 = (unsigned)sx < (unsigned)sw, x1 = (unsigned)(sx + 1) < (unsigned)sw;
        const bool y0 = (unsigned)sy < (unsigned)sh, y1 = (unsigned)(sy + 1) < (unsigned)sh;
        v00 = y0 && x0 ? src[(size_t)sy * ss + sx] : 0.f;
        v01 = y0 && x1 ? src[(size_t)sy * ss + sx + 1] : 0.f;
        v10 = y1 && x0 ? src[(size_t)(sy + 1) * ss + sx] : 0.f;
        v11 = y1 && x1 ? src[(size_t)(sy + 1) * ss + sx + 1] : 0.f;
    }
    return ((v00 * t.w.x + v01 * t.w.y) + v10 * t.w.z) + v11 * t.w.w;
}

__global__ void __launch_bounds__(POL_BX * POL_BY) k_remap_linear_f32(const float* __restrict__ src, int sw, int sh, size_t ss,
                                                                      const float* __restrict__ mx, const float* __restrict__ my, int dw, int dh,
                                                                      float* __restrict__ dst, const float4* __restrict__ tab)
{
    const int x = blockIdx.x * POL_BX + threadIdx.x, y = blockIdx.y * POL_BY + threadIdx.y;
    if (x >= dw || y >= dh) return;
    const size_t i = (size_t)y * dw + x;
    PolTap t;
    dst[i] = pol_tap(mx[i], my[i], tab, t) ? sample_linear(src, sw, sh, ss, t) : 0.f;
}

static int pol_picture_ok(wass_ctx* c, int sw, int sh, size_t ss)
{
    if (sw < 1 || sh < 1 || sw >= 32767 || sh >= 32767 || ss < (size_t)sw)
        return set_err(c, WASS_ERR_INVALID_ARG, "a %d x %d picture with a row stride of %zu (sides from 1 to 32766)", sw, sh, ss);
    return WASS_OK;
}

static int remap_f32_run(wass_ctx* c, bool host, const float* src, int sw, int sh, size_t ss, const float* mx, const float* my, int dw, int dh,
                         float* dst)
{
    if (!c) return WASS_ERR_INVALID_ARG;
    if (!src || !mx || !my || !dst) return set_err(c, WASS_ERR_INVALID_ARG, "null argument");
    int rc = pol_picture_ok(c, sw, sh, ss);
    if (rc) return rc;
    if (dw < 1 || dh < 1 || dw > 65536 || dh > 65536) return set_err(c, WASS_ERR_INVALID_ARG, "a %d x %d output", dw, dh);
    WASS_HIP(c, hipSetDevice(c->device));
    rc = ensure_bilinear_tab(c);
    if (rc) return rc;
    hipStream_t s = c->ts();
    const size_t n = (size_t)dw * dh, src_bytes = align256((size_t)sh * sw * 4), nb = align256(n * 4);
    Arena mem;
    const float *dsrc = src, *dmx = mx, *dmy = my;
    float* ddst = dst;
    size_t dss = ss;
    hipError_t e = hipSuccess;
    if (host) {
        if ((rc = mem.reserve(c, src_bytes + 3 * nb, "the remap"))) return rc;
        float* a = mem.take<float>(src_bytes);
        float* b = mem.take<float>(nb);
        float* d = mem.take<float>(nb);
        ddst = mem.take<float>(nb);
        e = upload_rows(a, src, 4, 1, 0, sh, sw, 0, ss, s);
        if (e == hipSuccess) e = hipMemcpyAsync(b, mx, n * 4, hipMemcpyHostToDevice, s);
        if (e == hipSuccess) e = hipMemcpyAsync(d, my, n * 4, hipMemcpyHostToDevice, s);
        dsrc = a; dmx = b; dmy = d; dss = (size_t)sw;
    }
    if (e == hipSuccess) {
        const dim3 block(POL_BX, POL_BY), grid((dw + POL_BX - 1) / POL_BX, (dh + POL_BY - 1) / POL_BY);
        hipLaunchKernelGGL(k_remap_linear_f32, grid, block, 0, s, dsrc, sw, sh, dss, dmx, dmy, dw, dh, ddst, (const float4*)c->bilinear_tab.p);
        e = hipGetLastError();
        if (e == hipSuccess && host) e = hipMemcpyAsync(dst, ddst, n * 4, hipMemcpyDeviceToHost, s);
    }
    return finish(c, WASS_OK, e, s, "remap_linear_f32", host);
}

// ---------------------------------------------------------------- polarimetric_setup
struct PolGeom {
    double p[12];                  // Pcam, row-major 3 x 4
    double ki[9];                  // inv(K), row-major
    double dx, dy;
    float scale;                   // (float)datascale
};

struct PolOut {                    // per-frame results of a launch; S and mask always, the rest where asked for
    float* S;                      // [nb][H][W][3]
    const unsigned char* mask;     // [nb][H][W], made by wass_visibility_dev
    float* dolp;                   // [nb][H][W]
    double* normals;               // [nb][H][W][3]
    double* rays;                  // [nb][3][H * W]
};

// pictures: frame f, channel k at st + f * st_t + k * st_c, rows st_y apart (elements)
__global__ void __launch_bounds__(POL_BX * POL_BY) k_pol_sample(const float* __restrict__ st, size_t st_t, size_t st_c, size_t st_y, int sw, int sh,
                                                                const float* __restrict__ Z, long long zt, long long zy, int H, int W,
                                                                const double* __restrict__ XX, const double* __restrict__ YY, const PolGeom g,
                                                                const PolOut o, const float4* __restrict__ tab)
{
    const int j = blockIdx.x * POL_BX + threadIdx.x, i = blockIdx.y * POL_BY + threadIdx.y;
    if (i >= H || j >= W) return;
    const size_t f = blockIdx.z, HW = (size_t)H * W, c = (size_t)i * W + j;
    const float* __restrict__ zp = Z + (long long)f * zt + (long long)i * zy + j;
    double n0, n1, n2;
    float zf;
    if (o.normals) {
        zf = surface_normal(zp, zy, i, j, H, W, g.scale, g.dx, g.dy, n0, n1, n2);
        double* n = o.normals + (f * HW + c) * 3;
        n[0] = n0; n[1] = n1; n[2] = n2;
    } else {
        zf = zp[0] * g.scale;
    }
    const double X = XX[c], Y = YY[c], z = (double)zf;
    const double r0 = ((g.p[0] * X + g.p[1] * Y) + g.p[2] * z) + g.p[3];
    const double r1 = ((g.p[4] * X + g.p[5] * Y) + g.p[6] * z) + g.p[7];
    const double r2 = ((g.p[8] * X + g.p[9] * Y) + g.p[10] * z) + g.p[11];
    const double u = r0 / r2, v = r1 / r2;
    if (o.rays) {
        const double q0 = (g.ki[0] * u + g.ki[1] * v) + g.ki[2];
        const double q1 = (g.ki[3] * u + g.ki[4] * v) + g.ki[5];
        const double q2 = (g.ki[6] * u + g.ki[7] * v) + g.ki[8];
        const double qn = sqrt((q0 * q0 + q1 * q1) + q2 * q2);
        double* r = o.rays + f * HW * 3 + c;
        r[0] = q0 / qn; r[HW] = q1 / qn; r[2 * HW] = q2 / qn;
    }
    float s0, s1, s2;
    if (o.mask[f * HW + c]) {
        s0 = s1 = s2 = __uint_as_float(0x7fc00000u);
    } else {
        PolTap t;
        s0 = s1 = s2 = 0.f;
        if (pol_tap((float)u, (float)v, tab, t)) {
            const float* __restrict__ pic = st + f * st_t;
            s0 = sample_linear(pic, sw, sh, st_y, t);
            s1 = sample_linear(pic + st_c, sw, sh, st_y, t);
            s2 = sample_linear(pic + 2 * st_c, sw, sh, st_y, t);
        }
    }
    float* S = o.S + (f * HW + c) * 3;
    S[0] = s0; S[1] = s1; S[2] = s2;
    if (o.dolp) {
        // a float32 root or quotient of float32 values formed in fp64 and rounded once more is the correctly rounded float32 result
        const float q = s1 * s1 + s2 * s2;
        const float r = (float)sqrt((double)q);
        o.dolp[f * HW + c] = (float)((double)r / (double)s0);
    }
}

// np.nan_to_num of a float32 value, as the fp64 term of the sum
__device__ __forceinline__ double pol_nan_to_num(float v)
{
    if (v != v) return 0.0;
    if (v > FLT_MAX) return (double)FLT_MAX;
    if (v < -FLT_MAX) return -(double)FLT_MAX;
    return (double)v;
}

// acc: [Savg HW x 3 | Navg HW x 3 | Zavg HW | valid HW] doubles; the frames of the launch are added in order
__global__ void __launch_bounds__(POL_BX * POL_BY) k_pol_acc(const float* __restrict__ Z, long long zt, long long zy, int H, int W, int nb,
                                                             const PolGeom g, const float* __restrict__ S,
                                                             const unsigned char* __restrict__ mask, double* __restrict__ acc)
{
    const int j = blockIdx.x * POL_BX + threadIdx.x, i = blockIdx.y * POL_BY + threadIdx.y;
    if (i >= H || j >= W) return;
    const size_t HW = (size_t)H * W, c = (size_t)i * W + j;
    double* aS = acc + 3 * c;
    double* aN = acc + 3 * HW + 3 * c;
    double* aZ = acc + 6 * HW + c;
    double* aV = acc + 7 * HW + c;
    double s0 = aS[0], s1 = aS[1], s2 = aS[2], m0 = aN[0], m1 = aN[1], m2 = aN[2], zs = aZ[0], vs = aV[0];
    for (int f = 0; f < nb; ++f) {
        double n0, n1, n2;
        const float zf = surface_normal(Z + (long long)f * zt + (long long)i * zy + j, zy, i, j, H, W, g.scale, g.dx, g.dy, n0, n1, n2);
        const float* s = S + ((size_t)f * HW + c) * 3;
        s0 += pol_nan_to_num(s[0]);
        s1 += pol_nan_to_num(s[1]);
        s2 += pol_nan_to_num(s[2]);
        m0 += n0; m1 += n1; m2 += n2;
        zs += (double)zf;
        vs += 1.0 - (double)mask[(size_t)f * HW + c];
    }
    aS[0] = s0; aS[1] = s1; aS[2] = s2;
    aN[0] = m0; aN[1] = m1; aN[2] = m2;
    aZ[0] = zs;
    aV[0] = vs;
}

__global__ void __launch_bounds__(256) k_pol_finish(double* __restrict__ acc, size_t HW, double total_frames)
{
    const size_t c = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= HW) return;
    double* aS = acc + 3 * c;
    double* aN = acc + 3 * HW + 3 * c;
    const double v = acc[7 * HW + c];
    aS[0] = aS[0] / v; aS[1] = aS[1] / v; aS[2] = aS[2] / v;
    const double n = sqrt((aN[0] * aN[0] + aN[1] * aN[1]) + aN[2] * aN[2]);
    aN[0] = aN[0] / n; aN[1] = aN[1] / n; aN[2] = aN[2] / n;
    acc[6 * HW + c] = acc[6 * HW + c] / total_frames;
}

enum { POL_OUT_S = 1, POL_OUT_OCC = 2, POL_OUT_ANG = 4, POL_OUT_DOLP = 8, POL_OUT_NRM = 16, POL_OUT_RAYS = 32, POL_OUT_ALL = 63 };

struct PolPlan {
    int batch = 0;
    size_t grid_bytes = 0, acc_bytes = 0, st_bytes = 0, z_bytes = 0, mask_bytes = 0, ang_bytes = 0, S_bytes = 0, dolp_bytes = 0, nrm_bytes = 0,
           ray_bytes = 0, own = 0, vis_bytes = 0, total = 0;
};

// The device form needs the mask, the angles and S of a batch where they are not asked for as outputs, and what the visibility
// map allocates for a batch; the host form stages XX, YY, the accumulators and, per frame of a batch, the three pictures, the
// heights and every result asked for.
static int pol_plan(int count, int H, int W, int Ih, int Iw, int batch, bool host, int outputs, PolPlan& p)
{
    if (count < 1 || H < 2 || W < 2 || batch < 0 || H > 65536 || W > 65536 || Ih < 1 || Iw < 1 || Ih >= 32767 || Iw >= 32767 ||
        (outputs & ~POL_OUT_ALL))
        return WASS_ERR_INVALID_ARG;
    const size_t HW = (size_t)H * W;
    if (HW > 0x7fffff00u) return WASS_ERR_UNSUPPORTED;
    p.grid_bytes = host ? 2 * align256(HW * 8) : 0;
    p.acc_bytes = host ? align256(HW * 64) : 0;
    p.batch = fit_batch(batch, POL_DEFAULT_BATCH, POL_MAX_BATCH, count, POL_SCRATCH_CAP, [&](int b) {
        const size_t n = (size_t)b * HW;
        p.st_bytes = host ? align256((size_t)b * 3 * Ih * Iw * 4) : 0;
        p.z_bytes = host ? align256(n * 4) : 0;
        p.mask_bytes = host || !(outputs & POL_OUT_OCC) ? align256(n) : 0;
        p.ang_bytes = host || !(outputs & POL_OUT_ANG) ? align256(n * 4) : 0;
        p.S_bytes = host || !(outputs & POL_OUT_S) ? align256(n * 12) : 0;
        p.dolp_bytes = host && (outputs & POL_OUT_DOLP) ? align256(n * 4) : 0;
        p.nrm_bytes = host && (outputs & POL_OUT_NRM) ? align256(n * 24) : 0;
        p.ray_bytes = host && (outputs & POL_OUT_RAYS) ? align256(n * 24) : 0;
        p.own = p.grid_bytes + p.acc_bytes + p.st_bytes + p.z_bytes + p.mask_bytes + p.ang_bytes + p.S_bytes + p.dolp_bytes + p.nrm_bytes + p.ray_bytes;
        int used = 0;
        // the sizes were checked above, so the visibility map's plan can only fail for want of memory
        if (wass_visibility_scratch_bytes(b, H, W, b, 0, &p.vis_bytes, &used)) return ~(size_t)0;
        return p.total = p.own + p.vis_bytes;
    });
    return p.batch ? WASS_OK : WASS_ERR_NO_MEMORY;
}

static int pol_run(wass_ctx* c, bool host, const float* stokes, size_t sst, size_t ssc, size_t ssy, int Ih, int Iw, const float* in, size_t st,
                   size_t sy, int count, int H, int W, const double* XX, const double* YY, const wass_pol_params* prm, double* acc,
                   const wass_pol_out* out, uint64_t* occluded, uint64_t* not_upward)
{
    if (!c) return WASS_ERR_INVALID_ARG;
    if (!stokes || !in || !XX || !YY || !prm || !acc) return set_err(c, WASS_ERR_INVALID_ARG, "null argument");
    static const wass_pol_out none = {};
    const wass_pol_out& o = out ? *out : none;
    const int outputs = (o.S ? POL_OUT_S : 0) | (o.occlusion ? POL_OUT_OCC : 0) | (o.angles ? POL_OUT_ANG : 0) | (o.dolp ? POL_OUT_DOLP : 0) |
                        (o.normals ? POL_OUT_NRM : 0) | (o.rays_cam ? POL_OUT_RAYS : 0);
    PolPlan p;
    int rc = pol_plan(count, H, W, Ih, Iw, prm->batch, host, outputs, p);
    if (rc) return set_err(c, rc, "cannot plan the polarimetric set-up of a %d x %d x %d cube (H, W from 2 to 65536) from %d x %d pictures under the "
                                  "scratch cap of %zu bytes", count, H, W, Ih, Iw, POL_SCRATCH_CAP);
    if (prm->total_frames < 0) return set_err(c, WASS_ERR_INVALID_ARG, "total_frames must not be negative");
    if (sy < (size_t)W || ssy < (size_t)Iw || ssc < (size_t)Iw || (count > 1 && (st < (size_t)W || sst < (size_t)Iw)))
        return set_err(c, WASS_ERR_INVALID_ARG, "bad strides");
    WASS_HIP(c, hipSetDevice(c->device));
    rc = ensure_bilinear_tab(c);
    if (rc) return rc;
    hipStream_t s = c->ts();
    double x01[2], y01[2];
    if (host) {
        x01[0] = XX[0]; x01[1] = XX[1]; y01[0] = YY[0]; y01[1] = YY[W];
    } else {
        WASS_HIP(c, hipMemcpy(x01, XX, 16, hipMemcpyDeviceToHost));
        WASS_HIP(c, hipMemcpy(&y01[0], YY, 8, hipMemcpyDeviceToHost));
        WASS_HIP(c, hipMemcpy(&y01[1], YY + W, 8, hipMemcpyDeviceToHost));
    }
    PolGeom g;
    for (int k = 0; k < 12; ++k) g.p[k] = prm->Pcam[k];
    for (int k = 0; k < 9; ++k) g.ki[k] = prm->Kinv[k];
    g.dx = x01[1] - x01[0];
    g.dy = y01[1] - y01[0];
    g.scale = (float)prm->datascale;
    if (!(g.dx > 0.0) || !(g.dy > 0.0)) return set_err(c, WASS_ERR_INVALID_ARG, "the grid spacing must be positive (dx = %g, dy = %g)", g.dx, g.dy);
    const size_t HW = (size_t)H * W, II = (size_t)Ih * Iw;
    Arena mem;                                              // the device form with every per-frame output given: nothing
    if ((rc = mem.reserve(c, p.own, "the polarimetric scratch"))) return rc;
    double* dXX = mem.take<double>(p.grid_bytes / 2);
    double* dYY = mem.take<double>(p.grid_bytes / 2);
    double* dacc = mem.take<double>(p.acc_bytes);
    float* sst_ = mem.take<float>(p.st_bytes);
    float* sz = mem.take<float>(p.z_bytes);
    unsigned char* smask = mem.take<unsigned char>(p.mask_bytes);
    float* sang = mem.take<float>(p.ang_bytes);
    float* sS = mem.take<float>(p.S_bytes);
    float* sdolp = mem.take<float>(p.dolp_bytes);
    double* snrm = mem.take<double>(p.nrm_bytes);
    double* sray = mem.take<double>(p.ray_bytes);
    hipError_t e = hipSuccess;
    if (host) {
        e = hipMemcpyAsync(dXX, XX, HW * 8, hipMemcpyHostToDevice, s);
        if (e == hipSuccess) e = hipMemcpyAsync(dYY, YY, HW * 8, hipMemcpyHostToDevice, s);
        if (e == hipSuccess) e = hipMemcpyAsync(dacc, acc, HW * 64, hipMemcpyHostToDevice, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);      // the visibility map reads the grid's spacing with a blocking copy
    } else {
        dXX = const_cast<double*>(XX); dYY = const_cast<double*>(YY); dacc = acc;
    }
    unsigned long long up_total = 0;
    rc = WASS_OK;
    const dim3 block(POL_BX, POL_BY);
    for (int t0 = 0; t0 < count && e == hipSuccess && !rc; t0 += p.batch) {
        const int nb = count - t0 < p.batch ? count - t0 : p.batch;
        const dim3 grid((W + POL_BX - 1) / POL_BX, (H + POL_BY - 1) / POL_BY, nb);
        const float* pic = stokes + (size_t)t0 * sst;
        size_t pt = sst, pc = ssc, py = ssy;
        const float* zin = in + (size_t)t0 * st;
        long long zst = (long long)st, zsy = (long long)sy;
        if (host) {
            for (int t = 0; t < nb && e == hipSuccess; ++t)     // a frame's three channels: a cube of three pictures, ssc apart
                e = upload_rows(sst_ + (size_t)t * 3 * II, pic + t * sst, 4, 3, 0, Ih, Iw, ssc, ssy, s);
            if (e == hipSuccess) e = upload_rows(sz, zin, 4, nb, 0, H, W, st, sy, s);
            if (e != hipSuccess) break;
            pic = sst_; pt = 3 * II; pc = II; py = (size_t)Iw; zin = sz; zst = (long long)HW; zsy = W;
        }
        unsigned char* m = !host && o.occlusion ? o.occlusion + (size_t)t0 * HW : smask;
        float* a = !host && o.angles ? o.angles + (size_t)t0 * HW : sang;
        PolOut k;
        k.mask = m;
        k.S = !host && o.S ? o.S + (size_t)t0 * HW * 3 : sS;
        k.dolp = o.dolp ? (host ? sdolp : o.dolp + (size_t)t0 * HW) : nullptr;
        k.normals = o.normals ? (host ? snrm : o.normals + (size_t)t0 * HW * 3) : nullptr;
        k.rays = o.rays_cam ? (host ? sray : o.rays_cam + (size_t)t0 * HW * 3) : nullptr;
        unsigned long long up = 0;
        // the march and the angles are visibility.hip's, through its device entry (same context, same stream); it returns synchronised
        rc = wass_visibility_dev(c, zin, (size_t)zst, (size_t)zsy, nb, H, W, dXX, dYY, prm->origin, prm->datascale, prm->angle_limit, nb, m, a,
                                 occluded ? occluded + t0 : nullptr, (uint64_t*)&up);
        if (rc) break;
        up_total += up;
        hipLaunchKernelGGL(k_pol_sample, grid, block, 0, s, pic, pt, pc, py, Iw, Ih, zin, zst, zsy, H, W, (const double*)dXX, (const double*)dYY, g, k,
                           (const float4*)c->bilinear_tab.p);
        hipLaunchKernelGGL(k_pol_acc, dim3(grid.x, grid.y), block, 0, s, zin, zst, zsy, H, W, nb, g, (const float*)k.S, (const unsigned char*)m, dacc);
        e = hipGetLastError();
        if (e == hipSuccess && host) {
            const size_t n = (size_t)nb * HW, at = (size_t)t0 * HW;
            if (o.S) e = hipMemcpyAsync(o.S + at * 3, sS, n * 12, hipMemcpyDeviceToHost, s);
            if (e == hipSuccess && o.occlusion) e = hipMemcpyAsync(o.occlusion + at, smask, n, hipMemcpyDeviceToHost, s);
            if (e == hipSuccess && o.angles) e = hipMemcpyAsync(o.angles + at, sang, n * 4, hipMemcpyDeviceToHost, s);
            if (e == hipSuccess && o.dolp) e = hipMemcpyAsync(o.dolp + at, sdolp, n * 4, hipMemcpyDeviceToHost, s);
            if (e == hipSuccess && o.normals) e = hipMemcpyAsync(o.normals + at * 3, snrm, n * 24, hipMemcpyDeviceToHost, s);
            if (e == hipSuccess && o.rays_cam) e = hipMemcpyAsync(o.rays_cam + at * 3, sray, n * 24, hipMemcpyDeviceToHost, s);
        }
    }
    if (!rc && e == hipSuccess && prm->total_frames > 0 && !up_total) {
        hipLaunchKernelGGL(k_pol_finish, dim3((unsigned)((HW + 255) / 256)), dim3(256), 0, s, dacc, HW, (double)prm->total_frames);
        e = hipGetLastError();
    }
    if (!rc && e == hipSuccess && host) e = hipMemcpyAsync(acc, dacc, HW * 64, hipMemcpyDeviceToHost, s);
    rc = finish(c, rc, e, s, "polarimetric set-up");
    if (!rc && not_upward) *not_upward = up_total;
    return rc;
}

// ---------------------------------------------------------------- clip and zeromean
// rec[0] = the largest ~key (the minimum), rec[1] = the largest key (the maximum) of the clipped values that are not NaN; 0 = none
__global__ void __launch_bounds__(POL_BX * POL_BY) k_clip(const float* x, long long st, long long sy, int H, int W, float lo, float hi, float* out,
                                                          long long ot, long long oy, unsigned* __restrict__ rec)
{
    __shared__ unsigned part[2][POL_BY];
    const int j = blockIdx.x * POL_BX + threadIdx.x, i = blockIdx.y * POL_BY + threadIdx.y;
    unsigned klo = 0, khi = 0;
    if (i < H && j < W) {
        float v = x[(long long)blockIdx.z * st + (long long)i * sy + j];
        v = v < lo ? lo : v;                            // np.maximum, then np.minimum; NaN fails both comparisons and stays
        v = v > hi ? hi : v;
        out[(long long)blockIdx.z * ot + (long long)i * oy + j] = v;
        if (v == v) { khi = order_key(v); klo = ~khi; }
    }
    klo = wave_max(klo);
    khi = wave_max(khi);
    if (threadIdx.x == 0) { part[0][threadIdx.y] = klo; part[1][threadIdx.y] = khi; }
    __syncthreads();
    if (threadIdx.x == 0 && threadIdx.y == 0) {
#pragma unroll
        for (int w = 1; w < POL_BY; ++w) {
            klo = part[0][w] > klo ? part[0][w] : klo;
            khi = part[1][w] > khi ? part[1][w] : khi;
        }
        if (klo) atomicMax(rec, klo);
        if (khi) atomicMax(rec + 1, khi);
    }
}

// series i: row i / W, column i % W.  The sum in frame order in fp64, POL_U frames' loads in flight ahead of the chain.  out may be x.
__global__ void __launch_bounds__(256) k_zeromean(const float* x, long long st, long long sy, int W, unsigned nser, int count, float* out,
                                                  long long ot, long long oy)
{
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= nser) return;
    const float* p = x + (long long)(i / (unsigned)W) * sy + (i % (unsigned)W);
    float* o = out + (long long)(i / (unsigned)W) * oy + (i % (unsigned)W);
    double sum = 0.0;
    int t = 0;
    for (; t + POL_U <= count; t += POL_U) {
        float v[POL_U];
#pragma unroll
        for (int u = 0; u < POL_U; ++u) v[u] = p[(long long)(t + u) * st];
#pragma unroll
        for (int u = 0; u < POL_U; ++u) sum += (double)v[u];
    }
    for (; t < count; ++t) sum += (double)p[(long long)t * st];
    const double mean = sum / (double)count;
    for (t = 0; t + POL_U <= count; t += POL_U) {
        float v[POL_U];
#pragma unroll
        for (int u = 0; u < POL_U; ++u) v[u] = p[(long long)(t + u) * st];
#pragma unroll
        for (int u = 0; u < POL_U; ++u) o[(long long)(t + u) * ot] = (float)((double)v[u] - mean);
    }
    for (; t < count; ++t) o[(long long)t * ot] = (float)((double)p[(long long)t * st] - mean);
}

static int cube_ok(wass_ctx* c, const float* in, const float* out, size_t st, size_t sy, size_t ost, size_t osy, int count, int H, int W)
{
    if (!in || !out) return set_err(c, WASS_ERR_INVALID_ARG, "null argument");
    if (count < 1 || H < 1 || W < 1 || H > 65536 || W > 65536 || (size_t)H * W > 0x7fffff00u)
        return set_err(c, WASS_ERR_INVALID_ARG, "a %d x %d x %d cube", count, H, W);
    if (sy < (size_t)W || osy < (size_t)W || (count > 1 && (st < (size_t)W || ost < (size_t)W))) return set_err(c, WASS_ERR_INVALID_ARG, "bad strides");
    return WASS_OK;
}

// the host form stages the frames of a batch, in and out
static int clip_run(wass_ctx* c, bool host, const float* in, size_t st, size_t sy, int count, int H, int W, float lo, float hi, float* out, size_t ost,
                    size_t osy, float* vmin, float* vmax)
{
    if (!c) return WASS_ERR_INVALID_ARG;
    int rc = cube_ok(c, in, out, st, sy, ost, osy, count, H, W);
    if (rc) return rc;
    if (lo != lo || hi != hi) return set_err(c, WASS_ERR_INVALID_ARG, "the bounds of a clip must be numbers");
    WASS_HIP(c, hipSetDevice(c->device));
    hipStream_t s = c->ts();
    const size_t HW = (size_t)H * W;
    size_t b = count < POL_MAX_BATCH ? count : POL_MAX_BATCH;
    if (host)
        while (b > 1 && 256 + 2 * align256(b * HW * 4) > POL_SCRATCH_CAP) b /= 2;
    const size_t stage = host ? align256(b * HW * 4) : 0, total = 256 + 2 * stage;
    Arena mem;
    if ((rc = mem.reserve(c, total, "the clip"))) return rc;
    unsigned* rec = mem.take<unsigned>(256);
    float* sin_ = mem.take<float>(stage);
    float* sout = mem.take<float>(stage);
    hipError_t e = hipMemsetAsync(rec, 0, 256, s);
    const dim3 block(POL_BX, POL_BY);
    for (int t0 = 0; t0 < count && e == hipSuccess; t0 += (int)b) {
        const int nb = count - t0 < (int)b ? count - t0 : (int)b;
        const dim3 grid((W + POL_BX - 1) / POL_BX, (H + POL_BY - 1) / POL_BY, nb);
        if (host) {
            e = upload_rows(sin_, in + (size_t)t0 * st, 4, nb, 0, H, W, st, sy, s);
            if (e != hipSuccess) break;
            hipLaunchKernelGGL(k_clip, grid, block, 0, s, (const float*)sin_, (long long)HW, (long long)W, H, W, lo, hi, sout, (long long)HW, (long long)W, rec);
            e = hipGetLastError();
            if (e == hipSuccess) e = download_rows(out + (size_t)t0 * ost, sout, 4, nb, 0, H, W, ost, osy, s);
        } else {
            hipLaunchKernelGGL(k_clip, grid, block, 0, s, in + (size_t)t0 * st, (long long)st, (long long)sy, H, W, lo, hi, out + (size_t)t0 * ost,
                               (long long)ost, (long long)osy, rec);
            e = hipGetLastError();
        }
    }
    unsigned r[2] = { 0, 0 };
    if (e == hipSuccess) e = hipMemcpyAsync(r, rec, 8, hipMemcpyDeviceToHost, s);
    rc = finish(c, WASS_OK, e, s, "clip");
    if (!rc) {
        if (vmin) *vmin = r[0] ? order_unkey(~r[0]) : NAN;
        if (vmax) *vmax = r[1] ? order_unkey(r[1]) : NAN;
    }
    return rc;
}

// the host form goes in slabs of rows, all frames of a slab staged; a series never crosses a slab
static int zeromean_run(wass_ctx* c, bool host, const float* in, size_t st, size_t sy, int count, int H, int W, float* out, size_t ost, size_t osy)
{
    if (!c) return WASS_ERR_INVALID_ARG;
    int rc = cube_ok(c, in, out, st, sy, ost, osy, count, H, W);
    if (rc) return rc;
    WASS_HIP(c, hipSetDevice(c->device));
    hipStream_t s = c->ts();
    int rows = H;
    if (host && slab_rows(POL_SCRATCH_CAP - 256, (size_t)count * (size_t)W * 4, H, W, 0, &rows))
        return set_err(c, WASS_ERR_NO_MEMORY, "one row of %d frames does not fit the scratch cap of %zu bytes", count, POL_SCRATCH_CAP);
    Arena mem;                                              // the device form: nothing
    const size_t stage_bytes = host ? align256((size_t)count * (size_t)rows * (size_t)W * 4) : 0;
    if ((rc = mem.reserve(c, stage_bytes, "zeromean"))) return rc;
    float* stage = mem.take<float>(stage_bytes);
    hipError_t e = hipSuccess;
    for (int r0 = 0; r0 < H && e == hipSuccess; r0 += rows) {
        const int nr = H - r0 < rows ? H - r0 : rows;
        const unsigned nser = (unsigned)((size_t)nr * W);
        const dim3 grid((nser + 255u) / 256u), block(256);
        if (host) {
            const size_t plane = (size_t)nr * W;
            e = upload_rows(stage, in, 4, count, r0, nr, W, st, sy, s);
            if (e != hipSuccess) break;
            hipLaunchKernelGGL(k_zeromean, grid, block, 0, s, (const float*)stage, (long long)plane, (long long)W, W, nser, count, stage, (long long)plane,
                               (long long)W);
            e = hipGetLastError();
            if (e == hipSuccess) e = download_rows(out, stage, 4, count, r0, nr, W, ost, osy, s);
        } else {
            hipLaunchKernelGGL(k_zeromean, grid, block, 0, s, in, (long long)st, (long long)sy, W, nser, count, out, (long long)ost, (long long)osy);
            e = hipGetLastError();
        }
    }
    return finish(c, WASS_OK, e, s, "zeromean", host);
}

}  // namespace wass

using namespace wass;

extern "C" int wass_bilinear_table_f32(float* out)
{
    if (!out) return WASS_ERR_INVALID_ARG;
    build_bilinear_tab(out);
    return WASS_OK;
}

extern "C" int wass_remap_linear_f32(wass_ctx* c, const float* src, int sw, int sh, size_t src_stride, const float* map_x, const float* map_y, int dw,
                                     int dh, float* dst)
{
    return remap_f32_run(c, true, src, sw, sh, src_stride, map_x, map_y, dw, dh, dst);
}

extern "C" int wass_remap_linear_f32_dev(wass_ctx* c, const float* d_src, int sw, int sh, size_t src_stride, const float* d_map_x,
                                         const float* d_map_y, int dw, int dh, float* d_dst)
{
    return remap_f32_run(c, false, d_src, sw, sh, src_stride, d_map_x, d_map_y, dw, dh, d_dst);
}

extern "C" int wass_polarimetric_scratch_bytes(int count, int H, int W, int Ih, int Iw, int batch, int host, int outputs, size_t* bytes,
                                               int* batch_used)
{
    if (!bytes) return WASS_ERR_INVALID_ARG;
    PolPlan p;
    const int rc = pol_plan(count, H, W, Ih, Iw, batch, host != 0, outputs, p);
    if (rc) return rc;
    *bytes = p.total;
    if (batch_used) *batch_used = p.batch;
    return WASS_OK;
}

extern "C" int wass_polarimetric(wass_ctx* c, const float* stokes, size_t stokes_stride_t, size_t stokes_stride_c, size_t stokes_stride_y, int Ih,
                                 int Iw, const float* in, size_t stride_t, size_t stride_y, int count, int H, int W, const double* XX,
                                 const double* YY, const wass_pol_params* params, double* acc, const wass_pol_out* out, uint64_t* occluded,
                                 uint64_t* not_upward)
{
    return pol_run(c, true, stokes, stokes_stride_t, stokes_stride_c, stokes_stride_y, Ih, Iw, in, stride_t, stride_y, count, H, W, XX, YY, params, acc,
                   out, occluded, not_upward);
}

extern "C" int wass_polarimetric_dev(wass_ctx* c, const float* d_stokes, size_t stokes_stride_t, size_t stokes_stride_c, size_t stokes_stride_y,
                                     int Ih, int Iw, const float* d_in, size_t stride_t, size_t stride_y, int count, int H, int W,
                                     const double* d_XX, const double* d_YY, const wass_pol_params* params, double* d_acc, const wass_pol_out* out,
                                     uint64_t* occluded, uint64_t* not_upward)
{
    return pol_run(c, false, d_stokes, stokes_stride_t, stokes_stride_c, stokes_stride_y, Ih, Iw, d_in, stride_t, stride_y, count, H, W, d_XX, d_YY,
                   params, d_acc, out, occluded, not_upward);
}

extern "C" int wass_clip_cube(wass_ctx* c, const float* in, size_t stride_t, size_t stride_y, int count, int H, int W, float lo, float hi, float* out,
                              size_t out_stride_t, size_t out_stride_y, float* vmin, float* vmax)
{
    return clip_run(c, true, in, stride_t, stride_y, count, H, W, lo, hi, out, out_stride_t, out_stride_y, vmin, vmax);
}

extern "C" int wass_clip_cube_dev(wass_ctx* c, const float* d_in, size_t stride_t, size_t stride_y, int count, int H, int W, float lo, float hi,
                                  float* d_out, size_t out_stride_t, size_t out_stride_y, float* vmin, float* vmax)
{
    return clip_run(c, false, d_in, stride_t, stride_y, count, H, W, lo, hi, d_out, out_stride_t, out_stride_y, vmin, vmax);
}

extern "C" int wass_zeromean(wass_ctx* c, const float* in, size_t stride_t, size_t stride_y, int count, int H, int W, float* out,
                             size_t out_stride_t, size_t out_stride_y)
{
    return zeromean_run(c, true, in, stride_t, stride_y, count, H, W, out, out_stride_t, out_stride_y);
}

extern "C" int wass_zeromean_dev(wass_ctx* c, const float* d_in, size_t stride_t, size_t stride_y, int count, int H, int W, float* d_out,
                                 size_t out_stride_t, size_t out_stride_y)
{
    return zeromean_run(c, false, d_in, stride_t, stride_y, count, H, W, d_out, out_stride_t, out_stride_y);
}
