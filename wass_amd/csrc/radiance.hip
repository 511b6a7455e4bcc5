// radiance.hip -- wasspost's radiance chain as array functions: `radiance` (postproc/wasspost/wasspost.py:813-919), `bgimage`
// (:1010-1074) and `radiance_threshold` (:1079-1145).
//
//   k_remap_lanczos4  cv::remap(u8, CV_32FC1 maps, INTER_LANCZOS4, BORDER_CONSTANT 0) restated as rectify.hip restates the cubic
//                     one: coordinates quantised to 1/32 pixel (float product, round half to even), the 64 int16 weights of the
//                     phase from a 1024 x 8 x 8 table (OpenCV's initInterTab2D with its sum fix-up), int32 sum,
//                     (v + 2^14) >> 15 clamped to 0 .. 255, taps outside the picture contribute 0.  OpenCV is absent here, so the
//                     table and the pipeline are written from knowledge of OpenCV 4.5.5's imgwarp.cpp: PARITY UNPINNED against
//                     OpenCV, bit-exact against the numpy restatement of tests/radiance_oracle.py.
//   k_radiance        the same sampler behind the projection of the grid: per cell zf = Z * (float)datascale in float32,
//                     r_k = ((P[k][0] X + P[k][1] Y) + P[k][2] zf) + P[k][3] in fp64 (no contraction: -ffp-contract=off),
//                     mapx = (float)(r_0 / r_2), mapy = (float)(r_1 / r_2); out = u8 / 255 in float32.  No map array is written.
//   Where OpenCV is undefined: a map value that is NaN, infinite or whose product with 32 is outside the int32 range gives 0 (x86's
//   cvRound yields INT_MIN there, which lands outside the picture as well).
//   k_bgimage         scipy.ndimage.uniform_filter1d(x, size, axis=0, mode='reflect') of a float32 cube: one lane per series,
//                     consecutive lanes along x, the running sum in fp64 and UNdivided (out[t] = (float)(sum / size), as scipy
//                     1.15 does), reflected indices computed per step (they are wave-uniform), BG_U steps' loads in flight ahead of
//                     the chain.  Rows go in slabs under the scratch cap; a series never crosses a slab.  No atomics.
//   k_thr_*           Isub = I - (Ibg - min(Ibg)) in float32; per frame the minimum of Ibg, the range of Isub, the 30-bin histogram
//                     of Isub against 31 given float32 edges (numpy's rule: left edge inclusive, last bin closed) and the mask
//                     Isub > thr.  Integer atomics only (reduce.h's ordered keys and block maximum): the same input gives the same bits.
// Host side: every *_plan keeps its byte formula; the batch and slab rules, the scratch, the staging of a host batch or slab
// (pictures too: they are cubes of bytes) and the end of a call are cube.h's.
#include "common.h"
#include "cube.h"

#include <cfloat>
#include <cmath>
#include <vector>

namespace wass {

constexpr size_t RAD_SCRATCH_CAP = (size_t)16 << 30;    // bytes one call may allocate
constexpr int RAD_MAX_BATCH = 1024;                     // frames per launch (blockIdx.z)
constexpr int RAD_DEFAULT_BATCH = 8;
constexpr int RAD_BX = 64, RAD_BY = 4;                  // a block: 4 waves, each 64 cells of one row
constexpr int RAD_BITS = 5, RAD_TAB = 1 << RAD_BITS, RAD_TAB2 = RAD_TAB * RAD_TAB, RAD_COEF = 1 << 15;
constexpr int BG_U = 8;                                 // time steps loaded ahead of the running sum
constexpr int THR_BINS = 30;

// ---------------------------------------------------------------- the Lanczos4 table (imgwarp.cpp interpolateLanczos4, initInterTab2D)
static void lanczos4_1d(float x, float* c)
{
    static const double s45 = 0.70710678118654752440084436210485;
    static const double cs[8][2] = { { 1, 0 }, { -s45, -s45 }, { 0, 1 }, { s45, -s45 }, { -1, 0 }, { s45, s45 }, { 0, -1 }, { -s45, s45 } };
    if (x < FLT_EPSILON) {
        for (int i = 0; i < 8; ++i) c[i] = 0.f;
        c[3] = 1.f;
        return;
    }
    float sum = 0.f;
    const double y0 = -(x + 3) * 3.1415926535897932384626433832795 * 0.25, s0 = sin(y0), c0 = cos(y0);
    for (int i = 0; i < 8; ++i) {
        const double y = -(x + 3 - i) * 3.1415926535897932384626433832795 * 0.25;
        c[i] = (float)((cs[i][0] * s0 + cs[i][1] * c0) / (y * y));
        sum += c[i];
    }
    sum = 1.f / sum;
    for (int i = 0; i < 8; ++i) c[i] *= sum;
}

static short rad_sat_short(float v)
{
    const long r = lrintf(v);      // cvRound: nearest even
    return (short)(r < -32768 ? -32768 : r > 32767 ? 32767 : r);
}

// tab[(fy * 32 + fx) * 64 + ky * 8 + kx]; the fix-up scans OpenCV's window [ksize / 2, ksize / 2 + 2), taps 4 .. 5 of 8
static void build_lanczos4_tab(short* tab)
{
    constexpr int K = 8, KK = 64;
    float t1[RAD_TAB * K];
    const float scale = 1.f / RAD_TAB;
    for (int i = 0; i < RAD_TAB; ++i) lanczos4_1d(i * scale, t1 + i * K);
    for (int i = 0; i < RAD_TAB; ++i)
        for (int j = 0; j < RAD_TAB; ++j) {
            short* it = tab + (size_t)(i * RAD_TAB + j) * KK;
            int isum = 0;
            for (int k1 = 0; k1 < K; ++k1) {
                const float vy = t1[i * K + k1];
                for (int k2 = 0; k2 < K; ++k2) {
                    const float v = vy * t1[j * K + k2];
                    isum += it[k1 * K + k2] = rad_sat_short(v * RAD_COEF);
                }
            }
            if (isum != RAD_COEF) {
                const int diff = isum - RAD_COEF, k0 = K / 2;
                int Mk1 = k0, Mk2 = k0, mk1 = k0, mk2 = k0;
                for (int k1 = k0; k1 < k0 + 2; ++k1)
                    for (int k2 = k0; k2 < k0 + 2; ++k2) {
                        if (it[k1 * K + k2] < it[mk1 * K + mk2]) { mk1 = k1; mk2 = k2; }
                        else if (it[k1 * K + k2] > it[Mk1 * K + Mk2]) { Mk1 = k1; Mk2 = k2; }
                    }
                if (diff < 0) it[Mk1 * K + Mk2] = (short)(it[Mk1 * K + Mk2] - diff);
                else it[mk1 * K + mk2] = (short)(it[mk1 * K + mk2] - diff);
            }
        }
}

constexpr size_t LANCZOS_TAB_BYTES = (size_t)RAD_TAB2 * 64 * sizeof(short);      // 128 KiB

static int ensure_lanczos_tab(wass_ctx* c)
{
    if (c->lanczos_tab_ready) return WASS_OK;
    int rc = ensure(c, c->lanczos_tab, LANCZOS_TAB_BYTES);
    if (rc) return rc;
    std::vector<short> tab((size_t)RAD_TAB2 * 64);
    build_lanczos4_tab(tab.data());
    WASS_HIP(c, hipMemcpy(c->lanczos_tab.p, tab.data(), LANCZOS_TAB_BYTES, hipMemcpyHostToDevice));
    c->lanczos_tab_ready = true;
    return WASS_OK;
}

// ---------------------------------------------------------------- the sampler
__device__ __forceinline__ int rad_sat_s16(int v) { return v < -32768 ? -32768 : v > 32767 ? 32767 : v; }

// q = cvRound(m * 32) where that is defined: the float product is finite and inside the int32 range
__device__ __forceinline__ bool rad_quant(float m, int& q)
{
    const float p = m * (float)RAD_TAB;
    if (!(fabsf(p) < 2147483648.f)) return false;       // NaN, infinite or out of range
    q = __float2int_rn(p);
    return true;
}

// the 8 weights of row i of a phase: 16 bytes, aligned
__device__ __forceinline__ void rad_wrow(const short* __restrict__ w, int i, int (&k)[8])
{
    const uint4 r = reinterpret_cast<const uint4*>(w)[i];
    k[0] = (short)(r.x & 0xffffu); k[1] = (int)r.x >> 16;
    k[2] = (short)(r.y & 0xffffu); k[3] = (int)r.y >> 16;
    k[4] = (short)(r.z & 0xffffu); k[5] = (int)r.z >> 16;
    k[6] = (short)(r.w & 0xffffu); k[7] = (int)r.w >> 16;
}

// remapLanczos4 (imgwarp.cpp), BORDER_CONSTANT 0; (sx, sy) is the integer source position (tap 3 of 8)
__device__ __forceinline__ uint8_t sample_lanczos4(const uint8_t* __restrict__ src, int sw, int sh, size_t ss, int sx, int sy,
                                                   const short* __restrict__ w)
{
    sx -= 3; sy -= 3;
    int sum = 0, k[8];
    if ((unsigned)sx < (unsigned)max(sw - 7, 0) && (unsigned)sy < (unsigned)max(sh - 7, 0)) {
        const uint8_t* s = src + (size_t)sy * ss + sx;
#pragma unroll
        for (int i = 0; i < 8; ++i, s += ss) {
            rad_wrow(w, i, k);
#pragma unroll
            for (int j = 0; j < 8; ++j) sum += s[j] * k[j];
        }
    } else {
        if (sx >= sw || sx + 8 <= 0 || sy >= sh || sy + 8 <= 0) return 0;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int yy = sy + i;
            if ((unsigned)yy >= (unsigned)sh) continue;
            rad_wrow(w, i, k);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int xx = sx + j;
                if ((unsigned)xx < (unsigned)sw) sum += src[(size_t)yy * ss + xx] * k[j];
            }
        }
    }
    sum = (sum + (1 << 14)) >> 15;
    return (uint8_t)(sum < 0 ? 0 : sum > 255 ? 255 : sum);
}

__device__ __forceinline__ uint8_t remap_lanczos4_at(const uint8_t* __restrict__ src, int sw, int sh, size_t ss, float mx, float my,
                                                     const short* __restrict__ tab)
{
    int X, Y;
    if (!rad_quant(mx, X) || !rad_quant(my, Y)) return 0;
    const int sx = rad_sat_s16(X >> RAD_BITS), sy = rad_sat_s16(Y >> RAD_BITS);
    const int a = (Y & (RAD_TAB - 1)) * RAD_TAB + (X & (RAD_TAB - 1));
    return sample_lanczos4(src, sw, sh, ss, sx, sy, tab + (size_t)a * 64);
}

__global__ void __launch_bounds__(RAD_BX * RAD_BY) k_remap_lanczos4(const uint8_t* __restrict__ src, int sw, int sh, size_t ss,
                                                                    const float* __restrict__ mx, const float* __restrict__ my, int dw, int dh,
                                                                    uint8_t* __restrict__ dst, const short* __restrict__ tab)
{
    const int x = blockIdx.x * RAD_BX + threadIdx.x, y = blockIdx.y * RAD_BY + threadIdx.y;
    if (x >= dw || y >= dh) return;
    const size_t i = (size_t)y * dw + x;
    dst[i] = remap_lanczos4_at(src, sw, sh, ss, mx[i], my[i], tab);
}

struct RadProj { double p[12]; float scale; };          // Pcam, row-major 3 x 4; (float)datascale

__global__ void __launch_bounds__(RAD_BX * RAD_BY) k_radiance(const uint8_t* __restrict__ img, size_t img_t, size_t img_y, int sw, int sh,
                                                              const float* __restrict__ Z, long long st, long long sy, int H, int W,
                                                              const double* __restrict__ XX, const double* __restrict__ YY, const RadProj P,
                                                              float* __restrict__ out, const short* __restrict__ tab)
{
    const int j = blockIdx.x * RAD_BX + threadIdx.x, i = blockIdx.y * RAD_BY + threadIdx.y;
    if (i >= H || j >= W) return;
    const size_t f = blockIdx.z, c = (size_t)i * W + j;
    const float zf = Z[(long long)f * st + (long long)i * sy + j] * P.scale;
    const double X = XX[c], Y = YY[c], z = (double)zf;
    const double r0 = ((P.p[0] * X + P.p[1] * Y) + P.p[2] * z) + P.p[3];
    const double r1 = ((P.p[4] * X + P.p[5] * Y) + P.p[6] * z) + P.p[7];
    const double r2 = ((P.p[8] * X + P.p[9] * Y) + P.p[10] * z) + P.p[11];
    const float mx = (float)(r0 / r2), my = (float)(r1 / r2);
    const uint8_t v = remap_lanczos4_at(img + f * img_t, sw, sh, img_y, mx, my, tab);
    // a float32 quotient of two float32 values formed in fp64 and rounded once more is the correctly rounded float32 quotient
    out[f * (size_t)H * W + c] = (float)((double)v / 255.0);
}

static int rad_picture_ok(wass_ctx* c, int sw, int sh, size_t ss)
{
    if (sw < 1 || sh < 1 || sw >= 32767 || sh >= 32767 || ss < (size_t)sw)
        return set_err(c, WASS_ERR_INVALID_ARG, "a %d x %d picture with a row stride of %zu (sides from 1 to 32766)", sw, sh, ss);
    return WASS_OK;
}

static int remap_run(wass_ctx* c, bool host, const uint8_t* src, int sw, int sh, size_t ss, const float* mx, const float* my, int dw, int dh,
                     uint8_t* dst)
{
    if (!c) return WASS_ERR_INVALID_ARG;
    if (!src || !mx || !my || !dst) return set_err(c, WASS_ERR_INVALID_ARG, "null argument");
    int rc = rad_picture_ok(c, sw, sh, ss);
    if (rc) return rc;
    if (dw < 1 || dh < 1 || dw > 65536 || dh > 65536) return set_err(c, WASS_ERR_INVALID_ARG, "a %d x %d output", dw, dh);
    WASS_HIP(c, hipSetDevice(c->device));
    rc = ensure_lanczos_tab(c);
    if (rc) return rc;
    hipStream_t s = c->ts();
    const size_t n = (size_t)dw * dh, src_bytes = align256((size_t)sh * sw);
    Arena mem;
    const uint8_t* dsrc = src;
    const float *dmx = mx, *dmy = my;
    uint8_t* ddst = dst;
    size_t dss = ss;
    hipError_t e = hipSuccess;
    if (host) {
        if ((rc = mem.reserve(c, src_bytes + 2 * align256(n * 4) + align256(n), "the remap"))) return rc;
        uint8_t* a = mem.take<uint8_t>(src_bytes);
        float* b = mem.take<float>(n * 4);
        float* d = mem.take<float>(n * 4);
        ddst = mem.take<uint8_t>(n);
        e = upload_rows(a, src, 1, 1, 0, sh, sw, 0, ss, s);
        if (e == hipSuccess) e = hipMemcpyAsync(b, mx, n * 4, hipMemcpyHostToDevice, s);
        if (e == hipSuccess) e = hipMemcpyAsync(d, my, n * 4, hipMemcpyHostToDevice, s);
        dsrc = a; dmx = b; dmy = d; dss = (size_t)sw;
    }
    if (e == hipSuccess) {
        const dim3 block(RAD_BX, RAD_BY), grid((dw + RAD_BX - 1) / RAD_BX, (dh + RAD_BY - 1) / RAD_BY);
        hipLaunchKernelGGL(k_remap_lanczos4, grid, block, 0, s, dsrc, sw, sh, dss, dmx, dmy, dw, dh, ddst, (const short*)c->lanczos_tab.p);
        e = hipGetLastError();
        if (e == hipSuccess && host) e = hipMemcpyAsync(dst, ddst, n, hipMemcpyDeviceToHost, s);
    }
    return finish(c, WASS_OK, e, s, "remap_lanczos4", host);
}

struct RadPlan {
    int batch = 0;
    size_t grid_bytes = 0, img_bytes = 0, z_bytes = 0, out_bytes = 0, total = 0;
};

// the device form needs no scratch at all; the host form stages XX, YY and, per frame of a batch, the picture, the heights and the result
static int rad_plan(int count, int H, int W, int Ih, int Iw, int batch, bool host, RadPlan& p)
{
    if (count < 1 || H < 1 || W < 1 || batch < 0 || H > 65536 || W > 65536 || Ih < 1 || Iw < 1 || Ih >= 32767 || Iw >= 32767)
        return WASS_ERR_INVALID_ARG;
    const size_t HW = (size_t)H * W;
    if (HW > 0x7fffff00u) return WASS_ERR_UNSUPPORTED;
    p.grid_bytes = host ? 2 * align256(HW * 8) : 0;
    p.batch = fit_batch(batch, RAD_DEFAULT_BATCH, RAD_MAX_BATCH, count, RAD_SCRATCH_CAP, [&](int b) {
        p.img_bytes = host ? align256((size_t)b * Ih * Iw) : 0;
        p.z_bytes = host ? align256((size_t)b * HW * 4) : 0;
        p.out_bytes = p.z_bytes;
        return p.total = p.grid_bytes + p.img_bytes + p.z_bytes + p.out_bytes;
    });
    return p.batch ? WASS_OK : WASS_ERR_NO_MEMORY;
}

static int rad_run(wass_ctx* c, bool host, const uint8_t* img, size_t img_t, size_t img_y, int Ih, int Iw, const float* in, size_t st, size_t sy,
                   int count, int H, int W, const double* XX, const double* YY, const double* Pcam, double datascale, int batch, float* out)
{
    if (!c) return WASS_ERR_INVALID_ARG;
    if (!img || !in || !XX || !YY || !Pcam || !out) return set_err(c, WASS_ERR_INVALID_ARG, "null argument");
    RadPlan p;
    int rc = rad_plan(count, H, W, Ih, Iw, batch, host, p);
    if (rc) return set_err(c, rc, "cannot plan the radiance of a %d x %d x %d cube from %d x %d pictures under the scratch cap of %zu bytes", count, H,
                           W, Ih, Iw, RAD_SCRATCH_CAP);
    if (sy < (size_t)W || img_y < (size_t)Iw || (count > 1 && (st < (size_t)W || img_t < (size_t)Iw))) return set_err(c, WASS_ERR_INVALID_ARG, "bad strides");
    WASS_HIP(c, hipSetDevice(c->device));
    rc = ensure_lanczos_tab(c);
    if (rc) return rc;
    hipStream_t s = c->ts();
    RadProj P;
    for (int k = 0; k < 12; ++k) P.p[k] = Pcam[k];
    P.scale = (float)datascale;
    const size_t HW = (size_t)H * W, II = (size_t)Ih * Iw;
    Arena mem;                                              // the device form: nothing
    if ((rc = mem.reserve(c, p.total, "the radiance scratch"))) return rc;
    double* sXX = mem.take<double>(p.grid_bytes / 2);
    double* sYY = mem.take<double>(p.grid_bytes / 2);
    uint8_t* simg = mem.take<uint8_t>(p.img_bytes);
    float* sz = mem.take<float>(p.z_bytes);
    float* sout = mem.take<float>(p.out_bytes);
    const double *dXX = XX, *dYY = YY;
    hipError_t e = hipSuccess;
    if (host) {
        e = hipMemcpyAsync(sXX, XX, HW * 8, hipMemcpyHostToDevice, s);
        if (e == hipSuccess) e = hipMemcpyAsync(sYY, YY, HW * 8, hipMemcpyHostToDevice, s);
        dXX = sXX; dYY = sYY;
    }
    const dim3 block(RAD_BX, RAD_BY);
    for (int t0 = 0; t0 < count && e == hipSuccess; t0 += p.batch) {
        const int nb = count - t0 < p.batch ? count - t0 : p.batch;
        const dim3 grid((W + RAD_BX - 1) / RAD_BX, (H + RAD_BY - 1) / RAD_BY, nb);
        const uint8_t* im = img + (size_t)t0 * img_t;
        size_t it = img_t, iy = img_y;
        const float* zin = in + (size_t)t0 * st;
        long long zst = (long long)st, zsy = (long long)sy;
        float* o = out + (size_t)t0 * HW;
        if (host) {
            e = upload_rows(simg, im, 1, nb, 0, Ih, Iw, img_t, img_y, s);
            if (e == hipSuccess) e = upload_rows(sz, zin, 4, nb, 0, H, W, st, sy, s);
            if (e != hipSuccess) break;
            im = simg; it = II; iy = (size_t)Iw; zin = sz; zst = (long long)HW; zsy = W; o = sout;
        }
        hipLaunchKernelGGL(k_radiance, grid, block, 0, s, im, it, iy, Iw, Ih, zin, zst, zsy, H, W, dXX, dYY, P, o, (const short*)c->lanczos_tab.p);
        e = hipGetLastError();
        if (e == hipSuccess && host) e = hipMemcpyAsync(out + (size_t)t0 * HW, sout, (size_t)nb * HW * 4, hipMemcpyDeviceToHost, s);
    }
    return finish(c, WASS_OK, e, s, "radiance", host);
}

// k_radiance for nb frames of device memory on stream s, for pyramid.hip: the heights arrive as the caller formed them and are
// multiplied by `scale` (1 leaves them as they are)
int radiance_enqueue(wass_ctx* c, const uint8_t* d_img, size_t img_t, size_t img_y, int Ih, int Iw, const float* d_z, size_t st, size_t sy, int nb,
                     int H, int W, const double* d_XX, const double* d_YY, const double* Pcam, float scale, float* d_out, hipStream_t s)
{
    int rc = rad_picture_ok(c, Iw, Ih, img_y);
    if (rc) return rc;
    if (nb < 1 || nb > RAD_MAX_BATCH || H < 1 || W < 1 || H > 65536 || W > 65536 || (size_t)H * W > 0x7fffff00u || sy < (size_t)W)
        return set_err(c, WASS_ERR_INVALID_ARG, "%d frames of %d x %d", nb, H, W);
    rc = ensure_lanczos_tab(c);
    if (rc) return rc;
    RadProj P;
    for (int k = 0; k < 12; ++k) P.p[k] = Pcam[k];
    P.scale = scale;
    const dim3 block(RAD_BX, RAD_BY), grid((W + RAD_BX - 1) / RAD_BX, (H + RAD_BY - 1) / RAD_BY, nb);
    hipLaunchKernelGGL(k_radiance, grid, block, 0, s, d_img, img_t, img_y, Iw, Ih, d_z, (long long)st, (long long)sy, H, W, d_XX, d_YY, P, d_out,
                       (const short*)c->lanczos_tab.p);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? WASS_OK : set_err(c, WASS_ERR_DEVICE, "radiance: %s", hipGetErrorString(e));
}

// ---------------------------------------------------------------- bgimage: the box filter along time
// `reflect` of scipy.ndimage (d c b a | a b c d | d c b a): phase a in [0, 2 n) stands for index a or 2 n - 1 - a
struct BgPhase {
    int a, n;
    __device__ __forceinline__ BgPhase(long long k, int n_) : n(n_)
    {
        const long long per = 2ll * n_;
        long long m = k % per;
        a = (int)(m < 0 ? m + per : m);
    }
    __device__ __forceinline__ int next()               // the index of this phase; then one step on
    {
        const int i = a < n ? a : 2 * n - 1 - a;
        a = a + 1 == 2 * n ? 0 : a + 1;
        return i;
    }
};

// series i of the slab: row i / W, column i % W of x (element strides st, sy); out likewise (ot, oy).  The window at t covers
// t - size / 2 .. t + size - size / 2 - 1.
__global__ void __launch_bounds__(256) k_bgimage(const float* __restrict__ x, long long st, long long sy, int W, unsigned nser, int count, int size,
                                                 float* __restrict__ out, long long ot, long long oy)
{
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= nser) return;
    const float* __restrict__ p = x + (long long)(i / (unsigned)W) * sy + (i % (unsigned)W);
    float* __restrict__ o = out + (long long)(i / (unsigned)W) * oy + (i % (unsigned)W);
    const int size1 = size / 2;
    const double dsize = (double)size;
    double tmp = 0.0;
    {
        BgPhase ph(-(long long)size1, count);
        int k = 0;
        for (; k + BG_U <= size; k += BG_U) {
            float v[BG_U];
#pragma unroll
            for (int u = 0; u < BG_U; ++u) v[u] = p[(long long)ph.next() * st];
#pragma unroll
            for (int u = 0; u < BG_U; ++u) tmp += (double)v[u];
        }
        for (; k < size; ++k) tmp += (double)p[(long long)ph.next() * st];
    }
    o[0] = (float)(tmp / dsize);
    BgPhase pn((long long)size - size1, count), po(-(long long)size1, count);    // the sample that enters at t = 1, the one that leaves
    float cn[BG_U], co[BG_U], nn[BG_U], no[BG_U];
    const int n = count - 1;                            // steps t = 1 .. count - 1
    int j = 0;
    if (n >= BG_U) {
#pragma unroll
        for (int u = 0; u < BG_U; ++u) {
            cn[u] = p[(long long)pn.next() * st];
            co[u] = p[(long long)po.next() * st];
        }
    }
    for (; j + BG_U <= n; j += BG_U) {
        const bool more = j + 2 * BG_U <= n;
        if (more) {
#pragma unroll
            for (int u = 0; u < BG_U; ++u) {
                nn[u] = p[(long long)pn.next() * st];
                no[u] = p[(long long)po.next() * st];
            }
        }
#pragma unroll
        for (int u = 0; u < BG_U; ++u) {
            tmp += (double)cn[u] - (double)co[u];
            o[(long long)(1 + j + u) * ot] = (float)(tmp / dsize);
        }
        if (more) {
#pragma unroll
            for (int u = 0; u < BG_U; ++u) {
                cn[u] = nn[u];
                co[u] = no[u];
            }
        }
    }
    for (; j < n; ++j) {
        const float a = p[(long long)pn.next() * st], b = p[(long long)po.next() * st];
        tmp += (double)a - (double)b;
        o[(long long)(1 + j) * ot] = (float)(tmp / dsize);
    }
}

struct BgPlan {
    int rows = 0;
    size_t stage_bytes = 0, total = 0;                  // the host form stages the slab and its result; the device form needs nothing
};

static int bg_plan(int count, int H, int W, int size, int slab, bool host, BgPlan& p)
{
    if (count < 1 || H < 1 || W < 1 || size < 1 || slab < 0) return WASS_ERR_INVALID_ARG;
    const int rc = slab_rows(RAD_SCRATCH_CAP - 512, host ? (size_t)count * (size_t)W * 4 * 2 : 0, H, W, slab, &p.rows);
    if (rc) return rc;
    p.stage_bytes = host ? align256((size_t)count * (size_t)p.rows * (size_t)W * 4) : 0;
    p.total = 2 * p.stage_bytes;
    return WASS_OK;
}

static int bg_run(wass_ctx* c, bool host, const float* in, size_t st, size_t sy, int count, int H, int W, int size, int slab_rows, float* out,
                  size_t ost, size_t osy)
{
    if (!c) return WASS_ERR_INVALID_ARG;
    if (!in || !out) return set_err(c, WASS_ERR_INVALID_ARG, "null argument");
    BgPlan p;
    int rc = bg_plan(count, H, W, size, slab_rows, host, p);
    if (rc) return set_err(c, rc, "cannot plan a box filter of %d frames over a %d x %d x %d cube under the scratch cap of %zu bytes", size, count, H, W,
                           RAD_SCRATCH_CAP);
    if (sy < (size_t)W || osy < (size_t)W || (count > 1 && (st < (size_t)W || ost < (size_t)W))) return set_err(c, WASS_ERR_INVALID_ARG, "bad strides");
    if (!host && in == out) return set_err(c, WASS_ERR_INVALID_ARG, "the box filter cannot work in place");
    WASS_HIP(c, hipSetDevice(c->device));
    hipStream_t s = c->ts();
    Arena mem;                                              // the device form: nothing
    if ((rc = mem.reserve(c, p.total, "the box filter"))) return rc;
    float* stage = mem.take<float>(p.stage_bytes);
    float* sout = mem.take<float>(p.stage_bytes);
    hipError_t e = hipSuccess;
    for (int r0 = 0; r0 < H && e == hipSuccess; r0 += p.rows) {
        const int rows = H - r0 < p.rows ? H - r0 : p.rows;
        const unsigned nser = (unsigned)((size_t)rows * W);
        const dim3 grid((nser + 255u) / 256u), block(256);
        if (host) {
            const size_t plane = (size_t)rows * W;
            e = upload_rows(stage, in, 4, count, r0, rows, W, st, sy, s);
            if (e != hipSuccess) break;
            hipLaunchKernelGGL(k_bgimage, grid, block, 0, s, (const float*)stage, (long long)plane, (long long)W, W, nser, count, size, sout,
                               (long long)plane, (long long)W);
            e = hipGetLastError();
            if (e == hipSuccess) e = download_rows(out, sout, 4, count, r0, rows, W, ost, osy, s);
        } else {
            hipLaunchKernelGGL(k_bgimage, grid, block, 0, s, in + (size_t)r0 * sy, (long long)st, (long long)sy, W, nser, count, size,
                               out + (size_t)r0 * osy, (long long)ost, (long long)osy);
            e = hipGetLastError();
        }
    }
    return finish(c, WASS_OK, e, s, "box filter", host);
}

// ---------------------------------------------------------------- radiance_threshold
// per frame 8 words: [0] ~key of min(Ibg)  [1] ~key of min(Isub)  [2] key of max(Isub)  [3] cells of Isub that are not finite
// [4] cells of Ibg that are NaN.  All start at 0.
constexpr int THR_WORDS = 8;

__global__ void __launch_bounds__(RAD_BX * RAD_BY) k_thr_bgmin(const float* __restrict__ B, long long bt, long long by, int H, int W,
                                                               unsigned* __restrict__ rec)
{
    const int j = blockIdx.x * RAD_BX + threadIdx.x, i = blockIdx.y * RAD_BY + threadIdx.y;
    unsigned* r = rec + (size_t)blockIdx.z * THR_WORDS;
    unsigned k = 0;
    bool nan = false;
    if (i < H && j < W) {
        const float v = B[(long long)blockIdx.z * bt + (long long)i * by + j];
        nan = v != v;
        if (!nan) k = ~order_key(v);
    }
    const unsigned long long wn = __ballot(nan);
    if (wn && threadIdx.x == 0) atomicAdd(r + 4, (unsigned)__popcll(wn));
    block_max<RAD_BY>(k, r);
}

__device__ __forceinline__ float thr_bgmin(const unsigned* r)
{
    if (r[4]) return __uint_as_float(0x7fc00000u);      // np.amin of a frame with a NaN
    return order_unkey(~r[0]);
}

__global__ void __launch_bounds__(RAD_BX * RAD_BY) k_thr_range(const float* __restrict__ I, long long it, long long iy,
                                                               const float* __restrict__ B, long long bt, long long by, int H, int W,
                                                               unsigned* __restrict__ rec)
{
    const int j = blockIdx.x * RAD_BX + threadIdx.x, i = blockIdx.y * RAD_BY + threadIdx.y;
    unsigned* r = rec + (size_t)blockIdx.z * THR_WORDS;
    const float m = thr_bgmin(r);
    unsigned klo = 0, khi = 0;
    bool bad = false;
    if (i < H && j < W) {
        const float v = I[(long long)blockIdx.z * it + (long long)i * iy + j] - (B[(long long)blockIdx.z * bt + (long long)i * by + j] - m);
        bad = !(fabsf(v) <= 3.402823466e38f);
        if (!bad) { khi = order_key(v); klo = ~khi; }
    }
    const unsigned long long wb = __ballot(bad);
    if (wb && threadIdx.x == 0) atomicAdd(r + 3, (unsigned)__popcll(wb));
    block_max<RAD_BY>(klo, r + 1);
    block_max<RAD_BY>(khi, r + 2);
}

// counts[f][30] += the histogram of Isub of frame f against edges[f][31]; m[f] = min(Ibg)
__global__ void __launch_bounds__(RAD_BX * RAD_BY) k_thr_hist(const float* __restrict__ I, long long it, long long iy, const float* __restrict__ B,
                                                              long long bt, long long by, int H, int W, const float* __restrict__ mv,
                                                              const float* __restrict__ edges, unsigned* __restrict__ counts)
{
    __shared__ float e[THR_BINS + 1];
    __shared__ unsigned h[THR_BINS];
    const int j = blockIdx.x * RAD_BX + threadIdx.x, i = blockIdx.y * RAD_BY + threadIdx.y;
    const int tid = threadIdx.y * RAD_BX + threadIdx.x;
    if (tid <= THR_BINS) e[tid] = edges[(size_t)blockIdx.z * (THR_BINS + 1) + tid];
    if (tid < THR_BINS) h[tid] = 0;
    __syncthreads();
    if (i < H && j < W) {
        const float m = mv[blockIdx.z];
        const float v = I[(long long)blockIdx.z * it + (long long)i * iy + j] - (B[(long long)blockIdx.z * bt + (long long)i * by + j] - m);
        const float e0 = e[0], e1 = e[THR_BINS];
        if (v >= e0 && v <= e1) {
            const float fi = ((v - e0) / (e1 - e0)) * (float)THR_BINS;
            int b = fi >= 0.f ? (fi < (float)THR_BINS ? (int)fi : THR_BINS - 1) : 0;
            while (b > 0 && v < e[b]) --b;              // numpy corrects its estimate against the edges, and so the edges decide
            while (b < THR_BINS - 1 && v >= e[b + 1]) ++b;
            atomicAdd(&h[b], 1u);
        }
    }
    __syncthreads();
    if (tid < THR_BINS && h[tid]) atomicAdd(counts + (size_t)blockIdx.z * THR_BINS + tid, h[tid]);
}

__global__ void __launch_bounds__(RAD_BX * RAD_BY) k_thr_mask(const float* __restrict__ I, long long it, long long iy, const float* __restrict__ B,
                                                              long long bt, long long by, int H, int W, const float* __restrict__ mv,
                                                              const float* __restrict__ thr, unsigned char* __restrict__ mask)
{
    const int j = blockIdx.x * RAD_BX + threadIdx.x, i = blockIdx.y * RAD_BY + threadIdx.y;
    if (i >= H || j >= W) return;
    const float m = mv[blockIdx.z];
    const float v = I[(long long)blockIdx.z * it + (long long)i * iy + j] - (B[(long long)blockIdx.z * bt + (long long)i * by + j] - m);
    mask[((size_t)blockIdx.z * H + i) * W + j] = v > thr[blockIdx.z] ? 1 : 0;
}

struct ThrPlan {
    int batch = 0;
    size_t head_bytes = 0, stage_bytes = 0, mask_bytes = 0, total = 0;
};

// head: per frame of the cube the 8-word record, min(Ibg), the threshold, 31 edges and 30 counts; the host form stages I, Ibg and
// the mask per frame of a batch
static int thr_plan(int count, int H, int W, int batch, bool host, ThrPlan& p)
{
    if (count < 1 || H < 1 || W < 1 || batch < 0 || H > 65536 || W > 65536) return WASS_ERR_INVALID_ARG;
    const size_t HW = (size_t)H * W;
    if (HW > 0x7fffff00u) return WASS_ERR_UNSUPPORTED;
    p.head_bytes = align256((size_t)count * THR_WORDS * 4) + 2 * align256((size_t)count * 4) + align256((size_t)count * (THR_BINS + 1) * 4) +
                   align256((size_t)count * THR_BINS * 4);
    p.batch = fit_batch(batch, RAD_DEFAULT_BATCH, RAD_MAX_BATCH, count, RAD_SCRATCH_CAP, [&](int b) {
        p.stage_bytes = host ? align256((size_t)b * HW * 4) : 0;
        p.mask_bytes = host ? align256((size_t)b * HW) : 0;
        return p.total = p.head_bytes + 2 * p.stage_bytes + p.mask_bytes;
    });
    return p.batch ? WASS_OK : WASS_ERR_NO_MEMORY;
}

enum ThrMode { THR_RANGE, THR_HIST, THR_MASK };

struct ThrIO {
    const float* m_in = nullptr;       // HIST, MASK: min(Ibg) per frame (host)
    const float* edges = nullptr;      // HIST: count x 31 (host)
    const float* thr = nullptr;        // MASK: count (host)
    float *m_out = nullptr, *lo = nullptr, *hi = nullptr;   // RANGE (host)
    unsigned* nonfinite = nullptr;     // RANGE (host)
    unsigned* counts = nullptr;        // HIST: count x 30 (host)
    unsigned char* mask = nullptr;     // MASK: count x H x W, host or device like the cube
};

static int thr_run(wass_ctx* c, bool host, ThrMode mode, const float* I, size_t ist, size_t isy, const float* B, size_t bst, size_t bsy, int count,
                   int H, int W, int batch, const ThrIO& io)
{
    if (!c) return WASS_ERR_INVALID_ARG;
    if (!I || !B) return set_err(c, WASS_ERR_INVALID_ARG, "null argument");
    if ((mode == THR_RANGE && !(io.m_out && io.lo && io.hi && io.nonfinite)) || (mode == THR_HIST && !(io.m_in && io.edges && io.counts)) ||
        (mode == THR_MASK && !(io.m_in && io.thr && io.mask)))
        return set_err(c, WASS_ERR_INVALID_ARG, "null argument");
    ThrPlan p;
    int rc = thr_plan(count, H, W, batch, host, p);
    if (rc) return set_err(c, rc, "cannot plan the threshold of a %d x %d x %d cube under the scratch cap of %zu bytes", count, H, W, RAD_SCRATCH_CAP);
    if (isy < (size_t)W || bsy < (size_t)W || (count > 1 && (ist < (size_t)W || bst < (size_t)W))) return set_err(c, WASS_ERR_INVALID_ARG, "bad strides");
    WASS_HIP(c, hipSetDevice(c->device));
    hipStream_t s = c->ts();
    const size_t HW = (size_t)H * W, n = (size_t)count;
    Arena mem;
    if ((rc = mem.reserve(c, p.total, "the threshold scratch"))) return rc;
    unsigned* rec = mem.take<unsigned>(n * THR_WORDS * 4);
    float* dm = mem.take<float>(n * 4);
    float* dthr = mem.take<float>(n * 4);
    float* dedges = mem.take<float>(n * (THR_BINS + 1) * 4);
    unsigned* dcounts = mem.take<unsigned>(n * THR_BINS * 4);
    float* sI = mem.take<float>(p.stage_bytes);
    float* sB = mem.take<float>(p.stage_bytes);
    unsigned char* smask = mem.take<unsigned char>(p.mask_bytes);
    hipError_t e = hipMemsetAsync(rec, 0, p.head_bytes, s);   // the head: everything before the staging
    if (e == hipSuccess && mode != THR_RANGE) e = hipMemcpyAsync(dm, io.m_in, n * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess && mode == THR_HIST) e = hipMemcpyAsync(dedges, io.edges, n * (THR_BINS + 1) * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess && mode == THR_MASK) e = hipMemcpyAsync(dthr, io.thr, n * 4, hipMemcpyHostToDevice, s);
    const dim3 block(RAD_BX, RAD_BY);
    for (int t0 = 0; t0 < count && e == hipSuccess; t0 += p.batch) {
        const int nb = count - t0 < p.batch ? count - t0 : p.batch;
        const dim3 grid((W + RAD_BX - 1) / RAD_BX, (H + RAD_BY - 1) / RAD_BY, nb);
        const float *pi = I + (size_t)t0 * ist, *pb = B + (size_t)t0 * bst;
        long long it = (long long)ist, iy = (long long)isy, bt = (long long)bst, by = (long long)bsy;
        unsigned char* m = io.mask ? io.mask + (size_t)t0 * HW : nullptr;
        if (host) {
            e = upload_rows(sI, pi, 4, nb, 0, H, W, ist, isy, s);
            if (e == hipSuccess) e = upload_rows(sB, pb, 4, nb, 0, H, W, bst, bsy, s);
            if (e != hipSuccess) break;
            pi = sI; pb = sB; it = bt = (long long)HW; iy = by = W; m = smask;
        }
        if (mode == THR_RANGE) {
            hipLaunchKernelGGL(k_thr_bgmin, grid, block, 0, s, pb, bt, by, H, W, rec + (size_t)t0 * THR_WORDS);
            hipLaunchKernelGGL(k_thr_range, grid, block, 0, s, pi, it, iy, pb, bt, by, H, W, rec + (size_t)t0 * THR_WORDS);
        } else if (mode == THR_HIST) {
            hipLaunchKernelGGL(k_thr_hist, grid, block, 0, s, pi, it, iy, pb, bt, by, H, W, (const float*)(dm + t0),
                               (const float*)(dedges + (size_t)t0 * (THR_BINS + 1)), dcounts + (size_t)t0 * THR_BINS);
        } else {
            hipLaunchKernelGGL(k_thr_mask, grid, block, 0, s, pi, it, iy, pb, bt, by, H, W, (const float*)(dm + t0), (const float*)(dthr + t0), m);
        }
        e = hipGetLastError();
        if (e == hipSuccess && host && mode == THR_MASK) e = hipMemcpyAsync(io.mask + (size_t)t0 * HW, smask, (size_t)nb * HW, hipMemcpyDeviceToHost, s);
    }
    rc = finish(c, WASS_OK, e, s, "radiance threshold");
    if (!rc && mode == THR_RANGE) {
        std::vector<unsigned> r(n * THR_WORDS);
        e = hipMemcpy(r.data(), rec, n * THR_WORDS * 4, hipMemcpyDeviceToHost);
        if (e != hipSuccess) rc = set_err(c, WASS_ERR_DEVICE, "radiance threshold: %s", hipGetErrorString(e));
        else
            for (size_t t = 0; t < n; ++t) {
                const unsigned* w = &r[t * THR_WORDS];
                io.m_out[t] = w[4] ? NAN : order_unkey(~w[0]);
                io.lo[t] = w[1] ? order_unkey(~w[1]) : NAN;   // no finite cell at all: there is no range
                io.hi[t] = w[2] ? order_unkey(w[2]) : NAN;
                io.nonfinite[t] = w[3];
            }
    }
    if (!rc && mode == THR_HIST) {
        e = hipMemcpy(io.counts, dcounts, n * THR_BINS * 4, hipMemcpyDeviceToHost);
        if (e != hipSuccess) rc = set_err(c, WASS_ERR_DEVICE, "radiance threshold: %s", hipGetErrorString(e));
    }
    return rc;
}

}  // namespace wass

using namespace wass;

extern "C" int wass_lanczos4_table(int16_t* out)
{
    if (!out) return WASS_ERR_INVALID_ARG;
    build_lanczos4_tab(out);
    return WASS_OK;
}

extern "C" int wass_remap_lanczos4(wass_ctx* c, const uint8_t* src, int sw, int sh, size_t src_stride, const float* map_x, const float* map_y, int dw,
                                   int dh, uint8_t* dst)
{
    return remap_run(c, true, src, sw, sh, src_stride, map_x, map_y, dw, dh, dst);
}

extern "C" int wass_remap_lanczos4_dev(wass_ctx* c, const uint8_t* d_src, int sw, int sh, size_t src_stride, const float* d_map_x,
                                       const float* d_map_y, int dw, int dh, uint8_t* d_dst)
{
    return remap_run(c, false, d_src, sw, sh, src_stride, d_map_x, d_map_y, dw, dh, d_dst);
}

extern "C" int wass_radiance_scratch_bytes(int count, int H, int W, int Ih, int Iw, int batch, int host, size_t* bytes, int* batch_used)
{
    if (!bytes) return WASS_ERR_INVALID_ARG;
    RadPlan p;
    const int rc = rad_plan(count, H, W, Ih, Iw, batch, host != 0, p);
    if (rc) return rc;
    *bytes = p.total;
    if (batch_used) *batch_used = p.batch;
    return WASS_OK;
}

extern "C" int wass_radiance(wass_ctx* c, const uint8_t* images, size_t image_stride_t, size_t image_stride_y, int Ih, int Iw, const float* in,
                             size_t stride_t, size_t stride_y, int count, int H, int W, const double* XX, const double* YY, const double Pcam[12],
                             double datascale, int batch, float* out)
{
    return rad_run(c, true, images, image_stride_t, image_stride_y, Ih, Iw, in, stride_t, stride_y, count, H, W, XX, YY, Pcam, datascale, batch, out);
}

extern "C" int wass_radiance_dev(wass_ctx* c, const uint8_t* d_images, size_t image_stride_t, size_t image_stride_y, int Ih, int Iw,
                                 const float* d_in, size_t stride_t, size_t stride_y, int count, int H, int W, const double* d_XX,
                                 const double* d_YY, const double Pcam[12], double datascale, int batch, float* d_out)
{
    return rad_run(c, false, d_images, image_stride_t, image_stride_y, Ih, Iw, d_in, stride_t, stride_y, count, H, W, d_XX, d_YY, Pcam, datascale,
                   batch, d_out);
}

extern "C" int wass_bgimage_scratch_bytes(int count, int H, int W, int size, int slab_rows, int host, size_t* bytes, int* rows_per_slab)
{
    if (!bytes) return WASS_ERR_INVALID_ARG;
    BgPlan p;
    const int rc = bg_plan(count, H, W, size, slab_rows, host != 0, p);
    if (rc) return rc;
    *bytes = p.total;
    if (rows_per_slab) *rows_per_slab = p.rows;
    return WASS_OK;
}

extern "C" int wass_bgimage(wass_ctx* c, const float* in, size_t stride_t, size_t stride_y, int count, int H, int W, int size, int slab_rows,
                            float* out, size_t out_stride_t, size_t out_stride_y)
{
    return bg_run(c, true, in, stride_t, stride_y, count, H, W, size, slab_rows, out, out_stride_t, out_stride_y);
}

extern "C" int wass_bgimage_dev(wass_ctx* c, const float* d_in, size_t stride_t, size_t stride_y, int count, int H, int W, int size, int slab_rows,
                                float* d_out, size_t out_stride_t, size_t out_stride_y)
{
    return bg_run(c, false, d_in, stride_t, stride_y, count, H, W, size, slab_rows, d_out, out_stride_t, out_stride_y);
}

extern "C" int wass_radiance_threshold_scratch_bytes(int count, int H, int W, int batch, int host, size_t* bytes, int* batch_used)
{
    if (!bytes) return WASS_ERR_INVALID_ARG;
    ThrPlan p;
    const int rc = thr_plan(count, H, W, batch, host != 0, p);
    if (rc) return rc;
    *bytes = p.total;
    if (batch_used) *batch_used = p.batch;
    return WASS_OK;
}

#define WASS_THR_ENTRY(name, host)                                                                                                              \
    extern "C" int wass_radiance_range##name(wass_ctx* c, const float* I, size_t ist, size_t isy, const float* B, size_t bst, size_t bsy,      \
                                             int count, int H, int W, int batch, float* bgmin, float* lo, float* hi, uint32_t* nonfinite)       \
    {                                                                                                                                           \
        ThrIO io;                                                                                                                               \
        io.m_out = bgmin; io.lo = lo; io.hi = hi; io.nonfinite = nonfinite;                                                                     \
        return thr_run(c, host, THR_RANGE, I, ist, isy, B, bst, bsy, count, H, W, batch, io);                                                   \
    }                                                                                                                                           \
    extern "C" int wass_radiance_hist##name(wass_ctx* c, const float* I, size_t ist, size_t isy, const float* B, size_t bst, size_t bsy,       \
                                            int count, int H, int W, int batch, const float* bgmin, const float* edges, uint32_t* counts)       \
    {                                                                                                                                           \
        ThrIO io;                                                                                                                               \
        io.m_in = bgmin; io.edges = edges; io.counts = counts;                                                                                  \
        return thr_run(c, host, THR_HIST, I, ist, isy, B, bst, bsy, count, H, W, batch, io);                                                    \
    }                                                                                                                                           \
    extern "C" int wass_radiance_mask##name(wass_ctx* c, const float* I, size_t ist, size_t isy, const float* B, size_t bst, size_t bsy,       \
                                            int count, int H, int W, int batch, const float* bgmin, const float* thr, uint8_t* mask)            \
    {                                                                                                                                           \
        ThrIO io;                                                                                                                               \
        io.m_in = bgmin; io.thr = thr; io.mask = mask;                                                                                          \
        return thr_run(c, host, THR_MASK, I, ist, isy, B, bst, bsy, count, H, W, batch, io);                                                    \
    }

WASS_THR_ENTRY(, true)
WASS_THR_ENTRY(_dev, false)
