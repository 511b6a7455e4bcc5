// pyramid.hip -- cv::pyrUp of float32 / float64 pictures (the option `wasspost radiance --upscalefactor N`,
// postproc/wasspost/wasspost.py:840-843, 880-896) and the radiance of the cube on the finer grid built on it.
//
//   k_pyrup<T>     one level: an h x w picture becomes 2h x 2w (h, w >= 2).  Restated from knowledge of OpenCV 4.5.5's scalar
//                  pyrUp_ (modules/imgproc/src/pyramids.cpp); OpenCV is absent here, so this is PARITY UNPINNED against OpenCV
//                  (whose vector code may fuse multiply and add) and bit-exact against the numpy restatement of
//                  tests/pyramid_oracle.py.  All arithmetic in T, no contraction (-ffp-contract=off), x first, then y.
//                  Along x, source row s of length w gives r of length 2w; every product is formed first, the sums go left to
//                  right as bracketed:
//                      0 < j < w-1   r[2j] = (s[j-1] + s[j]*6) + s[j+1]     r[2j+1] = (s[j] + s[j+1])*4
//                      j = 0         r[0]  = s[0]*6 + s[1]*2                r[1]    = (s[0] + s[1])*4
//                      j = w-1       r[2w-2] = s[w-2] + s[w-1]*7            r[2w-1] = s[w-1]*8
//                  (OpenCV writes the two ends of a row out by hand: that form is kept on this axis.)
//                  Along y the three-tap form is kept at the ends as well, on reflected row indices, as OpenCV's row loop does:
//                  with up(i) = i-1 (1 for i = 0) and dn(i) = i+1 (h-1 for i = h-1), and R_k the x-upsampled source row k,
//                      out[2i]   = ((R_up(i) + R_i*6) + R_dn(i)) * (1/64)
//                      out[2i+1] = ((R_i + R_dn(i))*4) * (1/64)
//                  so the first row weighs row 1 twice ((R_1 + R_0*6) + R_1) and the last row weighs itself 6 + 1 and 4 + 4.
//                  1/64 is a power of two: the product is exact short of underflow.  NaN and infinities propagate as the sums say.
//                  One lane per SOURCE cell: it reads its 3 x 3 neighbourhood (the overlap is served by the vector cache; no LDS)
//                  and writes the 2 x 2 destination cells, each row's pair as one vector store where the destination allows it.
//                  Blocks of 64 x 4 source cells, frames in blockIdx.z.  No atomics: the same input gives the same bits.
//   k_pyr_scale    zf = in * scale in float32: the height rule of wass_radiance (zf = Z * (float)datascale) as a pass of its own,
//                  so that the pyramid works on the very bits the sampler would have formed.
//   wass_pyrup_*   `levels` (1 .. 4) levels, frames `batch` (8) at a time; every level but the last writes tightly packed scratch.
//   wass_radiance_up*   per batch: k_pyr_scale, `levels` times k_pyrup<float>, then radiance.hip's k_radiance (unchanged, called
//                  with scale 1, which leaves zf as it is) on the upsampled heights and the grid upsampled once per call with
//                  k_pyrup<double>.
// Host side: pyr_plan and radup_plan keep their byte formulas; the batch rule, the scratch, the staging of a host batch and the
// end of a call are cube.h's.
#include "common.h"
#include "cube.h"

namespace wass {

constexpr size_t PYR_SCRATCH_CAP = (size_t)16 << 30;    // bytes one call may allocate
constexpr int PYR_MAX_BATCH = 1024;                     // frames per launch (blockIdx.z)
constexpr int PYR_DEFAULT_BATCH = 8;
constexpr int PYR_BX = 64, PYR_BY = 4;                  // a block: 4 waves, each 64 source cells of one row
constexpr int PYR_MAX_LEVELS = 4;
constexpr int PYR_MAX_SIDE = 65536;                     // of the result

template <typename T> struct PyrPair;
template <> struct PyrPair<float> { typedef float2 type; };
template <> struct PyrPair<double> { typedef double2 type; };

// the two x-upsampled values (even, odd) of source column j from its row p; jm = j-1 and jp = j+1 where they exist
template <typename T>
__device__ __forceinline__ void pyr_row(const T* __restrict__ p, int j, int W, T& e, T& o)
{
    const T b = p[j];
    if (j == 0) {
        const T c = p[1];
        e = b * (T)6 + c * (T)2;
        o = (b + c) * (T)4;
    } else if (j == W - 1) {
        const T a = p[j - 1];
        e = a + b * (T)7;
        o = b * (T)8;
    } else {
        const T a = p[j - 1], c = p[j + 1];
        e = (a + b * (T)6) + c;
        o = (b + c) * (T)4;
    }
}

template <typename T>
__global__ void __launch_bounds__(PYR_BX * PYR_BY) k_pyrup(const T* __restrict__ in, long long it, long long iy, int H, int W,
                                                           T* __restrict__ out, long long ot, long long oy, int vec)
{
    const int j = blockIdx.x * PYR_BX + threadIdx.x, i = blockIdx.y * PYR_BY + threadIdx.y;
    if (i >= H || j >= W) return;
    const T* __restrict__ src = in + (long long)blockIdx.z * it;
    const int iu = i == 0 ? 1 : i - 1, id = i == H - 1 ? H - 1 : i + 1;
    T eu, ou, em, om, ed, od;
    pyr_row(src + (long long)iu * iy, j, W, eu, ou);
    pyr_row(src + (long long)i * iy, j, W, em, om);
    pyr_row(src + (long long)id * iy, j, W, ed, od);
    const T k = (T)0.015625;
    const T e0 = ((eu + em * (T)6) + ed) * k, o0 = ((ou + om * (T)6) + od) * k;
    const T e1 = ((em + ed) * (T)4) * k, o1 = ((om + od) * (T)4) * k;
    T* __restrict__ d0 = out + (long long)blockIdx.z * ot + (long long)(2 * i) * oy + 2 * j;
    T* __restrict__ d1 = d0 + oy;
    if (vec) {
        typedef typename PyrPair<T>::type T2;
        T2 a, b;
        a.x = e0; a.y = o0; b.x = e1; b.y = o1;
        *reinterpret_cast<T2*>(d0) = a;
        *reinterpret_cast<T2*>(d1) = b;
    } else {
        d0[0] = e0; d0[1] = o0;
        d1[0] = e1; d1[1] = o1;
    }
}

__global__ void __launch_bounds__(PYR_BX * PYR_BY) k_pyr_scale(const float* __restrict__ in, long long it, long long iy, int H, int W, float scale,
                                                               float* __restrict__ out)
{
    const int j = blockIdx.x * PYR_BX + threadIdx.x, i = blockIdx.y * PYR_BY + threadIdx.y;
    if (i >= H || j >= W) return;
    out[((size_t)blockIdx.z * H + i) * W + j] = in[(long long)blockIdx.z * it + (long long)i * iy + j] * scale;
}

// one level of nb frames, device memory; pairs are stored as vectors where every pair of the destination is aligned
template <typename T>
static hipError_t pyr_level(const T* in, long long it, long long iy, int nb, int h, int w, T* out, long long ot, long long oy, hipStream_t s)
{
    const int vec = ((uintptr_t)out % (2 * sizeof(T)) == 0 && ot % 2 == 0 && oy % 2 == 0) ? 1 : 0;
    const dim3 block(PYR_BX, PYR_BY), grid((w + PYR_BX - 1) / PYR_BX, (h + PYR_BY - 1) / PYR_BY, nb);
    hipLaunchKernelGGL(k_pyrup<T>, grid, block, 0, s, in, it, iy, h, w, out, ot, oy, vec);
    return hipGetLastError();
}

// `levels` levels of nb frames: level l (1-based) below the last goes into mid[l - 1], tightly packed; the last into out
template <typename T>
static hipError_t pyr_levels(const T* in, long long it, long long iy, int nb, int H, int W, int levels, T* const* mid, T* out, long long ot,
                             long long oy, hipStream_t s)
{
    hipError_t e = hipSuccess;
    int h = H, w = W;
    for (int l = 1; l <= levels && e == hipSuccess; ++l, h *= 2, w *= 2) {
        const bool last = l == levels;
        T* dst = last ? out : mid[l - 1];
        const long long dt = last ? ot : (long long)(2 * h) * (2 * w), dy = last ? oy : 2 * w;
        e = pyr_level<T>(in, it, iy, nb, h, w, dst, dt, dy, s);
        in = dst; it = dt; iy = dy;
    }
    return e;
}

static int pyr_sizes_ok(int H, int W, int levels)
{
    if (levels < 1 || levels > PYR_MAX_LEVELS || H < 2 || W < 2) return WASS_ERR_INVALID_ARG;
    if (((long long)H << levels) > PYR_MAX_SIDE || ((long long)W << levels) > PYR_MAX_SIDE) return WASS_ERR_UNSUPPORTED;
    return WASS_OK;
}

struct PyrPlan {
    int batch = 0;
    size_t in_bytes = 0, mid_bytes[PYR_MAX_LEVELS] = {}, out_bytes = 0, total = 0;
};

// per frame of a batch: the levels below the last (device and host form alike); the host form also stages the input and the result
static int pyr_plan(int count, int H, int W, int levels, int elem, int batch, bool host, PyrPlan& p)
{
    if (count < 1 || batch < 0 || (elem != 4 && elem != 8)) return WASS_ERR_INVALID_ARG;
    const int rc = pyr_sizes_ok(H, W, levels);
    if (rc) return rc;
    const size_t HW = (size_t)H * W;
    p.batch = fit_batch(batch, PYR_DEFAULT_BATCH, PYR_MAX_BATCH, count, PYR_SCRATCH_CAP, [&](int b) {
        p.in_bytes = host ? align256((size_t)b * HW * elem) : 0;
        p.out_bytes = host ? align256(((size_t)b * HW << (2 * levels)) * elem) : 0;
        p.total = p.in_bytes + p.out_bytes;
        for (int l = 1; l < levels; ++l) p.total += p.mid_bytes[l - 1] = align256(((size_t)b * HW << (2 * l)) * elem);
        return p.total;
    });
    return p.batch ? WASS_OK : WASS_ERR_NO_MEMORY;
}

template <typename T>
static int pyr_run(wass_ctx* c, bool host, const T* in, size_t ist, size_t isy, int count, int H, int W, int levels, T* out, size_t ost, size_t osy)
{
    if (!c) return WASS_ERR_INVALID_ARG;
    if (!in || !out) return set_err(c, WASS_ERR_INVALID_ARG, "null argument");
    PyrPlan p;
    int rc = pyr_plan(count, H, W, levels, (int)sizeof(T), 0, host, p);
    if (rc) return set_err(c, rc, "cannot plan %d levels of pyrUp over a %d x %d x %d cube (sides from 2, the result's up to %d, levels 1 to %d, "
                           "scratch cap %zu bytes)", levels, count, H, W, PYR_MAX_SIDE, PYR_MAX_LEVELS, PYR_SCRATCH_CAP);
    const size_t Ho = (size_t)H << levels, Wo = (size_t)W << levels;
    if (isy < (size_t)W || osy < Wo || (count > 1 && (ist < (size_t)W || ost < (Ho - 1) * osy + Wo))) return set_err(c, WASS_ERR_INVALID_ARG, "bad strides");
    if (!host && (const void*)in == (const void*)out) return set_err(c, WASS_ERR_INVALID_ARG, "pyrUp cannot work in place");
    WASS_HIP(c, hipSetDevice(c->device));
    hipStream_t s = c->ts();
    Arena mem;                                              // one level on the device: nothing
    if ((rc = mem.reserve(c, p.total, "pyrUp"))) return rc;
    T* sin = mem.take<T>(p.in_bytes);
    T* mid[PYR_MAX_LEVELS] = {};
    for (int l = 1; l < levels; ++l) mid[l - 1] = mem.take<T>(p.mid_bytes[l - 1]);
    T* sout = mem.take<T>(p.out_bytes);
    const size_t HW = (size_t)H * W, HWo = Ho * Wo;
    hipError_t e = hipSuccess;
    for (int t0 = 0; t0 < count && e == hipSuccess; t0 += p.batch) {
        const int nb = count - t0 < p.batch ? count - t0 : p.batch;
        const T* src = in + (size_t)t0 * ist;
        T* dst = out + (size_t)t0 * ost;
        if (host) {
            e = upload_rows(sin, src, sizeof(T), nb, 0, H, W, ist, isy, s);
            if (e != hipSuccess) break;
            e = pyr_levels<T>(sin, (long long)HW, W, nb, H, W, levels, mid, sout, (long long)HWo, (long long)Wo, s);
            if (e == hipSuccess) e = download_rows(dst, sout, sizeof(T), nb, 0, (int)Ho, (int)Wo, ost, osy, s);
        } else {
            e = pyr_levels<T>(src, (long long)ist, (long long)isy, nb, H, W, levels, mid, dst, (long long)ost, (long long)osy, s);
        }
    }
    return finish(c, WASS_OK, e, s, "pyrUp", p.total != 0);
}

// ---------------------------------------------------------------- radiance on the upsampled grid
struct RadUpPlan {
    int batch = 0;
    size_t gsrc_bytes = 0, gmid_bytes[PYR_MAX_LEVELS] = {}, gup_bytes = 0;      // the grid: per call
    size_t img_bytes = 0, zin_bytes = 0, zf_bytes = 0, zmid_bytes[PYR_MAX_LEVELS] = {}, zup_bytes = 0, out_bytes = 0, total = 0;
};

// per call: XX and YY upsampled (their lower levels share one set of buffers; the host form stages the two sources); per frame of
// a batch: zf, its levels; the host form also stages the picture, the heights and the result
static int radup_plan(int count, int H, int W, int Ih, int Iw, int levels, int batch, bool host, RadUpPlan& p)
{
    if (count < 1 || batch < 0 || Ih < 1 || Iw < 1 || Ih >= 32767 || Iw >= 32767) return WASS_ERR_INVALID_ARG;
    const int rc = pyr_sizes_ok(H, W, levels);
    if (rc) return rc;
    const size_t HW = (size_t)H * W, HWu = HW << (2 * levels);
    if (HWu > 0x7fffff00u) return WASS_ERR_UNSUPPORTED;     // as wass_radiance
    p.gsrc_bytes = host ? 2 * align256(HW * 8) : 0;
    p.gup_bytes = 2 * align256(HWu * 8);
    size_t fixed = p.gsrc_bytes + p.gup_bytes;
    for (int l = 1; l < levels; ++l) fixed += p.gmid_bytes[l - 1] = align256((HW << (2 * l)) * 8);
    p.batch = fit_batch(batch, PYR_DEFAULT_BATCH, PYR_MAX_BATCH, count, PYR_SCRATCH_CAP, [&](int b) {
        p.img_bytes = host ? align256((size_t)b * Ih * Iw) : 0;
        p.zin_bytes = host ? align256((size_t)b * HW * 4) : 0;
        p.zf_bytes = align256((size_t)b * HW * 4);
        p.zup_bytes = align256((size_t)b * HWu * 4);
        p.out_bytes = host ? p.zup_bytes : 0;
        p.total = fixed + p.img_bytes + p.zin_bytes + p.zf_bytes + p.zup_bytes + p.out_bytes;
        for (int l = 1; l < levels; ++l) p.total += p.zmid_bytes[l - 1] = align256(((size_t)b * HW << (2 * l)) * 4);
        return p.total;
    });
    return p.batch ? WASS_OK : WASS_ERR_NO_MEMORY;
}

static int radup_run(wass_ctx* c, bool host, const uint8_t* img, size_t img_t, size_t img_y, int Ih, int Iw, const float* in, size_t st, size_t sy,
                     int count, int H, int W, const double* XX, const double* YY, const double* Pcam, double datascale, int batch, int levels,
                     float* out)
{
    if (!c) return WASS_ERR_INVALID_ARG;
    if (!img || !in || !XX || !YY || !Pcam || !out) return set_err(c, WASS_ERR_INVALID_ARG, "null argument");
    RadUpPlan p;
    int rc = radup_plan(count, H, W, Ih, Iw, levels, batch, host, p);
    if (rc) return set_err(c, rc, "cannot plan the radiance of a %d x %d x %d cube upsampled by %d levels from %d x %d pictures under the scratch "
                           "cap of %zu bytes", count, H, W, levels, Ih, Iw, PYR_SCRATCH_CAP);
    if (sy < (size_t)W || img_y < (size_t)Iw || (count > 1 && (st < (size_t)W || img_t < (size_t)Iw))) return set_err(c, WASS_ERR_INVALID_ARG, "bad strides");
    WASS_HIP(c, hipSetDevice(c->device));
    hipStream_t s = c->ts();
    const int Hu = H << levels, Wu = W << levels;
    const size_t HW = (size_t)H * W, HWu = (size_t)Hu * Wu, II = (size_t)Ih * Iw;
    Arena mem;
    if ((rc = mem.reserve(c, p.total, "the upsampled radiance"))) return rc;
    double* gsrc[2] = { mem.take<double>(p.gsrc_bytes / 2), mem.take<double>(p.gsrc_bytes / 2) };
    double* gmid[PYR_MAX_LEVELS] = {};
    for (int l = 1; l < levels; ++l) gmid[l - 1] = mem.take<double>(p.gmid_bytes[l - 1]);
    double* gup[2] = { mem.take<double>(p.gup_bytes / 2), mem.take<double>(p.gup_bytes / 2) };
    uint8_t* simg = mem.take<uint8_t>(p.img_bytes);
    float* szin = mem.take<float>(p.zin_bytes);
    float* zf = mem.take<float>(p.zf_bytes);
    float* zmid[PYR_MAX_LEVELS] = {};
    for (int l = 1; l < levels; ++l) zmid[l - 1] = mem.take<float>(p.zmid_bytes[l - 1]);
    float* zup = mem.take<float>(p.zup_bytes);
    float* sout = mem.take<float>(p.out_bytes);
    hipError_t e = hipSuccess;
    const double* g[2] = { XX, YY };
    for (int k = 0; k < 2 && e == hipSuccess; ++k) {
        const double* src = g[k];
        if (host) {
            e = hipMemcpyAsync(gsrc[k], src, HW * 8, hipMemcpyHostToDevice, s);
            src = gsrc[k];
        }
        if (e == hipSuccess) e = pyr_levels<double>(src, (long long)HW, W, 1, H, W, levels, gmid, gup[k], (long long)HWu, Wu, s);
    }
    const dim3 block(PYR_BX, PYR_BY);
    rc = WASS_OK;
    for (int t0 = 0; t0 < count && e == hipSuccess && !rc; t0 += p.batch) {
        const int nb = count - t0 < p.batch ? count - t0 : p.batch;
        const uint8_t* im = img + (size_t)t0 * img_t;
        size_t it = img_t, iy = img_y;
        const float* zin = in + (size_t)t0 * st;
        long long zst = (long long)st, zsy = (long long)sy;
        float* o = out + (size_t)t0 * HWu;
        if (host) {
            e = upload_rows(simg, im, 1, nb, 0, Ih, Iw, img_t, img_y, s);
            if (e == hipSuccess) e = upload_rows(szin, zin, 4, nb, 0, H, W, st, sy, s);
            if (e != hipSuccess) break;
            im = simg; it = II; iy = (size_t)Iw; zin = szin; zst = (long long)HW; zsy = W; o = sout;
        }
        const dim3 grid((W + PYR_BX - 1) / PYR_BX, (H + PYR_BY - 1) / PYR_BY, nb);
        hipLaunchKernelGGL(k_pyr_scale, grid, block, 0, s, zin, zst, zsy, H, W, (float)datascale, zf);
        e = hipGetLastError();
        if (e == hipSuccess) e = pyr_levels<float>(zf, (long long)HW, W, nb, H, W, levels, zmid, zup, (long long)HWu, Wu, s);
        if (e != hipSuccess) break;
        rc = radiance_enqueue(c, im, it, iy, Ih, Iw, zup, HWu, (size_t)Wu, nb, Hu, Wu, gup[0], gup[1], Pcam, 1.0f, o, s);
        if (!rc && host) e = hipMemcpyAsync(out + (size_t)t0 * HWu, sout, (size_t)nb * HWu * 4, hipMemcpyDeviceToHost, s);
    }
    return finish(c, rc, e, s, "upsampled radiance");
}

}  // namespace wass

using namespace wass;

extern "C" int wass_pyrup_scratch_bytes(int count, int H, int W, int levels, int elem_size, int batch, int host, size_t* bytes, int* batch_used)
{
    if (!bytes) return WASS_ERR_INVALID_ARG;
    PyrPlan p;
    const int rc = pyr_plan(count, H, W, levels, elem_size, batch, host != 0, p);
    if (rc) return rc;
    *bytes = p.total;
    if (batch_used) *batch_used = p.batch;
    return WASS_OK;
}

extern "C" int wass_pyrup_f32(wass_ctx* c, const float* in, size_t in_stride_t, size_t in_stride_y, int count, int H, int W, int levels, float* out,
                              size_t out_stride_t, size_t out_stride_y)
{
    return pyr_run<float>(c, true, in, in_stride_t, in_stride_y, count, H, W, levels, out, out_stride_t, out_stride_y);
}

extern "C" int wass_pyrup_f32_dev(wass_ctx* c, const float* d_in, size_t in_stride_t, size_t in_stride_y, int count, int H, int W, int levels,
                                  float* d_out, size_t out_stride_t, size_t out_stride_y)
{
    return pyr_run<float>(c, false, d_in, in_stride_t, in_stride_y, count, H, W, levels, d_out, out_stride_t, out_stride_y);
}

extern "C" int wass_pyrup_f64(wass_ctx* c, const double* in, size_t in_stride_t, size_t in_stride_y, int count, int H, int W, int levels, double* out,
                              size_t out_stride_t, size_t out_stride_y)
{
    return pyr_run<double>(c, true, in, in_stride_t, in_stride_y, count, H, W, levels, out, out_stride_t, out_stride_y);
}

extern "C" int wass_pyrup_f64_dev(wass_ctx* c, const double* d_in, size_t in_stride_t, size_t in_stride_y, int count, int H, int W, int levels,
                                  double* d_out, size_t out_stride_t, size_t out_stride_y)
{
    return pyr_run<double>(c, false, d_in, in_stride_t, in_stride_y, count, H, W, levels, d_out, out_stride_t, out_stride_y);
}

extern "C" int wass_radiance_up_scratch_bytes(int count, int H, int W, int Ih, int Iw, int levels, int batch, int host, size_t* bytes,
                                              int* batch_used)
{
    if (!bytes) return WASS_ERR_INVALID_ARG;
    RadUpPlan p;
    const int rc = radup_plan(count, H, W, Ih, Iw, levels, batch, host != 0, p);
    if (rc) return rc;
    *bytes = p.total;
    if (batch_used) *batch_used = p.batch;
    return WASS_OK;
}

extern "C" int wass_radiance_up(wass_ctx* c, const uint8_t* images, size_t image_stride_t, size_t image_stride_y, int Ih, int Iw, const float* in,
                                size_t stride_t, size_t stride_y, int count, int H, int W, const double* XX, const double* YY,
                                const double Pcam[12], double datascale, int batch, int levels, float* out)
{
    return radup_run(c, true, images, image_stride_t, image_stride_y, Ih, Iw, in, stride_t, stride_y, count, H, W, XX, YY, Pcam, datascale, batch,
                     levels, out);
}

extern "C" int wass_radiance_up_dev(wass_ctx* c, const uint8_t* d_images, size_t image_stride_t, size_t image_stride_y, int Ih, int Iw,
                                    const float* d_in, size_t stride_t, size_t stride_y, int count, int H, int W, const double* d_XX,
                                    const double* d_YY, const double Pcam[12], double datascale, int batch, int levels, float* d_out)
{
    return radup_run(c, false, d_images, image_stride_t, image_stride_y, Ih, Iw, d_in, stride_t, stride_y, count, H, W, d_XX, d_YY,
                     Pcam, datascale, batch, levels, d_out);
}
