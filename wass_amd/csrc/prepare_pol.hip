// prepare_pol.hip -- the polarimetric branch of wass_prepare (src/wass_prepare/wass_prepare.cpp:52-85, :103-255): a polarising-filter-array
// mosaic to Stokes pictures, the stereo input picture and the optional index / channel pictures, in one pass.
//
//   k_prepare_pol   one lane per pixel of the 2m x 2n output (m = rows / 2, n = cols / 2).  The lane computes where cv::undistort reads
//                   (undistort_map.h, the tables of rectify.hip's per-camera cache), then, for each of the four channels, the 2 x 2 taps
//                   of the UPSCALED quarter picture, formed on the fly from the raw mosaic bytes: float(u8) * (1.0f / 255.0f), the x2
//                   cv::resize INTER_LINEAR float path along x and then along y (weights 0.25 / 0.75, the first and last row and column
//                   copied), the four float32 weights of polarimetric.hip's 1024 x 2 x 2 table, ((v00 w00 + v01 w01) + v10 w10) + v11 w11,
//                   taps outside the picture 0.  A recomputed upscaled pixel has the bits of a stored one, so the result equals the staged
//                   chain (tests/prepare_pol_oracle.py) exactly.  Then the mix that enforces I0 + I90 = I45 + I135, S0 S1 S2, the stereo
//                   picture (S0 x 127, or the HDR picture x 255) and whatever else was asked for.  The two taps along an axis read from at
//                   most three neighbouring quarter rows / columns, so a lane loads a 3 x 3 window of macro-pixels (36 bytes).
//                   Every float32 product and sum is rounded on its own (the library is built with -ffp-contract=off); quotients and
//                   roots are formed in fp64 and rounded again, which is the correctly rounded float32 result; exp and atan2 are fp64.
//   k_prepare_pol_ranges   the ranges of S0, S1, S2 and DOLP (NaN skipped): k_prepare_pol leaves one record of ordered integer keys per
//                   block (reduce.h's order_key), this kernel takes their maxima.  No float atomics, no dependence on the order of execution.
//
// OpenCV is absent here: written from knowledge of OpenCV 4.5.5 (resize.cpp, imgwarp.cpp, undistort.dispatch.cpp), PARITY UNPINNED.
#include "common.h"
#include "undistort_map.h"

#include <cmath>

namespace wass {

constexpr int PP_BX = 64, PP_BY = 4;                    // a block: 4 waves, each 64 pixels of one row
constexpr int PP_TAB = 32;
constexpr int PP_NKEY = 8;                              // per block: ~key of the minimum, key of the maximum of S0, S1, S2, DOLP

struct PrepOut {
    float* S;                      // [3][H][W] or null
    uint8_t* image;                // [H][W]
    uint8_t* dolp;                 // [H][W] or null
    uint8_t* aolp;                 // [H][W] or null
    uint8_t* channels;             // [4][H][W] or null
    float* image_f32;              // [H][W] or null: the stereo picture before rounding
    float* aolp_f32;               // [H][W] or null: the AOLP index before rounding
};

struct Q4 { float i0, i45, i90, i135; };                // the four channels of one position

// destination index d of the x2 upscale of `size` samples: src[a] * wa + src[b] * wb.  Where OpenCV clamps (the weight of the second tap is
// 0 there) both indices name the one sample that counts.  ok: d is inside the upscaled picture (d is clamped into it for the indices).
struct UpTap { int a, b; float wa, wb; bool ok; };

__device__ __forceinline__ UpTap up_tap(int d, int size)
{
    UpTap t;
    t.ok = (unsigned)d < (unsigned)(2 * size);
    d = min(max(d, 0), 2 * size - 1);
    const int j = d >> 1;
    if (d & 1) {                                        // f = j + 0.25
        if (j >= size - 1) { t.a = t.b = size - 1; t.wa = 1.f; t.wb = 0.f; }
        else { t.a = j; t.b = j + 1; t.wa = 0.75f; t.wb = 0.25f; }
    } else {                                            // f = j - 0.25
        if (j == 0) { t.a = t.b = 0; t.wa = 1.f; t.wb = 0.f; }
        else { t.a = j - 1; t.b = j; t.wa = 0.25f; t.wb = 0.75f; }
    }
    return t;
}

// macro-pixel (i, j), 0 <= i < m, 0 <= j < n:   I90 I45 / I135 I0
__device__ __forceinline__ Q4 load_quad(const uint8_t* __restrict__ mosaic, size_t stride, int i, int j)
{
    const uint8_t* p = mosaic + (size_t)(2 * i) * stride + 2 * j;
    const float s = 1.0f / 255.0f;
    Q4 q;
    q.i90 = (float)p[0] * s;
    q.i45 = (float)p[1] * s;
    q.i135 = (float)p[stride] * s;
    q.i0 = (float)p[stride + 1] * s;
    return q;
}

__device__ __forceinline__ Q4 lerp2(const Q4& a, const Q4& b, float wa, float wb)
{
    Q4 r;
    r.i0 = a.i0 * wa + b.i0 * wb;
    r.i45 = a.i45 * wa + b.i45 * wb;
    r.i90 = a.i90 * wa + b.i90 * wb;
    r.i135 = a.i135 * wa + b.i135 * wb;
    return r;
}

__device__ __forceinline__ Q4 pick(bool first, const Q4& a, const Q4& b)
{
    Q4 r;
    r.i0 = first ? a.i0 : b.i0; r.i45 = first ? a.i45 : b.i45; r.i90 = first ? a.i90 : b.i90; r.i135 = first ? a.i135 : b.i135;
    return r;
}

__device__ __forceinline__ Q4 masked(bool ok, const Q4& a)
{
    Q4 r;
    r.i0 = ok ? a.i0 : 0.f; r.i45 = ok ? a.i45 : 0.f; r.i90 = ok ? a.i90 : 0.f; r.i135 = ok ? a.i135 : 0.f;
    return r;
}

__device__ __forceinline__ float tap_sum(float v00, float v01, float v10, float v11, const float4& w)
{
    return ((v00 * w.x + v01 * w.y) + v10 * w.z) + v11 * w.w;
}

// cv::saturate_cast<uchar> of a float: round half to even, clamp, NaN -> 0
__device__ __forceinline__ uint8_t sat_u8(float v)
{
    const float r = rintf(v);
    if (!(r == r)) return 0;
    return (uint8_t)(r < 0.f ? 0.f : r > 255.f ? 255.f : r);
}

__device__ __forceinline__ float div_f32(float a, float b) { return (float)((double)a / (double)b); }

// the weight of a channel in the HDR picture: exp(-(I - 0.5)^2 / (2 sigma^2)), sigma = 0.3
__device__ __forceinline__ float hdr_weight(float I)
{
    const float d = I - 0.5f;
    const float den = 2.0f * 0.3f * 0.3f;
    const float arg = div_f32(-1.0f * (d * d), den);
    return (float)exp((double)arg);
}

__global__ void __launch_bounds__(PP_BX * PP_BY) k_prepare_pol(const uint8_t* __restrict__ mosaic, size_t stride, int m, int n,
                                                               const double* __restrict__ xs, const double* __restrict__ ys, const Dist12 D,
                                                               double fx, double fy, double u0, double v0, int hdr, const PrepOut o,
                                                               const float4* __restrict__ tab, unsigned* __restrict__ part)
{
    __shared__ unsigned red[PP_NKEY][PP_BY];
    const int W = 2 * n, H = 2 * m;
    const int x = blockIdx.x * PP_BX + threadIdx.x, y = blockIdx.y * PP_BY + threadIdx.y;
    const bool inside = x < W && y < H;
    unsigned key[PP_NKEY] = { 0, 0, 0, 0, 0, 0, 0, 0 };
    if (inside) {
        int iu, iv;
        undistort_map(xs[x], ys[y], D, fx, fy, u0, v0, iu, iv);
        const float4 w = tab[(iv & (PP_TAB - 1)) * PP_TAB + (iu & (PP_TAB - 1))];
        const int sx = (int)(short)(iu >> 5), sy = (int)(short)(iv >> 5);
        // the taps (sy, sx), (sy, sx + 1), (sy + 1, sx), (sy + 1, sx + 1) of the upscaled pictures
        const UpTap tx0 = up_tap(sx, n), tx1 = up_tap(sx + 1, n), ty0 = up_tap(sy, m), ty1 = up_tap(sy + 1, m);
        // tx1.a is tx0.a or tx0.b, ty1.a is ty0.a or ty0.b: three columns and three rows of macro-pixels
        const int col[3] = { tx0.a, tx0.b, tx1.b }, row[3] = { ty0.a, ty0.b, ty1.b };
        const bool x1_first = tx1.a == tx0.a, y1_first = ty1.a == ty0.a;
        Q4 h0[3], h1[3];                                // the rows resized along x at sx and at sx + 1
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const Q4 qa = load_quad(mosaic, stride, row[r], col[0]);
            const Q4 qb = load_quad(mosaic, stride, row[r], col[1]);
            const Q4 qc = load_quad(mosaic, stride, row[r], col[2]);
            h0[r] = lerp2(qa, qb, tx0.wa, tx0.wb);
            h1[r] = lerp2(pick(x1_first, qa, qb), qc, tx1.wa, tx1.wb);
        }
        const Q4 v00 = masked(ty0.ok && tx0.ok, lerp2(h0[0], h0[1], ty0.wa, ty0.wb));
        const Q4 v01 = masked(ty0.ok && tx1.ok, lerp2(h1[0], h1[1], ty0.wa, ty0.wb));
        const Q4 v10 = masked(ty1.ok && tx0.ok, lerp2(pick(y1_first, h0[0], h0[1]), h0[2], ty1.wa, ty1.wb));
        const Q4 v11 = masked(ty1.ok && tx1.ok, lerp2(pick(y1_first, h1[0], h1[1]), h1[2], ty1.wa, ty1.wb));
        // the undistorted channels
        const float a0 = tap_sum(v00.i0, v01.i0, v10.i0, v11.i0, w);
        const float a45 = tap_sum(v00.i45, v01.i45, v10.i45, v11.i45, w);
        const float a90 = tap_sum(v00.i90, v01.i90, v10.i90, v11.i90, w);
        const float a135 = tap_sum(v00.i135, v01.i135, v10.i135, v11.i135, w);
        // enforce I0 + I90 = I45 + I135
        const float k1 = 0.75f, k2 = 0.25f;
        const float I0 = ((k1 * a0 + k2 * a45) - k2 * a90) + k2 * a135;
        const float I45 = ((k2 * a0 + k1 * a45) + k2 * a90) - k2 * a135;
        const float I90 = ((-k2 * a0 + k2 * a45) + k1 * a90) + k2 * a135;
        const float I135 = ((k2 * a0 - k2 * a45) + k2 * a90) + k1 * a135;
        const float S0 = (((I0 + I45) + I90) + I135) * 0.5f;
        const float S1 = I0 - I90;
        const float S2 = I45 - I135;
        const size_t HW = (size_t)H * W, i = (size_t)y * W + x;
        if (o.S) { o.S[i] = S0; o.S[HW + i] = S1; o.S[2 * HW + i] = S2; }
        if (S0 == S0) { key[1] = order_key(S0); key[0] = ~key[1]; }
        if (S1 == S1) { key[3] = order_key(S1); key[2] = ~key[3]; }
        if (S2 == S2) { key[5] = order_key(S2); key[4] = ~key[5]; }
        float pic;
        if (hdr) {
            const float w0 = hdr_weight(I0), w45 = hdr_weight(I45), w90 = hdr_weight(I90), w135 = hdr_weight(I135);
            const float num = ((w0 * I0 + w45 * I45) + w90 * I90) + w135 * I135;
            const float den = ((w0 + w45) + w90) + w135;
            pic = div_f32(num, den) * 255.0f;
        } else {
            pic = S0 * 127.0f;
        }
        o.image[i] = sat_u8(pic);
        if (o.image_f32) o.image_f32[i] = pic;
        if (o.dolp) {
            const float q = S1 * S1 + S2 * S2;
            const float dolp = div_f32((float)sqrt((double)q), S0);
            if (dolp == dolp) { key[7] = order_key(dolp); key[6] = ~key[7]; }
            o.dolp[i] = sat_u8(dolp * 255.0f);
        }
        if (o.aolp || o.aolp_f32) {
            double ang = atan2((double)S1, (double)S2);
            if (ang < 0.0) ang += 6.283185307179586;
            const float aolp = ((float)ang - 3.1415f) * 0.5f;
            const float idx = aolp * (float)(255.0 / 3.1415) + 127.0f;
            if (o.aolp) o.aolp[i] = sat_u8(idx);
            if (o.aolp_f32) o.aolp_f32[i] = idx;
        }
        if (o.channels) {
            o.channels[i] = sat_u8(I0 * 255.0f);
            o.channels[HW + i] = sat_u8(I45 * 255.0f);
            o.channels[2 * HW + i] = sat_u8(I90 * 255.0f);
            o.channels[3 * HW + i] = sat_u8(I135 * 255.0f);
        }
    }
    // the block's record: every lane takes part, the ones outside the picture with key 0 (= nothing)
#pragma unroll
    for (int k = 0; k < PP_NKEY; ++k) {
        const unsigned v = wave_max(key[k]);
        if (threadIdx.x == 0) red[k][threadIdx.y] = v;
    }
    __syncthreads();
    if (threadIdx.y == 0 && threadIdx.x < PP_NKEY) {
        unsigned v = red[threadIdx.x][0];
#pragma unroll
        for (int wv = 1; wv < PP_BY; ++wv) v = red[threadIdx.x][wv] > v ? red[threadIdx.x][wv] : v;
        part[((size_t)blockIdx.y * gridDim.x + blockIdx.x) * PP_NKEY + threadIdx.x] = v;
    }
}

// one block: ranges[2 q] = the minimum, ranges[2 q + 1] = the maximum of quantity q, NaN where no value was seen
__global__ void __launch_bounds__(256) k_prepare_pol_ranges(const unsigned* __restrict__ part, unsigned nblocks, float* __restrict__ ranges)
{
    __shared__ unsigned red[PP_NKEY][4];
    unsigned key[PP_NKEY] = { 0, 0, 0, 0, 0, 0, 0, 0 };
    for (unsigned b = threadIdx.x; b < nblocks; b += 256) {
#pragma unroll
        for (int k = 0; k < PP_NKEY; ++k) {
            const unsigned v = part[(size_t)b * PP_NKEY + k];
            key[k] = v > key[k] ? v : key[k];
        }
    }
#pragma unroll
    for (int k = 0; k < PP_NKEY; ++k) {
        const unsigned v = wave_max(key[k]);
        if ((threadIdx.x & 63) == 0) red[k][threadIdx.x >> 6] = v;
    }
    __syncthreads();
    if (threadIdx.x < PP_NKEY) {
        const int k = threadIdx.x;
        unsigned v = red[k][0];
#pragma unroll
        for (int wv = 1; wv < 4; ++wv) v = red[k][wv] > v ? red[k][wv] : v;
        ranges[k] = !v ? __uint_as_float(0x7fc00000u) : order_unkey((k & 1) ? v : ~v);
    }
}

static int prep_check(wass_ctx* c, const void* mosaic, int cols, int rows, size_t stride, const double* K, const double* dist, int n_dist,
                      const wass_pol_prep_params* prm, const wass_pol_prep_out* out)
{
    if (!mosaic || !K || (!dist && n_dist) || !prm || !out || !out->image) return set_err(c, WASS_ERR_INVALID_ARG, "null argument");
    if (rows < 2 || cols < 2 || stride < (size_t)cols)
        return set_err(c, WASS_ERR_INVALID_ARG, "a %d x %d mosaic with a row stride of %zu (at least 2 x 2)", cols, rows, stride);
    if (!(n_dist == 0 || n_dist == 4 || n_dist == 5 || n_dist == 8 || n_dist == 12))
        return set_err(c, WASS_ERR_UNSUPPORTED, "%d distortion coefficients (4, 5, 8 or 12 supported; no tilt model)", n_dist);
    if (cols / 2 * 2 > 32767 || rows / 2 * 2 > 32767) return set_err(c, WASS_ERR_UNSUPPORTED, "pictures larger than 32767 px are not supported");
    if (prm->outputs & ~WASS_PREP_ALL) return set_err(c, WASS_ERR_INVALID_ARG, "unknown bits in outputs (%#x)", prm->outputs);
    if (prm->clahe_tiles < 0) return set_err(c, WASS_ERR_INVALID_ARG, "clahe_tiles must not be negative");
    const int b = prm->outputs;
    if (((b & WASS_PREP_STOKES) && !out->S) || ((b & WASS_PREP_DOLP) && !out->dolp) || ((b & WASS_PREP_AOLP) && !out->aolp) ||
        ((b & WASS_PREP_CHANNELS) && !out->channels) || ((b & WASS_PREP_IMAGE_F32) && !out->image_f32) ||
        ((b & WASS_PREP_AOLP_F32) && !out->aolp_f32))
        return set_err(c, WASS_ERR_INVALID_ARG, "an output named in outputs has no destination");
    return WASS_OK;
}

// everything on the device; returns synchronised (the ranges are host values)
static int prep_dev(wass_ctx* c, const uint8_t* d_mosaic, int cols, int rows, size_t stride, const double* K, const double* dist, int n_dist,
                    const wass_pol_prep_params* prm, wass_pol_prep_out* out)
{
    const int m = rows / 2, n = cols / 2, W = 2 * n, H = 2 * m;
    WASS_HIP(c, hipSetDevice(c->device));
    Dist12 D;
    for (int i = 0; i < 12; ++i) D.k[i] = i < n_dist ? dist[i] : 0.0;
    int rc = ensure_bilinear_tab(c);
    if (rc) return rc;
    if ((rc = wait_uploads(c, d_mosaic, c->stream))) return rc;
    const double* dxy = nullptr;
    if ((rc = undistort_tables(c, K, W, H, &dxy))) return rc;
    const dim3 block(PP_BX, PP_BY), grid((W + PP_BX - 1) / PP_BX, (H + PP_BY - 1) / PP_BY);
    const size_t nblocks = (size_t)grid.x * grid.y;
    unsigned* part;
    float* d_ranges;
    if ((rc = carve_buf(c, c->prep_pol, [&](Carve& a) {
            part = a.take<unsigned>(nblocks * PP_NKEY * sizeof(unsigned)); d_ranges = a.take<float>(PP_NKEY * sizeof(float));
        })))
        return rc;
    const int b = prm->outputs;
    PrepOut o;
    o.S = (b & WASS_PREP_STOKES) ? out->S : nullptr;
    o.dolp = (b & WASS_PREP_DOLP) ? out->dolp : nullptr;
    o.aolp = (b & WASS_PREP_AOLP) ? out->aolp : nullptr;
    o.channels = (b & WASS_PREP_CHANNELS) ? out->channels : nullptr;
    o.image_f32 = (b & WASS_PREP_IMAGE_F32) ? out->image_f32 : nullptr;
    o.aolp_f32 = (b & WASS_PREP_AOLP_F32) ? out->aolp_f32 : nullptr;
    o.image = out->image;
    if (prm->clahe_tiles > 0) {                         // the equalisation reads the plain picture from the staging buffer
        if ((rc = ensure(c, c->tmp_in1, (size_t)W * H))) return rc;
        o.image = (uint8_t*)c->tmp_in1.p;
    }
    hipStream_t s = c->stream;
    hipLaunchKernelGGL(k_prepare_pol, grid, block, 0, s, d_mosaic, stride, m, n, dxy, dxy + W, D, K[0], K[4], K[2], K[5], prm->hdr ? 1 : 0, o,
                       (const float4*)c->bilinear_tab.p, part);
    hipLaunchKernelGGL(k_prepare_pol_ranges, dim3(1), dim3(256), 0, s, (const unsigned*)part, (unsigned)nblocks, d_ranges);
    WASS_HIP(c, hipGetLastError());
    if (prm->clahe_tiles > 0 &&
        (rc = wass_clahe_dev(c, o.image, W, H, (size_t)W, prm->clahe_clip, prm->clahe_tiles, prm->clahe_tiles, out->image)))
        return rc;
    WASS_HIP(c, hipMemcpyAsync(out->ranges, d_ranges, PP_NKEY * sizeof(float), hipMemcpyDeviceToHost, s));
    WASS_HIP(c, hipStreamSynchronize(s));
    if (!(b & WASS_PREP_DOLP)) out->ranges[6] = out->ranges[7] = NAN;
    return WASS_OK;
}

}  // namespace wass

using namespace wass;

extern "C" int wass_prepare_pol_dev(wass_ctx* c, const uint8_t* d_mosaic, int cols, int rows, size_t stride, const double K[9], const double* dist,
                                    int n_dist, const wass_pol_prep_params* params, wass_pol_prep_out* out)
{
    if (!c) return WASS_ERR_INVALID_ARG;
    const int rc = prep_check(c, d_mosaic, cols, rows, stride, K, dist, n_dist, params, out);
    if (rc) return rc;
    return prep_dev(c, d_mosaic, cols, rows, stride, K, dist, n_dist, params, out);
}

extern "C" int wass_prepare_pol(wass_ctx* c, const uint8_t* mosaic, int cols, int rows, size_t stride, const double K[9], const double* dist,
                                int n_dist, const wass_pol_prep_params* params, wass_pol_prep_out* out)
{
    if (!c) return WASS_ERR_INVALID_ARG;
    int rc = prep_check(c, mosaic, cols, rows, stride, K, dist, n_dist, params, out);
    if (rc) return rc;
    WASS_HIP(c, hipSetDevice(c->device));
    const int W = cols / 2 * 2, H = rows / 2 * 2, b = params->outputs;
    const size_t HW = (size_t)W * H;
    // the staged results, in the order of the members; what was not asked for is not taken and stays null
    wass_pol_prep_out d = {};
    if ((rc = ensure(c, c->tmp_in0, HW)) || (rc = carve_buf(c, c->tmp_out, [&](Carve& a) {
            if (b & WASS_PREP_STOKES) d.S = a.take<float>(HW * 12);
            d.image = a.take<uint8_t>(HW);
            if (b & WASS_PREP_DOLP) d.dolp = a.take<uint8_t>(HW);
            if (b & WASS_PREP_AOLP) d.aolp = a.take<uint8_t>(HW);
            if (b & WASS_PREP_CHANNELS) d.channels = a.take<uint8_t>(HW * 4);
            if (b & WASS_PREP_IMAGE_F32) d.image_f32 = a.take<float>(HW * 4);
            if (b & WASS_PREP_AOLP_F32) d.aolp_f32 = a.take<float>(HW * 4);
        })))
        return rc;
    hipStream_t s = c->stream;
    // the odd last row and column are dropped here
    WASS_HIP(c, hipMemcpy2DAsync(c->tmp_in0.p, (size_t)W, mosaic, stride, (size_t)W, (size_t)H, hipMemcpyHostToDevice, s));
    if ((rc = prep_dev(c, (const uint8_t*)c->tmp_in0.p, W, H, (size_t)W, K, dist, n_dist, params, &d))) return rc;
    void* const dst[7] = { out->S, out->image, out->dolp, out->aolp, out->channels, out->image_f32, out->aolp_f32 };
    const void* const src[7] = { d.S, d.image, d.dolp, d.aolp, d.channels, d.image_f32, d.aolp_f32 };
    const size_t bytes[7] = { HW * 12, HW, HW, HW, HW * 4, HW * 4, HW * 4 };
    for (int k = 0; k < 7; ++k)
        if (src[k]) WASS_HIP(c, hipMemcpyAsync(dst[k], src[k], bytes[k], hipMemcpyDeviceToHost, s));
    WASS_HIP(c, hipStreamSynchronize(s));
    memcpy(out->ranges, d.ranges, sizeof d.ranges);
    return WASS_OK;
}
