// kaze.hip -- the KAZE feature detector of wass_match (FeatureSet::detect calls cv::KAZE): a non-linear scale space at full
// resolution, the Hessian-determinant response, its 3-level extrema with sub-pixel refinement, the dominant orientation and
// the 64-value M-SURF descriptor.  include/wass_gpu.h states every operation order; DESIGN.md "Feature detector" the layout.
//
// Every stencil kernel runs 64 x 4 threads on a 64 x 4 tile of the picture and reads global memory directly: a row of a
// wave is one 256-byte line and the neighbouring rows come out of L2.  For the scaled Scharr (taps up to 22 pixels apart) no
// tile of LDS covers the reach without reading more than it saves.  For the Gaussian passes and the diffusion step an LDS
// tile, and several diffusion steps per launch through halos, would save traffic and launches; that is not built and not
// measured (DESIGN.md "Feature detector": the diffusion reaches a third of the HBM rate as it stands).
// Everything is float32 without contraction (-ffp-contract=off), division and square root correctly rounded, so a stage made
// of + - x / sqrt is the same number on the device and in numpy (the square root is taken in fp64 and rounded once more, which is
// the correctly rounded float32 root; the fast intrinsic is not).

#include "common.h"

#include <math.h>

namespace wass {

constexpr int KZ_TX = 64, KZ_TY = 4;
constexpr int KZ_MAX_TAPS = 15;
constexpr int KZ_HIST = 300;
constexpr int KZ_MAX_LEVELS = 32;

struct KazeTaps {
    float t[KZ_MAX_TAPS];
    int n;
};

struct KazeSigmas {
    float esigma[KZ_MAX_LEVELS];
};

static dim3 kz_grid(int h, int w, int z = 1) { return dim3((unsigned)((w + KZ_TX - 1) / KZ_TX), (unsigned)((h + KZ_TY - 1) / KZ_TY), (unsigned)z); }

__device__ __forceinline__ int kz_clamp(int i, int n) { return i < 0 ? 0 : (i >= n ? n - 1 : i); }
__device__ __forceinline__ int kz_r101(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i); }   // the caller keeps the reach below n

// ------------------------------------------------------------------------------------------------------------- pre-smoothing
__global__ __launch_bounds__(256) void k_kaze_u8(const uint8_t* __restrict__ src, size_t pitch, float* __restrict__ dst, int h, int w, float scale)
{
    const int x = blockIdx.x * KZ_TX + threadIdx.x, y = blockIdx.y * KZ_TY + threadIdx.y;
    if (x >= w || y >= h) return;
    dst[(size_t)y * w + x] = (float)src[(size_t)y * pitch + x] * scale;
}

// one pass of the separable Gaussian, border replicated; the taps are summed from the first to the last
template <bool VERT>
__global__ __launch_bounds__(256) void k_kaze_conv(const float* __restrict__ src, float* __restrict__ dst, int h, int w, KazeTaps taps)
{
    const int x = blockIdx.x * KZ_TX + threadIdx.x, y = blockIdx.y * KZ_TY + threadIdx.y;
    if (x >= w || y >= h) return;
    const int r = taps.n / 2;
    float acc = 0.0f;
    for (int j = 0; j < taps.n; ++j) {
        const int xx = VERT ? x : kz_clamp(x + j - r, w), yy = VERT ? kz_clamp(y + j - r, h) : y;
        acc = acc + taps.t[j] * src[(size_t)yy * w + xx];
    }
    dst[(size_t)y * w + x] = acc;
}

// ------------------------------------------------------------------------------------------------------------- derivatives
// scaled Scharr, reach s, reflect-101.  Rows first, then columns:
//   Lx = (n * d(y-s) + wn * d(y)) + n * d(y+s),    d(r) = src[r][x+s] - src[r][x-s]
//   Ly = m(y+s) - m(y-s),                          m(r) = (n * src[r][x-s] + wn * src[r][x]) + n * src[r][x+s]
__device__ __forceinline__ float kz_dx(const float* __restrict__ p, int h, int w, int y, int x, int s, float n, float wn)
{
    const int xm = kz_r101(x - s, w), xp = kz_r101(x + s, w);
    const float* r0 = p + (size_t)kz_r101(y - s, h) * w;
    const float* r1 = p + (size_t)y * w;
    const float* r2 = p + (size_t)kz_r101(y + s, h) * w;
    const float d0 = r0[xp] - r0[xm], d1 = r1[xp] - r1[xm], d2 = r2[xp] - r2[xm];
    return (n * d0 + wn * d1) + n * d2;
}

__device__ __forceinline__ float kz_dy(const float* __restrict__ p, int h, int w, int y, int x, int s, float n, float wn)
{
    const int xm = kz_r101(x - s, w), xp = kz_r101(x + s, w);
    const float* r0 = p + (size_t)kz_r101(y - s, h) * w;
    const float* r2 = p + (size_t)kz_r101(y + s, h) * w;
    const float m0 = (n * r0[xm] + wn * r0[x]) + n * r0[xp];
    const float m2 = (n * r2[xm] + wn * r2[x]) + n * r2[xp];
    return m2 - m0;
}

__global__ __launch_bounds__(256) void k_kaze_scharr(const float* __restrict__ src, float* __restrict__ lx, float* __restrict__ ly, int h, int w, int s,
                                                     float n, float wn)
{
    const int x = blockIdx.x * KZ_TX + threadIdx.x, y = blockIdx.y * KZ_TY + threadIdx.y;
    if (x >= w || y >= h) return;
    lx[(size_t)y * w + x] = kz_dx(src, h, w, y, x, s, n, wn);
    ly[(size_t)y * w + x] = kz_dy(src, h, w, y, x, s, n, wn);
}

// second derivatives of the UNSCALED first ones, each times ss2 = sigma_size^2, and Ldet = Lxx * Lyy - Lxy * Lxy
__global__ __launch_bounds__(256) void k_kaze_hessian(const float* __restrict__ lx, const float* __restrict__ ly, float* __restrict__ ldet,
                                                      float* __restrict__ oxx, float* __restrict__ oxy, float* __restrict__ oyy, int h, int w, int s,
                                                      float n, float wn, float ss2)
{
    const int x = blockIdx.x * KZ_TX + threadIdx.x, y = blockIdx.y * KZ_TY + threadIdx.y;
    if (x >= w || y >= h) return;
    const float lxx = kz_dx(lx, h, w, y, x, s, n, wn) * ss2;
    const float lxy = kz_dy(lx, h, w, y, x, s, n, wn) * ss2;
    const float lyy = kz_dy(ly, h, w, y, x, s, n, wn) * ss2;
    const size_t i = (size_t)y * w + x;
    if (oxx) oxx[i] = lxx;
    if (oxy) oxy[i] = lxy;
    if (oyy) oyy[i] = lyy;
    ldet[i] = lxx * lyy - lxy * lxy;
}

__global__ __launch_bounds__(256) void k_kaze_scale2(float* __restrict__ a, float* __restrict__ b, size_t count, float m)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    a[i] = a[i] * m;
    b[i] = b[i] * m;
}

// ----------------------------------------------------------------------------------------------------------- contrast factor
// the largest gradient modulus over the interior: moduli are not negative, so their bit patterns order like the numbers
__global__ __launch_bounds__(256) void k_kaze_hmax(const float* __restrict__ lx, const float* __restrict__ ly, int h, int w, unsigned* __restrict__ rec)
{
    const int x = blockIdx.x * KZ_TX + threadIdx.x, y = blockIdx.y * KZ_TY + threadIdx.y;
    unsigned bits = 0;
    if (x >= 1 && x < w - 1 && y >= 1 && y < h - 1) {
        const float a = lx[(size_t)y * w + x], b = ly[(size_t)y * w + x];
        bits = __float_as_uint((float)sqrt((double)(a * a + b * b)));
    }
    __shared__ unsigned best;
    if (threadIdx.x == 0 && threadIdx.y == 0) best = 0;
    __syncthreads();
    if (bits) atomicMax(&best, bits);
    __syncthreads();
    if (threadIdx.x == 0 && threadIdx.y == 0 && best) atomicMax(&rec[0], best);
}

// rec[0] = bits of hmax, rec[1] = number of non-zero moduli, rec[2 ..] = the 300 bins: integer sums, the same in any order
__global__ __launch_bounds__(256) void k_kaze_hist(const float* __restrict__ lx, const float* __restrict__ ly, int h, int w, unsigned* __restrict__ rec)
{
    __shared__ unsigned bins[KZ_HIST + 1];
    const int t = threadIdx.y * KZ_TX + threadIdx.x;
    for (int i = t; i <= KZ_HIST; i += 256) bins[i] = 0;
    __syncthreads();
    const int x = blockIdx.x * KZ_TX + threadIdx.x, y = blockIdx.y * KZ_TY + threadIdx.y;
    const float hmax = __uint_as_float(rec[0]);
    if (x >= 1 && x < w - 1 && y >= 1 && y < h - 1) {
        const float a = lx[(size_t)y * w + x], b = ly[(size_t)y * w + x];
        const float m = (float)sqrt((double)(a * a + b * b));
        if (m != 0.0f) {
            int bin = (int)floorf((float)KZ_HIST * (m / hmax));
            bin = bin >= KZ_HIST ? KZ_HIST - 1 : bin;
            atomicAdd(&bins[bin], 1u);
            atomicAdd(&bins[KZ_HIST], 1u);
        }
    }
    __syncthreads();
    for (int i = t; i <= KZ_HIST; i += 256)
        if (bins[i]) atomicAdd(&rec[i == KZ_HIST ? 1 : 2 + i], bins[i]);
}

// --------------------------------------------------------------------------------------------------------------- diffusion
__global__ __launch_bounds__(256) void k_kaze_flow(const float* __restrict__ lx, const float* __restrict__ ly, float* __restrict__ flow, size_t count,
                                                   float k2)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    const float a = lx[i], b = ly[i];
    flow[i] = 1.0f / (1.0f + (a * a + b * b) / k2);
}

// one explicit step: out = L + half_tau * (((xpos - xneg) + ypos) - yneg); a term whose neighbour is outside the picture is 0
__global__ __launch_bounds__(256) void k_kaze_step(const float* __restrict__ L, const float* __restrict__ c, float* __restrict__ out, int h, int w,
                                                   float half_tau)
{
    const int x = blockIdx.x * KZ_TX + threadIdx.x, y = blockIdx.y * KZ_TY + threadIdx.y;
    if (x >= w || y >= h) return;
    const size_t i = (size_t)y * w + x;
    const float l = L[i], cc = c[i];
    const float xpos = x + 1 < w ? (c[i + 1] + cc) * (L[i + 1] - l) : 0.0f;
    const float xneg = x > 0 ? (cc + c[i - 1]) * (l - L[i - 1]) : 0.0f;
    const float ypos = y + 1 < h ? (c[i + w] + cc) * (L[i + w] - l) : 0.0f;
    const float yneg = y > 0 ? (cc + c[i - w]) * (l - L[i - w]) : 0.0f;
    out[i] = l + half_tau * (((xpos - xneg) + ypos) - yneg);
}

// ----------------------------------------------------------------------------------------------------------------- extrema
// levels 1 .. nlev-2, interior pixels: v above the threshold and 1e-5, strictly above its 8 neighbours and the 9 + 9 of the levels
// next to it, and round(x -+ 3 esigma), round(y -+ 3 esigma) inside the picture.  A candidate is the key (level * h + y) * w + x;
// count[0] counts every candidate, keys holds the first `cap` that arrive.
__global__ __launch_bounds__(256) void k_kaze_extrema(const float* __restrict__ ldet, size_t plane, int nlev, int h, int w, float threshold,
                                                      KazeSigmas sg, long long* __restrict__ keys, int cap, unsigned* __restrict__ count)
{
    const int x = blockIdx.x * KZ_TX + threadIdx.x, y = blockIdx.y * KZ_TY + threadIdx.y, lev = 1 + (int)blockIdx.z;
    if (x < 1 || x >= w - 1 || y < 1 || y >= h - 1 || lev > nlev - 2) return;
    const float* C = ldet + (size_t)lev * plane;
    const size_t i = (size_t)y * w + x;
    const float v = C[i];
    if (!(v > threshold) || !(v >= 1e-5f)) return;
    for (int dl = -1; dl <= 1; ++dl) {
        const float* P = dl < 0 ? C - plane : (dl > 0 ? C + plane : C);
        for (int dy = -1; dy <= 1; ++dy)
            for (int dx = -1; dx <= 1; ++dx) {
                if (dl == 0 && dy == 0 && dx == 0) continue;
                if (!(v > P[i + (ptrdiff_t)dy * w + dx])) return;
            }
    }
    const float r = 3.0f * sg.esigma[lev];
    if (rintf((float)x - r) < 0.0f || rintf((float)x + r) >= (float)w || rintf((float)y - r) < 0.0f || rintf((float)y + r) >= (float)h) return;
    const unsigned slot = atomicAdd(count, 1u);
    if (slot < (unsigned)cap) keys[slot] = ((long long)lev * h + y) * w + x;
}

// 3 x 3 system in float32, elimination with partial pivoting (the first of equal pivots), operation order of the header
__device__ bool kz_solve3(float a[3][4], float* sol)
{
    for (int k = 0; k < 3; ++k) {
        int p = k;
        for (int r = k + 1; r < 3; ++r)
            if (fabsf(a[r][k]) > fabsf(a[p][k])) p = r;
        if (p != k)
            for (int c = 0; c < 4; ++c) {
                const float t = a[k][c];
                a[k][c] = a[p][c];
                a[p][c] = t;
            }
        if (a[k][k] == 0.0f) return false;
        for (int r = k + 1; r < 3; ++r) {
            const float f = a[r][k] / a[k][k];
            for (int c = k + 1; c < 4; ++c) a[r][c] = a[r][c] - f * a[k][c];
        }
    }
    sol[2] = a[2][3] / a[2][2];
    sol[1] = (a[1][3] - a[1][2] * sol[2]) / a[1][1];
    sol[0] = ((a[0][3] - a[0][1] * sol[1]) - a[0][2] * sol[2]) / a[0][0];
    return true;
}

// out[i] = x + dx, y + dy, ds, |v|, kept (1 / 0)
__global__ __launch_bounds__(64) void k_kaze_refine(const float* __restrict__ ldet, size_t plane, int nlev, int h, int w,
                                                    const long long* __restrict__ keys, int n, float* __restrict__ out)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const long long key = keys[i];
    const int x = (int)(key % w), y = (int)((key / w) % h), lev = (int)(key / ((long long)w * h));
    float* o = out + (size_t)i * 5;
    o[0] = (float)x; o[1] = (float)y; o[2] = 0.0f; o[3] = 0.0f; o[4] = 0.0f;
    if (x < 1 || x >= w - 1 || y < 1 || y >= h - 1 || lev < 1 || lev > nlev - 2) return;     // not a key of k_kaze_extrema: refused
    const float* C = ldet + (size_t)lev * plane + (size_t)y * w + x;
    const float* D = C - plane;
    const float* U = C + plane;
    const float v = C[0];
    const float Dx = 0.5f * (C[1] - C[-1]), Dy = 0.5f * (C[w] - C[-w]), Ds = 0.5f * (U[0] - D[0]);
    const float Dxx = (C[1] + C[-1]) - 2.0f * v, Dyy = (C[w] + C[-w]) - 2.0f * v, Dss = (U[0] + D[0]) - 2.0f * v;
    const float Dxy = 0.25f * ((C[w + 1] + C[-w - 1]) - (C[-w + 1] + C[w - 1]));
    const float Dxs = 0.25f * ((U[1] + D[-1]) - (U[-1] + D[1]));
    const float Dys = 0.25f * ((U[w] + D[-w]) - (U[-w] + D[w]));
    float a[3][4] = {{Dxx, Dxy, Dxs, -Dx}, {Dxy, Dyy, Dys, -Dy}, {Dxs, Dys, Dss, -Ds}};
    float d[3];
    o[3] = fabsf(v);
    if (!kz_solve3(a, d)) return;
    if (!(fabsf(d[0]) <= 1.0f && fabsf(d[1]) <= 1.0f && fabsf(d[2]) <= 1.0f)) return;
    o[0] = (float)x + d[0];
    o[1] = (float)y + d[1];
    o[2] = d[2];
    o[4] = 1.0f;
}

// ------------------------------------------------------------------------------------------------------------- orientation
__constant__ float kz_gauss25[7][7] = {
    {0.02546481f, 0.02350698f, 0.01849125f, 0.01239505f, 0.00708017f, 0.00344629f, 0.00142946f},
    {0.02350698f, 0.02169968f, 0.01706957f, 0.01144208f, 0.00653582f, 0.00318132f, 0.00131956f},
    {0.01849125f, 0.01706957f, 0.01342740f, 0.00900066f, 0.00514126f, 0.00250252f, 0.00103800f},
    {0.01239505f, 0.01144208f, 0.00900066f, 0.00603332f, 0.00344629f, 0.00167749f, 0.00069579f},
    {0.00708017f, 0.00653582f, 0.00514126f, 0.00344629f, 0.00196855f, 0.00095820f, 0.00039744f},
    {0.00344629f, 0.00318132f, 0.00250252f, 0.00167749f, 0.00095820f, 0.00046640f, 0.00019346f},
    {0.00142946f, 0.00131956f, 0.00103800f, 0.00069579f, 0.00039744f, 0.00019346f, 0.00008024f}};

constexpr int KZ_ORI_SAMPLES = 109;
constexpr int KZ_ORI_WINDOWS = 42;          // ang1 = 0, 0.15, ... while below 2 pi
#define KZ_2PI 6.2831853071795864769f
#define KZ_PI_3 1.0471975511965976f
#define KZ_5PI_3 5.2359877559829887f

__device__ __forceinline__ float kz_angle(float x, float y)
{
    float a = atan2f(y, x);
    if (a < 0.0f) a += KZ_2PI;
    return a;
}

// kp: n x 5 float32 (x, y, size, level, angle).  One wave per keypoint: a lane takes samples lane and lane + 64 (in the order i outer,
// j inner of the 109 lattice points with i^2 + j^2 < 36), then lane w < 42 sums window w over the samples in that order.
__global__ __launch_bounds__(64) void k_kaze_orientation(const float* __restrict__ kp, int n, const float* __restrict__ lxs, const float* __restrict__ lys,
                                                         size_t plane, int nlev, int h, int w, float* __restrict__ angle)
{
    const int k = blockIdx.x, lane = threadIdx.x;
    if (k >= n) return;
    __shared__ float sx[128], sy[128], sa[128], score[64], wx[64], wy[64];
    const float xf = kp[(size_t)k * 5], yf = kp[(size_t)k * 5 + 1];
    const int s = (int)(kp[(size_t)k * 5 + 2] / 2.0f + 0.5f);
    int lev = (int)kp[(size_t)k * 5 + 3];
    lev = kz_clamp(lev, nlev);
    const float* Lx = lxs + (size_t)lev * plane;
    const float* Ly = lys + (size_t)lev * plane;
    // the lattice, enumerated the same way by every lane
    int idx = 0;
    for (int i = -6; i <= 6; ++i)
        for (int j = -6; j <= 6; ++j) {
            if (i * i + j * j >= 36) continue;
            if ((idx & 63) == lane) {
                const int iy = (int)(yf + (float)(j * s) + 0.5f), ix = (int)(xf + (float)(i * s) + 0.5f);
                float rx = 0.0f, ry = 0.0f;
                if (iy >= 0 && iy < h && ix >= 0 && ix < w) {
                    const float g = kz_gauss25[i < 0 ? -i : i][j < 0 ? -j : j];
                    rx = g * Lx[(size_t)iy * w + ix];
                    ry = g * Ly[(size_t)iy * w + ix];
                }
                sx[idx] = rx;
                sy[idx] = ry;
                sa[idx] = kz_angle(rx, ry);
            }
            ++idx;
        }
    __syncthreads();
    float sumX = 0.0f, sumY = 0.0f;
    if (lane < KZ_ORI_WINDOWS) {
        float ang1 = 0.0f;
        for (int t = 0; t < lane; ++t) ang1 += 0.15f;
        const float ang2 = ang1 + KZ_PI_3 > KZ_2PI ? ang1 - KZ_5PI_3 : ang1 + KZ_PI_3;
        for (int q = 0; q < KZ_ORI_SAMPLES; ++q) {
            const float a = sa[q];
            const bool in = ang1 < ang2 ? (ang1 < a && a < ang2) : (ang2 < ang1 && ((a > 0.0f && a < ang2) || (a > ang1 && a < KZ_2PI)));
            if (in) {
                sumX += sx[q];
                sumY += sy[q];
            }
        }
    }
    score[lane] = sumX * sumX + sumY * sumY;
    wx[lane] = sumX;
    wy[lane] = sumY;
    __syncthreads();
    if (lane == 0) {
        float best = 0.0f, a = 0.0f;
        for (int t = 0; t < KZ_ORI_WINDOWS; ++t)
            if (score[t] > best) {
                best = score[t];
                a = kz_angle(wx[t], wy[t]);
            }
        angle[k] = a;
    }
}

// -------------------------------------------------------------------------------------------------------------- descriptor
constexpr int KZ_DESC_SAMPLES = 16 * 81;

__device__ __forceinline__ float kz_gaussian(float x, float y, float sig) { return expf(-(x * x + y * y) / (2.0f * sig * sig)); }

// One workgroup per keypoint.  Sample q = (subregion, k, l): 256 threads fill the rotated responses of the 1296 samples, 64 threads add
// the 81 of their (subregion, component) in sample order, one thread adds the squared length over the 16 subregions in order.
__global__ __launch_bounds__(256) void k_kaze_descriptor(const float* __restrict__ kp, int n, const float* __restrict__ lxs, const float* __restrict__ lys,
                                                         size_t plane, int nlev, int h, int w, float* __restrict__ desc)
{
    const int kpi = blockIdx.x, t = threadIdx.x;
    if (kpi >= n) return;
    __shared__ float rrxs[KZ_DESC_SAMPLES], rrys[KZ_DESC_SAMPLES], part[64], len2;
    const float xf = kp[(size_t)kpi * 5], yf = kp[(size_t)kpi * 5 + 1];
    const float scale = (float)(int)(kp[(size_t)kpi * 5 + 2] / 2.0f + 0.5f);
    int lev = (int)kp[(size_t)kpi * 5 + 3];
    lev = kz_clamp(lev, nlev);
    const float ang = kp[(size_t)kpi * 5 + 4];
    const float co = cosf(ang), si = sinf(ang);
    const float* Lx = lxs + (size_t)lev * plane;
    const float* Ly = lys + (size_t)lev * plane;
    for (int q = t; q < KZ_DESC_SAMPLES; q += 256) {
        const int sub = q / 81, r = q % 81;
        const int i = -12 + 5 * (sub / 4), j = -12 + 5 * (sub % 4);
        const int k = i + r / 9, l = j + r % 9;
        const float ky = (float)(i + 5), kx = (float)(j + 5);
        const float xs = xf + (-kx * scale * si + ky * scale * co);
        const float ys = yf + (kx * scale * co + ky * scale * si);
        const float sample_y = yf + ((float)l * scale * co + (float)k * scale * si);
        const float sample_x = xf + (-(float)l * scale * si + (float)k * scale * co);
        const float g1 = kz_gaussian(xs - sample_x, ys - sample_y, 2.5f * scale);
        // bilinear: the pixel below the sample and the next one, the fraction taken before the indices are clamped into the picture
        const float flx = floorf(sample_x), fly = floorf(sample_y);
        const float fx = sample_x - flx, fy = sample_y - fly;
        const int y1 = kz_clamp((int)fly, h), x1 = kz_clamp((int)flx, w);
        const int y2 = kz_clamp((int)fly + 1, h), x2 = kz_clamp((int)flx + 1, w);
        const size_t i11 = (size_t)y1 * w + x1, i12 = (size_t)y1 * w + x2, i21 = (size_t)y2 * w + x1, i22 = (size_t)y2 * w + x2;
        const float w1 = (1.0f - fx) * (1.0f - fy), w2 = fx * (1.0f - fy), w3 = (1.0f - fx) * fy, w4 = fx * fy;
        float rx = ((w1 * Lx[i11] + w2 * Lx[i12]) + w3 * Lx[i21]) + w4 * Lx[i22];
        float ry = ((w1 * Ly[i11] + w2 * Ly[i12]) + w3 * Ly[i21]) + w4 * Ly[i22];
        rx = g1 * rx;
        ry = g1 * ry;
        rrys[q] = rx * co + ry * si;
        rrxs[q] = -rx * si + ry * co;
    }
    __syncthreads();
    if (t < 64) {
        const int sub = t / 4, comp = t % 4;
        const float* v = (comp & 1) ? rrys : rrxs;
        float acc = 0.0f;
        for (int r = 0; r < 81; ++r) {
            const float e = v[sub * 81 + r];
            acc += comp >= 2 ? fabsf(e) : e;
        }
        const float cx = (float)(sub / 4) + 0.5f, cy = (float)(sub % 4) + 0.5f;
        part[t] = acc * kz_gaussian(cx - 2.0f, cy - 2.0f, 1.5f);
    }
    __syncthreads();
    if (t == 0) {
        float len = 0.0f;
        for (int q = 0; q < 64; q += 4) len += ((part[q] * part[q] + part[q + 1] * part[q + 1]) + part[q + 2] * part[q + 2]) + part[q + 3] * part[q + 3];
        len2 = (float)sqrt((double)len);
    }
    __syncthreads();
    if (t < 64) desc[(size_t)kpi * 64 + t] = part[t] / len2;
}

static int kz_dims(wass_ctx* c, int h, int w)
{
    if (h < 3 || w < 3 || h > 32768 || w > 32768) return set_err(c, WASS_ERR_INVALID_ARG, "a picture of %d x %d: 3 .. 32768 rows and columns", h, w);
    return WASS_OK;
}

static int kz_done(wass_ctx* c, hipStream_t s)
{
    WASS_HIP(c, hipGetLastError());
    WASS_HIP(c, hipStreamSynchronize(s));
    return WASS_OK;
}

}  // namespace wass

using namespace wass;

extern "C" {

int wass_kaze_scratch_bytes(int h, int w, int n_levels, size_t* bytes)
{
    if (!bytes || h < 3 || w < 3 || h > 32768 || w > 32768 || n_levels < 3 || n_levels > WASS_KAZE_MAX_LEVELS) return WASS_ERR_INVALID_ARG;
    const size_t plane = (size_t)h * w * sizeof(float);
    // Lx, Ly, Ldet of every level; the chain: Lt, its ping-pong twin, Lsmooth, the convolution's row pass, flow, and two planes of
    // first derivatives for the flow and the contrast factor; the picture itself
    *bytes = plane * 3 * (size_t)n_levels + plane * 7 + (size_t)h * w + (size_t)WASS_KAZE_MAX_CANDIDATES * (8 + 20) + 4 * (2 + KZ_HIST);
    return WASS_OK;
}

int wass_kaze_convert_dev(wass_ctx* c, const uint8_t* d_src, size_t pitch, int h, int w, float scale, float* d_dst)
{
    if (!c) return WASS_ERR_INVALID_ARG;
    if (!d_src || !d_dst || pitch < (size_t)w) return set_err(c, WASS_ERR_INVALID_ARG, "null argument or a pitch below the width");
    int rc = kz_dims(c, h, w);
    if (rc) return rc;
    WASS_HIP(c, hipSetDevice(c->device));
    hipLaunchKernelGGL(k_kaze_u8, kz_grid(h, w), dim3(KZ_TX, KZ_TY), 0, c->ts(), d_src, pitch, d_dst, h, w, scale);
    return kz_done(c, c->ts());
}

int wass_kaze_gauss_dev(wass_ctx* c, const float* d_src, int h, int w, const float* taps, int ntaps, float* d_tmp, float* d_dst)
{
    if (!c) return WASS_ERR_INVALID_ARG;
    if (!d_src || !taps || !d_tmp || !d_dst) return set_err(c, WASS_ERR_INVALID_ARG, "null argument");
    if (ntaps < 1 || ntaps > KZ_MAX_TAPS || !(ntaps & 1)) return set_err(c, WASS_ERR_INVALID_ARG, "%d taps: an odd number up to %d", ntaps, KZ_MAX_TAPS);
    if (d_tmp == d_src || d_tmp == d_dst) return set_err(c, WASS_ERR_INVALID_ARG, "the row pass needs a plane of its own");
    int rc = kz_dims(c, h, w);
    if (rc) return rc;
    WASS_HIP(c, hipSetDevice(c->device));
    KazeTaps t = {};
    t.n = ntaps;
    for (int i = 0; i < ntaps; ++i) t.t[i] = taps[i];
    hipLaunchKernelGGL(k_kaze_conv<false>, kz_grid(h, w), dim3(KZ_TX, KZ_TY), 0, c->ts(), d_src, d_tmp, h, w, t);
    hipLaunchKernelGGL(k_kaze_conv<true>, kz_grid(h, w), dim3(KZ_TX, KZ_TY), 0, c->ts(), (const float*)d_tmp, d_dst, h, w, t);
    return kz_done(c, c->ts());
}

static int kz_reach(wass_ctx* c, int h, int w, int s)
{
    if (s < 1 || s >= h || s >= w) return set_err(c, WASS_ERR_INVALID_ARG, "a reflect-101 reach of %d pixels in a picture of %d x %d", s, h, w);
    return WASS_OK;
}

int wass_kaze_scharr_dev(wass_ctx* c, const float* d_src, int h, int w, int sigma_size, float norm, float wnorm, float* d_lx, float* d_ly)
{
    if (!c) return WASS_ERR_INVALID_ARG;
    if (!d_src || !d_lx || !d_ly || d_lx == d_src || d_ly == d_src || d_lx == d_ly) return set_err(c, WASS_ERR_INVALID_ARG, "three different planes");
    int rc = kz_dims(c, h, w);
    if (rc || (rc = kz_reach(c, h, w, sigma_size))) return rc;
    WASS_HIP(c, hipSetDevice(c->device));
    hipLaunchKernelGGL(k_kaze_scharr, kz_grid(h, w), dim3(KZ_TX, KZ_TY), 0, c->ts(), d_src, d_lx, d_ly, h, w, sigma_size, norm, wnorm);
    return kz_done(c, c->ts());
}

int wass_kaze_hessian_dev(wass_ctx* c, float* d_lx, float* d_ly, int h, int w, int sigma_size, float norm, float wnorm, float* d_ldet, float* d_lxx,
                          float* d_lxy, float* d_lyy)
{
    if (!c) return WASS_ERR_INVALID_ARG;
    if (!d_lx || !d_ly || !d_ldet || d_ldet == d_lx || d_ldet == d_ly || d_lx == d_ly) return set_err(c, WASS_ERR_INVALID_ARG, "three different planes");
    int rc = kz_dims(c, h, w);
    if (rc || (rc = kz_reach(c, h, w, sigma_size))) return rc;
    WASS_HIP(c, hipSetDevice(c->device));
    const float ss = (float)sigma_size;
    hipLaunchKernelGGL(k_kaze_hessian, kz_grid(h, w), dim3(KZ_TX, KZ_TY), 0, c->ts(), (const float*)d_lx, (const float*)d_ly, d_ldet, d_lxx, d_lxy, d_lyy,
                       h, w, sigma_size, norm, wnorm, ss * ss);
    const size_t count = (size_t)h * w;
    hipLaunchKernelGGL(k_kaze_scale2, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, c->ts(), d_lx, d_ly, count, ss);
    return kz_done(c, c->ts());
}

int wass_kaze_contrast_dev(wass_ctx* c, const float* d_lx, const float* d_ly, int h, int w, uint32_t* d_rec, float* hmax, uint32_t* npoints,
                           uint32_t* hist)
{
    if (!c) return WASS_ERR_INVALID_ARG;
    if (!d_lx || !d_ly || !d_rec || !hmax || !npoints || !hist) return set_err(c, WASS_ERR_INVALID_ARG, "null argument");
    int rc = kz_dims(c, h, w);
    if (rc) return rc;
    WASS_HIP(c, hipSetDevice(c->device));
    hipStream_t s = c->ts();
    uint32_t rec[2 + KZ_HIST];
    WASS_HIP(c, hipMemsetAsync(d_rec, 0, sizeof rec, s));
    hipLaunchKernelGGL(k_kaze_hmax, kz_grid(h, w), dim3(KZ_TX, KZ_TY), 0, s, d_lx, d_ly, h, w, d_rec);
    hipLaunchKernelGGL(k_kaze_hist, kz_grid(h, w), dim3(KZ_TX, KZ_TY), 0, s, d_lx, d_ly, h, w, d_rec);
    WASS_HIP(c, hipGetLastError());
    WASS_HIP(c, hipMemcpyAsync(rec, d_rec, sizeof rec, hipMemcpyDeviceToHost, s));
    WASS_HIP(c, hipStreamSynchronize(s));
    memcpy(hmax, &rec[0], 4);
    *npoints = rec[1];
    memcpy(hist, rec + 2, KZ_HIST * sizeof(uint32_t));
    return WASS_OK;
}

int wass_kaze_flow_dev(wass_ctx* c, const float* d_lx, const float* d_ly, int h, int w, float k, float* d_flow)
{
    if (!c) return WASS_ERR_INVALID_ARG;
    if (!d_lx || !d_ly || !d_flow) return set_err(c, WASS_ERR_INVALID_ARG, "null argument");
    int rc = kz_dims(c, h, w);
    if (rc) return rc;
    WASS_HIP(c, hipSetDevice(c->device));
    const size_t count = (size_t)h * w;
    hipLaunchKernelGGL(k_kaze_flow, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, c->ts(), d_lx, d_ly, d_flow, count, k * k);
    return kz_done(c, c->ts());
}

int wass_kaze_diffuse_dev(wass_ctx* c, float* d_lt, float* d_tmp, const float* d_flow, int h, int w, const float* taus, int ntaus)
{
    if (!c) return WASS_ERR_INVALID_ARG;
    if (!d_lt || !d_tmp || !d_flow || !taus || d_lt == d_tmp) return set_err(c, WASS_ERR_INVALID_ARG, "null argument or one plane for both sides of a step");
    if (ntaus < 0 || ntaus > 65536) return set_err(c, WASS_ERR_INVALID_ARG, "%d steps", ntaus);
    int rc = kz_dims(c, h, w);
    if (rc) return rc;
    WASS_HIP(c, hipSetDevice(c->device));
    hipStream_t s = c->ts();
    float *a = d_lt, *b = d_tmp;
    for (int i = 0; i < ntaus; ++i) {
        hipLaunchKernelGGL(k_kaze_step, kz_grid(h, w), dim3(KZ_TX, KZ_TY), 0, s, (const float*)a, d_flow, b, h, w, 0.5f * taus[i]);
        float* t = a;
        a = b;
        b = t;
    }
    WASS_HIP(c, hipGetLastError());
    if (a != d_lt) WASS_HIP(c, hipMemcpyAsync(d_lt, a, (size_t)h * w * sizeof(float), hipMemcpyDeviceToDevice, s));
    WASS_HIP(c, hipStreamSynchronize(s));
    return WASS_OK;
}

int wass_kaze_extrema_dev(wass_ctx* c, const float* d_ldet, size_t plane_stride, int n_levels, int h, int w, float threshold, const float* esigma,
                          int64_t* d_keys, int cap, uint32_t* d_count, uint32_t* count)
{
    if (!c) return WASS_ERR_INVALID_ARG;
    if (!d_ldet || !esigma || !d_keys || !d_count || !count) return set_err(c, WASS_ERR_INVALID_ARG, "null argument");
    if (n_levels < 3 || n_levels > WASS_KAZE_MAX_LEVELS) return set_err(c, WASS_ERR_INVALID_ARG, "%d levels: 3 .. %d", n_levels, WASS_KAZE_MAX_LEVELS);
    if (cap < 1 || cap > WASS_KAZE_MAX_CANDIDATES) return set_err(c, WASS_ERR_INVALID_ARG, "a cap of %d candidates: 1 .. %d", cap, WASS_KAZE_MAX_CANDIDATES);
    if (plane_stride < (size_t)h * w) return set_err(c, WASS_ERR_INVALID_ARG, "a plane stride below the plane");
    int rc = kz_dims(c, h, w);
    if (rc) return rc;
    WASS_HIP(c, hipSetDevice(c->device));
    hipStream_t s = c->ts();
    KazeSigmas sg = {};
    for (int i = 0; i < n_levels; ++i) sg.esigma[i] = esigma[i];
    WASS_HIP(c, hipMemsetAsync(d_count, 0, sizeof(uint32_t), s));
    hipLaunchKernelGGL(k_kaze_extrema, kz_grid(h, w, n_levels - 2), dim3(KZ_TX, KZ_TY), 0, s, d_ldet, plane_stride, n_levels, h, w, threshold, sg,
                       (long long*)d_keys, cap, d_count);
    WASS_HIP(c, hipGetLastError());
    WASS_HIP(c, hipMemcpyAsync(count, d_count, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    WASS_HIP(c, hipStreamSynchronize(s));
    if (*count > (uint32_t)cap) return WASS_KAZE_CAP_REACHED;
    return WASS_OK;
}

int wass_kaze_refine_dev(wass_ctx* c, const float* d_ldet, size_t plane_stride, int n_levels, int h, int w, const int64_t* d_keys, int n, float* d_out)
{
    if (!c) return WASS_ERR_INVALID_ARG;
    if (!d_ldet || !d_keys || !d_out) return set_err(c, WASS_ERR_INVALID_ARG, "null argument");
    if (n_levels < 3 || n_levels > WASS_KAZE_MAX_LEVELS) return set_err(c, WASS_ERR_INVALID_ARG, "%d levels: 3 .. %d", n_levels, WASS_KAZE_MAX_LEVELS);
    if (n < 1) return set_err(c, WASS_ERR_INVALID_ARG, "no keypoints");
    if (plane_stride < (size_t)h * w) return set_err(c, WASS_ERR_INVALID_ARG, "a plane stride below the plane");
    int rc = kz_dims(c, h, w);
    if (rc) return rc;
    WASS_HIP(c, hipSetDevice(c->device));
    hipLaunchKernelGGL(k_kaze_refine, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, c->ts(), d_ldet, plane_stride, n_levels, h, w,
                       (const long long*)d_keys, n, d_out);
    return kz_done(c, c->ts());
}

static int kz_kp_args(wass_ctx* c, const void* kp, int n, const void* lx, const void* ly, size_t plane_stride, int n_levels, int h, int w, const void* out)
{
    if (!c) return WASS_ERR_INVALID_ARG;
    if (!kp || !lx || !ly || !out) return set_err(c, WASS_ERR_INVALID_ARG, "null argument");
    if (n < 1) return set_err(c, WASS_ERR_INVALID_ARG, "no keypoints");
    if (n_levels < 1 || n_levels > WASS_KAZE_MAX_LEVELS) return set_err(c, WASS_ERR_INVALID_ARG, "%d levels: 1 .. %d", n_levels, WASS_KAZE_MAX_LEVELS);
    if (plane_stride < (size_t)h * w) return set_err(c, WASS_ERR_INVALID_ARG, "a plane stride below the plane");
    return kz_dims(c, h, w);
}

int wass_kaze_orientation_dev(wass_ctx* c, const float* d_kp, int n, const float* d_lx, const float* d_ly, size_t plane_stride, int n_levels, int h, int w,
                              float* d_angle)
{
    int rc = kz_kp_args(c, d_kp, n, d_lx, d_ly, plane_stride, n_levels, h, w, d_angle);
    if (rc) return rc;
    WASS_HIP(c, hipSetDevice(c->device));
    hipLaunchKernelGGL(k_kaze_orientation, dim3((unsigned)n), dim3(64), 0, c->ts(), d_kp, n, d_lx, d_ly, plane_stride, n_levels, h, w, d_angle);
    return kz_done(c, c->ts());
}

int wass_kaze_descriptors_dev(wass_ctx* c, const float* d_kp, int n, const float* d_lx, const float* d_ly, size_t plane_stride, int n_levels, int h, int w,
                              float* d_desc)
{
    int rc = kz_kp_args(c, d_kp, n, d_lx, d_ly, plane_stride, n_levels, h, w, d_desc);
    if (rc) return rc;
    WASS_HIP(c, hipSetDevice(c->device));
    hipLaunchKernelGGL(k_kaze_descriptor, dim3((unsigned)n), dim3(256), 0, c->ts(), d_kp, n, d_lx, d_ly, plane_stride, n_levels, h, w, d_desc);
    return kz_done(c, c->ts());
}

}  // extern "C"
