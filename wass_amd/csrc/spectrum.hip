// spectrum.hip -- wave spectra of the gridded cube: the two array functions of postproc/wasspost/spectra.py,
// compute_3D_spectrum (:53-171, Welch's method over 3-D segments) and compute_spectrum (:9-49, scipy.signal.csd of the centre
// series and its neighbours).  The host side (wass_amd/postproc.py) computes axes, windows and the scale in fp64; segments come
// here.
//
// The window lengths are whatever two thirds of the grid gives (683 is prime, 684 is not, Nt is any even number), so the DFT is
// a product with a twiddle matrix on v_mfma_f32_16x16x4_f32 (exact f32, a k-ordered fma chain), the idiom of grid_dct.hip, for
// every length alike:
//   k_seg_cell / k_seg_mean / k_seg_window   NaN fill by the cell's mean over the segment, global mean, separable Hann window
//   k_dft_stage  x:  real [t][y][x]      -> complex [t][y][kx],  kx = 0 .. nx/2 only (the input is real)
//   k_dft_stage  y:  complex [t][y][kx]  -> complex [t][ky][kx]  (one product per t)
//   k_dft_stage  t:  complex [t][ky][kx] -> complex [f][ky][kx]
//   k_spec_power     S[fftshift] += |X|^2 in fp64, the other half of kx read at the mirrored (-f, -ky, -kx)
// Every stage is  Out[m][n] = sum_k (cos - i sin)(2 pi m k / len) In[k][n]  with the twiddle as the A operand: only the strides of
// In and Out differ.  A workgroup of four waves makes a 64 x 64 tile of Out: the twiddle and input tiles of 16 k go through LDS
// (the next pair is in flight from global memory while the current one is multiplied), every wave keeps a 32 x 32 patch, i.e.
// eight 16 x 16 accumulators (real and imaginary).  No reduction uses an atomic: the same input gives the same bits.
//
// Scratch of one handle, in units of one real f32 copy of the window (nt * ny * nx * 4 bytes): 1 for the prepared segment, 1 for
// the host-pointer staging, about 2 for the two complex half-spectra the stages alternate between, 2 for the fp64 Welch sum:
// about 6, i.e. 1.1 GB at 100 x 684 x 684 and 3.4 GB at 300 x 684 x 684.  SPEC_SCRATCH_CAP bounds it.
#include "cube.h"

#include <math.h>
#include <new>
#include <vector>

namespace wass {

typedef float sp_f32x4 __attribute__((ext_vector_type(4)));

constexpr size_t SPEC_SCRATCH_CAP = (size_t)16 << 30;   // bytes one handle / one wass_spec1d_welch call may allocate
constexpr int SPEC_MAX_AXIS = 8192;                     // longest transform
constexpr int SP_TM = 64, SP_TN = 64, SP_TK = 16;       // tile of k_dft_stage
constexpr int SP_LD = 80;                               // LDS row pitch: the four k rows of one MFMA operand fall on banks 0 / 16 / 32 / 48

static inline int sp_round_up(int v, int m) { return (v + m - 1) / m * m; }

// C[k][m] = cos(2 pi k m / n), S[k][m] = sin(2 pi k m / n) for k < n, m < nm; 0 in the padding (Kp rows of Mp).  fp64 with the angle
// reduced exactly, (k m) mod n in integers, then cast to f32.
__global__ void __launch_bounds__(256) k_dft_twiddle(float* __restrict__ Cm, float* __restrict__ Sm, int n, int nm, int Mp)
{
    const int m = blockIdx.x * 256 + threadIdx.x, k = blockIdx.y;
    if (m >= Mp) return;
    double c = 0.0, s = 0.0;
    if (k < n && m < nm) {
        const long long r = ((long long)k * m) % n;
        const double a = 6.283185307179586476925286766559 * (double)r / (double)n;
        c = cos(a);
        s = sin(a);
    }
    Cm[(size_t)k * Mp + m] = (float)c;
    Sm[(size_t)k * Mp + m] = (float)s;
}

struct DftArgs {
    const float* Tc; const float* Ts; int Mp;       // twiddle pair, [Kp][Mp]
    const float* Bre; const float* Bim;             // input planes (Bim unused for a real input)
    float* Ore; float* Oim;                         // output planes
    int M, N, K;                                    // output rows, columns, contraction length (unpadded)
    long long b_sk, b_sn, b_sb;                     // element strides of the input: k, n, batch (blockIdx.z)
    long long o_sm, o_sn, o_sb;                     // ... of the output
};

// KCONTIG: the input's k is its contiguous axis (the x stage), else n is.  Loads outside K x N read as 0, stores outside M x N are
// dropped; the twiddle's padding is 0, so nothing outside the problem reaches an accumulator.
template <bool CPLX, bool KCONTIG>
__global__ void __launch_bounds__(256) k_dft_stage(const DftArgs a)
{
    __shared__ __attribute__((aligned(16))) float As_c[SP_TK][SP_LD];
    __shared__ __attribute__((aligned(16))) float As_s[SP_TK][SP_LD];
    __shared__ float Bs_r[SP_TK][SP_LD];
    __shared__ float Bs_i[CPLX ? SP_TK : 1][SP_LD];

    const int tid = threadIdx.x, l = tid & 63, w = tid >> 6, lo = l & 15, hi = l >> 4;
    const int m0 = blockIdx.y * SP_TM, n0 = blockIdx.x * SP_TN;
    const float* __restrict__ Bre = a.Bre + (long long)blockIdx.z * a.b_sb;
    const float* __restrict__ Bim = CPLX ? a.Bim + (long long)blockIdx.z * a.b_sb : nullptr;

    // this thread's part of a tile pair: one float4 of each twiddle, four scalars of each input plane
    const int ak = tid >> 4, am = (tid & 15) * 4;
    const int bk = KCONTIG ? (tid & 15) : (tid >> 6), bn = KCONTIG ? (tid >> 4) : (tid & 63);
    constexpr int BK_STEP = KCONTIG ? 0 : 4, BN_STEP = KCONTIG ? 16 : 0;
    sp_f32x4 pc, ps;
    float pr[4], pi[4];
    auto fetch = [&](int k0) {
        pc = *(const sp_f32x4*)&a.Tc[(size_t)(k0 + ak) * a.Mp + m0 + am];
        ps = *(const sp_f32x4*)&a.Ts[(size_t)(k0 + ak) * a.Mp + m0 + am];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int k = k0 + bk + i * BK_STEP, n = n0 + bn + i * BN_STEP;
            const bool in = k < a.K && n < a.N;
            const long long q = (long long)k * a.b_sk + (long long)n * a.b_sn;
            pr[i] = in ? Bre[q] : 0.f;
            if (CPLX) pi[i] = in ? Bim[q] : 0.f;
        }
    };

    sp_f32x4 acc_re[2][2], acc_im[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            acc_re[i][j] = sp_f32x4{0.f, 0.f, 0.f, 0.f};
            acc_im[i][j] = sp_f32x4{0.f, 0.f, 0.f, 0.f};
        }
    const int wm = (w & 1) * 32, wn = (w >> 1) * 32;
    const int nk = (a.K + SP_TK - 1) / SP_TK;
    fetch(0);
    for (int kt = 0; kt < nk; ++kt) {
        __syncthreads();                               // the previous tile pair has been read by every wave
        *(sp_f32x4*)&As_c[ak][am] = pc;
        *(sp_f32x4*)&As_s[ak][am] = ps;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            Bs_r[bk + i * BK_STEP][bn + i * BN_STEP] = pr[i];
            if (CPLX) Bs_i[bk + i * BK_STEP][bn + i * BN_STEP] = pi[i];
        }
        __syncthreads();
        if (kt + 1 < nk) fetch((kt + 1) * SP_TK);      // in flight under the MFMAs below
#pragma unroll
        for (int s = 0; s < SP_TK / 4; ++s) {
            const int kk = 4 * s + hi;
            float ac[2], as[2], an[2], br[2], bi[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                ac[i] = As_c[kk][wm + 16 * i + lo];
                as[i] = As_s[kk][wm + 16 * i + lo];
                an[i] = -as[i];
                br[i] = Bs_r[kk][wn + 16 * i + lo];
                bi[i] = CPLX ? Bs_i[kk][wn + 16 * i + lo] : 0.f;
            }
            // (c - i s)(br + i bi) = (c br + s bi) + i (c bi - s br)
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    acc_re[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(ac[i], br[j], acc_re[i][j], 0, 0, 0);
                    acc_im[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(an[i], br[j], acc_im[i][j], 0, 0, 0);
                    if (CPLX) {
                        acc_re[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(as[i], bi[j], acc_re[i][j], 0, 0, 0);
                        acc_im[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(ac[i], bi[j], acc_im[i][j], 0, 0, 0);
                    }
                }
        }
    }
    // acc[i][j][r] = Out[m0 + wm + 16 i + 4 hi + r][n0 + wn + 16 j + lo]
    float* __restrict__ Ore = a.Ore + (long long)blockIdx.z * a.o_sb;
    float* __restrict__ Oim = a.Oim + (long long)blockIdx.z * a.o_sb;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int m = m0 + wm + 16 * i + 4 * hi + r, n = n0 + wn + 16 * j + lo;
                if (m < a.M && n < a.N) {
                    const long long q = (long long)m * a.o_sm + (long long)n * a.o_sn;
                    Ore[q] = acc_re[i][j][r];
                    Oim[q] = acc_im[i][j][r];
                }
            }
}

// One thread per cell, the frames in order: the cell's mean over its frames that are not NaN (np.nanmean(axis=0) of the float32
// segment times datascale: a float32 sum), NaN and *flag = 1 for a cell that is NaN throughout.  part[block] = the fp64 sum of
// the block's cells after the fill (the cells of all-NaN columns count as 0).
__global__ void __launch_bounds__(256) k_seg_cell(const float* __restrict__ src, long long st, long long sy, int nt, int ny, int nx, float ds,
                                                  float* __restrict__ cellmean, double* __restrict__ part, int* __restrict__ flag)
{
    __shared__ double sh[256];
    const int i = blockIdx.x * 256 + threadIdx.x;
    double tot = 0.0;
    if (i < ny * nx) {
        const float* p = src + (long long)(i / nx) * sy + (i % nx);
        float s = 0.f;
        double sd = 0.0;
        int cnt = 0;
        for (int t = 0; t < nt; ++t) {
            const float v = p[(long long)t * st] * ds;
            if (!isnan(v)) { s += v; sd += (double)v; ++cnt; }
        }
        const float m = cnt ? s / (float)cnt : __builtin_nanf("");
        cellmean[i] = m;
        if (!cnt) *flag = 1;
        else tot = sd + (double)(nt - cnt) * (double)m;
    }
    tot = block_sum<256>(tot, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = tot;
}

// mean[0] = (the partials, thread-strided then a tree) / count
__global__ void __launch_bounds__(256) k_seg_mean(const double* __restrict__ part, int npart, double count, double* __restrict__ mean)
{
    __shared__ double sh[256];
    double s = 0.0;
    for (int i = threadIdx.x; i < npart; i += 256) s += part[i];
    s = block_sum<256>(s, sh);
    if (threadIdx.x == 0) mean[0] = s / count;
}

// out[t][y][x] = (fill(src * datascale) - mean) * ((wy[y] wx[x]) wt[t]): float32 up to the subtraction like the reference, the window
// product in fp64, then f32 for the MFMA.  A cell that is NaN throughout gives 0 (the flag has recorded it): no NaN reaches the MFMA.
__global__ void __launch_bounds__(256) k_seg_window(const float* __restrict__ src, long long st, long long sy, int nt, int ny, int nx, float ds,
                                                    const float* __restrict__ cellmean, const double* __restrict__ mean,
                                                    const double* __restrict__ wt, const double* __restrict__ wy, const double* __restrict__ wx,
                                                    float* __restrict__ out)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x, cells = (size_t)ny * nx;
    if (i >= (size_t)nt * cells) return;
    const int t = (int)(i / cells), c = (int)(i % cells), y = c / nx, x = c % nx;
    float v = src[(long long)t * st + (long long)y * sy + x] * ds;
    if (isnan(v)) v = cellmean[c];
    float r = 0.f;
    if (!isnan(v)) r = (float)((double)(v - (float)mean[0]) * ((wy[y] * wx[x]) * wt[t]));
    out[i] = r;
}

// S[it][iy][ix] (np.fft.fftshift on the three axes) += |X(f, ky, kx)|^2 in fp64.  Only kx <= nx / 2 was computed: the rest is read
// at (-f, -ky, -kx), where the spectrum of a real input has the same modulus -- nx - kx <= nx / 2 for even and odd nx alike.
__global__ void __launch_bounds__(256) k_spec_power(const float* __restrict__ Xre, const float* __restrict__ Xim, int nt, int ny, int nx, int nxh,
                                                    double* __restrict__ S)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x, cells = (size_t)ny * nx;
    if (i >= (size_t)nt * cells) return;
    const int it = (int)(i / cells), c = (int)(i % cells), iy = c / nx, ix = c % nx;
    int f = (it + nt - nt / 2) % nt, ky = (iy + ny - ny / 2) % ny, kx = (ix + nx - nx / 2) % nx;
    if (kx > nx / 2) {
        kx = nx - kx;
        ky = (ny - ky) % ny;
        f = (nt - f) % nt;
    }
    const size_t q = ((size_t)f * ny + ky) * nxh + kx;
    const double re = (double)Xre[q], im = (double)Xim[q];
    S[i] += re * re + im * im;
}

__global__ void __launch_bounds__(256) k_spec_scale(double* __restrict__ S, size_t n, double scale)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) S[i] *= scale;
}

// ---- the batched 1-D Welch estimate -----------------------------------------------------------------------------------------
// smean[k] = mean over the series of (float)(x * scale), fp64, thread-strided then a tree
__global__ void __launch_bounds__(256) k_w1_mean(const float* __restrict__ x, int T, float scale, double* __restrict__ smean)
{
    __shared__ double sh[256];
    x += (size_t)blockIdx.x * T;
    double s = 0.0;
    for (int i = threadIdx.x; i < T; i += 256) s += (double)(x[i] * scale);
    s = block_sum<256>(s, sh);
    if (threadIdx.x == 0) smean[blockIdx.x] = s / (double)T;
}

// Segment blockIdx.x of series blockIdx.y: d = x * scale - smean, minus the segment's own mean (detrend='constant'), times the
// window; written as column (series * nseg + segment) of B[nps][ncol], the layout k_dft_stage contracts.
__global__ void __launch_bounds__(256) k_w1_prep(const float* __restrict__ x, int T, float scale, const double* __restrict__ smean, int nps, int step,
                                                 int nseg, const double* __restrict__ win, float* __restrict__ B)
{
    __shared__ double sh[256];
    const int seg = blockIdx.x, ser = blockIdx.y;
    const size_t ncol = (size_t)gridDim.y * nseg, col = (size_t)ser * nseg + seg;
    const float* p = x + (size_t)ser * T + (size_t)seg * step;
    const double m = smean[ser];
    double s = 0.0;
    for (int i = threadIdx.x; i < nps; i += 256) s += (double)(p[i] * scale) - m;
    const double sm = block_sum<256>(s, sh) / (double)nps;
    for (int i = threadIdx.x; i < nps; i += 256) B[(size_t)i * ncol + col] = (float)((((double)(p[i] * scale) - m) - sm) * win[i]);
}

// out[m] = factor[m] * sum over the columns (series-major, segments in order) of |X[m][col]|^2, fp64
__global__ void __launch_bounds__(256) k_w1_power(const float* __restrict__ Xre, const float* __restrict__ Xim, size_t ncol, double dens, int nps,
                                                  double* __restrict__ out)
{
    __shared__ double sh[256];
    const int m = blockIdx.x;
    double s = 0.0;
    for (size_t i = threadIdx.x; i < ncol; i += 256) {
        const double re = (double)Xre[(size_t)m * ncol + i], im = (double)Xim[(size_t)m * ncol + i];
        s += re * re + im * im;
    }
    s = block_sum<256>(s, sh);
    // one-sided: every bin but DC and (even nps) Nyquist stands for two
    const bool twice = m != 0 && !(nps % 2 == 0 && m == nps / 2);
    if (threadIdx.x == 0) out[m] = s * dens * (twice ? 2.0 : 1.0);
}

static int launch_dft(wass_ctx* c, hipStream_t s, const DftArgs& a, bool cplx, bool kcontig, int batch)
{
    const dim3 grid((a.N + SP_TN - 1) / SP_TN, (a.M + SP_TM - 1) / SP_TM, batch);
    if (grid.y > 65535 || grid.z > 65535) return set_err(c, WASS_ERR_UNSUPPORTED, "transform too large");
    if (cplx && kcontig) hipLaunchKernelGGL((k_dft_stage<true, true>), grid, dim3(256), 0, s, a);
    else if (cplx) hipLaunchKernelGGL((k_dft_stage<true, false>), grid, dim3(256), 0, s, a);
    else if (kcontig) hipLaunchKernelGGL((k_dft_stage<false, true>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((k_dft_stage<false, false>), grid, dim3(256), 0, s, a);
    WASS_HIP(c, hipGetLastError());
    return WASS_OK;
}

// p + n, or nullptr for a piece of an Arena that only measures
template <class T> static T* piece_at(T* p, size_t n) { return p ? p + n : nullptr; }

struct Twiddle {
    float* c = nullptr;
    float* s = nullptr;
    int n = 0, nm = 0, Kp = 0, Mp = 0;
};

// one twiddle pair for a transform of length n with nm outputs, taken from the arena: 2 * Kp * Mp floats (a multiple of 256 bytes)
static Twiddle make_twiddle(Arena& a, int n, int nm)
{
    Twiddle t;
    t.n = n;
    t.nm = nm;
    t.Kp = sp_round_up(n, SP_TK);
    t.Mp = sp_round_up(nm, SP_TM);
    t.c = a.take<float>((size_t)2 * t.Kp * t.Mp * 4);
    t.s = piece_at(t.c, (size_t)t.Kp * t.Mp);
    return t;
}

static int fill_twiddle(wass_ctx* c, hipStream_t s, const Twiddle& t)
{
    hipLaunchKernelGGL(k_dft_twiddle, dim3((t.Mp + 255) / 256, t.Kp), dim3(256), 0, s, t.c, t.s, t.n, t.nm, t.Mp);
    WASS_HIP(c, hipGetLastError());
    return WASS_OK;
}

}  // namespace wass

using namespace wass;

struct wass_spec3d {
    wass_spec3d(wass_ctx* c_, int nt_, int ny_, int nx_) : c(c_), nt(nt_), ny(ny_), nx(nx_), nxh(nx_ / 2 + 1) {}
    wass_ctx* c;
    int nt, ny, nx, nxh;
    Arena arena;                   // one allocation, carved by carve()
    float* raw = nullptr;          // staging of a host segment, [nt][ny][nx]
    float* prep = nullptr;         // the prepared segment
    float* a_re = nullptr; float* a_im = nullptr;   // [nt][ny][nxh]: x stage out, t stage out
    float* b_re = nullptr; float* b_im = nullptr;   // y stage out
    double* S = nullptr;           // the Welch sum, fftshifted
    double* wt = nullptr; double* wy = nullptr; double* wx = nullptr;
    float* cellmean = nullptr;
    double* part = nullptr; double* mean = nullptr;
    int* flag = nullptr;
    int npart = 0, nseg = 0;
    Twiddle tx, ty, tt;
};

namespace {

// The handle's pieces, in the order of its allocation.  Run on an Arena that has reserved nothing it measures: a.used is what
// the handle needs.
void carve(wass_spec3d& h, Arena& a)
{
    const size_t cells = (size_t)h.ny * h.nx, win = (size_t)h.nt * cells, half = (size_t)h.nt * h.ny * h.nxh;
    h.npart = (int)((cells + 255) / 256);
    h.raw = a.take<float>(win * 4);
    h.prep = a.take<float>(win * 4);
    h.a_re = a.take<float>(2 * half * 4); h.a_im = piece_at(h.a_re, half);
    h.b_re = a.take<float>(2 * half * 4); h.b_im = piece_at(h.b_re, half);
    h.S = a.take<double>(win * 8);
    h.wt = a.take<double>((size_t)(h.nt + h.ny + h.nx) * 8); h.wy = piece_at(h.wt, h.nt); h.wx = piece_at(h.wy, h.ny);
    h.cellmean = a.take<float>(cells * 4);
    h.part = a.take<double>(((size_t)h.npart + 1) * 8); h.mean = piece_at(h.part, h.npart);
    h.flag = a.take<int>(256);
    h.tx = make_twiddle(a, h.nx, h.nxh);
    h.ty = make_twiddle(a, h.ny, h.ny);
    h.tt = make_twiddle(a, h.nt, h.nt);
}

size_t spec3d_bytes(int nt, int ny, int nx)
{
    wass_spec3d h(nullptr, nt, ny, nx);
    carve(h, h.arena);
    return h.arena.used;
}

bool spec3d_dims_ok(int nt, int ny, int nx)
{
    return nt >= 1 && ny >= 1 && nx >= 1 && nt <= SPEC_MAX_AXIS && ny <= SPEC_MAX_AXIS && nx <= SPEC_MAX_AXIS;
}

// symmetric Hann, scipy.signal.windows.hann(n): 0.5 - 0.5 cos(2 pi i / (n - 1)); hann(1) = [1]
void hann_symmetric(int n, double* w)
{
    for (int i = 0; i < n; ++i) w[i] = n == 1 ? 1.0 : 0.5 - 0.5 * cos(6.283185307179586476925286766559 * (double)i / (double)(n - 1));
}

int spec3d_run(wass_spec3d* h, const float* d_seg, size_t stride_t, size_t stride_y, double datascale)
{
    wass_ctx* c = h->c;
    hipStream_t s = c->ts();
    const int nt = h->nt, ny = h->ny, nx = h->nx, nxh = h->nxh;
    const size_t win = (size_t)nt * ny * nx;
    const float ds = (float)datascale;
    hipLaunchKernelGGL(k_seg_cell, dim3(h->npart), dim3(256), 0, s, d_seg, (long long)stride_t, (long long)stride_y, nt, ny, nx, ds, h->cellmean,
                       h->part, h->flag);
    hipLaunchKernelGGL(k_seg_mean, dim3(1), dim3(256), 0, s, (const double*)h->part, h->npart, (double)win, h->mean);
    hipLaunchKernelGGL(k_seg_window, dim3((unsigned)((win + 255) / 256)), dim3(256), 0, s, d_seg, (long long)stride_t, (long long)stride_y, nt, ny,
                       nx, ds, (const float*)h->cellmean, (const double*)h->mean, (const double*)h->wt, (const double*)h->wy,
                       (const double*)h->wx, h->prep);
    WASS_HIP(c, hipGetLastError());
    int rc;
    const long long plane = (long long)ny * nxh;
    DftArgs x = {h->tx.c, h->tx.s, h->tx.Mp, h->prep, nullptr, h->a_re, h->a_im, nxh, nt * ny, nx, 1, nx, 0, 1, nxh, 0};
    if ((rc = launch_dft(c, s, x, false, true, 1))) return rc;
    DftArgs y = {h->ty.c, h->ty.s, h->ty.Mp, h->a_re, h->a_im, h->b_re, h->b_im, ny, nxh, ny, nxh, 1, plane, nxh, 1, plane};
    if ((rc = launch_dft(c, s, y, true, false, nt))) return rc;
    DftArgs t = {h->tt.c, h->tt.s, h->tt.Mp, h->b_re, h->b_im, h->a_re, h->a_im, nt, (int)plane, nt, plane, 1, 0, plane, 1, 0};
    if ((rc = launch_dft(c, s, t, true, false, 1))) return rc;
    hipLaunchKernelGGL(k_spec_power, dim3((unsigned)((win + 255) / 256)), dim3(256), 0, s, (const float*)h->a_re, (const float*)h->a_im, nt, ny, nx,
                       nxh, h->S);
    WASS_HIP(c, hipGetLastError());
    ++h->nseg;
    return WASS_OK;
}

}  // namespace

extern "C" int wass_spec3d_scratch_bytes(int nt, int ny, int nx, size_t* bytes)
{
    if (!bytes || !spec3d_dims_ok(nt, ny, nx)) return WASS_ERR_INVALID_ARG;
    *bytes = spec3d_bytes(nt, ny, nx);
    return WASS_OK;
}

extern "C" void wass_spec3d_destroy(wass_spec3d* h)
{
    if (!h) return;
    if (h->c) (void)hipSetDevice(h->c->device);
    delete h;                      // the arena frees the scratch
}

extern "C" int wass_spec3d_create(wass_ctx* c, int nt, int ny, int nx, const double* win_t, const double* win_y, const double* win_x,
                                  wass_spec3d** out)
{
    if (!c || !out) return set_err(c, WASS_ERR_INVALID_ARG, "null argument");
    *out = nullptr;
    if (!spec3d_dims_ok(nt, ny, nx)) return set_err(c, WASS_ERR_INVALID_ARG, "bad window size %d x %d x %d (each axis 1 .. %d)", nt, ny, nx, SPEC_MAX_AXIS);
    const size_t total = spec3d_bytes(nt, ny, nx);
    if ((size_t)ny * (nx / 2 + 1) > 0x7fffffffu || (size_t)nt * ny > 0x7fffffffu) return set_err(c, WASS_ERR_UNSUPPORTED, "window too large");
    if (total > SPEC_SCRATCH_CAP)
        return set_err(c, WASS_ERR_NO_MEMORY, "a %d x %d x %d window needs %zu bytes of scratch, the cap is %zu", nt, ny, nx, total, SPEC_SCRATCH_CAP);
    WASS_HIP(c, hipSetDevice(c->device));
    wass_spec3d* h = new (std::nothrow) wass_spec3d(c, nt, ny, nx);
    if (!h) return set_err(c, WASS_ERR_NO_MEMORY, "out of host memory");
    int rc = h->arena.reserve(c, total, "the spectrum scratch");
    if (rc) {
        wass_spec3d_destroy(h);
        return rc;
    }
    carve(*h, h->arena);
    hipStream_t s = c->ts();
    std::vector<double> w((size_t)nt + ny + nx);
    if (win_t) memcpy(&w[0], win_t, (size_t)nt * 8); else hann_symmetric(nt, &w[0]);
    if (win_y) memcpy(&w[nt], win_y, (size_t)ny * 8); else hann_symmetric(ny, &w[nt]);
    if (win_x) memcpy(&w[(size_t)nt + ny], win_x, (size_t)nx * 8); else hann_symmetric(nx, &w[(size_t)nt + ny]);
    if (hipMemcpyAsync(h->wt, w.data(), w.size() * 8, hipMemcpyHostToDevice, s) != hipSuccess ||
        hipMemsetAsync(h->S, 0, (size_t)nt * ny * nx * 8, s) != hipSuccess || hipMemsetAsync(h->flag, 0, 256, s) != hipSuccess)
        rc = set_err(c, WASS_ERR_DEVICE, "spectrum set-up failed");
    if (!rc) rc = fill_twiddle(c, s, h->tx);
    if (!rc) rc = fill_twiddle(c, s, h->ty);
    if (!rc) rc = fill_twiddle(c, s, h->tt);
    if (!rc && hipStreamSynchronize(s) != hipSuccess) rc = set_err(c, WASS_ERR_DEVICE, "spectrum set-up failed");   // w leaves scope
    if (rc) {
        wass_spec3d_destroy(h);
        return rc;
    }
    *out = h;
    return WASS_OK;
}

extern "C" int wass_spec3d_push_dev(wass_spec3d* h, const float* d_seg, size_t stride_t, size_t stride_y, double datascale)
{
    if (!h) return WASS_ERR_INVALID_ARG;
    wass_ctx* c = h->c;
    if (!d_seg || stride_y < (size_t)h->nx || stride_t < (size_t)h->nx) return set_err(c, WASS_ERR_INVALID_ARG, "bad segment pointer or strides");
    WASS_HIP(c, hipSetDevice(c->device));
    return spec3d_run(h, d_seg, stride_t, stride_y, datascale);
}

extern "C" int wass_spec3d_push(wass_spec3d* h, const float* seg, size_t stride_t, size_t stride_y, double datascale)
{
    if (!h) return WASS_ERR_INVALID_ARG;
    wass_ctx* c = h->c;
    if (!seg || stride_y < (size_t)h->nx || stride_t < (size_t)h->nx) return set_err(c, WASS_ERR_INVALID_ARG, "bad segment pointer or strides");
    WASS_HIP(c, hipSetDevice(c->device));
    hipStream_t s = c->ts();
    WASS_HIP(c, upload_rows(h->raw, seg, 4, h->nt, 0, h->ny, h->nx, stride_t, stride_y, s));
    return spec3d_run(h, h->raw, (size_t)h->ny * h->nx, h->nx, datascale);
}

// the end of a Welch accumulation: the scaled sum to S, which `kind` says is host or device memory
static int spec3d_finish(wass_spec3d* h, double scale, double* S, hipMemcpyKind kind, int* n_segments, int* had_all_nan_cell)
{
    if (!h) return WASS_ERR_INVALID_ARG;
    wass_ctx* c = h->c;
    if (!S) return set_err(c, WASS_ERR_INVALID_ARG, "null argument");
    if (!h->nseg) return set_err(c, WASS_ERR_INVALID_ARG, "no segment was pushed");
    WASS_HIP(c, hipSetDevice(c->device));
    hipStream_t s = c->ts();
    const size_t win = (size_t)h->nt * h->ny * h->nx;
    int flag = 0;
    hipLaunchKernelGGL(k_spec_scale, dim3((unsigned)((win + 255) / 256)), dim3(256), 0, s, h->S, win, scale);
    WASS_HIP(c, hipGetLastError());
    WASS_HIP(c, hipMemcpyAsync(S, h->S, win * 8, kind, s));
    WASS_HIP(c, hipMemcpyAsync(&flag, h->flag, sizeof flag, hipMemcpyDeviceToHost, s));
    WASS_HIP(c, hipMemsetAsync(h->S, 0, win * 8, s));          // the handle starts over
    WASS_HIP(c, hipMemsetAsync(h->flag, 0, 256, s));
    WASS_HIP(c, hipStreamSynchronize(s));
    if (n_segments) *n_segments = h->nseg;
    if (had_all_nan_cell) *had_all_nan_cell = flag;
    h->nseg = 0;
    return WASS_OK;
}

extern "C" int wass_spec3d_finish(wass_spec3d* h, double scale, double* S, int* n_segments, int* had_all_nan_cell)
{
    return spec3d_finish(h, scale, S, hipMemcpyDeviceToHost, n_segments, had_all_nan_cell);
}

extern "C" int wass_spec3d_finish_dev(wass_spec3d* h, double scale, double* d_S, int* n_segments, int* had_all_nan_cell)
{
    return spec3d_finish(h, scale, d_S, hipMemcpyDeviceToDevice, n_segments, had_all_nan_cell);
}

extern "C" int wass_spec1d_welch(wass_ctx* c, const float* series, int n_series, int n_samples, int nperseg, double fs, double scale, double* S)
{
    if (!c || !series || !S) return set_err(c, WASS_ERR_INVALID_ARG, "null argument");
    if (n_series < 1 || n_series > 65535 || n_samples < 2 || nperseg < 2 || !(fs > 0))
        return set_err(c, WASS_ERR_INVALID_ARG, "bad argument (series %d, samples %d, nperseg %d, fs %g)", n_series, n_samples, nperseg, fs);
    const int nps = nperseg < n_samples ? nperseg : n_samples;       // scipy.signal.csd shrinks nperseg to the series
    if (nps > SPEC_MAX_AXIS) return set_err(c, WASS_ERR_UNSUPPORTED, "nperseg %d > %d", nps, SPEC_MAX_AXIS);
    const int nov = nps / 2, step = nps - nov, nseg = (n_samples - nov) / step, nf = nps / 2 + 1;
    if (nseg < 1 || nseg > 65535) return set_err(c, WASS_ERR_INVALID_ARG, "no segment fits");
    const size_t ncol = (size_t)n_series * nseg;
    if (ncol > 0x7fffffffu) return set_err(c, WASS_ERR_UNSUPPORTED, "too many segments");
    float *d_x, *d_B, *d_Xre, *d_Xim;
    double *d_m, *d_w, *d_o;
    Twiddle tw;
    auto carve = [&](Arena& a) {
        d_x = a.take<float>((size_t)n_series * n_samples * 4);
        d_m = a.take<double>((size_t)n_series * 8);
        d_w = a.take<double>((size_t)nps * 8);
        d_B = a.take<float>((size_t)nps * ncol * 4);
        d_Xre = a.take<float>((size_t)2 * nf * ncol * 4); d_Xim = piece_at(d_Xre, (size_t)nf * ncol);
        d_o = a.take<double>((size_t)nf * 8);
        tw = make_twiddle(a, nps, nf);
    };
    Arena measure, arena;
    carve(measure);
    const size_t total = measure.used;
    if (total > SPEC_SCRATCH_CAP)
        return set_err(c, WASS_ERR_NO_MEMORY, "the Welch estimate needs %zu bytes of scratch, the cap is %zu", total, SPEC_SCRATCH_CAP);
    WASS_HIP(c, hipSetDevice(c->device));
    hipStream_t s = c->ts();
    int rc = arena.reserve(c, total, "the Welch scratch");
    if (rc) return rc;
    carve(arena);
    // periodic Hann (scipy's get_window('hann', n)): 0.5 - 0.5 cos(2 pi i / n)
    std::vector<double> w(nps);
    double sw2 = 0.0;
    for (int i = 0; i < nps; ++i) {
        w[i] = 0.5 - 0.5 * cos(6.283185307179586476925286766559 * (double)i / (double)nps);
        sw2 += w[i] * w[i];
    }
    const double dens = 1.0 / (fs * sw2) / (double)nseg;             // density scaling, mean over the segments
    hipError_t e = hipMemcpyAsync(d_x, series, (size_t)n_series * n_samples * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(d_w, w.data(), (size_t)nps * 8, hipMemcpyHostToDevice, s);
    if (e != hipSuccess) rc = set_err(c, WASS_ERR_DEVICE, "upload of the series: %s", hipGetErrorString(e));
    if (!rc) rc = fill_twiddle(c, s, tw);
    if (!rc) {
        const float sc = (float)scale;
        hipLaunchKernelGGL(k_w1_mean, dim3(n_series), dim3(256), 0, s, (const float*)d_x, n_samples, sc, d_m);
        hipLaunchKernelGGL(k_w1_prep, dim3(nseg, n_series), dim3(256), 0, s, (const float*)d_x, n_samples, sc, (const double*)d_m, nps, step, nseg,
                           (const double*)d_w, d_B);
        DftArgs a = {tw.c, tw.s, tw.Mp, d_B, nullptr, d_Xre, d_Xim, nf, (int)ncol, nps, (long long)ncol, 1, 0, (long long)ncol, 1, 0};
        rc = launch_dft(c, s, a, false, false, 1);
    }
    if (!rc) {
        hipLaunchKernelGGL(k_w1_power, dim3(nf), dim3(256), 0, s, (const float*)d_Xre, (const float*)d_Xim, ncol, dens, nps, d_o);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(S, d_o, (size_t)nf * 8, hipMemcpyDeviceToHost, s);
    }
    return finish(c, rc, e, s, "Welch estimate");
}

// ---- the spatial Butterworth low-pass (postproc/wasspost/spectra.py:176-202, wasspost spatial_lowpass) -------------------------
// real(ifft2(fft2(z) * H)) per frame with the stages above, a batch of frames per launch (blockIdx.z):
//   x   real [b][r][x]      -> complex [b][r][kx], kx = 0 .. cols / 2
//   y   complex [b][r][kx]  -> complex [b][ky][kx]
//   k_spat_mul              X -> conj(X) * H[ky][kx] * w[kx] / (rows cols), fp64 product, one rounding; w = 2 for the columns that
//                           stand for their mirror image too (all but kx = 0 and, cols even, Nyquist)
//   y   again: H is real and even, so the inverse is the conjugate of the forward transform of the conjugate
//   x   complex [b][r][kx]  -> [b][r][x], contraction over kx <= cols / 2 only; its real part is the result: the row's spectrum
//                           is Hermitian, Re(conj(Z) e^{+i a}) = Re(Z e^{-i a}) is what the forward stage computes
// H comes from the host un-shifted: the reference's fftshift / ifftshift pair around the product is a permutation of H.
// A NaN spreads over its frame in the x and y stages and over no other: the frames of a batch share no tile.
namespace wass {

__global__ void __launch_bounds__(256) k_spat_mul(float* __restrict__ re, float* __restrict__ im, const double* __restrict__ Hw, size_t plane,
                                                  size_t total)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const double h = Hw[i % plane];
    re[i] = (float)((double)re[i] * h);
    im[i] = (float)(-((double)im[i] * h));
}

}  // namespace wass

struct wass_spatial_filter {
    wass_spatial_filter(wass_ctx* c_, int rows_, int cols_, int batch_) : c(c_), rows(rows_), cols(cols_), ch(cols_ / 2 + 1), batch(batch_) {}
    wass_ctx* c;
    int rows, cols, ch, batch;
    Arena arena;
    float* io = nullptr;           // [batch][rows][cols]: staged input of the host entry, then the result
    float* dump = nullptr;          // the last stage's imaginary part
    float* a_re = nullptr; float* a_im = nullptr;   // [batch][rows][ch]
    float* b_re = nullptr; float* b_im = nullptr;
    double* Hw = nullptr;           // [rows][ch]
    Twiddle tx, ty;
};

namespace {

bool spat_dims_ok(int rows, int cols, int batch)
{
    return rows >= 1 && cols >= 1 && rows <= SPEC_MAX_AXIS && cols <= SPEC_MAX_AXIS && batch >= 1 && batch <= 65535;
}

// The handle's pieces, in the order of its allocation; on an Arena that has reserved nothing it measures, like the spectrum's.
void carve(wass_spatial_filter& h, Arena& a)
{
    const size_t frames = (size_t)h.rows * h.cols * h.batch, half = (size_t)h.rows * h.ch, halves = half * h.batch;
    h.io = a.take<float>(frames * 4);
    h.dump = a.take<float>(frames * 4);
    h.a_re = a.take<float>(2 * halves * 4); h.a_im = piece_at(h.a_re, halves);
    h.b_re = a.take<float>(2 * halves * 4); h.b_im = piece_at(h.b_re, halves);
    h.Hw = a.take<double>(half * 8);
    h.tx = make_twiddle(a, h.cols, h.cols);
    h.ty = make_twiddle(a, h.rows, h.rows);
}

size_t spat_bytes(int rows, int cols, int batch)
{
    wass_spatial_filter h(nullptr, rows, cols, batch);
    carve(h, h.arena);
    return h.arena.used;
}

// nb frames at d_in (element strides st, sy) -> h->io, [nb][rows][cols]
int spat_run(wass_spatial_filter* h, const float* d_in, long long st, long long sy, int nb)
{
    wass_ctx* c = h->c;
    hipStream_t s = c->ts();
    const int R = h->rows, Cn = h->cols, ch = h->ch;
    const long long half = (long long)R * ch, frame = (long long)R * Cn;
    int rc;
    DftArgs x = {h->tx.c, h->tx.s, h->tx.Mp, d_in, nullptr, h->a_re, h->a_im, ch, R, Cn, 1, sy, st, 1, ch, half};
    if ((rc = launch_dft(c, s, x, false, true, nb))) return rc;
    DftArgs y = {h->ty.c, h->ty.s, h->ty.Mp, h->a_re, h->a_im, h->b_re, h->b_im, R, ch, R, ch, 1, half, ch, 1, half};
    if ((rc = launch_dft(c, s, y, true, false, nb))) return rc;
    const size_t total = (size_t)half * nb;
    hipLaunchKernelGGL(k_spat_mul, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, h->b_re, h->b_im, (const double*)h->Hw, (size_t)half, total);
    WASS_HIP(c, hipGetLastError());
    DftArgs yi = {h->ty.c, h->ty.s, h->ty.Mp, h->b_re, h->b_im, h->a_re, h->a_im, R, ch, R, ch, 1, half, ch, 1, half};
    if ((rc = launch_dft(c, s, yi, true, false, nb))) return rc;
    DftArgs xi = {h->tx.c, h->tx.s, h->tx.Mp, h->a_re, h->a_im, h->io, h->dump, Cn, R, ch, 1, ch, half, 1, Cn, frame};
    return launch_dft(c, s, xi, true, true, nb);
}

int spat_apply(wass_spatial_filter* h, bool host, const float* in, size_t st, size_t sy, int n, float* out, size_t ost, size_t osy)
{
    if (!h) return WASS_ERR_INVALID_ARG;
    wass_ctx* c = h->c;
    if (!in || !out || n < 0 || sy < (size_t)h->cols || osy < (size_t)h->cols || (n > 1 && (st < (size_t)h->cols || ost < (size_t)h->cols)))
        return set_err(c, WASS_ERR_INVALID_ARG, "bad frame pointer, count or strides");
    WASS_HIP(c, hipSetDevice(c->device));
    hipStream_t s = c->ts();
    const int R = h->rows, Cn = h->cols;
    for (int f0 = 0; f0 < n; f0 += h->batch) {
        const int nb = n - f0 < h->batch ? n - f0 : h->batch;
        const float* frames = in + (size_t)f0 * st;
        int rc;
        if (host) {
            WASS_HIP(c, upload_rows(h->io, frames, 4, nb, 0, R, Cn, st, sy, s));
            rc = spat_run(h, h->io, (long long)R * Cn, Cn, nb);
        } else {
            rc = spat_run(h, frames, (long long)st, (long long)sy, nb);
        }
        if (rc) return rc;
        WASS_HIP(c, download_rows(out + (size_t)f0 * ost, h->io, 4, nb, 0, R, Cn, ost, osy, s, host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice));
    }
    if (host) WASS_HIP(c, hipStreamSynchronize(s));
    return WASS_OK;
}

}  // namespace

extern "C" int wass_spatial_filter_scratch_bytes(int rows, int cols, int batch, size_t* bytes)
{
    if (!bytes || !spat_dims_ok(rows, cols, batch)) return WASS_ERR_INVALID_ARG;
    *bytes = spat_bytes(rows, cols, batch);
    return WASS_OK;
}

extern "C" void wass_spatial_filter_destroy(wass_spatial_filter* h)
{
    if (!h) return;
    if (h->c) (void)hipSetDevice(h->c->device);
    if (h->arena.mem) (void)hipDeviceSynchronize();     // the device form of apply returns with its copies in flight
    delete h;                                           // the arena frees the scratch
}

extern "C" int wass_spatial_filter_create(wass_ctx* c, int rows, int cols, const double* H, int batch, wass_spatial_filter** out)
{
    if (!c || !out) return set_err(c, WASS_ERR_INVALID_ARG, "null argument");
    *out = nullptr;
    if (!H) return set_err(c, WASS_ERR_INVALID_ARG, "null argument");
    if (!spat_dims_ok(rows, cols, batch))
        return set_err(c, WASS_ERR_INVALID_ARG, "bad frame size %d x %d (each axis 1 .. %d) or batch %d", rows, cols, SPEC_MAX_AXIS, batch);
    // no more frames per batch than the cap allows
    while (batch > 1 && spat_bytes(rows, cols, batch) > SPEC_SCRATCH_CAP) batch /= 2;
    const size_t total = spat_bytes(rows, cols, batch);
    if (total > SPEC_SCRATCH_CAP)
        return set_err(c, WASS_ERR_NO_MEMORY, "a %d x %d frame needs %zu bytes of scratch, the cap is %zu", rows, cols, total, SPEC_SCRATCH_CAP);
    WASS_HIP(c, hipSetDevice(c->device));
    wass_spatial_filter* h = new (std::nothrow) wass_spatial_filter(c, rows, cols, batch);
    if (!h) return set_err(c, WASS_ERR_NO_MEMORY, "out of host memory");
    int rc = h->arena.reserve(c, total, "the spatial filter's scratch");
    if (rc) {
        wass_spatial_filter_destroy(h);
        return rc;
    }
    carve(*h, h->arena);
    const int ch = h->ch;
    const size_t half = (size_t)rows * ch;
    std::vector<double> hw(half);
    const double inv = 1.0 / ((double)rows * (double)cols);
    for (int ky = 0; ky < rows; ++ky)
        for (int kx = 0; kx < ch; ++kx) {
            const bool alone = kx == 0 || (cols % 2 == 0 && kx == cols / 2);
            hw[(size_t)ky * ch + kx] = H[(size_t)ky * cols + kx] * (alone ? 1.0 : 2.0) * inv;
        }
    hipStream_t s = c->ts();
    if (hipMemcpyAsync(h->Hw, hw.data(), half * 8, hipMemcpyHostToDevice, s) != hipSuccess) rc = set_err(c, WASS_ERR_DEVICE, "spatial filter set-up failed");
    if (!rc) rc = fill_twiddle(c, s, h->tx);
    if (!rc) rc = fill_twiddle(c, s, h->ty);
    if (!rc && hipStreamSynchronize(s) != hipSuccess) rc = set_err(c, WASS_ERR_DEVICE, "spatial filter set-up failed");   // hw leaves scope
    if (rc) {
        wass_spatial_filter_destroy(h);
        return rc;
    }
    *out = h;
    return WASS_OK;
}

extern "C" int wass_spatial_filter_apply(wass_spatial_filter* h, const float* frames, size_t stride_t, size_t stride_y, int n_frames, float* out,
                                         size_t out_stride_t, size_t out_stride_y)
{
    return spat_apply(h, true, frames, stride_t, stride_y, n_frames, out, out_stride_t, out_stride_y);
}

extern "C" int wass_spatial_filter_apply_dev(wass_spatial_filter* h, const float* d_frames, size_t stride_t, size_t stride_y, int n_frames,
                                             float* d_out, size_t out_stride_t, size_t out_stride_y)
{
    return spat_apply(h, false, d_frames, stride_t, stride_y, n_frames, d_out, out_stride_t, out_stride_y);
}

// ---- the wavenumber-frequency filter of the whole cube (beyond the reference; DESIGN.md, "Dispersion filter") -------------------
// y = real(ifftn(fftn(p) * H)) over nt x ny x nx, p the cube minus every cell's time mean with its NaN samples at 0, H real and even,
// f32, in the un-shifted half layout [nt][ny][ch] of np.fft.rfftn.  The stages above do the work:
//   k_kf_prepare   cell mean (fp64, frame order), p, one bit per NaN sample, the counts and sum p^2
//   x, y, t        k_dft_stage, as spec3d_run
//   k_kf_mul       X -> conj(X) * H * w / (nt ny nx), the rule of k_spat_mul with the weight made on the fly from the f32 mask
//   t, y           k_dft_stage again: H is even, so the inverse is the conjugate of the forward transform of the conjugate
//   k_dft_close    x: complex half spectrum [row][kx] -> real [row][x].  Only the real accumulators of k_dft_stage<true, true>, in its k
//                  order (the same bits), no imaginary plane stored anywhere; the tile goes through LDS so that a wave stores whole
//                  256-byte pieces of rows; the epilogue adds the cell mean, puts the NaN samples back and sums y^2
// k_kf_shell makes the dispersion-shell mask on the device from host maps: comparisons, one subtraction and two products, nothing else.
// No atomic on a floating-point number anywhere: the same input gives the same bits.
namespace wass {

constexpr int KF_RESTORE_MEAN = 1, KF_KEEP_NAN = 2, KF_NO_CENTRE = 4;
constexpr int KF_STAGES = 10;                           // upload + prepare, x, y, t, mul, t, y, (k_dft_stage<true, true>,) close, download
constexpr int KF_CL_LD = 68;                            // LDS row pitch of k_dft_close's output tile: 16-byte aligned rows

// One thread per cell, the frames in order, twice: the fp64 sum and count of the samples that are not NaN, then p and the bitmap.
// bits[t * wpf + (cell >> 6)] bit (cell & 63) = sample (t, cell) is NaN: one wave's ballot is one word.  means[cell] = m_c, NaN for a
// cell that is NaN throughout (it enters as zeros; k_dft_close reads the NaN as "empty").  part[block * 4 ..] = the block's sum of
// p^2 over its samples that are not NaN, its NaN samples, its empty cells and its infinite samples, fp64 (exact for the counts).
// src and out may be the same dense cube: a thread writes no element another thread reads.
__global__ void __launch_bounds__(256) k_kf_prepare(const float* src, long long st, long long sy, int nt, int ny, int nx, int centre, float* out,
                                                    double* __restrict__ means, unsigned long long* __restrict__ bits, int wpf,
                                                    double* __restrict__ part)
{
    __shared__ double sh[256];
    const int cells = ny * nx, i = blockIdx.x * 256 + threadIdx.x;
    const bool live = i < cells;
    const float* p = src + (live ? (long long)(i / nx) * sy + (i % nx) : 0);
    double sd = 0.0, ninf = 0.0;
    int cnt = 0;
    if (live)
        for (int t = 0; t < nt; ++t) {
            const float v = p[(long long)t * st];
            if (!isnan(v)) { sd += (double)v; ++cnt; }
            if (isinf(v)) ninf += 1.0;
        }
    const double m = cnt && centre ? sd / (double)cnt : 0.0;
    if (live) means[i] = cnt ? m : (double)__builtin_nanf("");
    double s2 = 0.0;
    for (int t = 0; t < nt; ++t) {                       // every lane of the wave stays in the loop: the ballot needs them all
        float r = 0.f;
        bool nan = false;
        if (live) {
            const float v = p[(long long)t * st];
            nan = isnan(v);
            if (!nan) {
                r = (float)((double)v - m);
                s2 += (double)r * (double)r;
            }
            out[(size_t)t * cells + i] = r;
        }
        const unsigned long long b = __ballot(nan);
        if ((threadIdx.x & 63) == 0 && i < cells) bits[(size_t)t * wpf + (i >> 6)] = b;
    }
    const double a0 = block_sum<256>(s2, sh), a1 = block_sum<256>(live ? (double)(nt - cnt) : 0.0, sh),
                 a2 = block_sum<256>(live && !cnt ? 1.0 : 0.0, sh), a3 = block_sum<256>(ninf, sh);
    if (threadIdx.x == 0) {
        part[(size_t)blockIdx.x * 4 + 0] = a0;
        part[(size_t)blockIdx.x * 4 + 1] = a1;
        part[(size_t)blockIdx.x * 4 + 2] = a2;
        part[(size_t)blockIdx.x * 4 + 3] = a3;
    }
}

// dst[j] = the sum of part[i * nv + j] over i < npart, thread-strided then a tree; one block per j
__global__ void __launch_bounds__(256) k_kf_fold(const double* __restrict__ part, size_t npart, int nv, double* __restrict__ dst)
{
    __shared__ double sh[256];
    const int j = blockIdx.x;
    double s = 0.0;
    for (size_t i = threadIdx.x; i < npart; i += 256) s += part[i * nv + j];
    s = block_sum<256>(s, sh);
    if (threadIdx.x == 0) dst[j] = s;
}

struct ShellArgs {
    const double* omega; const double* kap_x; const double* kap_y; const double* sigma0; const unsigned char* used;   // fftshifted axes
    double U, V, G, lo, hi;
    int nt, ny, nx, ch, complement;
};

// H[f][ky][kx] of the un-shifted half layout.  0 on the zero-frequency plane and on the Nyquist index of every even axis; a bin of
// positive frequency (1 <= f <= (nt - 1) / 2) is decided at its own fftshifted indices (p, i, j) = (f + nt / 2, ..) mod n, one of negative
// frequency at those of its mirror image (-f, -ky, -kx):  used[i][j] and lo <= omega[p] <= hi and |r| <= G,
// r = (omega[p] - sigma0[i][j]) - (kap_x[j] U + kap_y[i] V), not contracted (the library is built with -ffp-contract=off).
// count[0] += the bins of the FULL cube that pass (a column that stands for its mirror image counts twice): an integer atomic.
__global__ void __launch_bounds__(256) k_kf_shell(const ShellArgs a, float* __restrict__ H, unsigned long long* __restrict__ count)
{
    const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x, plane = (size_t)a.ny * a.ch;
    unsigned n = 0;
    if (q < (size_t)a.nt * plane) {
        int f = (int)(q / plane), ky = (int)(q % plane) / a.ch, kx = (int)(q % plane) % a.ch;
        const bool alone = kx == 0 || (a.nx % 2 == 0 && kx == a.nx / 2);
        const bool nyq = (a.nt % 2 == 0 && f == a.nt / 2) || (a.ny % 2 == 0 && ky == a.ny / 2) || (a.nx % 2 == 0 && kx == a.nx / 2);
        bool pass = false;
        if (f != 0 && !nyq) {
            if (f > a.nt / 2) {
                f = a.nt - f;
                ky = (a.ny - ky) % a.ny;
                kx = (a.nx - kx) % a.nx;
            }
            const int p = (f + a.nt / 2) % a.nt, i = (ky + a.ny / 2) % a.ny, j = (kx + a.nx / 2) % a.nx;
            const double w = a.omega[p], d = w - a.sigma0[(size_t)i * a.nx + j];
            const double r = d - (a.kap_x[j] * a.U + a.kap_y[i] * a.V);
            pass = a.used[(size_t)i * a.nx + j] && w >= a.lo && w <= a.hi && fabs(r) <= a.G;
            if (a.complement) pass = !pass;
        }
        H[q] = pass ? 1.f : 0.f;
        n = pass ? (alone ? 1u : 2u) : 0u;
    }
    n = wave_fold(n, [](unsigned x, unsigned y) { return x + y; });
    if ((threadIdx.x & 63) == 0 && n) atomicAdd(count, (unsigned long long)n);
}

// X -> conj(X) * (H * w * inv) over [nt][ny][ch]: the products in fp64, one rounding; w = 2 for the columns that stand for their mirror
// image too, inv = 1 / (nt ny nx)
__global__ void __launch_bounds__(256) k_kf_mul(float* __restrict__ re, float* __restrict__ im, const float* __restrict__ H, int ch, int nx, double inv,
                                                size_t total)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int kx = (int)(i % ch);
    const bool alone = kx == 0 || (nx % 2 == 0 && kx == nx / 2);
    const double h = (double)H[i] * (alone ? 1.0 : 2.0) * inv;
    re[i] = (float)((double)re[i] * h);
    im[i] = (float)(-((double)im[i] * h));
}

struct CloseArgs {
    const float* Tc; const float* Ts; int Mp;       // twiddle pair of the x axis, [Kp][Mp]
    const float* Bre; const float* Bim;             // the half spectrum, [N][K]
    float* out;                                     // [N][M], dense
    const double* means;                            // [ny * M]
    const unsigned long long* bits; int wpf;        // the NaN bitmap of k_kf_prepare
    double* part;                                   // [blocks]: the block's sum of y^2 over the samples that were not NaN
    int M, N, K, ny, flags;                         // x, rows = nt * ny, kx <= nx / 2
};

// The closing x stage: Out[m][n] = Re sum_k (cos - i sin)(2 pi m k / nx) In[n][k] = sum_k (c br + s bi), the acc_re chain of
// k_dft_stage<true, true> MFMA for MFMA (c br, then s bi, per k step), so the bits are that stage's real part; acc_im is never made.
// Loads outside K x N read as 0, stores outside M x N are dropped, the twiddle's padding is 0, as there.
__global__ void __launch_bounds__(256) k_dft_close(const CloseArgs a)
{
    // the four operand tiles of k_dft_stage, then (after the last MFMA) the 64 x 64 output tile [n][m]
    __shared__ __attribute__((aligned(16))) float lds[4 * SP_TK * SP_LD];
    __shared__ double sh[256];
    static_assert(4 * SP_TK * SP_LD >= SP_TN * KF_CL_LD, "the output tile fits the operand tiles");
    float (*As_c)[SP_LD] = (float (*)[SP_LD])lds;
    float (*As_s)[SP_LD] = (float (*)[SP_LD])(lds + SP_TK * SP_LD);
    float (*Bs_r)[SP_LD] = (float (*)[SP_LD])(lds + 2 * SP_TK * SP_LD);
    float (*Bs_i)[SP_LD] = (float (*)[SP_LD])(lds + 3 * SP_TK * SP_LD);

    const int tid = threadIdx.x, l = tid & 63, w = tid >> 6, lo = l & 15, hi = l >> 4;
    const int m0 = blockIdx.y * SP_TM, n0 = blockIdx.x * SP_TN;
    const int ak = tid >> 4, am = (tid & 15) * 4;
    const int bk = tid & 15, bn = tid >> 4;             // k is the input's contiguous axis
    sp_f32x4 pc, ps;
    float pr[4], pi[4];
    auto fetch = [&](int k0) {
        pc = *(const sp_f32x4*)&a.Tc[(size_t)(k0 + ak) * a.Mp + m0 + am];
        ps = *(const sp_f32x4*)&a.Ts[(size_t)(k0 + ak) * a.Mp + m0 + am];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int k = k0 + bk, n = n0 + bn + i * 16;
            const bool in = k < a.K && n < a.N;
            const long long q = (long long)n * a.K + k;
            pr[i] = in ? a.Bre[q] : 0.f;
            pi[i] = in ? a.Bim[q] : 0.f;
        }
    };

    sp_f32x4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = sp_f32x4{0.f, 0.f, 0.f, 0.f};
    const int wm = (w & 1) * 32, wn = (w >> 1) * 32;
    const int nk = (a.K + SP_TK - 1) / SP_TK;
    fetch(0);
    for (int kt = 0; kt < nk; ++kt) {
        __syncthreads();
        *(sp_f32x4*)&As_c[ak][am] = pc;
        *(sp_f32x4*)&As_s[ak][am] = ps;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            Bs_r[bk][bn + i * 16] = pr[i];
            Bs_i[bk][bn + i * 16] = pi[i];
        }
        __syncthreads();
        if (kt + 1 < nk) fetch((kt + 1) * SP_TK);
#pragma unroll
        for (int s = 0; s < SP_TK / 4; ++s) {
            const int kk = 4 * s + hi;
            float ac[2], as[2], br[2], bi[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                ac[i] = As_c[kk][wm + 16 * i + lo];
                as[i] = As_s[kk][wm + 16 * i + lo];
                br[i] = Bs_r[kk][wn + 16 * i + lo];
                bi[i] = Bs_i[kk][wn + 16 * i + lo];
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(ac[i], br[j], acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(as[i], bi[j], acc[i][j], 0, 0, 0);
                }
        }
    }
    // acc[i][j][r] = Out[m0 + wm + 16 i + 4 hi + r][n0 + wn + 16 j + lo]  ->  tile[n][m]: four consecutive m are one 16-byte write
    __syncthreads();                                   // every wave has read the last operand tiles
    float* tile = lds;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) *(sp_f32x4*)&tile[(wn + 16 * j + lo) * KF_CL_LD + wm + 16 * i + 4 * hi] = acc[i][j];
    __syncthreads();
    // a thread takes four consecutive x of one row, sixteen threads a row's 256 bytes, four rows per wave and pass
    const bool restore = a.flags & KF_RESTORE_MEAN, keep = a.flags & KF_KEEP_NAN;
    const bool wide = a.M % 4 == 0;                     // every row of out starts 16-byte aligned
    double s2 = 0.0;
#pragma unroll
    for (int ps4 = 0; ps4 < 4; ++ps4) {
        const int nl = ps4 * 16 + (tid >> 4), ml = (tid & 15) * 4;
        const int n = n0 + nl, m = m0 + ml;
        if (n >= a.N || m >= a.M) continue;
        const sp_f32x4 y = *(const sp_f32x4*)&tile[nl * KF_CL_LD + ml];
        const int t = n / a.ny, cell0 = (n % a.ny) * a.M + m;
        sp_f32x4 o;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float v = __builtin_nanf("");
            if (m + r < a.M) {
                const int cell = cell0 + r;
                const double mc = a.means[cell];
                const bool nan = (a.bits[(size_t)t * a.wpf + (cell >> 6)] >> (cell & 63)) & 1ull;
                if (!nan) s2 += (double)y[r] * (double)y[r];
                if (mc == mc && !(nan && keep)) v = restore ? (float)((double)y[r] + mc) : y[r];
            }
            o[r] = v;
        }
        float* dst = a.out + (long long)n * a.M + m;
        if (wide) *(sp_f32x4*)dst = o;                  // m + 3 < M: M and m are multiples of 4
        else
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (m + r < a.M) dst[r] = o[r];
    }
    s2 = block_sum<256>(s2, sh);
    if (tid == 0) a.part[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = s2;
}

}  // namespace wass

struct wass_kfilter {
    wass_kfilter(wass_ctx* c_, int nt_, int ny_, int nx_) : c(c_), nt(nt_), ny(ny_), nx(nx_), ch(nx_ / 2 + 1) {}
    wass_ctx* c;
    int nt, ny, nx, ch;
    Arena arena;
    float* cube = nullptr;          // [nt][ny][nx]: staging of a host cube, the prepared cube, then the result
    float* a_re = nullptr; float* a_im = nullptr;   // [nt][ny][ch]
    float* b_re = nullptr; float* b_im = nullptr;
    float* H = nullptr;             // [nt][ny][ch]
    unsigned long long* bits = nullptr;   // [nt][wpf]
    double* means = nullptr;        // [ny][nx]
    double* part = nullptr;         // the partial sums of k_kf_prepare (4 per block) or k_dft_close (1 per block)
    double* sums = nullptr;         // [8]: s2_in, n_nan, n_empty, n_inf, s2_out
    unsigned long long* count = nullptr;
    int wpf = 0, nprep = 0;
    size_t nclose = 0;
    bool has_mask = false;
    Twiddle tx, ty, tt;
    // stage timing (wass_kfilter_set_timing): events around every stage of an apply, made on first use
    bool timing = false;
    hipEvent_t ev[KF_STAGES + 1] = {};
    float stage_ms[KF_STAGES] = {};
    ~wass_kfilter()
    {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
};

namespace {

void carve(wass_kfilter& h, Arena& a)
{
    const size_t cells = (size_t)h.ny * h.nx, win = (size_t)h.nt * cells, half = (size_t)h.nt * h.ny * h.ch;
    h.wpf = (int)((cells + 63) / 64);
    h.nprep = (int)((cells + 255) / 256);
    h.nclose = (((size_t)h.nt * h.ny + SP_TN - 1) / SP_TN) * (size_t)((h.nx + SP_TM - 1) / SP_TM);
    const size_t npart = (size_t)h.nprep * 4 > h.nclose ? (size_t)h.nprep * 4 : h.nclose;
    h.cube = a.take<float>(win * 4);
    h.a_re = a.take<float>(2 * half * 4); h.a_im = piece_at(h.a_re, half);
    h.b_re = a.take<float>(2 * half * 4); h.b_im = piece_at(h.b_re, half);
    h.H = a.take<float>(half * 4);
    h.bits = a.take<unsigned long long>((size_t)h.nt * h.wpf * 8);
    h.means = a.take<double>(cells * 8);
    h.part = a.take<double>(npart * 8);
    h.sums = a.take<double>(8 * 8);
    h.count = a.take<unsigned long long>(256);
    h.tx = make_twiddle(a, h.nx, h.nx);
    h.ty = make_twiddle(a, h.ny, h.ny);
    h.tt = make_twiddle(a, h.nt, h.nt);
}

size_t kfilter_bytes(int nt, int ny, int nx)
{
    wass_kfilter h(nullptr, nt, ny, nx);
    carve(h, h.arena);
    return h.arena.used;
}

int kfilter_apply(wass_kfilter* h, bool host, const float* in, size_t st, size_t sy, float* out, size_t ost, size_t osy, int flags,
                  wass_kfilter_stats* stats)
{
    if (!h) return WASS_ERR_INVALID_ARG;
    wass_ctx* c = h->c;
    const int nt = h->nt, ny = h->ny, nx = h->nx, ch = h->ch;
    if (!in || !out || sy < (size_t)nx || osy < (size_t)nx || (nt > 1 && (st < (size_t)nx || ost < (size_t)nx)) || (flags & ~7))
        return set_err(c, WASS_ERR_INVALID_ARG, "bad cube pointer, strides or flags");
    if (!h->has_mask) return set_err(c, WASS_ERR_INVALID_ARG, "no mask was set");
    WASS_HIP(c, hipSetDevice(c->device));
    hipStream_t s = c->ts();
    const size_t cells = (size_t)ny * nx, half = (size_t)nt * ny * ch;
    int nmark = 0;
    auto mark = [&]() {                                   // the end of a stage (and the start of the next one)
        if (h->timing && nmark <= KF_STAGES) (void)hipEventRecord(h->ev[nmark++], s);
    };
    if (h->timing)
        for (hipEvent_t& e : h->ev)
            if (!e) WASS_HIP(c, hipEventCreate(&e));
    mark();
    const float* src = in;
    long long sst = (long long)st, ssy = (long long)sy;
    if (host) {
        WASS_HIP(c, upload_rows(h->cube, in, 4, nt, 0, ny, nx, st, sy, s));
        src = h->cube;
        sst = (long long)cells;
        ssy = nx;
    }
    hipLaunchKernelGGL(k_kf_prepare, dim3(h->nprep), dim3(256), 0, s, src, sst, ssy, nt, ny, nx, (flags & KF_NO_CENTRE) ? 0 : 1, h->cube, h->means,
                       h->bits, h->wpf, h->part);
    hipLaunchKernelGGL(k_kf_fold, dim3(4), dim3(256), 0, s, (const double*)h->part, (size_t)h->nprep, 4, h->sums);
    WASS_HIP(c, hipGetLastError());
    mark();
    int rc;
    const long long plane = (long long)ny * ch;
    DftArgs x = {h->tx.c, h->tx.s, h->tx.Mp, h->cube, nullptr, h->a_re, h->a_im, ch, nt * ny, nx, 1, nx, 0, 1, ch, 0};
    if ((rc = launch_dft(c, s, x, false, true, 1))) return rc;
    mark();
    DftArgs y = {h->ty.c, h->ty.s, h->ty.Mp, h->a_re, h->a_im, h->b_re, h->b_im, ny, ch, ny, ch, 1, plane, ch, 1, plane};
    if ((rc = launch_dft(c, s, y, true, false, nt))) return rc;
    mark();
    DftArgs t = {h->tt.c, h->tt.s, h->tt.Mp, h->b_re, h->b_im, h->a_re, h->a_im, nt, (int)plane, nt, plane, 1, 0, plane, 1, 0};
    if ((rc = launch_dft(c, s, t, true, false, 1))) return rc;
    mark();
    hipLaunchKernelGGL(k_kf_mul, dim3((unsigned)((half + 255) / 256)), dim3(256), 0, s, h->a_re, h->a_im, (const float*)h->H, ch, nx,
                       1.0 / ((double)nt * (double)ny * (double)nx), half);
    WASS_HIP(c, hipGetLastError());
    mark();
    DftArgs ti = {h->tt.c, h->tt.s, h->tt.Mp, h->a_re, h->a_im, h->b_re, h->b_im, nt, (int)plane, nt, plane, 1, 0, plane, 1, 0};
    if ((rc = launch_dft(c, s, ti, true, false, 1))) return rc;
    mark();
    DftArgs yi = {h->ty.c, h->ty.s, h->ty.Mp, h->b_re, h->b_im, h->a_re, h->a_im, ny, ch, ny, ch, 1, plane, ch, 1, plane};
    if ((rc = launch_dft(c, s, yi, true, false, nt))) return rc;
    mark();
    if (h->timing) {
        // the yardstick of k_dft_close: the full stage on the same operands, its real part to the cube (k_dft_close writes it again)
        // and its imaginary part to the b planes, which are free by now and hold 2 nt ny ch >= nt ny nx floats
        DftArgs xi = {h->tx.c, h->tx.s, h->tx.Mp, h->a_re, h->a_im, h->cube, h->b_re, nx, nt * ny, ch, 1, ch, 0, 1, nx, 0};
        if ((rc = launch_dft(c, s, xi, true, true, 1))) return rc;
    }
    mark();
    CloseArgs cl = {h->tx.c, h->tx.s, h->tx.Mp, h->a_re, h->a_im, h->cube, h->means, h->bits, h->wpf, h->part, nx, nt * ny, ch, ny, flags};
    const dim3 grid((nt * ny + SP_TN - 1) / SP_TN, (nx + SP_TM - 1) / SP_TM);
    hipLaunchKernelGGL(k_dft_close, grid, dim3(256), 0, s, cl);
    hipLaunchKernelGGL(k_kf_fold, dim3(1), dim3(256), 0, s, (const double*)h->part, h->nclose, 1, h->sums + 4);
    WASS_HIP(c, hipGetLastError());
    mark();
    double sums[5];
    WASS_HIP(c, hipMemcpyAsync(sums, h->sums, sizeof sums, hipMemcpyDeviceToHost, s));
    WASS_HIP(c, hipStreamSynchronize(s));
    if (sums[3] != 0.0) return set_err(c, WASS_ERR_INVALID_ARG, "the cube holds %.0f infinite samples", sums[3]);
    if (stats) {
        const double n = (double)nt * (double)cells - sums[1];
        stats->var_in = n > 0 ? sums[0] / n : (double)NAN;
        stats->var_out = n > 0 ? sums[4] / n : (double)NAN;
        stats->n_nan = (unsigned long long)sums[1];
        stats->n_empty_cells = (unsigned long long)sums[2];
    }
    WASS_HIP(c, download_rows(out, h->cube, 4, nt, 0, ny, nx, ost, osy, s, host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice));
    mark();
    if (host || h->timing) WASS_HIP(c, hipStreamSynchronize(s));
    if (h->timing)
        for (int i = 0; i < KF_STAGES; ++i) WASS_HIP(c, hipEventElapsedTime(&h->stage_ms[i], h->ev[i], h->ev[i + 1]));
    return WASS_OK;
}

}  // namespace

extern "C" int wass_kfilter_set_timing(wass_kfilter* h, int on)
{
    if (!h) return WASS_ERR_INVALID_ARG;
    h->timing = on != 0;
    return WASS_OK;
}

extern "C" int wass_kfilter_last_timings(wass_kfilter* h, float* stage_ms)
{
    if (!h || !stage_ms) return WASS_ERR_INVALID_ARG;
    memcpy(stage_ms, h->stage_ms, sizeof h->stage_ms);
    return WASS_OK;
}

extern "C" int wass_kfilter_scratch_bytes(int nt, int ny, int nx, size_t* bytes)
{
    if (!bytes || !spec3d_dims_ok(nt, ny, nx)) return WASS_ERR_INVALID_ARG;
    *bytes = kfilter_bytes(nt, ny, nx);
    return WASS_OK;
}

extern "C" void wass_kfilter_destroy(wass_kfilter* h)
{
    if (!h) return;
    if (h->c) (void)hipSetDevice(h->c->device);
    if (h->arena.mem) (void)hipDeviceSynchronize();     // the device form of apply returns with its copy in flight
    delete h;
}

extern "C" int wass_kfilter_create(wass_ctx* c, int nt, int ny, int nx, wass_kfilter** out)
{
    if (!c || !out) return set_err(c, WASS_ERR_INVALID_ARG, "null argument");
    *out = nullptr;
    if (!spec3d_dims_ok(nt, ny, nx)) return set_err(c, WASS_ERR_INVALID_ARG, "bad cube size %d x %d x %d (each axis 1 .. %d)", nt, ny, nx, SPEC_MAX_AXIS);
    // rows, cells and the columns of the t stage are indexed with 32 bits
    if ((size_t)ny * (nx / 2 + 1) > 0x7fffffffu || (size_t)nt * ny > 0x7fffff00u || (size_t)ny * nx > 0x7fffff00u)
        return set_err(c, WASS_ERR_UNSUPPORTED, "cube too large");
    const size_t total = kfilter_bytes(nt, ny, nx);
    if (total > SPEC_SCRATCH_CAP)
        return set_err(c, WASS_ERR_NO_MEMORY, "a %d x %d x %d cube needs %zu bytes of scratch, the cap is %zu", nt, ny, nx, total, SPEC_SCRATCH_CAP);
    WASS_HIP(c, hipSetDevice(c->device));
    wass_kfilter* h = new (std::nothrow) wass_kfilter(c, nt, ny, nx);
    if (!h) return set_err(c, WASS_ERR_NO_MEMORY, "out of host memory");
    int rc = h->arena.reserve(c, total, "the filter's scratch");
    if (rc) {
        wass_kfilter_destroy(h);
        return rc;
    }
    carve(*h, h->arena);
    hipStream_t s = c->ts();
    rc = fill_twiddle(c, s, h->tx);
    if (!rc) rc = fill_twiddle(c, s, h->ty);
    if (!rc) rc = fill_twiddle(c, s, h->tt);
    if (!rc && hipStreamSynchronize(s) != hipSuccess) rc = set_err(c, WASS_ERR_DEVICE, "filter set-up failed");
    if (rc) {
        wass_kfilter_destroy(h);
        return rc;
    }
    *out = h;
    return WASS_OK;
}

extern "C" int wass_kfilter_set_mask(wass_kfilter* h, const float* H)
{
    if (!h) return WASS_ERR_INVALID_ARG;
    wass_ctx* c = h->c;
    if (!H) return set_err(c, WASS_ERR_INVALID_ARG, "null argument");
    WASS_HIP(c, hipSetDevice(c->device));
    hipStream_t s = c->ts();
    WASS_HIP(c, hipMemcpyAsync(h->H, H, (size_t)h->nt * h->ny * h->ch * 4, hipMemcpyHostToDevice, s));
    WASS_HIP(c, hipStreamSynchronize(s));
    h->has_mask = true;
    return WASS_OK;
}

extern "C" int wass_kfilter_set_shell(wass_kfilter* h, const double* omega, const double* kappa_x, const double* kappa_y, const double* sigma0,
                                      const unsigned char* used, double U, double V, double G, double f_lo, double f_hi, int complement,
                                      uint64_t* n_pass)
{
    if (!h) return WASS_ERR_INVALID_ARG;
    wass_ctx* c = h->c;
    if (!omega || !kappa_x || !kappa_y || !sigma0 || !used) return set_err(c, WASS_ERR_INVALID_ARG, "null argument");
    if (!(U == U && V == V && G >= 0)) return set_err(c, WASS_ERR_INVALID_ARG, "U, V must be numbers and G >= 0");
    const int nt = h->nt, ny = h->ny, nx = h->nx;
    const size_t cells = (size_t)ny * nx, half = (size_t)nt * ny * h->ch;
    WASS_HIP(c, hipSetDevice(c->device));
    hipStream_t s = c->ts();
    // the maps are the call's own scratch (9 bytes per cell), freed when it returns
    double *d_om, *d_kx, *d_ky, *d_s0;
    unsigned char* d_used;
    auto lay = [&](Carve& a) {
        d_om = a.take<double>((size_t)nt * 8);
        d_kx = a.take<double>((size_t)nx * 8);
        d_ky = a.take<double>((size_t)ny * 8);
        d_s0 = a.take<double>(cells * 8);
        d_used = a.take<unsigned char>(cells);
    };
    Arena maps;
    if (int rc = maps.reserve(c, measure(lay), "the shell maps")) return rc;
    lay(maps);
    hipError_t e = hipMemcpyAsync(d_om, omega, (size_t)nt * 8, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(d_kx, kappa_x, (size_t)nx * 8, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(d_ky, kappa_y, (size_t)ny * 8, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(d_s0, sigma0, cells * 8, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(d_used, used, cells, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemsetAsync(h->count, 0, 8, s);
    unsigned long long n = 0;
    if (e == hipSuccess) {
        ShellArgs a = {d_om, d_kx, d_ky, d_s0, d_used, U, V, G, f_lo, f_hi, nt, ny, nx, h->ch, complement ? 1 : 0};
        hipLaunchKernelGGL(k_kf_shell, dim3((unsigned)((half + 255) / 256)), dim3(256), 0, s, a, h->H, h->count);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(&n, h->count, 8, hipMemcpyDeviceToHost, s);
    const int rc = finish(c, 0, e, s, "shell mask");      // synchronises: the maps are freed after this
    if (rc) return rc;
    if (n_pass) *n_pass = n;
    h->has_mask = true;
    return WASS_OK;
}

extern "C" int wass_kfilter_get_mask(wass_kfilter* h, float* H)
{
    if (!h) return WASS_ERR_INVALID_ARG;
    wass_ctx* c = h->c;
    if (!H) return set_err(c, WASS_ERR_INVALID_ARG, "null argument");
    if (!h->has_mask) return set_err(c, WASS_ERR_INVALID_ARG, "no mask was set");
    WASS_HIP(c, hipSetDevice(c->device));
    hipStream_t s = c->ts();
    WASS_HIP(c, hipMemcpyAsync(H, h->H, (size_t)h->nt * h->ny * h->ch * 4, hipMemcpyDeviceToHost, s));
    WASS_HIP(c, hipStreamSynchronize(s));
    return WASS_OK;
}

extern "C" int wass_kfilter_apply(wass_kfilter* h, const float* cube, size_t stride_t, size_t stride_y, float* out, size_t out_stride_t,
                                  size_t out_stride_y, int flags, wass_kfilter_stats* stats)
{
    return kfilter_apply(h, true, cube, stride_t, stride_y, out, out_stride_t, out_stride_y, flags, stats);
}

extern "C" int wass_kfilter_apply_dev(wass_kfilter* h, const float* d_cube, size_t stride_t, size_t stride_y, float* d_out, size_t out_stride_t,
                                      size_t out_stride_y, int flags, wass_kfilter_stats* stats)
{
    return kfilter_apply(h, false, d_cube, stride_t, stride_y, d_out, out_stride_t, out_stride_y, flags, stats);
}
