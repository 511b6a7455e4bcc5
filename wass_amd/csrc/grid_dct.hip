// grid_dct.hip -- the gridding stage's default interpolator: DCT surface interpolation.
//
// Reference: gridding/wassgridsurface/DCTInterpolator.py (the default of wassgridsurface --ia, wassgridsurface.py:639):
//   C = dct(eye(n), type=3, norm='ortho')        C[r,k] = r==0 ? 1/sqrt(n) : sqrt(2/n) cos(pi r (2k+1) / 2n)
//   A = C[:Nf, :]  (A_y with n = H, A_x with n = W)
//   Irec = A_y^T x A_x,   L = sum M (Irec - I)^2 / sum M + alpha |x|_1
//   G    = A_y (c M (Irec - I)) A_x^T + alpha sign(x),   c = 2 / sum M
//   torch.optim.Rprop(lr, etas (0.5, 1.2), step sizes (1e-6, 50)), MAX_ITERS + 1 steps, every 50th step stops when
//   max |x_ii - x_(ii-1)| < TOLERANCE_CHANGE; the output is Irec of the final x.
// The reference only runs square grids (one basis of size H on both sides); separate bases for rows and columns are an
// extension that equals it when W == H.
//
// One Rprop step is three kernels, every contraction on v_mfma_f32_16x16x4_f32 (exact f32, a k-ordered fma chain):
//   k_dct_T      T = x A_x                                      (nfp x Wp)
//   k_dct_resid  per block of 16 rows and a chunk of columns:   Irec = A_y^T T  ->  R = c M (Irec - I)  ->  U = R A_x^T
//                Irec and R live in registers only; the chunks write partial slabs U_part[chunk] (16 x nfp each)
//   k_dct_step   G = A_y sum_chunk U_part[chunk] + alpha sign(x), then the Rprop update and the tile's max |dx|
// Every reduction runs in a fixed order (no atomics): the same inputs give the same bits on every run.  Nf is padded to
// nfp (a multiple of 16); padded rows of the bases are 0, so padded gradients are 0 and padded coefficients stay 0 (the
// update also skips them).  H and W are padded to multiples of 16 with NaN cells (no data) and zero basis columns.
// The host looks at the device once per 50-step window: after each check step it reads max |dx| and stops below the
// tolerance, as the reference does.
//
// A batch: the frames of a sequence are independent problems of one shape with the same two bases.  Every kernel takes the
// frame from blockIdx.z (blockIdx.x / .y in the one-dimensional ones) and offsets zp, x, prev, step, T, Up, tmax, cnt, out
// and lossp by that frame's stride; A_y, A_x (and the seeded start value) are shared.  Nothing inside a frame changes -- the
// order of every reduction is the single solve's -- so frame i of a batch is bit for bit the single solve of frame i, and the
// single solve IS a batch of one.  The stopping rule is per frame: act[f] is 1 while frame f is being stepped; the check step's
// k_dct_maxred clears it when max |dx| falls below the tolerance and the workgroups of that frame leave at the top of every
// kernel from then on (before any MFMA: see the trap above k_dct_resid).  cnt[f] == 0 (no data) never sets it.  A batch of one
// passes no flags to the step kernels (the host loop ends with its only frame): a load at the top of a kernel whose time is
// launch latency cost the single solve 1 % (0.5 ms in 46 at 1024 x 1024, Nf 150: 1503 launches).
#include "common.h"

#include <math.h>
#include <vector>

namespace wass {

int grid_cells_dev(wass_ctx* c, const wass_mesh* m, const wass_grid_setup* gs, int cell_statistic, float* d_cells);

typedef float f32x4 __attribute__((ext_vector_type(4)));

static __device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 acc)
{
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc, 0, 0, 0);
}

constexpr int RESID_WAVES = 4;     // waves per workgroup of k_dct_resid
constexpr int FT_GROUP = 10;       // f-tiles (16 coefficients each) one k_dct_resid launch accumulates: nfp <= 160 in one pass
constexpr int STEP_WAVES = 16;     // waves per workgroup of k_dct_step (split of the contraction over H)

// A[r][k] for r < nf, k < n, 0 in the padding: rows nfp, columns np (fp64 cosine with the angle reduced exactly, cast to f32)
__global__ void __launch_bounds__(256) k_dct_basis(float* __restrict__ A, int n, int np, int nf, int nfp)
{
    const int k = blockIdx.x * 256 + threadIdx.x, r = blockIdx.y;
    if (k >= np || r >= nfp) return;
    double v = 0.0;
    if (r < nf && k < n) {
        if (r == 0) v = 1.0 / sqrt((double)n);
        else {
            const long long m = ((long long)r * (2 * k + 1)) % (4LL * n);          // cos has period 4n in units of pi / 2n
            v = sqrt(2.0 / n) * cos(M_PI * (double)m / (2.0 * n));
        }
    }
    A[(size_t)r * np + k] = (float)v;
}

// the cell maps into the padded buffer (NaN = no data, also in the padding), one workgroup per frame; cnt[f] = number of cells
// with data, act[f] = the frame has some
__global__ void __launch_bounds__(1024) k_dct_load(const float* __restrict__ zz, int W, int H, float* __restrict__ zp, int Wp, int Hp,
                                                   int* __restrict__ cnt, int* __restrict__ act)
{
    __shared__ int part[1024];
    int n = 0;
    const size_t tot = (size_t)Wp * Hp;
    zz += (size_t)blockIdx.x * W * H;
    zp += (size_t)blockIdx.x * tot;
    for (size_t i = threadIdx.x; i < tot; i += 1024) {
        const int x = (int)(i % Wp), y = (int)(i / Wp);
        const float v = (x < W && y < H) ? zz[(size_t)y * W + x] : __builtin_nanf("");
        zp[i] = v;
        n += !isnan(v);
    }
    part[threadIdx.x] = n;
    __syncthreads();
    block_tree<1024>([&](int t, int u) { part[t] += part[u]; });
    if (threadIdx.x == 0) { cnt[blockIdx.x] = part[0]; act[blockIdx.x] = part[0] != 0; }
}

// x (nf x nf, caller layout) into the padded state; prev = 0, step = lr.  Frame blockIdx.y; x0s = nf * nf, or 0 for one shared x0
__global__ void __launch_bounds__(256) k_dct_init(const float* __restrict__ x0, size_t x0s, int nf, int nfp, float lr, float* __restrict__ x,
                                                  float* __restrict__ prev, float* __restrict__ step)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nfp * nfp) return;
    const size_t fo = (size_t)blockIdx.y * nfp * nfp;
    x0 += blockIdx.y * x0s; x += fo; prev += fo; step += fo;
    const int f = i / nfp, g = i % nfp;
    x[i] = (f < nf && g < nf) ? x0[f * nf + g] : 0.f;
    prev[i] = 0.f;
    step[i] = lr;
}

// T = x A_x: one wave per 16 x 16 tile of T, 4 tiles per workgroup along the columns; frame blockIdx.z, skipped unless on[frame] (on may be null)
__global__ void __launch_bounds__(256) k_dct_T(const float* __restrict__ x, const float* __restrict__ Ax, float* __restrict__ T, int nfp, int Wp,
                                               const int* __restrict__ on)
{
    if (on && !on[blockIdx.z]) return;
    x += (size_t)blockIdx.z * nfp * nfp;
    T += (size_t)blockIdx.z * nfp * Wp;
    const int l = threadIdx.x & 63, w = threadIdx.x >> 6, lo = l & 15, hi = l >> 4;
    const int ct = blockIdx.x * 4 + w, kt = blockIdx.y;
    if (ct * 16 >= Wp) return;
    const int c0 = ct * 16, k0 = kt * 16;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int s = 0; s < nfp / 4; ++s)
        acc = mfma4(x[(size_t)(k0 + lo) * nfp + 4 * s + hi], Ax[(size_t)(4 * s + hi) * Wp + c0 + lo], acc);
    for (int r = 0; r < 4; ++r) T[(size_t)(k0 + 4 * hi + r) * Wp + c0 + lo] = acc[r];
}

// Irec^T of the 16 x 16 tile (columns c0.., rows r0..): lane (lo, hi) gets Irec[r0 + lo][c0 + 4 hi + r] in acc[r]
static __device__ __forceinline__ f32x4 irec_tile(const float* __restrict__ T, const float* __restrict__ Ay, int nfp, int Wp, int Hp, int r0,
                                                  int c0, int lo, int hi)
{
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int s = 0; s < nfp / 4; ++s)
        acc = mfma4(T[(size_t)(4 * s + hi) * Wp + c0 + lo], Ay[(size_t)(4 * s + hi) * Hp + r0 + lo], acc);
    return acc;
}

// One workgroup: rows r0 .. r0+15, the column tiles [chunk * tpc, (chunk + 1) * tpc) of the padded grid, split over its waves, and
// the NFT f-tiles from fg on.  Up[chunk][r][f] = sum over the chunk's columns of R[r][col] A_x[f][col], R = cs M (Irec - I)
// (cs = 2 / sum M).  NFT is a compile-time count: a data-dependent exit from the f-tile loop put a branch between the last MFMA
// and the read of its accumulator, and hipcc inserted no wait states on that edge (stale u values for Nf <= 16).  The frame
// (blockIdx.z) that has stopped leaves at the top, before any MFMA.
template <int NFT>
__global__ void __launch_bounds__(64 * RESID_WAVES) k_dct_resid(const float* __restrict__ T, const float* __restrict__ Ay,
                                                                const float* __restrict__ Ax, const float* __restrict__ zp,
                                                                const int* __restrict__ cnt, const int* __restrict__ act,
                                                                float* __restrict__ Up, int nfp, int Wp, int Hp, int tpc, int fg)
{
    __shared__ float red[RESID_WAVES][16][16 * NFT];
    if (act && !act[blockIdx.z]) return;
    T += (size_t)blockIdx.z * nfp * Wp;
    zp += (size_t)blockIdx.z * Hp * Wp;
    Up += (size_t)blockIdx.z * gridDim.x * Hp * nfp;
    cnt += blockIdx.z;
    const int l = threadIdx.x & 63, w = threadIdx.x >> 6, lo = l & 15, hi = l >> 4;
    const int r0 = blockIdx.y * 16, chunk = blockIdx.x, nct = Wp / 16;
    const float cs = 2.f * (1.f / (float)cnt[0]);
    f32x4 u[NFT];
#pragma unroll
    for (int j = 0; j < NFT; ++j) u[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int t_end = min(tpc, nct - chunk * tpc);
    for (int t = w; t < t_end; t += RESID_WAVES) {
        const int c0 = (chunk * tpc + t) * 16;
        const f32x4 ir = irec_tile(T, Ay, nfp, Wp, Hp, r0, c0, lo, hi);
        const f32x4 z = *(const f32x4*)&zp[(size_t)(r0 + lo) * Wp + c0 + 4 * hi];
        f32x4 res;
#pragma unroll
        for (int r = 0; r < 4; ++r) res[r] = isnan(z[r]) ? 0.f : (ir[r] - z[r]) * cs;
        // U[row lo][f] += sum_k R[lo][k] A_x[f][k]; the k order of the four MFMAs is (4 hi + r): the lane's own residuals
#pragma unroll
        for (int j = 0; j < NFT; ++j) {
            const f32x4 b = *(const f32x4*)&Ax[(size_t)((fg + j) * 16 + lo) * Wp + c0 + 4 * hi];
#pragma unroll
            for (int r = 0; r < 4; ++r) u[j] = mfma4(res[r], b[r], u[j]);
        }
    }
    // u[j][r] = U[row 4 hi + r][f = (fg + j) * 16 + lo]; the waves' partials are summed in wave order
#pragma unroll
    for (int j = 0; j < NFT; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) red[w][4 * hi + r][j * 16 + lo] = u[j][r];
    __syncthreads();
    for (int i = threadIdx.x; i < 16 * 16 * NFT; i += 64 * RESID_WAVES) {
        const int row = i / (16 * NFT), f = i % (16 * NFT);
        float s = red[0][row][f];
        for (int ww = 1; ww < RESID_WAVES; ++ww) s += red[ww][row][f];
        Up[((size_t)chunk * Hp + r0 + row) * nfp + fg * 16 + f] = s;
    }
}

// One workgroup per 16 x 16 tile of G: G = A_y U + alpha sign(x), U = the chunks' slabs summed in chunk order; the waves split
// the contraction over H and are summed in wave order.  RPROP: the torch.optim.Rprop update of the tile and its max |dx| into
// tmax[tile]; otherwise G into gout (nfp x nfp).  Frame blockIdx.z; one that has stopped leaves at the top.
template <bool RPROP>
__global__ void __launch_bounds__(64 * STEP_WAVES) k_dct_step(const float* __restrict__ Ay, const float* __restrict__ Up, int nchunk, int nfp,
                                                              int nf, int Hp, float alpha, const int* __restrict__ act, float* __restrict__ x,
                                                              float* __restrict__ prev, float* __restrict__ step, float* __restrict__ tmax,
                                                              float* __restrict__ gout)
{
    __shared__ float red[STEP_WAVES][256];
    __shared__ float mx[256];
    if (act && !act[blockIdx.z]) return;
    {
        const size_t fo = (size_t)blockIdx.z * nfp * nfp;
        Up += (size_t)blockIdx.z * nchunk * Hp * nfp;
        x += fo; prev += fo; step += fo;
        tmax += (size_t)blockIdx.z * gridDim.x * gridDim.y;
    }
    const int l = threadIdx.x & 63, w = threadIdx.x >> 6, lo = l & 15, hi = l >> 4;
    const int f0 = blockIdx.y * 16, g0 = blockIdx.x * 16;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    const size_t slab = (size_t)Hp * nfp;
    for (int s = w; s < Hp / 4; s += STEP_WAVES) {
        const int h = 4 * s + hi;
        const float* up = Up + (size_t)h * nfp + g0 + lo;
        float b = up[0];
        for (int ch = 1; ch < nchunk; ++ch) b += up[ch * slab];
        acc = mfma4(Ay[(size_t)(f0 + lo) * Hp + h], b, acc);
    }
    // acc[r] = G[f0 + 4 hi + r][g0 + lo]
#pragma unroll
    for (int r = 0; r < 4; ++r) red[w][(4 * hi + r) * 16 + lo] = acc[r];
    __syncthreads();
    if (threadIdx.x < 256) {
        const int t = threadIdx.x, f = f0 + t / 16, g = g0 + t % 16;
        const size_t i = (size_t)f * nfp + g;
        float gr = red[0][t];
        for (int ww = 1; ww < STEP_WAVES; ++ww) gr += red[ww][t];
        float d = 0.f;
        if (f < nf && g < nf) {
            const float xv = x[i];
            gr += alpha * (float)((xv > 0.f) - (xv < 0.f));
            if (RPROP) {
                const float pv = prev[i], sp = gr * pv;
                float st = step[i];
                if (sp > 0.f) st = fminf(fmaxf(st * 1.2f, 1e-6f), 50.f);
                else if (sp < 0.f) { st = fminf(fmaxf(st * 0.5f, 1e-6f), 50.f); gr = 0.f; }
                else st = fminf(fmaxf(st, 1e-6f), 50.f);
                const float xn = xv - (float)((gr > 0.f) - (gr < 0.f)) * st;
                x[i] = xn;
                prev[i] = gr;
                step[i] = st;
                d = fabsf(xn - xv);
            }
        } else gr = 0.f;
        if (!RPROP) gout[i] = gr;
        mx[t] = d;
    }
    __syncthreads();
    if (RPROP) {
        block_tree<256>([&](int t, int u) { mx[t] = fmaxf(mx[t], mx[u]); });
        if (threadIdx.x == 0) tmax[blockIdx.y * gridDim.x + blockIdx.x] = mx[0];
    }
}

// out[f] = max of frame f's tiles' max |dx| (one workgroup per frame); below the tolerance the frame is finished: act[f] = 0.
// A frame that had stopped before keeps the value of its last check.
__global__ void __launch_bounds__(256) k_dct_maxred(const float* __restrict__ tmax, int n, float* __restrict__ out, double tol,
                                                    int* __restrict__ act)
{
    __shared__ float m[256];
    if (!act[blockIdx.x]) return;
    tmax += (size_t)blockIdx.x * n;
    float v = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) v = fmaxf(v, tmax[i]);
    m[threadIdx.x] = v;
    __syncthreads();
    block_tree<256>([&](int t, int u) { m[t] = fmaxf(m[t], m[u]); });
    if (threadIdx.x == 0) {
        out[blockIdx.x] = m[0];
        if ((double)m[0] < tol) act[blockIdx.x] = 0;
    }
}

// Irec of the final x into out (padded, Hp x Wp; NaN where the user mask is 0); per workgroup sum M (Irec - I)^2 in fp64 into lossp.
// Frame blockIdx.z (the user mask is shared); a frame without data (cnt == 0) is skipped.
__global__ void __launch_bounds__(256) k_dct_recon(const float* __restrict__ T, const float* __restrict__ Ay, const float* __restrict__ zp,
                                                   const uint8_t* __restrict__ umask, const int* __restrict__ cnt, int W, int H, int nfp, int Wp,
                                                   int Hp, float* __restrict__ out, double* __restrict__ lossp)
{
    __shared__ double part[4];
    if (!cnt[blockIdx.z]) return;
    T += (size_t)blockIdx.z * nfp * Wp;
    zp += (size_t)blockIdx.z * Hp * Wp;
    if (out) out += (size_t)blockIdx.z * Hp * Wp;
    lossp += (size_t)blockIdx.z * gridDim.x * gridDim.y;
    const int l = threadIdx.x & 63, w = threadIdx.x >> 6, lo = l & 15, hi = l >> 4;
    const int r0 = blockIdx.y * 16, ct = blockIdx.x * 4 + w, nct = Wp / 16;
    double se = 0.0;
    if (ct < nct) {
        const int c0 = ct * 16, row = r0 + lo;
        const f32x4 ir = irec_tile(T, Ay, nfp, Wp, Hp, r0, c0, lo, hi);
        for (int r = 0; r < 4; ++r) {
            const int col = c0 + 4 * hi + r;
            const float z = zp[(size_t)row * Wp + col];
            if (!isnan(z)) { const double e = (double)(ir[r] - z); se += e * e; }
            if (out) out[(size_t)row * Wp + col] = (umask && row < H && col < W && !umask[(size_t)row * W + col]) ? __builtin_nanf("") : ir[r];
        }
    }
    // wave sum in a fixed order (lane order), then the four waves in order
    se = wave_fold(se, [](double a, double b) { return a + b; });
    if (l == 0) part[w] = se;
    __syncthreads();
    if (threadIdx.x == 0) lossp[blockIdx.y * gridDim.x + blockIdx.x] = part[0] + part[1] + part[2] + part[3];
}

// res[0] = sum of the loss partials / count, res[1] = sum |x| (both in fp64, in index order), res[2] = count; frame blockIdx.x, four
// doubles of res each
__global__ void __launch_bounds__(256) k_dct_final(const double* __restrict__ lossp, int nl, const float* __restrict__ x, int nf, int nfp,
                                                   const int* __restrict__ cnt, double* __restrict__ res)
{
    __shared__ double a[256], b[256];
    lossp += (size_t)blockIdx.x * nl;
    x += (size_t)blockIdx.x * nfp * nfp;
    cnt += blockIdx.x;
    res += 4 * blockIdx.x;
    if (!cnt[0]) {                                           // no data: the loss partials were never written
        if (threadIdx.x < 4) res[threadIdx.x] = 0.0;
        return;
    }
    double s = 0.0, t = 0.0;
    for (int i = threadIdx.x; i < nl; i += 256) s += lossp[i];
    for (int i = threadIdx.x; i < nf * nf; i += 256) t += fabs((double)x[(size_t)(i / nf) * nfp + i % nf]);
    a[threadIdx.x] = s; b[threadIdx.x] = t;
    __syncthreads();
    block_tree<256>([&](int t, int u) { a[t] += a[u]; b[t] += b[u]; });
    if (threadIdx.x == 0) { res[0] = cnt[0] ? a[0] / cnt[0] : 0.0; res[1] = b[0]; res[2] = (double)cnt[0]; }
}

// the padded nfp x nfp state back to nf x nf (frame blockIdx.y)
__global__ void __launch_bounds__(256) k_dct_unpad(const float* __restrict__ src, int nf, int nfp, float* __restrict__ dst)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    src += (size_t)blockIdx.y * nfp * nfp;
    dst += (size_t)blockIdx.y * nf * nf;
    if (i < nf * nf) dst[i] = src[(size_t)(i / nf) * nfp + i % nf];
}

// the padded grids into the caller's H x W ones (frame blockIdx.z, row blockIdx.y); all NaN for a frame without data
__global__ void __launch_bounds__(256) k_dct_store(const float* __restrict__ outp, const int* __restrict__ cnt, int W, int H, int Wp, int Hp,
                                                   float* __restrict__ dst)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= W) return;
    const float v = cnt[blockIdx.z] ? outp[((size_t)blockIdx.z * Hp + y) * Wp + x] : __builtin_nanf("");
    dst[((size_t)blockIdx.z * H + y) * W + x] = v;
}

static inline int rup16(int v) { return (v + 15) & ~15; }

// Deterministic uniform [0, 1) start value (splitmix64 of seed and index, 24 bits): torch's random stream is not reproduced.
static void dct_random_x0(uint64_t seed, int nf, std::vector<float>& x0)
{
    x0.resize((size_t)nf * nf);
    for (size_t i = 0; i < x0.size(); ++i) {
        uint64_t z = seed + 0x9E3779B97F4A7C15ull * (i + 1);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        z ^= z >> 31;
        x0[i] = (float)(z >> 40) * (1.0f / 16777216.0f);
    }
}

// Device layout of one sub-batch of nb problems of one shape inside c->dct: the bases and g are shared, every other array
// holds nb frames back to back.
struct DctPlan {
    int W, H, Wp, Hp, nf, nfp, nchunk, tpc, ntile, nloss, nb;
    float *Ay, *Ax, *zp, *x, *prev, *step, *T, *Up, *tmax, *out, *scal, *g;
    double *lossp, *res;
    int *cnt, *act;
};

static void dct_shape(int W, int H, int nf, DctPlan& p)
{
    p.W = W; p.H = H; p.nf = nf;
    p.Wp = rup16(W); p.Hp = rup16(H); p.nfp = rup16(nf);
    const int nct = p.Wp / 16, nrb = p.Hp / 16;
    // enough workgroups of k_dct_resid for every CU: column chunks per row block.  The split does not look at the batch size:
    // it sets the order of the sums over the columns, which a frame must keep whatever batch it is solved in.
    int nchunk = (512 + nrb - 1) / nrb;
    if (nchunk > nct) nchunk = nct;
    if (nchunk > 8) nchunk = 8;
    if (nchunk < 1) nchunk = 1;
    p.tpc = (nct + nchunk - 1) / nchunk;
    p.nchunk = (nct + p.tpc - 1) / p.tpc;
    p.ntile = (p.nfp / 16) * (p.nfp / 16);
    p.nloss = ((nct + 3) / 4) * nrb;
}

// The layout of c->dct for nb frames of the shape in p: the doubles, the two bases and g, which the frames share, then nb frames
// back to back in every other array.  Every kernel indexes a frame's arrays by the padded sizes they are taken with here (tiles
// of 16 inside Hp, Wp and nfp; ntile and nloss are the grids of k_dct_step and k_dct_recon): nothing reaches past a piece.
static void dct_carve(DctPlan& p, int nb, Carve& a)
{
    const size_t n = (size_t)nb, nfp2 = (size_t)p.nfp * p.nfp * 4, hw = (size_t)p.Hp * p.Wp * 4;
    p.nb = nb;
    p.lossp = a.take<double>(n * p.nloss * 8); p.res = a.take<double>(n * 4 * 8);
    p.Ay = a.take<float>((size_t)p.nfp * p.Hp * 4); p.Ax = a.take<float>((size_t)p.nfp * p.Wp * 4); p.g = a.take<float>(nfp2);
    p.zp = a.take<float>(n * hw); p.out = a.take<float>(n * hw);
    p.x = a.take<float>(n * nfp2); p.prev = a.take<float>(n * nfp2); p.step = a.take<float>(n * nfp2);
    p.T = a.take<float>(n * p.nfp * p.Wp * 4);
    p.Up = a.take<float>(n * p.nchunk * p.Hp * p.nfp * 4);
    p.tmax = a.take<float>(n * p.ntile * 4);
    p.scal = a.take<float>(n * 4); p.cnt = a.take<int>(n * 4); p.act = a.take<int>(n * 4);
}

// Frames one set of launches takes: the scratch of a sub-batch stays below 1 GiB (a 1024 x 1024, Nf 150 frame takes 14 MB) and
// blockIdx.z below its limit.  A frame alone takes no less than its share of a batch, so nb frames fit where nb * per do.
// Results do not depend on it.
static int dct_sub_batch(int W, int H, int nf, int n_frames)
{
    DctPlan p;
    dct_shape(W, H, nf, p);
    const auto bytes = [&](int nb) { return measure([&](Carve& a) { dct_carve(p, nb, a); }); };
    const size_t per = bytes(1) - bytes(0);                  // without a frame the shared arrays are all there is
    size_t nb = ((size_t)1 << 30) / per;
    if (nb > 1024) nb = 1024;
    if (nb < 1) nb = 1;
    return (size_t)n_frames < nb ? n_frames : (int)nb;
}

static int dct_plan(wass_ctx* c, int W, int H, int nf, int nb, DctPlan& p)
{
    dct_shape(W, H, nf, p);
    return carve_buf(c, c->dct, [&](Carve& a) { dct_carve(p, nb, a); });
}

// bases and the padded cell maps; ndata[f] = the number of cells with data of frame f (one synchronisation)
static int dct_setup(wass_ctx* c, hipStream_t s, DctPlan& p, const float* d_zz, int* ndata)
{
    hipLaunchKernelGGL(k_dct_basis, dim3((p.Hp + 255) / 256, p.nfp), dim3(256), 0, s, p.Ay, p.H, p.Hp, p.nf, p.nfp);
    hipLaunchKernelGGL(k_dct_basis, dim3((p.Wp + 255) / 256, p.nfp), dim3(256), 0, s, p.Ax, p.W, p.Wp, p.nf, p.nfp);
    hipLaunchKernelGGL(k_dct_load, dim3(p.nb), dim3(1024), 0, s, d_zz, p.W, p.H, p.zp, p.Wp, p.Hp, p.cnt, p.act);
    WASS_HIP(c, hipGetLastError());
    WASS_HIP(c, hipMemcpyAsync(ndata, p.cnt, sizeof(int) * p.nb, hipMemcpyDeviceToHost, s));
    WASS_HIP(c, hipStreamSynchronize(s));
    return WASS_OK;
}

// the data part of the gradient: T, then the fused residual kernel
static void dct_forward(hipStream_t s, const DctPlan& p)
{
    const int* act = p.nb > 1 ? p.act : nullptr;
    hipLaunchKernelGGL(k_dct_T, dim3((p.Wp / 16 + 3) / 4, p.nfp / 16, p.nb), dim3(256), 0, s, (const float*)p.x, (const float*)p.Ax, p.T, p.nfp,
                       p.Wp, act);
    for (int fg = 0; fg < p.nfp / 16; fg += FT_GROUP) {
        const dim3 grid(p.nchunk, p.Hp / 16, p.nb), blk(64 * RESID_WAVES);
        const int n = p.nfp / 16 - fg < FT_GROUP ? p.nfp / 16 - fg : FT_GROUP;
#define WASS_DCT_RESID(N) case N: hipLaunchKernelGGL(k_dct_resid<N>, grid, blk, 0, s, (const float*)p.T, (const float*)p.Ay, (const float*)p.Ax, \
                                                     (const float*)p.zp, (const int*)p.cnt, act, p.Up, p.nfp, p.Wp, p.Hp, p.tpc, fg); break;
        switch (n) {
            WASS_DCT_RESID(1) WASS_DCT_RESID(2) WASS_DCT_RESID(3) WASS_DCT_RESID(4) WASS_DCT_RESID(5)
            WASS_DCT_RESID(6) WASS_DCT_RESID(7) WASS_DCT_RESID(8) WASS_DCT_RESID(9) WASS_DCT_RESID(10)
        }
#undef WASS_DCT_RESID
    }
}

// Irec of the current x of every frame with data (out may be null: loss only) and res[4 f ..] = {data loss, sum |x|, count}
static void dct_reconstruct(hipStream_t s, const DctPlan& p, const uint8_t* d_umask, float* out)
{
    hipLaunchKernelGGL(k_dct_T, dim3((p.Wp / 16 + 3) / 4, p.nfp / 16, p.nb), dim3(256), 0, s, (const float*)p.x, (const float*)p.Ax, p.T, p.nfp,
                       p.Wp, (const int*)p.cnt);
    hipLaunchKernelGGL(k_dct_recon, dim3((p.Wp / 16 + 3) / 4, p.Hp / 16, p.nb), dim3(256), 0, s, (const float*)p.T, (const float*)p.Ay,
                       (const float*)p.zp, d_umask, (const int*)p.cnt, p.W, p.H, p.nfp, p.Wp, p.Hp, out, p.lossp);
    hipLaunchKernelGGL(k_dct_final, dim3(p.nb), dim3(256), 0, s, (const double*)p.lossp, p.nloss, (const float*)p.x, p.nf, p.nfp,
                       (const int*)p.cnt, p.res);
}

static int dct_check_args(wass_ctx* c, int W, int H, int nf)
{
    if (W < 1 || H < 1) return set_err(c, WASS_ERR_INVALID_ARG, "bad grid size %d x %d", W, H);
    if ((size_t)W * H > ((size_t)1 << 28)) return set_err(c, WASS_ERR_UNSUPPORTED, "grid too large");
    if (nf < 1 || nf > (W < H ? W : H)) return set_err(c, WASS_ERR_INVALID_ARG, "nfreqs %d outside [1, min(width, height) = %d]", nf, W < H ? W : H);
    return WASS_OK;
}

// One sub-batch of nb frames on device pointers (d_zz, d_out: nb x H x W; d_x0, d_coeffs: nb x nf x nf or null; info, status: nb
// entries, status[f] = WASS_OK or WASS_ERR_TOO_FEW_POINTS).  The arguments have been checked.
static int dct_solve_sub(wass_ctx* c, hipStream_t s, const float* d_zz, int nb, int W, int H, const wass_dct_opts* o, const float* d_x0,
                         const uint8_t* d_umask, float* d_out, float* d_coeffs, wass_dct_info* info, int* status)
{
    int rc;
    DctPlan p;
    if ((rc = dct_plan(c, W, H, o->nfreqs, nb, p))) return rc;
    std::vector<int> ndata(nb), steps(nb, 0), converged(nb, 0);
    std::vector<char> active(nb);
    std::vector<float> fdelta(nb, 0.f), scal(nb);
    if ((rc = dct_setup(c, s, p, d_zz, ndata.data()))) return rc;
    int nactive = 0;
    for (int f = 0; f < nb; ++f) nactive += (active[f] = ndata[f] != 0);
    const bool any_data = nactive != 0;
    if (any_data) {
        // start value: the caller's x0, or the seeded uniform [0, 1) one for every frame
        const float* x0 = d_x0;
        if (!x0) {
            std::vector<float> hx;
            dct_random_x0(o->seed, p.nf, hx);
            WASS_HIP(c, hipMemcpyAsync(p.g, hx.data(), hx.size() * 4, hipMemcpyHostToDevice, s));
            WASS_HIP(c, hipStreamSynchronize(s));                 // hx leaves scope
            x0 = p.g;
        }
        const int n2 = p.nfp * p.nfp;
        hipLaunchKernelGGL(k_dct_init, dim3((n2 + 255) / 256, nb), dim3(256), 0, s, x0, d_x0 ? (size_t)p.nf * p.nf : (size_t)0, p.nf, p.nfp,
                           (float)o->learning_rate, p.x, p.prev, p.step);
        const float alpha = (float)o->regularizer_alpha;
        for (int ii = 0; ii <= o->max_iters && nactive; ++ii) {
            dct_forward(s, p);
            hipLaunchKernelGGL(k_dct_step<true>, dim3(p.nfp / 16, p.nfp / 16, nb), dim3(64 * STEP_WAVES), 0, s, (const float*)p.Ay,
                               (const float*)p.Up, p.nchunk, p.nfp, p.nf, p.Hp, alpha, nb > 1 ? (const int*)p.act : nullptr, p.x, p.prev, p.step,
                               p.tmax, (float*)nullptr);
            for (int f = 0; f < nb; ++f)
                if (active[f]) steps[f] = ii + 1;
            if (ii % 50 == 0) {
                // the device clears act[f] by the comparison the host makes below on the same value
                hipLaunchKernelGGL(k_dct_maxred, dim3(nb), dim3(256), 0, s, (const float*)p.tmax, p.ntile, p.scal, o->tolerance_change, p.act);
                WASS_HIP(c, hipGetLastError());
                WASS_HIP(c, hipMemcpyAsync(scal.data(), p.scal, 4 * (size_t)nb, hipMemcpyDeviceToHost, s));
                WASS_HIP(c, hipStreamSynchronize(s));
                for (int f = 0; f < nb; ++f) {
                    if (!active[f]) continue;
                    fdelta[f] = scal[f];
                    if ((double)fdelta[f] < o->tolerance_change) { converged[f] = 1; active[f] = 0; --nactive; }
                }
            }
        }
        dct_reconstruct(s, p, d_umask, p.out);
        if (d_coeffs) hipLaunchKernelGGL(k_dct_unpad, dim3((p.nf * p.nf + 255) / 256, nb), dim3(256), 0, s, (const float*)p.x, p.nf, p.nfp, d_coeffs);
    }
    hipLaunchKernelGGL(k_dct_store, dim3((W + 255) / 256, H, nb), dim3(256), 0, s, (const float*)p.out, (const int*)p.cnt, W, H, p.Wp, p.Hp, d_out);
    WASS_HIP(c, hipGetLastError());
    std::vector<double> res((size_t)4 * nb, 0.0);
    if (any_data)
        WASS_HIP(c, hipMemcpyAsync(res.data(), p.res, res.size() * 8, hipMemcpyDeviceToHost, s));
    WASS_HIP(c, hipStreamSynchronize(s));
    for (int f = 0; f < nb; ++f) {
        status[f] = ndata[f] ? WASS_OK : WASS_ERR_TOO_FEW_POINTS;
        if (!info) continue;
        memset(&info[f], 0, sizeof info[f]);
        if (!ndata[f]) continue;
        info[f].steps = steps[f];
        info[f].converged = converged[f];
        info[f].data_loss = res[4 * f];
        info[f].reg_loss = res[4 * f + 1];
        info[f].fdelta = fdelta[f];
    }
    return WASS_OK;
}

// The batch on device pointers, walked in sub-batches.
static int dct_solve_batch(wass_ctx* c, const float* d_zz, int n_frames, int W, int H, const wass_dct_opts* o, const float* d_x0,
                           const uint8_t* d_umask, float* d_out, float* d_coeffs, wass_dct_info* info, int* status)
{
    if (!c || !d_zz || !o || !d_out || !status) return set_err(c, WASS_ERR_INVALID_ARG, "null argument");
    if (n_frames < 1) return set_err(c, WASS_ERR_INVALID_ARG, "n_frames %d < 1", n_frames);
    int rc;
    if ((rc = dct_check_args(c, W, H, o->nfreqs))) return rc;
    if (o->max_iters < 0 || !(o->learning_rate > 0)) return set_err(c, WASS_ERR_INVALID_ARG, "bad options");
    WASS_HIP(c, hipSetDevice(c->device));
    hipStream_t s = c->ts();
    if (info) memset(info, 0, sizeof *info * (size_t)n_frames);
    const int sub = dct_sub_batch(W, H, o->nfreqs, n_frames);
    const size_t hw = (size_t)W * H, n2 = (size_t)o->nfreqs * o->nfreqs;
    for (int f0 = 0; f0 < n_frames; f0 += sub) {
        const int nb = n_frames - f0 < sub ? n_frames - f0 : sub;
        if ((rc = dct_solve_sub(c, s, d_zz + f0 * hw, nb, W, H, o, d_x0 ? d_x0 + f0 * n2 : nullptr, d_umask, d_out + f0 * hw,
                                d_coeffs ? d_coeffs + f0 * n2 : nullptr, info ? info + f0 : nullptr, status + f0)))
            return rc;
    }
    return WASS_OK;
}

// The single solve: a batch of one.  d_out: H x W float32 (pitch W); d_coeffs: nf x nf or null.
static int dct_solve(wass_ctx* c, const float* d_zz, int W, int H, const wass_dct_opts* o, const float* d_x0, const uint8_t* d_umask,
                     float* d_out, float* d_coeffs, wass_dct_info* info)
{
    int status = WASS_OK;
    const int rc = dct_solve_batch(c, d_zz, 1, W, H, o, d_x0, d_umask, d_out, d_coeffs, info, &status);
    if (rc) return rc;
    if (status == WASS_ERR_TOO_FEW_POINTS) return set_err(c, WASS_ERR_TOO_FEW_POINTS, "the grid holds no data");
    return WASS_OK;
}

// host staging of a call of n frames: zz, out, x0 and coeffs per frame, one mask
struct DctIo {
    float *zz, *out, *x0, *coeffs;
    uint8_t* mask;
};
static int dct_io(wass_ctx* c, int n, int W, int H, int nf, DctIo& io)
{
    const size_t hw = (size_t)W * H, n2 = (size_t)nf * nf;
    return carve_buf(c, c->dct_io, [&](Carve& a) {
        io.zz = a.take<float>(n * hw * 4); io.out = a.take<float>(n * hw * 4);
        io.x0 = a.take<float>(n * n2 * 4); io.coeffs = a.take<float>(n * n2 * 4);
        io.mask = a.take<uint8_t>(hw);
    });
}

}  // namespace wass

using namespace wass;

extern "C" int wass_grid_dct_batch_dev(wass_ctx* c, const float* d_zz, int n_frames, int width, int height, const wass_dct_opts* opts,
                                       const float* d_x0, const uint8_t* d_user_mask, float* d_grid_out, float* d_coeffs_out,
                                       wass_dct_info* info, int* status)
{
    return dct_solve_batch(c, d_zz, n_frames, width, height, opts, d_x0, d_user_mask, d_grid_out, d_coeffs_out, info, status);
}

extern "C" int wass_grid_dct_batch(wass_ctx* c, const float* zz, int n_frames, int width, int height, const wass_dct_opts* opts,
                                   const float* x0, const uint8_t* user_mask, float* grid_out, float* coeffs_out, wass_dct_info* info,
                                   int* status)
{
    if (!c || !zz || !opts || !grid_out || !status) return set_err(c, WASS_ERR_INVALID_ARG, "null argument");
    if (n_frames < 1) return set_err(c, WASS_ERR_INVALID_ARG, "n_frames %d < 1", n_frames);
    int rc;
    if ((rc = dct_check_args(c, width, height, opts->nfreqs))) return rc;
    WASS_HIP(c, hipSetDevice(c->device));
    DctIo io;
    if ((rc = dct_io(c, n_frames, width, height, opts->nfreqs, io))) return rc;
    hipStream_t s = c->ts();
    const size_t hw = (size_t)width * height, n2 = (size_t)opts->nfreqs * opts->nfreqs;
    WASS_HIP(c, hipMemcpyAsync(io.zz, zz, n_frames * hw * 4, hipMemcpyHostToDevice, s));
    if (x0) WASS_HIP(c, hipMemcpyAsync(io.x0, x0, n_frames * n2 * 4, hipMemcpyHostToDevice, s));
    if (user_mask) WASS_HIP(c, hipMemcpyAsync(io.mask, user_mask, hw, hipMemcpyHostToDevice, s));
    if ((rc = dct_solve_batch(c, io.zz, n_frames, width, height, opts, x0 ? io.x0 : nullptr, user_mask ? io.mask : nullptr, io.out,
                              coeffs_out ? io.coeffs : nullptr, info, status)))
        return rc;
    WASS_HIP(c, hipMemcpyAsync(grid_out, io.out, n_frames * hw * 4, hipMemcpyDeviceToHost, s));
    // the coefficients of a frame without data are not defined: only the frames that ran are copied
    if (coeffs_out)
        for (int f = 0; f < n_frames; ++f)
            if (status[f] == WASS_OK) WASS_HIP(c, hipMemcpyAsync(coeffs_out + f * n2, io.coeffs + f * n2, n2 * 4, hipMemcpyDeviceToHost, s));
    WASS_HIP(c, hipStreamSynchronize(s));
    return WASS_OK;
}

extern "C" void wass_dct_opts_default(wass_dct_opts* o)
{
    if (!o) return;
    memset(o, 0, sizeof *o);
    o->nfreqs = 150;
    o->max_iters = 500;
    o->tolerance_change = 1e-4;
    o->regularizer_alpha = 8e-7;
    o->learning_rate = 5.0;
    o->seed = 0;
}

extern "C" int wass_grid_dct_dev(wass_ctx* c, const float* d_zz, int width, int height, const wass_dct_opts* opts, const float* d_x0,
                                 const uint8_t* d_user_mask, float* d_grid_out, float* d_coeffs_out, wass_dct_info* info)
{
    return dct_solve(c, d_zz, width, height, opts, d_x0, d_user_mask, d_grid_out, d_coeffs_out, info);
}

extern "C" int wass_grid_dct(wass_ctx* c, const float* zz, int width, int height, const wass_dct_opts* opts, const float* x0,
                             const uint8_t* user_mask, float* grid_out, float* coeffs_out, wass_dct_info* info)
{
    if (!c || !zz || !opts || !grid_out) return set_err(c, WASS_ERR_INVALID_ARG, "null argument");
    int rc;
    if ((rc = dct_check_args(c, width, height, opts->nfreqs))) return rc;
    WASS_HIP(c, hipSetDevice(c->device));
    DctIo io;
    if ((rc = dct_io(c, 1, width, height, opts->nfreqs, io))) return rc;
    hipStream_t s = c->ts();
    const size_t hw = (size_t)width * height, n2 = (size_t)opts->nfreqs * opts->nfreqs;
    WASS_HIP(c, hipMemcpyAsync(io.zz, zz, hw * 4, hipMemcpyHostToDevice, s));
    if (x0) WASS_HIP(c, hipMemcpyAsync(io.x0, x0, n2 * 4, hipMemcpyHostToDevice, s));
    if (user_mask) WASS_HIP(c, hipMemcpyAsync(io.mask, user_mask, hw, hipMemcpyHostToDevice, s));
    rc = dct_solve(c, io.zz, width, height, opts, x0 ? io.x0 : nullptr, user_mask ? io.mask : nullptr, io.out, coeffs_out ? io.coeffs : nullptr, info);
    if (rc && rc != WASS_ERR_TOO_FEW_POINTS) return rc;
    WASS_HIP(c, hipMemcpyAsync(grid_out, io.out, hw * 4, hipMemcpyDeviceToHost, s));
    if (coeffs_out && !rc) WASS_HIP(c, hipMemcpyAsync(coeffs_out, io.coeffs, n2 * 4, hipMemcpyDeviceToHost, s));
    WASS_HIP(c, hipStreamSynchronize(s));
    return rc;
}

extern "C" int wass_mesh_grid_dct(wass_ctx* c, const wass_mesh* m, const wass_grid_setup* gs, int cell_statistic, const wass_dct_opts* opts,
                                  const float* x0, const uint8_t* user_mask, float* grid_out, float* cells_out, float* coeffs_out,
                                  wass_dct_info* info)
{
    if (!c || !m || !gs || !opts || !grid_out) return set_err(c, WASS_ERR_INVALID_ARG, "null argument");
    int rc;
    if ((rc = dct_check_args(c, gs->width, gs->height, opts->nfreqs))) return rc;
    WASS_HIP(c, hipSetDevice(c->device));
    DctIo io;
    if ((rc = dct_io(c, 1, gs->width, gs->height, opts->nfreqs, io))) return rc;
    if ((rc = grid_cells_dev(c, m, gs, cell_statistic, io.zz))) return rc;
    hipStream_t s = c->ts();
    const size_t hw = (size_t)gs->width * gs->height, n2 = (size_t)opts->nfreqs * opts->nfreqs;
    if (x0) WASS_HIP(c, hipMemcpyAsync(io.x0, x0, n2 * 4, hipMemcpyHostToDevice, s));
    if (user_mask) WASS_HIP(c, hipMemcpyAsync(io.mask, user_mask, hw, hipMemcpyHostToDevice, s));
    rc = dct_solve(c, io.zz, gs->width, gs->height, opts, x0 ? io.x0 : nullptr, user_mask ? io.mask : nullptr, io.out,
                   coeffs_out ? io.coeffs : nullptr, info);
    if (rc && rc != WASS_ERR_TOO_FEW_POINTS) return rc;
    WASS_HIP(c, hipMemcpyAsync(grid_out, io.out, hw * 4, hipMemcpyDeviceToHost, s));
    if (cells_out) WASS_HIP(c, hipMemcpyAsync(cells_out, io.zz, hw * 4, hipMemcpyDeviceToHost, s));
    if (coeffs_out && !rc) WASS_HIP(c, hipMemcpyAsync(coeffs_out, io.coeffs, n2 * 4, hipMemcpyDeviceToHost, s));
    WASS_HIP(c, hipStreamSynchronize(s));
    return rc;
}

extern "C" int wass_grid_dct_eval(wass_ctx* c, const float* zz, int width, int height, int nfreqs, double alpha, const float* x,
                                  float* grad_out, double* data_loss, double* reg_loss)
{
    if (!c || !zz || !x || !grad_out) return set_err(c, WASS_ERR_INVALID_ARG, "null argument");
    int rc;
    if ((rc = dct_check_args(c, width, height, nfreqs))) return rc;
    WASS_HIP(c, hipSetDevice(c->device));
    DctIo io;
    if ((rc = dct_io(c, 1, width, height, nfreqs, io))) return rc;
    hipStream_t s = c->ts();
    const size_t hw = (size_t)width * height, n2 = (size_t)nfreqs * nfreqs;
    WASS_HIP(c, hipMemcpyAsync(io.zz, zz, hw * 4, hipMemcpyHostToDevice, s));
    WASS_HIP(c, hipMemcpyAsync(io.x0, x, n2 * 4, hipMemcpyHostToDevice, s));
    DctPlan p;
    if ((rc = dct_plan(c, width, height, nfreqs, 1, p))) return rc;
    int ndata = 0;
    if ((rc = dct_setup(c, s, p, io.zz, &ndata))) return rc;
    if (!ndata) return set_err(c, WASS_ERR_TOO_FEW_POINTS, "the grid holds no data");
    const int np2 = p.nfp * p.nfp;
    hipLaunchKernelGGL(k_dct_init, dim3((np2 + 255) / 256), dim3(256), 0, s, (const float*)io.x0, (size_t)0, p.nf, p.nfp, 1.f, p.x, p.prev, p.step);
    dct_forward(s, p);
    hipLaunchKernelGGL(k_dct_step<false>, dim3(p.nfp / 16, p.nfp / 16), dim3(64 * STEP_WAVES), 0, s, (const float*)p.Ay, (const float*)p.Up,
                       p.nchunk, p.nfp, p.nf, p.Hp, (float)alpha, (const int*)nullptr, p.x, p.prev, p.step, p.tmax, p.g);
    hipLaunchKernelGGL(k_dct_unpad, dim3((unsigned)((n2 + 255) / 256)), dim3(256), 0, s, (const float*)p.g, p.nf, p.nfp, io.coeffs);
    dct_reconstruct(s, p, nullptr, nullptr);
    WASS_HIP(c, hipGetLastError());
    double res[3];
    WASS_HIP(c, hipMemcpyAsync(grad_out, io.coeffs, n2 * 4, hipMemcpyDeviceToHost, s));
    WASS_HIP(c, hipMemcpyAsync(res, p.res, sizeof res, hipMemcpyDeviceToHost, s));
    WASS_HIP(c, hipStreamSynchronize(s));
    if (data_loss) *data_loss = res[0];
    if (reg_loss) *reg_loss = res[1];
    return WASS_OK;
}
