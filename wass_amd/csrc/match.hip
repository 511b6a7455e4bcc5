// match.hip -- the game-theoretic feature matcher of wass_match (src/wass_match/GTMatcher.cpp, iidyn.cpp): candidates, payoff
// matrix, infection-immunization dynamics and the winning group.  See include/wass_gpu.h ("Feature matcher") for the contract.
//
//   k_match_knn       exact k nearest descriptors of B for every descriptor of A (squared L2, float32, summed in index order)
//   k_match_affine    compute_affine (GTMatcher.cpp:69-97) per candidate, fp64, into a record the payoff kernel reads
//   k_match_payoff    payoff() (:101-141) for every pair of candidates: a plain 2-D grid, one z-slice per problem
//   k_match_start     gt_create_population (a uniform start: rand() / RAND_MAX is an integer division) and the first simplexify
//   k_match_ax0       Ax = A x of the start, one wave per row
//   k_match_iidyn     gt_iidyn (iidyn.cpp:520-596), one workgroup per problem, x and Ax in registers, __syncthreads only;
//                     its epilogue picks the group of match_group (:273-293)
//
// The file is compiled without contraction (-ffp-contract=off): every fp64 product and sum rounds on its own, as in the
// reference's x86-64 build.  Reductions use one fixed tree that depends on N alone, never on the batch.
#include "common.h"

#include <float.h>
#include <limits.h>
#include <math.h>
#include <vector>

namespace wass {

constexpr int MATCH_REC = 10;            // doubles per candidate record: cos sin dx dy ds | sx sy tx ty | (src, tgt) as two ints
constexpr int IID_THREADS = 1024;
constexpr int IID_WAVES = IID_THREADS / 64;
constexpr int IID_E = WASS_MATCH_MAX_N / IID_THREADS;      // elements of x and Ax a thread keeps
constexpr int KNN_LANES = 64;
constexpr double MATCH_MAX_ANGLE = 1.0e4;                   // |angle difference| above this is refused: ang_diff's loops would not end

struct MatchRes {
    double err;
    int steps;
    int group;
};

enum : int { MATCH_BAD_INDEX = 1, MATCH_BAD_ANGLE = 2 };

// ---------------------------------------------------------------------------------------------------------------- candidates
__global__ void __launch_bounds__(KNN_LANES) k_match_knn(const float* __restrict__ A, int na, const float* __restrict__ B, int nb, int d,
                                                         int kk, int* __restrict__ idx, float* __restrict__ dist)
{
    extern __shared__ float sa[];                            // [d][64]: the block's 64 descriptors of A, transposed
    const int lane = threadIdx.x;
    const int i0 = blockIdx.x * KNN_LANES;
    const int rows = min(KNN_LANES, na - i0);
    for (int f = lane; f < KNN_LANES * d; f += KNN_LANES) {
        const int r = f / d, t = f - r * d;
        sa[t * KNN_LANES + r] = r < rows ? A[(size_t)(i0 + r) * d + t] : 0.0f;
    }
    __syncthreads();
    float bd[WASS_MATCH_MAX_K];
    int bi[WASS_MATCH_MAX_K];
#pragma unroll
    for (int q = 0; q < WASS_MATCH_MAX_K; ++q) { bd[q] = INFINITY; bi[q] = -1; }
    for (int j = 0; j < nb; ++j) {
        const float* b = B + (size_t)j * d;
        float s = 0.0f;
        for (int t = 0; t < d; ++t) {
            const float df = sa[t * KNN_LANES + lane] - b[t];
            s += df * df;
        }
        if (s < bd[WASS_MATCH_MAX_K - 1]) {                  // strict: of equal distances the lower index stays in front
            bd[WASS_MATCH_MAX_K - 1] = s;
            bi[WASS_MATCH_MAX_K - 1] = j;
#pragma unroll
            for (int q = WASS_MATCH_MAX_K - 1; q > 0; --q)
                if (bd[q] < bd[q - 1]) {
                    const float td = bd[q]; bd[q] = bd[q - 1]; bd[q - 1] = td;
                    const int ti = bi[q]; bi[q] = bi[q - 1]; bi[q - 1] = ti;
                }
        }
    }
    if (lane < rows) {
#pragma unroll
        for (int q = 0; q < WASS_MATCH_MAX_K; ++q)
            if (q < kk) {
                idx[(size_t)(i0 + lane) * kk + q] = bi[q];
                dist[(size_t)(i0 + lane) * kk + q] = bd[q];
            }
    }
}

// -------------------------------------------------------------------------------------------------------------------- payoff
__global__ void __launch_bounds__(256) k_match_affine(const float* __restrict__ fa, size_t fa_stride, const float* __restrict__ fb,
                                                      size_t fb_stride, const int* __restrict__ cand, size_t cand_stride,
                                                      const int* __restrict__ dims, int nmax, double* __restrict__ rec,
                                                      int* __restrict__ flag)
{
    const int p = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    const int n = dims[4 * p], na = dims[4 * p + 1], nb = dims[4 * p + 2];
    if (i >= n) return;
    double* r = rec + ((size_t)p * nmax + i) * MATCH_REC;
    const int src = cand[p * cand_stride + 2 * (size_t)i], tgt = cand[p * cand_stride + 2 * (size_t)i + 1];
    int* ri = (int*)(r + 9);
    ri[0] = src;
    ri[1] = tgt;
    if (src < 0 || src >= na || tgt < 0 || tgt >= nb) {
        atomicOr(flag, MATCH_BAD_INDEX);
        for (int q = 0; q < 9; ++q) r[q] = 0.0;
        return;
    }
    const float* s = fa + p * fa_stride + 4 * (size_t)src;   // x y scale angle
    const float* t = fb + p * fb_stride + 4 * (size_t)tgt;
    const double a = (double)t[3], b = (double)s[3];
    double diff = b - a;                                     // ang_diff(a, b)
    if (fabs(diff) <= MATCH_MAX_ANGLE) {
        while (diff < -M_PI) diff += 2.0 * M_PI;
        while (diff > M_PI) diff -= 2.0 * M_PI;
    } else {
        atomicOr(flag, MATCH_BAD_ANGLE);                     // NaN included
    }
    const double ca = cos(diff), sn = sin(diff);
    const double ds = (double)t[2] / (double)s[2];
    const double scx = (double)s[0] * ds, scy = (double)s[1] * ds;
    const double x = scx * ca - scy * sn;
    const double y = scx * sn + scy * ca;
    r[0] = ca;
    r[1] = sn;
    r[2] = (double)t[0] - x;
    r[3] = (double)t[1] - y;
    r[4] = ds;
    r[5] = (double)s[0];
    r[6] = (double)s[1];
    r[7] = (double)t[0];
    r[8] = (double)t[1];
}

__global__ void __launch_bounds__(256) k_match_payoff(const double* __restrict__ rec, const int* __restrict__ dims, int nmax, double lambda,
                                                      double* __restrict__ A, size_t A_stride)
{
    const int p = blockIdx.z, n = dims[4 * p];
    const int i0 = blockIdx.y * 16, j0 = blockIdx.x * 16;
    if (i0 >= n || j0 >= n) return;                          // uniform over the block
    __shared__ double sr[2][16][MATCH_REC];
    const int tid = threadIdx.y * 16 + threadIdx.x;
    for (int f = tid; f < 2 * 16 * MATCH_REC; f += 256) {
        const int side = f / (16 * MATCH_REC), g = f - side * 16 * MATCH_REC, c = g / MATCH_REC, q = g - c * MATCH_REC;
        const int cidx = (side ? j0 : i0) + c;
        sr[side][c][q] = cidx < n ? rec[((size_t)p * nmax + cidx) * MATCH_REC + q] : 0.0;
    }
    __syncthreads();
    const int i = i0 + threadIdx.y, j = j0 + threadIdx.x;
    if (i >= n || j >= n) return;
    const double* a1 = sr[0][threadIdx.y];
    const double* a2 = sr[1][threadIdx.x];
    const int* k1 = (const int*)(a1 + 9);
    const int* k2 = (const int*)(a2 + 9);
    double v = 0.0;
    if (!(k1[0] == k2[0] || k1[1] == k2[1])) {
        const double s1x = a1[5], s1y = a1[6], t1x = a1[7], t1y = a1[8];
        const double s2x = a2[5], s2y = a2[6], t2x = a2[7], t2y = a2[8];
        const double eX = t2x - (a1[4] * (s2x * a1[0] - s2y * a1[1]) + a1[2]);
        const double eY = t2y - (a1[4] * (s2x * a1[1] + s2y * a1[0]) + a1[3]);
        const double eX2 = t1x - (a2[4] * (a2[0] * s1x - a2[1] * s1y) + a2[2]);
        const double eY2 = t1y - (a2[4] * (a2[1] * s1x + a2[0] * s1y) + a2[3]);
        const double e1 = eX * eX + eY * eY, e2 = eX2 * eX2 + eY2 * eY2;
        const double ge = e1 < e2 ? e2 : e1;                 // std::max
        v = exp(-lambda * ge);
    }
    A[p * A_stride + (size_t)i * n + j] = v;
}

// ------------------------------------------------------------------------------------------------------------------ dynamics
// The sum over a wave.  A problem of at most 64 strategies lives in one wave with one element per lane, and is summed lane by lane:
// that is the reference's own order, so the exact ties of tiny degenerate games (two equal cliques from the uniform start) are
// broken by the same rounding as in the reference.  Larger problems take the butterfly.
__device__ __forceinline__ double wave_sum_f64(double v, bool seq)
{
    if (seq) {
        double s = __shfl(v, 0);
        for (int l = 1; l < 64; ++l) s += __shfl(v, l);
        return s;
    }
    return wave_all(v, [](double a, double b) { return a + b; });
}

// the sum over the workgroup: a thread's own terms in index order, the wave's sum, the sixteen waves in order
__device__ __forceinline__ double block_sum_f64(double v, double* slot, bool seq)
{
    v = wave_sum_f64(v, seq);
    if ((threadIdx.x & 63) == 0) slot[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = slot[0];
#pragma unroll
    for (int w = 1; w < IID_WAVES; ++w) s += slot[w];
    return s;
}

// simplexify (iidyn.cpp:58-69) on the registers of a workgroup
__device__ __forceinline__ void simplexify_regs(double (&x)[IID_E], int n, double* slot)
{
    double s = 0.0;
#pragma unroll
    for (int e = 0; e < IID_E; ++e)
        if ((int)threadIdx.x + e * IID_THREADS < n) {
            if (x[e] >= 0) s += x[e];
            else x[e] = 0.0;
        }
    const double sum = block_sum_f64(s, slot, n <= 64);
#pragma unroll
    for (int e = 0; e < IID_E; ++e) x[e] /= sum;
}

__global__ void __launch_bounds__(IID_THREADS) k_match_start(double* __restrict__ X, size_t x_stride, const int* __restrict__ dims, int uniform)
{
    __shared__ double slot[IID_WAVES];
    const int p = blockIdx.x, n = dims[4 * p];
    double* xp = X + p * x_stride;
    double x[IID_E];
#pragma unroll
    for (int e = 0; e < IID_E; ++e) {
        const int i = threadIdx.x + e * IID_THREADS;
        x[e] = i < n ? (uniform ? 1.0 / (double)n : xp[i]) : 0.0;       // gt_create_population: 1.0 each, divided by their sum
    }
    simplexify_regs(x, n, slot);
#pragma unroll
    for (int e = 0; e < IID_E; ++e) {
        const int i = threadIdx.x + e * IID_THREADS;
        if (i < n) xp[i] = x[e];
    }
}

__global__ void __launch_bounds__(256) k_match_ax0(const double* __restrict__ A, size_t A_stride, const double* __restrict__ X, size_t x_stride,
                                                   const int* __restrict__ dims, int nmax, double* __restrict__ Ax)
{
    const int p = blockIdx.y, n = dims[4 * p];
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= n) return;                                    // uniform over the wave; no barrier below
    const double* a = A + p * A_stride + (size_t)row * n;
    const double* x = X + p * x_stride;
    double s = 0.0;
    for (int j = lane; j < n; j += 64) s += a[j] * x[j];
    s = wave_sum_f64(s, n <= 64);
    if (lane == 0) Ax[(size_t)p * nmax + row] = s;
}

__global__ void __launch_bounds__(IID_THREADS) k_match_iidyn(const double* __restrict__ A, size_t A_stride, double* __restrict__ X, size_t x_stride,
                                                             const double* __restrict__ Ax0, int nmax, const int* __restrict__ dims, double toll2,
                                                             int max_iters, double pop_threshold, MatchRes* __restrict__ res,
                                                             uint8_t* __restrict__ group, size_t group_stride)
{
    __shared__ double r_max[IID_WAVES], r_min[IID_WAVES], r_dot[IID_WAVES], r_err[IID_WAVES], r_sum[IID_WAVES], r_fin[IID_WAVES];
    __shared__ int r_maxi[IID_WAVES], r_mini[IID_WAVES];
    __shared__ double b_x, b_ax;
    __shared__ int s_count;
    const int p = blockIdx.x, n = dims[4 * p];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool seq = n <= 64;
    const double* Ap = A + p * A_stride;
    double* xp = X + p * x_stride;
    double x[IID_E], ax[IID_E];
#pragma unroll
    for (int e = 0; e < IID_E; ++e) {
        const int i = tid + e * IID_THREADS;
        x[e] = i < n ? xp[i] : 0.0;
        ax[e] = i < n ? Ax0[(size_t)p * nmax + i] : 0.0;
    }
    if (tid == 0) s_count = 0;
    int niter = 0;
    double err = DBL_MAX;
    while (niter < max_iters) {
        // selectStrategy (:171-208): the first largest Ax, the first smallest Ax among x > 0, x'Ax
        double mx = -INFINITY, mn = INFINITY, dot = 0.0;
        int mxi = INT_MAX, mni = INT_MAX;
#pragma unroll
        for (int e = 0; e < IID_E; ++e) {
            const int i = tid + e * IID_THREADS;
            if (i < n) {
                if (ax[e] > mx) { mx = ax[e]; mxi = i; }
                if (x[e] > 0 && ax[e] < mn) { mn = ax[e]; mni = i; }
                dot += ax[e] * x[e];
            }
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            const double ov = __shfl_xor(mx, m), un = __shfl_xor(mn, m);
            const int oi = __shfl_xor(mxi, m), ui = __shfl_xor(mni, m);
            if (ov > mx || (ov == mx && oi < mxi)) { mx = ov; mxi = oi; }
            if (un < mn || (un == mn && ui < mni)) { mn = un; mni = ui; }
        }
        dot = wave_sum_f64(dot, seq);
        if (lane == 0) { r_max[wave] = mx; r_maxi[wave] = mxi; r_min[wave] = mn; r_mini[wave] = mni; r_dot[wave] = dot; }
        __syncthreads();
        mx = r_max[0]; mxi = r_maxi[0]; mn = r_min[0]; mni = r_mini[0];
        double xAx = r_dot[0];
#pragma unroll
        for (int w = 1; w < IID_WAVES; ++w) {
            if (r_max[w] > mx || (r_max[w] == mx && r_maxi[w] < mxi)) { mx = r_max[w]; mxi = r_maxi[w]; }
            if (r_min[w] < mn || (r_min[w] == mn && r_mini[w] < mni)) { mn = r_min[w]; mni = r_mini[w]; }
            xAx += r_dot[w];
        }
        const double maxv = mx - xAx, minv = xAx - mn;
        int idx = mxi;
        double delta = maxv;
        if (maxv < minv) { idx = mni; delta = -minv; }
        const bool have = idx >= 0 && idx < n;               // the reference's idx is -1 when nothing qualified (and it then reads A[-size-1])
        // the row of the chosen strategy is asked for now and used after the two reductions below
        double row[IID_E], aii = 0.0;
#pragma unroll
        for (int e = 0; e < IID_E; ++e) {
            const int i = tid + e * IID_THREADS;
            row[e] = (have && i < n) ? Ap[(size_t)idx * n + i] : 0.0;
        }
        if (have) aii = Ap[(size_t)idx * (n + 1)];
        const int e0 = have ? idx / IID_THREADS : -1;
        const bool owner = have && (idx % IID_THREADS) == tid;
        if (owner) {
#pragma unroll
            for (int e = 0; e < IID_E; ++e)
                if (e == e0) { b_x = x[e]; b_ax = ax[e]; }
        }
        // nash_error (:137-151)
        double ne = 0.0;
#pragma unroll
        for (int e = 0; e < IID_E; ++e)
            if (tid + e * IID_THREADS < n) {
                double tmp = xAx - ax[e];
                if (tmp > x[e]) tmp = x[e];
                ne += tmp * tmp;
            }
        err = block_sum_f64(ne, r_err, seq);
        if (err < toll2) break;
        if (!have) break;
        const double xi = b_x, axi = b_ax;
        const double den = aii - axi - delta;
        bool do_remove = false;
        double mu, tmp;
        if (delta >= 0) {
            mu = 1;
            if (den < 0) {
                tmp = -delta / den;
                if (mu > tmp) mu = tmp;
                if (mu < 0) mu = 0;
            }
        } else {
            mu = xi / (xi - 1);
            do_remove = true;
            if (den < 0) {
                tmp = -delta / den;
                if (mu < tmp) { mu = tmp; do_remove = false; }
                if (mu > 0) mu = 0;
            }
        }
        const double c = 1 - mu;
#pragma unroll
        for (int e = 0; e < IID_E; ++e) x[e] *= c;           // scale
        if (owner) {
#pragma unroll
            for (int e = 0; e < IID_E; ++e)
                if (e == e0) x[e] = do_remove ? 0.0 : x[e] + mu;
        }
        simplexify_regs(x, n, r_sum);
#pragma unroll
        for (int e = 0; e < IID_E; ++e) ax[e] = mu * (row[e] - ax[e]) + ax[e];   // linear_comb
        ++niter;
    }
    // match_group (GTMatcher.cpp:273-293): the strategies above max(x) * pop_threshold
    double m = -INFINITY;
#pragma unroll
    for (int e = 0; e < IID_E; ++e) {
        const int i = tid + e * IID_THREADS;
        if (i < n) {
            xp[i] = x[e];
            if (x[e] > m) m = x[e];
        }
    }
    m = wave_all(m, [](double a, double o) { return o > a ? o : a; });
    if (lane == 0) r_fin[wave] = m;
    __syncthreads();
    m = r_fin[0];
#pragma unroll
    for (int w = 1; w < IID_WAVES; ++w) if (r_fin[w] > m) m = r_fin[w];
    const double thr = m * pop_threshold;
    int mine = 0;
#pragma unroll
    for (int e = 0; e < IID_E; ++e) {
        const int i = tid + e * IID_THREADS;
        if (i < n) {
            const bool win = x[e] > thr;
            group[p * group_stride + i] = win ? 1 : 0;
            mine += win ? 1 : 0;
        }
    }
    if (mine) atomicAdd(&s_count, mine);
    __syncthreads();
    if (tid == 0) { res[p].err = err; res[p].steps = niter; res[p].group = s_count; }
}

// ---------------------------------------------------------------------------------------------------------------- host side
struct MatchPlan {
    int batch = 0, nmax = 0;
    int* d_flag = nullptr;
    int* d_dims = nullptr;
    MatchRes* d_res = nullptr;
    double* d_rec = nullptr;
    double* d_ax = nullptr;
};

// The layout of c->match for a batch whose largest problem has nmax candidates.  Every kernel indexes d_rec and d_ax by
// (problem * nmax + candidate) with candidate < n[problem] <= nmax: nothing is read or written past a piece, and none has slack.
static void match_carve(MatchPlan& pl, int batch, int nmax, Carve& a)
{
    const size_t cells = (size_t)batch * nmax;
    pl.batch = batch; pl.nmax = nmax;
    pl.d_flag = a.take<int>(256);
    pl.d_dims = a.take<int>((size_t)batch * 4 * sizeof(int));
    pl.d_res = a.take<MatchRes>((size_t)batch * sizeof(MatchRes));
    pl.d_rec = a.take<double>(cells * MATCH_REC * sizeof(double));
    pl.d_ax = a.take<double>(cells * sizeof(double));
}

static size_t match_ctx_bytes(int batch, int nmax) { MatchPlan pl; return measure([&](Carve& a) { match_carve(pl, batch, nmax, a); }); }

// checks the sizes of a batch, lays the context's scratch out and uploads the sizes
static int match_plan(wass_ctx* c, const int* n, const int* na, const int* nb, int batch, MatchPlan* pl, hipStream_t s)
{
    if (!n || batch < 1 || batch > 65535) return set_err(c, WASS_ERR_INVALID_ARG, "batch = %d: 1 .. 65535 problems with their sizes", batch);
    int nmax = 0;
    for (int p = 0; p < batch; ++p) {
        if (n[p] < 1 || n[p] > WASS_MATCH_MAX_N)
            return set_err(c, WASS_ERR_INVALID_ARG, "problem %d has %d candidates: 1 .. %d", p, n[p], WASS_MATCH_MAX_N);
        if ((na && na[p] < 1) || (nb && nb[p] < 1)) return set_err(c, WASS_ERR_INVALID_ARG, "problem %d has an empty feature set", p);
        nmax = n[p] > nmax ? n[p] : nmax;
    }
    int rc = carve_buf(c, c->match, [&](Carve& a) { match_carve(*pl, batch, nmax, a); });
    if (rc) return rc;
    std::vector<int> dims((size_t)batch * 4, 0);
    for (int p = 0; p < batch; ++p) {
        dims[4 * p] = n[p];
        dims[4 * p + 1] = na ? na[p] : 0;
        dims[4 * p + 2] = nb ? nb[p] : 0;
    }
    WASS_HIP(c, hipMemsetAsync(pl->d_flag, 0, 256, s));
    WASS_HIP(c, hipMemcpyAsync(pl->d_dims, dims.data(), dims.size() * sizeof(int), hipMemcpyHostToDevice, s));
    WASS_HIP(c, hipStreamSynchronize(s));                    // dims is about to go out of scope
    return WASS_OK;
}

static int match_strides(wass_ctx* c, const MatchPlan& pl, size_t A_stride, size_t x_stride, size_t group_stride)
{
    if (pl.batch > 1 && (A_stride < (size_t)pl.nmax * pl.nmax || x_stride < (size_t)pl.nmax || group_stride < (size_t)pl.nmax))
        return set_err(c, WASS_ERR_INVALID_ARG, "a batch stride is shorter than its largest problem (%d candidates)", pl.nmax);
    return WASS_OK;
}

static int payoff_enqueue(wass_ctx* c, const MatchPlan& pl, const float* d_fa, size_t fa_stride, const float* d_fb, size_t fb_stride,
                          const int* d_cand, size_t cand_stride, double lambda, double* d_A, size_t A_stride, hipStream_t s)
{
    hipLaunchKernelGGL(k_match_affine, dim3((unsigned)((pl.nmax + 255) / 256), (unsigned)pl.batch), dim3(256), 0, s, d_fa, fa_stride, d_fb,
                       fb_stride, d_cand, cand_stride, pl.d_dims, pl.nmax, pl.d_rec, pl.d_flag);
    const unsigned t = (unsigned)((pl.nmax + 15) / 16);
    hipLaunchKernelGGL(k_match_payoff, dim3(t, t, (unsigned)pl.batch), dim3(16, 16), 0, s, pl.d_rec, pl.d_dims, pl.nmax, lambda, d_A, A_stride);
    WASS_HIP(c, hipGetLastError());
    return WASS_OK;
}

static int iidyn_enqueue(wass_ctx* c, const MatchPlan& pl, const double* d_A, size_t A_stride, double* d_x, size_t x_stride, int uniform,
                         double toll, int max_iters, double pop_threshold, uint8_t* d_group, size_t group_stride, hipStream_t s)
{
    hipLaunchKernelGGL(k_match_start, dim3((unsigned)pl.batch), dim3(IID_THREADS), 0, s, d_x, x_stride, pl.d_dims, uniform);
    hipLaunchKernelGGL(k_match_ax0, dim3((unsigned)((pl.nmax + 3) / 4), (unsigned)pl.batch), dim3(256), 0, s, d_A, A_stride, d_x, x_stride, pl.d_dims,
                       pl.nmax, pl.d_ax);
    hipLaunchKernelGGL(k_match_iidyn, dim3((unsigned)pl.batch), dim3(IID_THREADS), 0, s, d_A, A_stride, d_x, x_stride, pl.d_ax, pl.nmax, pl.d_dims,
                       toll * toll, max_iters, pop_threshold, pl.d_res, d_group, group_stride);
    WASS_HIP(c, hipGetLastError());
    return WASS_OK;
}

// waits for the work, reads the flag of the candidate check and the per-problem records
static int match_collect(wass_ctx* c, const MatchPlan& pl, bool dynamics, int* steps, double* err, int* group_size, hipStream_t s)
{
    int flag = 0;
    std::vector<MatchRes> res((size_t)pl.batch);
    WASS_HIP(c, hipMemcpyAsync(&flag, pl.d_flag, sizeof flag, hipMemcpyDeviceToHost, s));
    if (dynamics) WASS_HIP(c, hipMemcpyAsync(res.data(), pl.d_res, res.size() * sizeof(MatchRes), hipMemcpyDeviceToHost, s));
    WASS_HIP(c, hipStreamSynchronize(s));
    if (flag & MATCH_BAD_INDEX) return set_err(c, WASS_ERR_INVALID_ARG, "a candidate names a feature outside its set");
    if (flag & MATCH_BAD_ANGLE)
        return set_err(c, WASS_ERR_INVALID_ARG, "two feature angles differ by more than %g or are not numbers", MATCH_MAX_ANGLE);
    if (dynamics)
        for (int p = 0; p < pl.batch; ++p) {
            if (steps) steps[p] = res[(size_t)p].steps;
            if (err) err[p] = res[(size_t)p].err;
            if (group_size) group_size[p] = res[(size_t)p].group;
        }
    return WASS_OK;
}

static int knn_args(wass_ctx* c, const void* a, int na, const void* b, int nb, int d, int k, const void* idx, const void* dist)
{
    if (!c) return WASS_ERR_INVALID_ARG;
    if (!a || !b || !idx || !dist) return set_err(c, WASS_ERR_INVALID_ARG, "null argument");
    if (na < 1 || nb < 1) return set_err(c, WASS_ERR_INVALID_ARG, "na = %d, nb = %d: both feature sets need a feature", na, nb);
    if (k < 1 || k > WASS_MATCH_MAX_K) return set_err(c, WASS_ERR_INVALID_ARG, "k = %d: 1 .. %d candidates per feature", k, WASS_MATCH_MAX_K);
    if (d < 1 || d > WASS_MATCH_MAX_DESC) return set_err(c, WASS_ERR_INVALID_ARG, "descriptors of %d values: 1 .. %d", d, WASS_MATCH_MAX_DESC);
    return WASS_OK;
}

}  // namespace wass

using namespace wass;

extern "C" {

int wass_match_scratch_bytes(int batch, int n_max, size_t* bytes)
{
    if (!bytes || batch < 1 || batch > 65535 || n_max < 1 || n_max > WASS_MATCH_MAX_N) return WASS_ERR_INVALID_ARG;
    const size_t n = (size_t)n_max;
    *bytes = (size_t)batch * (n * n * sizeof(double) + n * sizeof(double) + n + 2 * n * sizeof(int)) + match_ctx_bytes(batch, n_max);
    return WASS_OK;
}

int wass_match_knn_dev(wass_ctx* c, const float* d_desc_a, int na, const float* d_desc_b, int nb, int d, int k, int32_t* d_idx, float* d_dist)
{
    int rc = knn_args(c, d_desc_a, na, d_desc_b, nb, d, k, d_idx, d_dist);
    if (rc) return rc;
    WASS_HIP(c, hipSetDevice(c->device));
    const int kk = k < nb ? k : nb;
    hipLaunchKernelGGL(k_match_knn, dim3((unsigned)((na + KNN_LANES - 1) / KNN_LANES)), dim3(KNN_LANES), (size_t)d * KNN_LANES * sizeof(float), c->ts(),
                       d_desc_a, na, d_desc_b, nb, d, kk, d_idx, d_dist);
    WASS_HIP(c, hipGetLastError());
    WASS_HIP(c, hipStreamSynchronize(c->ts()));
    return WASS_OK;
}

int wass_match_knn(wass_ctx* c, const float* desc_a, int na, const float* desc_b, int nb, int d, int k, int32_t* idx, float* dist)
{
    int rc = knn_args(c, desc_a, na, desc_b, nb, d, k, idx, dist);
    if (rc) return rc;
    WASS_HIP(c, hipSetDevice(c->device));
    const int kk = k < nb ? k : nb;
    const size_t ba = (size_t)na * d * 4, bb = (size_t)nb * d * 4, bo = (size_t)na * kk * 4;
    float *d_a, *d_b, *d_dist;
    int32_t* d_idx;
    if ((rc = carve_buf(c, c->match_io, [&](Carve& a) {
            d_a = a.take<float>(ba); d_b = a.take<float>(bb); d_idx = a.take<int32_t>(bo); d_dist = a.take<float>(bo);
        })))
        return rc;
    hipStream_t s = c->ts();
    WASS_HIP(c, hipMemcpyAsync(d_a, desc_a, ba, hipMemcpyHostToDevice, s));
    WASS_HIP(c, hipMemcpyAsync(d_b, desc_b, bb, hipMemcpyHostToDevice, s));
    if ((rc = wass_match_knn_dev(c, d_a, na, d_b, nb, d, k, d_idx, d_dist))) return rc;
    WASS_HIP(c, hipMemcpyAsync(idx, d_idx, bo, hipMemcpyDeviceToHost, s));
    WASS_HIP(c, hipMemcpyAsync(dist, d_dist, bo, hipMemcpyDeviceToHost, s));
    WASS_HIP(c, hipStreamSynchronize(s));
    return WASS_OK;
}

int wass_match_payoff_dev(wass_ctx* c, const float* d_fa, size_t fa_stride, const float* d_fb, size_t fb_stride, const int32_t* d_cand,
                          size_t cand_stride, const int* n, const int* na, const int* nb, int batch, double lambda, double* d_A, size_t A_stride)
{
    if (!c) return WASS_ERR_INVALID_ARG;
    if (!d_fa || !d_fb || !d_cand || !na || !nb || !d_A) return set_err(c, WASS_ERR_INVALID_ARG, "null argument");
    WASS_HIP(c, hipSetDevice(c->device));
    MatchPlan pl;
    hipStream_t s = c->ts();
    int rc = match_plan(c, n, na, nb, batch, &pl, s);
    if (rc) return rc;
    if ((rc = match_strides(c, pl, A_stride, (size_t)pl.nmax, (size_t)pl.nmax))) return rc;
    if (batch > 1 && cand_stride < 2 * (size_t)pl.nmax) return set_err(c, WASS_ERR_INVALID_ARG, "cand_stride is shorter than the largest problem");
    if ((rc = payoff_enqueue(c, pl, d_fa, fa_stride, d_fb, fb_stride, d_cand, cand_stride, lambda, d_A, A_stride, s))) return rc;
    return match_collect(c, pl, false, nullptr, nullptr, nullptr, s);
}

int wass_match_payoff(wass_ctx* c, const float* fa, int na, const float* fb, int nb, const int32_t* cand, int n, double lambda, double* A)
{
    if (!c) return WASS_ERR_INVALID_ARG;
    if (!fa || !fb || !cand || !A) return set_err(c, WASS_ERR_INVALID_ARG, "null argument");
    if (n < 1 || n > WASS_MATCH_MAX_N) return set_err(c, WASS_ERR_INVALID_ARG, "%d candidates: 1 .. %d", n, WASS_MATCH_MAX_N);
    if (na < 1 || nb < 1) return set_err(c, WASS_ERR_INVALID_ARG, "an empty feature set");
    WASS_HIP(c, hipSetDevice(c->device));
    const size_t ba = (size_t)na * 16, bb = (size_t)nb * 16, bc = (size_t)n * 8, bA = (size_t)n * n * 8;
    float *d_fa, *d_fb;
    int32_t* d_cand;
    double* d_A;
    int rc = carve_buf(c, c->match_io, [&](Carve& a) {
        d_fa = a.take<float>(ba); d_fb = a.take<float>(bb); d_cand = a.take<int32_t>(bc); d_A = a.take<double>(bA);
    });
    if (rc) return rc;
    hipStream_t s = c->ts();
    WASS_HIP(c, hipMemcpyAsync(d_fa, fa, ba, hipMemcpyHostToDevice, s));
    WASS_HIP(c, hipMemcpyAsync(d_fb, fb, bb, hipMemcpyHostToDevice, s));
    WASS_HIP(c, hipMemcpyAsync(d_cand, cand, bc, hipMemcpyHostToDevice, s));
    if ((rc = wass_match_payoff_dev(c, d_fa, 0, d_fb, 0, d_cand, 0, &n, &na, &nb, 1, lambda, d_A, 0))) return rc;
    WASS_HIP(c, hipMemcpyAsync(A, d_A, bA, hipMemcpyDeviceToHost, s));
    WASS_HIP(c, hipStreamSynchronize(s));
    return WASS_OK;
}

int wass_match_iidyn_dev(wass_ctx* c, const double* d_A, size_t A_stride, double* d_x, size_t x_stride, int uniform_start, const int* n, int batch,
                         double toll, int max_iters, double pop_threshold, int* steps, double* err, uint8_t* d_group, size_t group_stride,
                         int* group_size)
{
    if (!c) return WASS_ERR_INVALID_ARG;
    if (!d_A || !d_x || !d_group) return set_err(c, WASS_ERR_INVALID_ARG, "null argument");
    if (max_iters < 0) return set_err(c, WASS_ERR_INVALID_ARG, "max_iters = %d", max_iters);
    WASS_HIP(c, hipSetDevice(c->device));
    MatchPlan pl;
    hipStream_t s = c->ts();
    int rc = match_plan(c, n, nullptr, nullptr, batch, &pl, s);
    if (rc) return rc;
    if ((rc = match_strides(c, pl, A_stride, x_stride, group_stride))) return rc;
    if ((rc = iidyn_enqueue(c, pl, d_A, A_stride, d_x, x_stride, uniform_start, toll, max_iters, pop_threshold, d_group, group_stride, s))) return rc;
    return match_collect(c, pl, true, steps, err, group_size, s);
}

int wass_match_iidyn(wass_ctx* c, const double* A, int n, double* x, int uniform_start, double toll, int max_iters, double pop_threshold, int* steps,
                     double* err, uint8_t* group, int* group_size)
{
    if (!c) return WASS_ERR_INVALID_ARG;
    if (!A || !x || !group) return set_err(c, WASS_ERR_INVALID_ARG, "null argument");
    if (n < 1 || n > WASS_MATCH_MAX_N) return set_err(c, WASS_ERR_INVALID_ARG, "%d candidates: 1 .. %d", n, WASS_MATCH_MAX_N);
    WASS_HIP(c, hipSetDevice(c->device));
    const size_t bA = (size_t)n * n * 8, bx = (size_t)n * 8;
    double *d_A, *d_x;
    uint8_t* d_group;
    int rc = carve_buf(c, c->match_io, [&](Carve& a) { d_A = a.take<double>(bA); d_x = a.take<double>(bx); d_group = a.take<uint8_t>((size_t)n); });
    if (rc) return rc;
    hipStream_t s = c->ts();
    WASS_HIP(c, hipMemcpyAsync(d_A, A, bA, hipMemcpyHostToDevice, s));
    if (!uniform_start) WASS_HIP(c, hipMemcpyAsync(d_x, x, bx, hipMemcpyHostToDevice, s));
    if ((rc = wass_match_iidyn_dev(c, d_A, 0, d_x, 0, uniform_start, &n, 1, toll, max_iters, pop_threshold, steps, err, d_group, 0, group_size)))
        return rc;
    WASS_HIP(c, hipMemcpyAsync(x, d_x, bx, hipMemcpyDeviceToHost, s));
    WASS_HIP(c, hipMemcpyAsync(group, d_group, (size_t)n, hipMemcpyDeviceToHost, s));
    WASS_HIP(c, hipStreamSynchronize(s));
    return WASS_OK;
}

int wass_match_round_dev(wass_ctx* c, const float* d_fa, size_t fa_stride, const float* d_fb, size_t fb_stride, const int32_t* d_cand,
                         size_t cand_stride, const int* n, const int* na, const int* nb, int batch, double lambda, double toll, int max_iters,
                         double pop_threshold, double* d_A, size_t A_stride, double* d_x, size_t x_stride, int* steps, double* err,
                         uint8_t* d_group, size_t group_stride, int* group_size)
{
    if (!c) return WASS_ERR_INVALID_ARG;
    if (!d_fa || !d_fb || !d_cand || !na || !nb || !d_A || !d_x || !d_group) return set_err(c, WASS_ERR_INVALID_ARG, "null argument");
    if (max_iters < 0) return set_err(c, WASS_ERR_INVALID_ARG, "max_iters = %d", max_iters);
    WASS_HIP(c, hipSetDevice(c->device));
    MatchPlan pl;
    hipStream_t s = c->ts();
    int rc = match_plan(c, n, na, nb, batch, &pl, s);
    if (rc) return rc;
    if ((rc = match_strides(c, pl, A_stride, x_stride, group_stride))) return rc;
    if (batch > 1 && cand_stride < 2 * (size_t)pl.nmax) return set_err(c, WASS_ERR_INVALID_ARG, "cand_stride is shorter than the largest problem");
    if ((rc = payoff_enqueue(c, pl, d_fa, fa_stride, d_fb, fb_stride, d_cand, cand_stride, lambda, d_A, A_stride, s))) return rc;
    if ((rc = iidyn_enqueue(c, pl, d_A, A_stride, d_x, x_stride, 1, toll, max_iters, pop_threshold, d_group, group_stride, s))) return rc;
    return match_collect(c, pl, true, steps, err, group_size, s);
}

}  // extern "C"
