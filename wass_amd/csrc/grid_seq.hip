// grid_seq.hip -- the sequence layer of the gridding stage: what wassgridsurface --action grid does
// with every interpolated surface Zi of a sequence besides interpolating it.
//
// Reference: gridding/wassgridsurface/wassgridsurface.py
//   --mf (:359-363)        Zi[mask == 0] = 0; Zi = cv.medianBlur(Zi, ksize = mf); Zi[mask == 0] = NaN     (float32; cv::medianBlur
//                          replicates the border and takes float32 for ksize 3 and 5 only)
//   per frame (:490-494)   Zmean_grid += Zi (fp64);  Zmeans / Zmins / Zmaxs += nanmean / nanmin / nanmax of Zi
//   push_Z (:513)          the cube stores Zi * 1000 (millimetres) as float32
//   at the end (:528-546)  Zmin = amin(Zmins), Zmax = amax(Zmaxs), Zmean = mean(Zmeans), Zmean_perpoint = Zmean_grid / N * 1000;
//                          --force-zero-mean: Zmean = 0, Zmax = -Zmin, and (:554-576) cube -= Zmean_perpoint (float32 chunk minus
//                          float64 mean, stored as float32)
// Nothing here uses a floating-point atomic: every sum runs in a fixed order that depends on the grid size only, so the same
// frames give the same bits however they are split over the push calls.
#include "common.h"

#include <math.h>
#include <vector>

namespace wass {

constexpr int MED_TX = 32, MED_TY = 8;      // cells per workgroup of k_grid_median

// One thread per cell: the K x K window (border replicated) from an LDS tile, sorted in registers by an odd-even transposition
// network; the median is the middle element, so the result is one of the inputs, bit for bit.  A window that holds a NaN gives
// NaN (numpy's median; the reference only ever has NaN where the mask is 0, and those cells are 0 here).  Frame blockIdx.z.
template <int K>
__global__ void __launch_bounds__(MED_TX * MED_TY) k_grid_median(const float* __restrict__ in, float* __restrict__ out, int W, int H,
                                                               const uint8_t* __restrict__ mask)
{
    constexpr int R = K / 2, TW = MED_TX + 2 * R, TH = MED_TY + 2 * R, N = K * K;
    __shared__ float tile[TH][TW];
    in += (size_t)blockIdx.z * W * H;
    out += (size_t)blockIdx.z * W * H;
    const int x0 = blockIdx.x * MED_TX, y0 = blockIdx.y * MED_TY;
    for (int i = threadIdx.y * MED_TX + threadIdx.x; i < TW * TH; i += MED_TX * MED_TY) {
        const int tx = i % TW, ty = i / TW;
        const int x = min(max(x0 + tx - R, 0), W - 1), y = min(max(y0 + ty - R, 0), H - 1);
        const size_t q = (size_t)y * W + x;
        tile[ty][tx] = (mask && !mask[q]) ? 0.f : in[q];
    }
    __syncthreads();
    const int x = x0 + threadIdx.x, y = y0 + threadIdx.y;
    if (x >= W || y >= H) return;
    float v[N];
    bool nan = false;
#pragma unroll
    for (int dy = 0; dy < K; ++dy)
#pragma unroll
        for (int dx = 0; dx < K; ++dx) {
            const float t = tile[threadIdx.y + dy][threadIdx.x + dx];
            nan = nan || isnan(t);
            v[dy * K + dx] = t;
        }
#pragma unroll
    for (int pass = 0; pass < N; ++pass)
#pragma unroll
        for (int i = pass & 1; i + 1 < N; i += 2) {
            const float a = v[i], b = v[i + 1];
            v[i] = a < b ? a : b;
            v[i + 1] = a < b ? b : a;
        }
    const size_t q = (size_t)y * W + x;
    out[q] = (nan || (mask && !mask[q])) ? __builtin_nanf("") : v[N / 2];
}

__global__ void __launch_bounds__(256) k_seq_copy_masked(const float* __restrict__ in, float* __restrict__ out, size_t hw,
                                                         const uint8_t* __restrict__ mask)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= hw) return;
    const size_t q = (size_t)blockIdx.y * hw + i;
    out[q] = (mask && !mask[i]) ? __builtin_nanf("") : in[q];
}

// per cell, the frames in push order: acc += (double)Zi (NaN propagates), mm = Zi * 1000 in float32
__global__ void __launch_bounds__(256) k_seq_acc(const float* __restrict__ zi, int n, size_t hw, double* __restrict__ acc, float* __restrict__ mm)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= hw) return;
    double a = acc[i];
    for (int f = 0; f < n; ++f) {
        const float z = zi[(size_t)f * hw + i];
        a += (double)z;
        if (mm) mm[(size_t)f * hw + i] = z * 1000.0f;
    }
    acc[i] = a;
}

struct SeqPart {
    double sum;
    unsigned long long cnt;
    float mn, mx;
};

static __device__ __forceinline__ void seq_merge(SeqPart& a, const SeqPart& b)
{
    a.sum += b.sum;
    a.cnt += b.cnt;
    a.mn = fminf(a.mn, b.mn);                                // fminf / fmaxf skip a NaN operand: NaN only when no cell had data
    a.mx = fmaxf(a.mx, b.mx);
}

// sum (fp64), count, min and max of the cells that are not NaN: workgroup blockIdx.x of frame blockIdx.y takes the cells
// blockIdx.x * 256 + threadIdx.x + k * gridDim.x * 256, then a tree over its threads.  The order depends on hw and gridDim.x only.
__global__ void __launch_bounds__(256) k_seq_stats(const float* __restrict__ zi, size_t hw, SeqPart* __restrict__ part)
{
    __shared__ SeqPart sh[256];
    zi += (size_t)blockIdx.y * hw;
    SeqPart p = {0.0, 0ull, __builtin_nanf(""), __builtin_nanf("")};
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < hw; i += (size_t)gridDim.x * 256) {
        const float z = zi[i];
        if (isnan(z)) continue;
        p.sum += (double)z;
        p.cnt += 1;
        p.mn = fminf(p.mn, z);
        p.mx = fmaxf(p.mx, z);
    }
    sh[threadIdx.x] = p;
    __syncthreads();
    block_tree<256>([&](int t, int u) { seq_merge(sh[t], sh[u]); });
    if (threadIdx.x == 0) part[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = sh[0];
}

// the workgroups' partials of frame blockIdx.x in index order: res[3 f ..] = {nanmean, nanmin, nanmax} (NaN for a frame of NaN)
__global__ void __launch_bounds__(256) k_seq_stats_final(const SeqPart* __restrict__ part, int nblk, double* __restrict__ res)
{
    __shared__ SeqPart sh[256];
    part += (size_t)blockIdx.x * nblk;
    SeqPart p = {0.0, 0ull, __builtin_nanf(""), __builtin_nanf("")};
    if ((int)threadIdx.x < nblk) p = part[threadIdx.x];      // nblk <= 256
    sh[threadIdx.x] = p;
    __syncthreads();
    block_tree<256>([&](int t, int u) { seq_merge(sh[t], sh[u]); });
    if (threadIdx.x == 0) {
        res[3 * blockIdx.x] = sh[0].cnt ? sh[0].sum / (double)sh[0].cnt : (double)__builtin_nanf("");
        res[3 * blockIdx.x + 1] = (double)sh[0].mn;
        res[3 * blockIdx.x + 2] = (double)sh[0].mx;
    }
}

// Zmean_perpoint = acc / N * 1000 (:534), in that order
__global__ void __launch_bounds__(256) k_seq_mean(const double* __restrict__ acc, size_t hw, double n, double* __restrict__ mean)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < hw) mean[i] = acc[i] / n * 1000.0;
}

// float32 chunk minus float64 mean, stored as float32 (:570-576)
__global__ void __launch_bounds__(256) k_seq_zero_mean(float* __restrict__ z, size_t hw, const double* __restrict__ mean)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= hw) return;
    const size_t q = (size_t)blockIdx.y * hw + i;
    z[q] = (float)((double)z[q] - mean[i]);
}

}  // namespace wass

using namespace wass;

struct wass_grid_seq {
    wass_ctx* c = nullptr;
    int W = 0, H = 0;
    double* acc = nullptr;         // per-point sum of the pushed frames (fp64)
    double* mean = nullptr;        // Zmean_perpoint in millimetres, filled by wass_grid_seq_finish
    bool finished = false;
    Buf part;                      // the statistics' partials and results of one push
    std::vector<double> fmean, fmin, fmax;
};

extern "C" int wass_grid_median_dev(wass_ctx* c, const float* d_in, float* d_out, int n_frames, int width, int height, int ksize,
                                    const uint8_t* d_mask)
{
    if (!c || !d_in || !d_out) return set_err(c, WASS_ERR_INVALID_ARG, "null argument");
    if (n_frames < 1 || width < 1 || height < 1 || n_frames > 65535) return set_err(c, WASS_ERR_INVALID_ARG, "bad size");
    if (ksize != 0 && ksize != 3 && ksize != 5)
        return set_err(c, WASS_ERR_INVALID_ARG, "median filter size %d: 3 or 5 (cv::medianBlur, which the reference calls, takes no other size for float32)", ksize);
    if (d_in == d_out) return set_err(c, WASS_ERR_INVALID_ARG, "the median filter does not run in place");
    WASS_HIP(c, hipSetDevice(c->device));
    hipStream_t s = c->ts();
    const size_t hw = (size_t)width * height;
    const dim3 grid((width + MED_TX - 1) / MED_TX, (height + MED_TY - 1) / MED_TY, n_frames), blk(MED_TX, MED_TY);
    if (grid.y > 65535) return set_err(c, WASS_ERR_UNSUPPORTED, "grid too large");
    if (ksize == 0) hipLaunchKernelGGL(k_seq_copy_masked, dim3((unsigned)((hw + 255) / 256), n_frames), dim3(256), 0, s, d_in, d_out, hw, d_mask);
    else if (ksize == 3) hipLaunchKernelGGL(k_grid_median<3>, grid, blk, 0, s, d_in, d_out, width, height, d_mask);
    else hipLaunchKernelGGL(k_grid_median<5>, grid, blk, 0, s, d_in, d_out, width, height, d_mask);
    WASS_HIP(c, hipGetLastError());
    return WASS_OK;
}

extern "C" void wass_grid_seq_destroy(wass_grid_seq* q)
{
    if (!q) return;
    if (q->c) (void)hipSetDevice(q->c->device);
    if (q->acc) (void)hipFree(q->acc);
    delete q;                                                // frees q->part: every call that used it has synchronised before it returned
}

extern "C" int wass_grid_seq_create(wass_ctx* c, int width, int height, wass_grid_seq** out)
{
    if (!c || !out) return set_err(c, WASS_ERR_INVALID_ARG, "null argument");
    if (width < 1 || height < 1 || (size_t)width * height > ((size_t)1 << 28)) return set_err(c, WASS_ERR_INVALID_ARG, "bad grid size %d x %d", width, height);
    WASS_HIP(c, hipSetDevice(c->device));
    wass_grid_seq* q = new wass_grid_seq;
    q->c = c; q->W = width; q->H = height;
    const size_t hw = (size_t)width * height;
    hipError_t e = hipMalloc((void**)&q->acc, 2 * hw * 8);
    if (e == hipSuccess) e = hipMemsetAsync(q->acc, 0, 2 * hw * 8, c->ts());
    if (e != hipSuccess) {
        wass_grid_seq_destroy(q);
        return set_err(c, WASS_ERR_NO_MEMORY, "grid sequence accumulator: %s", hipGetErrorString(e));
    }
    q->mean = q->acc + hw;
    *out = q;
    return WASS_OK;
}

extern "C" int wass_grid_seq_push_dev(wass_grid_seq* q, const float* d_zi, int n_frames, float* d_z_mm_out)
{
    if (!q) return WASS_ERR_INVALID_ARG;
    wass_ctx* c = q->c;
    if (!d_zi || n_frames < 1 || n_frames > 65535) return set_err(c, WASS_ERR_INVALID_ARG, "bad argument");
    WASS_HIP(c, hipSetDevice(c->device));
    hipStream_t s = c->ts();
    const size_t hw = (size_t)q->W * q->H;
    size_t nb = (hw + 255) / 256;
    const int nblk = (int)(nb < 256 ? nb : 256);             // a function of the grid size only
    int rc;
    if ((rc = ensure(c, q->part, (size_t)n_frames * (nblk * sizeof(SeqPart) + 3 * 8)))) return rc;
    double* res = (double*)q->part.p;
    SeqPart* part = (SeqPart*)(res + 3 * (size_t)n_frames);
    hipLaunchKernelGGL(k_seq_acc, dim3((unsigned)nb), dim3(256), 0, s, d_zi, n_frames, hw, q->acc, d_z_mm_out);
    hipLaunchKernelGGL(k_seq_stats, dim3(nblk, n_frames), dim3(256), 0, s, d_zi, hw, part);
    hipLaunchKernelGGL(k_seq_stats_final, dim3(n_frames), dim3(256), 0, s, (const SeqPart*)part, nblk, res);
    WASS_HIP(c, hipGetLastError());
    std::vector<double> h(3 * (size_t)n_frames);
    WASS_HIP(c, hipMemcpyAsync(h.data(), res, h.size() * 8, hipMemcpyDeviceToHost, s));
    WASS_HIP(c, hipStreamSynchronize(s));
    for (int f = 0; f < n_frames; ++f) {
        q->fmean.push_back(h[3 * f]); q->fmin.push_back(h[3 * f + 1]); q->fmax.push_back(h[3 * f + 2]);
    }
    q->finished = false;
    return WASS_OK;
}

extern "C" int wass_grid_seq_finish(wass_grid_seq* q, int force_zero_mean, wass_grid_seq_stats* stats, double* mean_perpoint_mm,
                                    double* frame_mean, double* frame_min, double* frame_max)
{
    if (!q) return WASS_ERR_INVALID_ARG;
    wass_ctx* c = q->c;
    const size_t n = q->fmean.size(), hw = (size_t)q->W * q->H;
    if (!n) return set_err(c, WASS_ERR_INVALID_ARG, "no frame was pushed");
    WASS_HIP(c, hipSetDevice(c->device));
    hipStream_t s = c->ts();
    hipLaunchKernelGGL(k_seq_mean, dim3((unsigned)((hw + 255) / 256)), dim3(256), 0, s, (const double*)q->acc, hw, (double)n, q->mean);
    WASS_HIP(c, hipGetLastError());
    if (mean_perpoint_mm) WASS_HIP(c, hipMemcpyAsync(mean_perpoint_mm, q->mean, hw * 8, hipMemcpyDeviceToHost, s));
    WASS_HIP(c, hipStreamSynchronize(s));
    q->finished = true;
    // np.amin / np.amax / np.mean of the per-frame lists: one NaN frame makes each of them NaN
    double zmin = q->fmin[0], zmax = q->fmax[0], sum = 0.0;
    for (size_t f = 0; f < n; ++f) {
        if (!isnan(zmin) && (isnan(q->fmin[f]) || q->fmin[f] < zmin)) zmin = q->fmin[f];
        if (!isnan(zmax) && (isnan(q->fmax[f]) || q->fmax[f] > zmax)) zmax = q->fmax[f];
        sum += q->fmean[f];
        if (frame_mean) frame_mean[f] = q->fmean[f];
        if (frame_min) frame_min[f] = q->fmin[f];
        if (frame_max) frame_max[f] = q->fmax[f];
    }
    if (stats) {
        stats->zmin = zmin;
        stats->zmax = force_zero_mean ? -zmin : zmax;
        stats->zmean = force_zero_mean ? 0.0 : sum / (double)n;
        stats->n_frames = (int)n;
    }
    return WASS_OK;
}

extern "C" int wass_grid_seq_zero_mean_dev(wass_grid_seq* q, float* d_z_mm, int n_frames)
{
    if (!q) return WASS_ERR_INVALID_ARG;
    wass_ctx* c = q->c;
    if (!d_z_mm || n_frames < 1 || n_frames > 65535) return set_err(c, WASS_ERR_INVALID_ARG, "bad argument");
    if (!q->finished) return set_err(c, WASS_ERR_INVALID_ARG, "wass_grid_seq_finish has not computed the per-point mean of the frames pushed so far");
    WASS_HIP(c, hipSetDevice(c->device));
    const size_t hw = (size_t)q->W * q->H;
    hipLaunchKernelGGL(k_seq_zero_mean, dim3((unsigned)((hw + 255) / 256), n_frames), dim3(256), 0, c->ts(), d_z_mm, hw, (const double*)q->mean);
    WASS_HIP(c, hipGetLastError());
    return WASS_OK;
}
