// grid.hip -- SURVEY.md section 8 row f3: the first step of the gridding stage, straight from the device-resident
// mesh (no mesh_cam.xyzC round trip through the disk).
//
// Reference: gridding/wassgridsurface/wassgridsurface.py:316-365 (_grid_task, algorithm "IDW"):
//   mesh_aligned = (Rpl @ mesh + Tpl, z negated) * CAM_BASELINE          (:318, wass_utils.py:54-61)
//   pts_x = floor((x - xmin) / (xmax - xmin) * (W - 1) + 0.5), pts_y likewise  (:322-326)
//   ZZ = per-cell value of the points that fall into a cell                (:330-345)
//   Zi, mask = IDWInterpolator(KSIZE=5, exp=2.4, reps=1)(ZZ)               (IDWInterpolator.py:23-58)
// Divergence, stated because it cannot be avoided: the reference fills ZZ by ten random sub-samples with a random
// last-writer-wins scatter and takes their nanmedian (:330-345) -- a randomised estimate of the cell's central value with
// no defined result to be identical to.  Two deterministic statistics are offered (wass_mesh_grid_idw_ex):
//   mean    the MEAN of all points that fall into a cell, accumulated in 2^-24 fixed point so that the result does not depend
//           on the order of the atomics (the form of rounds 2-3, and what wass_mesh_grid_idw still computes);
//   median  the exact MEDIAN of the cell's points (round 4): what the reference's estimator converges to, and like it not
//           moved by a few outliers in a cell.  Points are bucketed by cell (count, scan, fill) and every cell sorts its own
//           segment; the result does not depend on the point order either.  Everything after that (the 5x5 inverse-
// distance convolution, the 5x5 morphological closing of the mask) follows IDWInterpolator literally, in fp64.
#include "common.h"
#include "grid_align.h"

namespace wass {

constexpr unsigned int GRID_OUTSIDE = 0xFFFFFFFFu;

// Alignment and binning of one point, the one place where both cell statistics get their cell from: returns the cell
// (GRID_OUTSIDE: not in the grid, which a NaN or infinite coordinate is too) and the aligned height in az.  The bin follows the
// reference's sequence of roundings (:324-325): subtract, divide by the extent, multiply by W - 1, add 0.5, floor.  A
// precomputed scale (W - 1) / (xmax - xmin) rounds differently and moves a point within an ulp or two of a cell boundary into
// the neighbouring cell (tests/test_grid_bin.py counts them).
__device__ __forceinline__ unsigned int grid_align_bin(const GridDev& g, double x, double y, double z, double& az)
{
    double ax, ay;
    grid_align(g, x, y, z, ax, ay, az);
    const double fx = floor((ax - g.xmin) / g.xext * g.wm1 + 0.5), fy = floor((ay - g.ymin) / g.yext * g.hm1 + 0.5);
    if (!(fx >= 0 && fx < g.gw && fy >= 0 && fy < g.gh)) return GRID_OUTSIDE;
    return (unsigned int)((size_t)fy * g.gw + (size_t)fx);
}

__global__ void __launch_bounds__(256) k_grid_scatter(const uint8_t* __restrict__ valid, const double* __restrict__ X,
                                                      const double* __restrict__ Y, const double* __restrict__ Z, size_t n, GridDev g,
                                                      long long* __restrict__ sum, unsigned int* __restrict__ cnt)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n || !valid[i]) return;
    double az;
    const unsigned int cell = grid_align_bin(g, X[i], Y[i], Z[i], az);
    if (cell == GRID_OUTSIDE) return;
    atomicAdd((unsigned long long*)&sum[cell], (unsigned long long)(long long)llrint(az * 16777216.0));
    atomicAdd(&cnt[cell], 1u);
}

// ---- median mode: points bucketed by cell
// pass 1: the cell of every point (GRID_OUTSIDE: not in the grid) and its height, counts per cell
__global__ void __launch_bounds__(256) k_grid_bucket_count(const uint8_t* __restrict__ valid, const double* __restrict__ X,
                                                           const double* __restrict__ Y, const double* __restrict__ Z, size_t n, GridDev g,
                                                           unsigned int* __restrict__ pcell, double* __restrict__ pz, unsigned int* __restrict__ cnt)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    unsigned int cell = GRID_OUTSIDE;
    double az = 0.0;
    if (valid[i]) {
        cell = grid_align_bin(g, X[i], Y[i], Z[i], az);
        if (cell != GRID_OUTSIDE) atomicAdd(&cnt[cell], 1u);
    }
    pcell[i] = cell;
    pz[i] = az;
}
// exclusive scan of the cell counts, one workgroup (the grid has at most a few million cells: a few MB)
__global__ void __launch_bounds__(1024) k_grid_scan(const unsigned int* __restrict__ cnt, size_t ng, unsigned int* __restrict__ off)
{
    __shared__ unsigned int part[1024];
    const size_t per = (ng + 1023) / 1024, a = (size_t)threadIdx.x * per, b = a + per < ng ? a + per : ng;
    unsigned int s = 0;
    for (size_t i = a; i < b; ++i) s += cnt[i];
    part[threadIdx.x] = s;
    __syncthreads();
    lds_scan<1024>(part);
    unsigned int run = part[threadIdx.x] - s;                // exclusive prefix of this thread's chunk
    for (size_t i = a; i < b; ++i) { off[i] = run; run += cnt[i]; }
}
void grid_scan_enqueue(const unsigned int* cnt, size_t ng, unsigned int* off, hipStream_t s)
{
    hipLaunchKernelGGL(k_grid_scan, dim3(1), dim3(1024), 0, s, cnt, ng, off);
}
// pass 2: every point into its cell's segment (the order inside a segment depends on the atomics; the median does not)
__global__ void __launch_bounds__(256) k_grid_bucket_fill(const unsigned int* __restrict__ pcell, const double* __restrict__ pz, size_t n,
                                                          const unsigned int* __restrict__ off, unsigned int* __restrict__ fill,
                                                          double* __restrict__ vals)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const unsigned int c = pcell[i];
    if (c == GRID_OUTSIDE) return;
    vals[off[c] + atomicAdd(&fill[c], 1u)] = pz[i];
}
// every cell sorts its own segment in place (shell sort: cells hold a handful of points, a few hundred next to the cameras)
// and takes numpy's median: the middle value, or the mean of the two middle values
__global__ void __launch_bounds__(256) k_grid_cell_median(const unsigned int* __restrict__ cnt, const unsigned int* __restrict__ off, size_t ng,
                                                          double* __restrict__ vals, double* __restrict__ cellval)
{
    const size_t c = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= ng) return;
    const unsigned int n = cnt[c];
    if (!n) { cellval[c] = 0.0; return; }
    double* v = vals + off[c];
    for (unsigned int gap = n / 2; gap > 0; gap /= 2)
        for (unsigned int i = gap; i < n; ++i) {
            const double t = v[i];
            unsigned int j = i;
            for (; j >= gap && v[j - gap] > t; j -= gap) v[j] = v[j - gap];
            v[j] = t;
        }
    cellval[c] = (n & 1) ? v[n / 2] : 0.5 * (v[n / 2 - 1] + v[n / 2]);
}
__global__ void __launch_bounds__(256) k_grid_cell_mean(const long long* __restrict__ sum, const unsigned int* __restrict__ cnt, size_t ng,
                                                        double* __restrict__ cellval)
{
    const size_t c = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= ng) return;
    cellval[c] = cnt[c] ? (double)sum[c] / 16777216.0 / (double)cnt[c] : 0.0;
}

// IDWInterpolator.__call__ with reps = 1: I2 = conv(I, K) / (conv(mask, K) + 1e-9); Z = point cells keep their value, empty
// cells take I2; final mask = closing of the point mask with a 5x5 block (dilate, then erode; borders ignored)
__global__ void __launch_bounds__(256) k_grid_idw(const double* __restrict__ cellval, const unsigned int* __restrict__ cnt, int gw, int gh,
                                                  double* __restrict__ zi, uint8_t* __restrict__ dil)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= gw) return;
    const size_t i = (size_t)y * gw + x;
    double num = 0.0, den = 0.0;
    bool any = false;
    for (int dy = -2; dy <= 2; ++dy)
        for (int dx = -2; dx <= 2; ++dx) {
            const int xx = x + dx, yy = y + dy;
            if (xx < 0 || yy < 0 || xx >= gw || yy >= gh) continue;
            const size_t q = (size_t)yy * gw + xx;
            if (!cnt[q]) continue;
            any = true;
            if (!dx && !dy) continue;
            const double k = 1.0 / pow(sqrt((double)(dx * dx + dy * dy)), 2.4);
            num += cellval[q] * k;
            den += k;
        }
    zi[i] = cnt[i] ? cellval[i] : num / (den + 1e-9);
    dil[i] = any;
}
__global__ void __launch_bounds__(256) k_grid_close(const double* __restrict__ zi, const uint8_t* __restrict__ dil, int gw, int gh,
                                                    float* __restrict__ out, uint8_t* __restrict__ mask)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= gw) return;
    bool all = true;
    for (int dy = -2; dy <= 2; ++dy)
        for (int dx = -2; dx <= 2; ++dx) {
            const int xx = x + dx, yy = y + dy;
            if (xx < 0 || yy < 0 || xx >= gw || yy >= gh) continue;      // erosion ignores what lies outside the image
            all = all && dil[(size_t)yy * gw + xx];
        }
    const size_t i = (size_t)y * gw + x;
    out[i] = all ? (float)zi[i] : __builtin_nanf("");
    if (mask) mask[i] = all;
}

}  // namespace wass

using namespace wass;

namespace wass {

// the binned cell map as float32, NaN where no point fell (the ZZ the reference hands to its interpolator, :345)
__global__ void __launch_bounds__(256) k_grid_cells_f32(const double* __restrict__ cellval, const unsigned int* __restrict__ cnt, size_t ng,
                                                        float* __restrict__ cells)
{
    const size_t c = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= ng) return;
    cells[c] = cnt[c] ? (float)cellval[c] : __builtin_nanf("");
}

// Alignment and binning shared by the interpolators: fills c->grid and returns the per-cell values (fp64) and counts.
// With d_cells != NULL also writes the height x width float32 cell map there (NaN = empty cell).  Enqueued on c->ts().
static int grid_bin(wass_ctx* c, const wass_mesh* m, const wass_grid_setup* gs, int cell_statistic, GridDev& g, double** cellval_out,
                    unsigned int** cnt_out, float** out_p, uint8_t** dil_p, uint8_t** mask_p, double** zi_p, float* d_cells)
{
    if (!c || !m || !gs) return set_err(c, WASS_ERR_INVALID_ARG, "null argument");
    if (gs->width < 2 || gs->height < 2 || !(gs->xmax > gs->xmin) || !(gs->ymax > gs->ymin)) return set_err(c, WASS_ERR_INVALID_ARG, "bad grid");
    if (cell_statistic != WASS_GRID_CELL_MEAN && cell_statistic != WASS_GRID_CELL_MEDIAN) return set_err(c, WASS_ERR_INVALID_ARG, "unknown cell statistic");
    WASS_HIP(c, hipSetDevice(c->device));
    const size_t n = m->n(), ng = (size_t)gs->width * gs->height;
    if (ng > 0x7FFFFFF0ull) return set_err(c, WASS_ERR_UNSUPPORTED, "grid too large");
    const bool median = cell_statistic == WASS_GRID_CELL_MEDIAN;
    int rc;
    // Per cell, and per point in median mode only.  Every kernel stops at its array's last cell or point (the 5 x 5 windows skip
    // what lies outside the grid, and the cells' segments of vals add up to at most n), so no piece needs room behind it.
    long long* sum;
    double *zi, *cellval, *pz = nullptr, *vals = nullptr;
    float* out;
    unsigned int *cnt, *off, *fill, *pcell = nullptr;
    uint8_t *dil, *mask;
    if ((rc = carve_buf(c, c->grid, [&](Carve& a) {
            sum = a.take<long long>(ng * 8); zi = a.take<double>(ng * 8); cellval = a.take<double>(ng * 8);
            out = a.take<float>(ng * 4);
            cnt = a.take<unsigned int>(ng * 4); off = a.take<unsigned int>(ng * 4); fill = a.take<unsigned int>(ng * 4);
            dil = a.take<uint8_t>(ng); mask = a.take<uint8_t>(ng);
            if (median) { pz = a.take<double>(n * 8); vals = a.take<double>(n * 8); pcell = a.take<unsigned int>(n * 4); }
        })))
        return rc;
    memcpy(g.R, gs->R, sizeof g.R); memcpy(g.T, gs->T, sizeof g.T);
    g.baseline = gs->baseline; g.xmin = gs->xmin; g.ymin = gs->ymin;
    g.xext = gs->xmax - gs->xmin; g.yext = gs->ymax - gs->ymin; g.wm1 = gs->width - 1; g.hm1 = gs->height - 1;
    g.gw = gs->width; g.gh = gs->height;
    hipStream_t s = c->ts();
    const dim3 blk(256), gp((unsigned)((n + 255) / 256)), gc((unsigned)((ng + 255) / 256));
    WASS_HIP(c, hipMemsetAsync(cnt, 0, ng * 4, s));
    if (median) {
        WASS_HIP(c, hipMemsetAsync(fill, 0, ng * 4, s));
        hipLaunchKernelGGL(k_grid_bucket_count, gp, blk, 0, s, m->valid, m->x, m->y, m->z, n, g, pcell, pz, cnt);
        hipLaunchKernelGGL(k_grid_scan, dim3(1), dim3(1024), 0, s, (const unsigned int*)cnt, ng, off);
        hipLaunchKernelGGL(k_grid_bucket_fill, gp, blk, 0, s, (const unsigned int*)pcell, (const double*)pz, n, (const unsigned int*)off, fill, vals);
        hipLaunchKernelGGL(k_grid_cell_median, gc, blk, 0, s, (const unsigned int*)cnt, (const unsigned int*)off, ng, vals, cellval);
    } else {
        WASS_HIP(c, hipMemsetAsync(sum, 0, ng * 8, s));
        hipLaunchKernelGGL(k_grid_scatter, gp, blk, 0, s, m->valid, m->x, m->y, m->z, n, g, sum, cnt);
        hipLaunchKernelGGL(k_grid_cell_mean, gc, blk, 0, s, (const long long*)sum, (const unsigned int*)cnt, ng, cellval);
    }
    if (d_cells) hipLaunchKernelGGL(k_grid_cells_f32, gc, blk, 0, s, (const double*)cellval, (const unsigned int*)cnt, ng, d_cells);
    WASS_HIP(c, hipGetLastError());
    if (cellval_out) *cellval_out = cellval;
    if (cnt_out) *cnt_out = cnt;
    if (out_p) *out_p = out;
    if (dil_p) *dil_p = dil;
    if (mask_p) *mask_p = mask;
    if (zi_p) *zi_p = zi;
    return WASS_OK;
}

int grid_cells_dev(wass_ctx* c, const wass_mesh* m, const wass_grid_setup* gs, int cell_statistic, float* d_cells)
{
    GridDev g;
    return grid_bin(c, m, gs, cell_statistic, g, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, d_cells);
}

}  // namespace wass

extern "C" int wass_mesh_grid_cells_dev(wass_ctx* c, const wass_mesh* m, const wass_grid_setup* gs, int cell_statistic, float* d_cells)
{
    if (!d_cells) return set_err(c, WASS_ERR_INVALID_ARG, "null argument");
    return grid_cells_dev(c, m, gs, cell_statistic, d_cells);
}

extern "C" int wass_mesh_grid_idw_ex(wass_ctx* c, const wass_mesh* m, const wass_grid_setup* gs, int cell_statistic, float* grid_out,
                                     uint8_t* mask_out)
{
    if (!c || !m || !gs || !grid_out) return set_err(c, WASS_ERR_INVALID_ARG, "null argument");
    GridDev g;
    double *cellval, *zi;
    unsigned int* cnt;
    float* out;
    uint8_t *dil, *mask;
    int rc;
    if ((rc = grid_bin(c, m, gs, cell_statistic, g, &cellval, &cnt, &out, &dil, &mask, &zi, nullptr))) return rc;
    const size_t ng = (size_t)gs->width * gs->height;
    hipStream_t s = c->ts();
    const dim3 gg((gs->width + 255) / 256, gs->height), blk(256);
    hipLaunchKernelGGL(k_grid_idw, gg, blk, 0, s, (const double*)cellval, (const unsigned int*)cnt, g.gw, g.gh, zi, dil);
    hipLaunchKernelGGL(k_grid_close, gg, blk, 0, s, (const double*)zi, (const uint8_t*)dil, g.gw, g.gh, out, mask);
    WASS_HIP(c, hipGetLastError());
    WASS_HIP(c, hipMemcpyAsync(grid_out, out, ng * 4, hipMemcpyDeviceToHost, s));
    if (mask_out) WASS_HIP(c, hipMemcpyAsync(mask_out, mask, ng, hipMemcpyDeviceToHost, s));
    WASS_HIP(c, hipStreamSynchronize(s));
    return WASS_OK;
}

extern "C" int wass_mesh_grid_idw(wass_ctx* c, const wass_mesh* m, const wass_grid_setup* gs, float* grid_out, uint8_t* mask_out)
{
    return wass_mesh_grid_idw_ex(c, m, gs, WASS_GRID_CELL_MEAN, grid_out, mask_out);
}
