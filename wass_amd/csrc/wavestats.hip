// wavestats.hip -- wave-by-wave statistics of the gridded cube: for every cell of a count x H x W float32 cube the zero-crossing
// waves of its series, H1/3 and its period, Hmax, the mean zero-crossing period and the surface moments ("Wave-by-wave
// statistics", holds the definitions; they are the specification: the reference has no such tool).
//
// One lane per series, consecutive lanes along x, so every time step of a wave is one coalesced row segment.  All arithmetic is
// fp64 from the float32 samples, every product, quotient and sum a rounding of its own (the library is built with
// -ffp-contract=off), in the order the definitions give: the same input gives the same bits, and a numpy restatement gives them too.
//   k_ws_scan    with demean: the fp64 sum of the series first frame to last, / count; then one scan: the moments, the extremes,
//                the up-crossings (of -eta for crossing = down) and the waves between them, H_k and T_k as fp64 to the scratch,
//                laid out [wave][series of the slab]; the sums over all waves, Hmax and its period, Tz; n_cross
//   k_ws_select  the (Nw + 2) / 3 highest waves: a radix descent over the bits of H_k (H_k > 0, so the bits order like the values),
//                4 bits a pass with the 16 counters of every lane in LDS, finds the height at the cut; then the waves in time order:
//                those above the cut, and the first of those at the cut, are summed; the pooled histogram takes every wave, counted per
//                block in LDS first where it has at most WS_HIST_LDS bins
// A wave keeps WS_U rows in flight ahead of the one it is scanning (the chain is sequential in t; the loads are not).
// Two neighbouring samples cannot both be up-crossings, so a series has at most count / 2 of them and fewer waves: the scratch is
// 2 * (count / 2) doubles per series.  Rows go in slabs so that it, and the staging of a host cube and of its results, stay under
// WS_SCRATCH_CAP; a series never crosses a slab, so the result does not depend on the slab height.  No atomics but the
// histogram's integer ones.
// Host side: ws_plan keeps the byte formula; the slab rule, the scratch, the staging of a host slab and the end of the call are
// cube.h's.
#include "common.h"
#include "cube.h"

#include <math.h>

namespace wass {

constexpr size_t WS_SCRATCH_CAP = (size_t)16 << 30;     // bytes one wass_wavestats call may allocate
constexpr int WS_U = 8;                                 // time steps loaded ahead of the scan
constexpr int WS_NF = WASS_WS_NFIELDS;
constexpr int WS_HIST_LDS = 512;                        // bins a block counts in LDS before it adds them to the histogram; more: straight to memory

// what the scan carries from sample to sample
struct WsScan {
    double sum = 0.0, s2 = 0.0, s3 = 0.0, s4 = 0.0;     // of z; of eta^2, eta^3, eta^4
    double emax = -INFINITY, emin = INFINITY;
    double prev = 0.0;                                  // the sample before, in the sign the crossings are looked for
    double crest = -INFINITY, trough = INFINITY;        // since the last crossing, in that sign
    double tau0 = 0.0, taup = 0.0;                      // the first and the latest crossing
    double sh = 0.0, sh2 = 0.0, hmax = 0.0, thmax = 0.0;
    unsigned ncross = 0;
    bool finite = true;
};

// sample j of a series: zf as loaded.  hs, ts: the series' H_k and T_k, `pitch` doubles apart.
template <bool DOWN>
__device__ __forceinline__ void ws_step(WsScan& a, int j, float zf, double mean, double datascale, double dt, double* __restrict__ hs,
                                        double* __restrict__ ts, size_t pitch)
{
    a.finite = a.finite && fabsf(zf) <= 3.402823466e+38f;
    const double z = (double)zf;
    a.sum += z;
    const double e = (z - mean) * datascale;
    const double e2 = e * e;
    a.s2 += e2;
    a.s3 += e2 * e;
    a.s4 += e2 * e2;
    a.emax = e > a.emax ? e : a.emax;
    a.emin = e < a.emin ? e : a.emin;
    const double c = DOWN ? -e : e;
    if (j > 0 && a.prev < 0.0 && c >= 0.0) {            // an up-crossing at j - 1
        const double tau = (double)(j - 1) + a.prev / (a.prev - c);
        if (a.ncross) {                                 // closes wave ncross - 1: the samples after the crossing before, up to j - 1
            const size_t k = (size_t)(a.ncross - 1) * pitch;
            const double h = a.crest - a.trough, t = (tau - a.taup) * dt;
            hs[k] = h;
            ts[k] = t;
            a.sh += h;
            a.sh2 += h * h;
            if (a.ncross == 1 || h > a.hmax) { a.hmax = h; a.thmax = t; }
        } else {
            a.tau0 = tau;
        }
        a.taup = tau;
        ++a.ncross;
        a.crest = -INFINITY;
        a.trough = INFINITY;
    }
    a.crest = c > a.crest ? c : a.crest;
    a.trough = c < a.trough ? c : a.trough;
    a.prev = c;
}

// series i of the slab: row i / W, column i % W of x (element strides st, sy).  fields[f * fpitch + row * W + col] and
// ncr[row * W + col] are the slab's part of the results; wh[k * nser + i], wt[k * nser + i] the waves, k < count / 2.
template <bool DEMEAN, bool DOWN>
__global__ void __launch_bounds__(256) k_ws_scan(const float* __restrict__ x, long long st, long long sy, int W, unsigned nser, int count,
                                                 double datascale, double dt, double* __restrict__ fields, size_t fpitch,
                                                 int* __restrict__ ncr, double* __restrict__ wh, double* __restrict__ wt)
{
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= nser) return;
    const float* __restrict__ p = x + (long long)(i / (unsigned)W) * sy + (i % (unsigned)W);
    double mean = 0.0;
    if (DEMEAN) {
        double sum = 0.0;
        int t = 0;
        for (; t + WS_U <= count; t += WS_U) {
            float v[WS_U];
#pragma unroll
            for (int u = 0; u < WS_U; ++u) v[u] = p[(long long)(t + u) * st];
#pragma unroll
            for (int u = 0; u < WS_U; ++u) sum += (double)v[u];
        }
        for (; t < count; ++t) sum += (double)p[(long long)t * st];
        mean = sum / (double)count;
    }
    WsScan a;
    double* __restrict__ hs = wh + i;
    double* __restrict__ ts = wt + i;
    // blocks of WS_U samples, the next block's loads issued before the current block's chain
    float cur[WS_U], nxt[WS_U];
    int j = 0;
    if (count >= WS_U) {
#pragma unroll
        for (int u = 0; u < WS_U; ++u) cur[u] = p[(long long)u * st];
    }
    for (; j + WS_U <= count; j += WS_U) {
        const bool more = j + 2 * WS_U <= count;
        if (more) {
#pragma unroll
            for (int u = 0; u < WS_U; ++u) nxt[u] = p[(long long)(j + WS_U + u) * st];
        }
#pragma unroll
        for (int u = 0; u < WS_U; ++u) ws_step<DOWN>(a, j + u, cur[u], mean, datascale, dt, hs, ts, (size_t)nser);
        if (more) {
#pragma unroll
            for (int u = 0; u < WS_U; ++u) cur[u] = nxt[u];
        }
    }
    for (; j < count; ++j) ws_step<DOWN>(a, j, p[(long long)j * st], mean, datascale, dt, hs, ts, (size_t)nser);

    double* __restrict__ f = fields + i;
    if (!a.finite) {
#pragma unroll
        for (int q = 0; q < WS_NF; ++q) f[(size_t)q * fpitch] = NAN;
        ncr[i] = -1;
        return;
    }
    const double n = (double)count;
    if (!DEMEAN) mean = a.sum / n;
    f[(size_t)WASS_WS_MEAN * fpitch] = mean * datascale;
    f[(size_t)WASS_WS_M2 * fpitch] = a.s2 / n;
    f[(size_t)WASS_WS_M3 * fpitch] = a.s3 / n;
    f[(size_t)WASS_WS_M4 * fpitch] = a.s4 / n;
    f[(size_t)WASS_WS_ETA_MAX * fpitch] = a.emax;
    f[(size_t)WASS_WS_ETA_MIN * fpitch] = a.emin;
    ncr[i] = (int)a.ncross;
    const bool any = a.ncross > 1;
    const double nw = (double)(any ? a.ncross - 1 : 1u);
    f[(size_t)WASS_WS_H_MEAN * fpitch] = any ? a.sh / nw : NAN;
    f[(size_t)WASS_WS_H_SQMEAN * fpitch] = any ? a.sh2 / nw : NAN;
    f[(size_t)WASS_WS_H_MAX * fpitch] = any ? a.hmax : NAN;
    f[(size_t)WASS_WS_T_HMAX * fpitch] = any ? a.thmax : NAN;
    f[(size_t)WASS_WS_T_Z * fpitch] = any ? ((a.taup - a.tau0) * dt) / nw : NAN;
    if (!any) {                                         // k_ws_select leaves a series without waves alone
        f[(size_t)WASS_WS_H_13 * fpitch] = NAN;
        f[(size_t)WASS_WS_T_13 * fpitch] = NAN;
    }
}

// H_k > 0 in a series of finite samples (a wave's span begins at or above zero and ends below), so its bits, taken as an
// unsigned integer, order like its value
__device__ __forceinline__ unsigned long long ws_bits(double h) { return (unsigned long long)__double_as_longlong(h); }

__global__ void __launch_bounds__(256) k_ws_select(unsigned nser, const int* __restrict__ ncr, const double* __restrict__ wh,
                                                   const double* __restrict__ wt, double* __restrict__ fields, size_t fpitch,
                                                   unsigned long long* __restrict__ hist, int hist_bins, double hist_width)
{
    __shared__ unsigned cnt[16][256];                   // cnt[digit][lane of the block]: no two lanes of a wave share a bank
    __shared__ unsigned long long pool[WS_HIST_LDS];    // the block's part of a histogram of up to WS_HIST_LDS bins
    const unsigned tid = threadIdx.x, i = blockIdx.x * 256u + tid;
    const bool pooled = hist_bins > 0 && hist_bins <= WS_HIST_LDS;
    if (pooled) {
        for (int b = (int)tid; b < hist_bins; b += 256) pool[b] = 0;
        __syncthreads();
    }
    unsigned nw = 0;                                    // a lane past the slab, an invalid series or one without waves: nothing to do
    if (i < nser) {
        const int nc = ncr[i];
        if (nc >= 2) nw = (unsigned)nc - 1u;
    }
    if (nw) {
        const unsigned n13 = (nw + 2u) / 3u;
        const double* __restrict__ hs = wh + i;
        const double* __restrict__ ts = wt + i;
        // the n13-th highest key: its bits from the top, 4 at a time.  `want` of the keys that share the bits found so far lie at
        // or above it.
        unsigned long long cut = 0;
        unsigned want = n13;
        for (int shift = 60; shift >= 0; shift -= 4) {
#pragma unroll
            for (int d = 0; d < 16; ++d) cnt[d][tid] = 0;
            for (unsigned k = 0; k < nw; ++k) {
                const unsigned long long key = ws_bits(hs[(size_t)k * nser]);
                if (shift == 60 || (key >> (shift + 4)) == (cut >> (shift + 4))) ++cnt[(unsigned)(key >> shift) & 15u][tid];
            }
            int d = 15;
            for (; d > 0; --d) {                        // at least `want` keys are counted, so this ends by digit 0 at the latest
                const unsigned c = cnt[d][tid];
                if (c >= want) break;
                want -= c;
            }
            cut |= (unsigned long long)d << shift;
        }
        // `want` is now the number of waves exactly at the cut that belong to the third: the earliest ones
        double sh = 0.0, st = 0.0;
        for (unsigned k = 0; k < nw; ++k) {
            const double h = hs[(size_t)k * nser];
            const unsigned long long key = ws_bits(h);
            bool take = key > cut;
            if (key == cut && want) { take = true; --want; }
            if (take) {
                sh += h;
                st += ts[(size_t)k * nser];
            }
            if (hist_bins > 0) {
                const double q = floor(h / hist_width);
                int b = q < (double)(hist_bins - 1) ? (int)q : hist_bins - 1;
                b = b < 0 ? 0 : b;
                if (pooled) atomicAdd(pool + b, 1ull);
                else atomicAdd(hist + b, 1ull);
            }
        }
        fields[(size_t)WASS_WS_H_13 * fpitch + i] = sh / (double)n13;
        fields[(size_t)WASS_WS_T_13 * fpitch + i] = st / (double)n13;
    }
    if (pooled) {
        __syncthreads();
        for (int b = (int)tid; b < hist_bins; b += 256) {
            const unsigned long long v = pool[b];
            if (v) atomicAdd(hist + b, v);
        }
    }
}

struct WsPlan {
    int rows = 0;                  // rows per slab
    size_t wave_bytes = 0, stage_bytes = 0, field_bytes = 0, ncr_bytes = 0, hist_bytes = 0, total = 0;
};

// 0, or why the problem cannot be planned.  The device form needs the waves alone: its results go where the caller says.
static int ws_plan(int count, int H, int W, int slab, bool host, int hist_bins, WsPlan& p)
{
    if (count < 1 || H < 1 || W < 1 || slab < 0 || hist_bins < 0) return WASS_ERR_INVALID_ARG;
    const size_t nslot = (size_t)count / 2;
    const size_t per_row = (2 * nslot * 8 + (host ? (size_t)count * 4 + WS_NF * 8 + 4 : 0)) * (size_t)W;
    const size_t fixed = 2048 + (host ? align256((size_t)hist_bins * 8) : 0);   // 2048: what aligning the parts may add
    if (fixed >= WS_SCRATCH_CAP) return WASS_ERR_NO_MEMORY;
    const int rc = slab_rows(WS_SCRATCH_CAP - fixed, per_row, H, W, slab, &p.rows);
    if (rc) return rc;
    const size_t nser = (size_t)p.rows * (size_t)W;
    p.wave_bytes = align256(2 * nslot * nser * 8);
    p.stage_bytes = host ? align256((size_t)count * nser * 4) : 0;
    p.field_bytes = host ? align256((size_t)WS_NF * nser * 8) : 0;
    p.ncr_bytes = host ? align256(nser * 4) : 0;
    p.hist_bytes = host ? align256((size_t)hist_bins * 8) : 0;
    p.total = p.wave_bytes + p.stage_bytes + p.field_bytes + p.ncr_bytes + p.hist_bytes;
    if (p.total == 0) p.total = 256;                     // count = 1 on the device: no waves, nothing staged
    return WASS_OK;
}

static int ws_args(double dt, double datascale, int crossing, int hist_bins, double hist_width)
{
    if (!(dt > 0.0) || !isfinite(dt) || !isfinite(datascale)) return WASS_ERR_INVALID_ARG;
    if (crossing != WASS_WS_UP && crossing != WASS_WS_DOWN) return WASS_ERR_INVALID_ARG;
    if (hist_bins < 0 || (hist_bins > 0 && !(hist_width > 0.0))) return WASS_ERR_INVALID_ARG;
    return WASS_OK;
}

static void ws_launch(hipStream_t s, const float* x, long long st, long long sy, int W, unsigned nser, int count, double datascale, double dt,
                      bool down, bool demean, double* fields, size_t fpitch, int* ncr, double* wh, double* wt, unsigned long long* hist,
                      int hist_bins, double hist_width)
{
    const dim3 grid((nser + 255u) / 256u), block(256);
    if (demean && down) hipLaunchKernelGGL((k_ws_scan<true, true>), grid, block, 0, s, x, st, sy, W, nser, count, datascale, dt, fields, fpitch, ncr, wh, wt);
    else if (demean) hipLaunchKernelGGL((k_ws_scan<true, false>), grid, block, 0, s, x, st, sy, W, nser, count, datascale, dt, fields, fpitch, ncr, wh, wt);
    else if (down) hipLaunchKernelGGL((k_ws_scan<false, true>), grid, block, 0, s, x, st, sy, W, nser, count, datascale, dt, fields, fpitch, ncr, wh, wt);
    else hipLaunchKernelGGL((k_ws_scan<false, false>), grid, block, 0, s, x, st, sy, W, nser, count, datascale, dt, fields, fpitch, ncr, wh, wt);
    if (count >= 4)                                     // two crossings, i.e. one wave, need four samples
        hipLaunchKernelGGL(k_ws_select, grid, block, 0, s, nser, (const int*)ncr, (const double*)wh, (const double*)wt, fields, fpitch, hist,
                           hist_bins, hist_width);
}

static int ws_run(wass_ctx* c, bool host, const float* in, size_t st, size_t sy, int count, int H, int W, double dt, double datascale, int crossing,
                  int demean, int hist_bins, double hist_width, int slab_rows, double* fields, int* n_cross, unsigned long long* hist)
{
    if (!c) return WASS_ERR_INVALID_ARG;
    if (!in || !fields || !n_cross || (hist_bins > 0 && !hist)) return set_err(c, WASS_ERR_INVALID_ARG, "null argument");
    if (ws_args(dt, datascale, crossing, hist_bins, hist_width))
        return set_err(c, WASS_ERR_INVALID_ARG, "dt = %g (positive), datascale = %g (finite), crossing = %d (WASS_WS_UP or _DOWN), %d bins of %g", dt,
                       datascale, crossing, hist_bins, hist_width);
    if (count < 1 || H < 1 || W < 1 || slab_rows < 0) return set_err(c, WASS_ERR_INVALID_ARG, "a %d x %d x %d cube in slabs of %d rows", count, H, W, slab_rows);
    WsPlan p;
    int rc = ws_plan(count, H, W, slab_rows, host, hist_bins, p);
    if (rc) return set_err(c, rc, "cannot plan the wave statistics of a %d x %d x %d cube under the scratch cap of %zu bytes", count, H, W, WS_SCRATCH_CAP);
    if (sy < (size_t)W || (count > 1 && st < (size_t)W)) return set_err(c, WASS_ERR_INVALID_ARG, "bad strides");
    WASS_HIP(c, hipSetDevice(c->device));
    hipStream_t s = c->ts();
    Arena mem;
    if ((rc = mem.reserve(c, p.total, "the wave statistics"))) return rc;
    const size_t nslot = (size_t)count / 2, HW = (size_t)H * W;
    double* wh = mem.take<double>(p.wave_bytes);
    float* stage = mem.take<float>(p.stage_bytes);
    double* sfields = mem.take<double>(p.field_bytes);
    int* sncr = mem.take<int>(p.ncr_bytes);
    unsigned long long* dhist = host ? mem.take<unsigned long long>(p.hist_bytes) : hist;
    hipError_t e = hipSuccess;
    if (hist_bins > 0) e = hipMemsetAsync(dhist, 0, (size_t)hist_bins * 8, s);
    for (int r0 = 0; r0 < H && e == hipSuccess; r0 += p.rows) {
        const int rows = H - r0 < p.rows ? H - r0 : p.rows;
        const size_t plane = (size_t)rows * W;
        const unsigned nser = (unsigned)plane;
        double* wt = wh + nslot * plane;
        if (host) {
            e = upload_rows(stage, in, 4, count, r0, rows, W, st, sy, s);
            if (e != hipSuccess) break;
            ws_launch(s, stage, (long long)plane, W, W, nser, count, datascale, dt, crossing == WASS_WS_DOWN, demean != 0, sfields, plane, sncr, wh, wt,
                      dhist, hist_bins, hist_width);
            e = hipGetLastError();
            for (int q = 0; q < WS_NF && e == hipSuccess; ++q)
                e = hipMemcpyAsync(fields + q * HW + (size_t)r0 * W, sfields + q * plane, plane * 8, hipMemcpyDeviceToHost, s);
            if (e == hipSuccess) e = hipMemcpyAsync(n_cross + (size_t)r0 * W, sncr, plane * 4, hipMemcpyDeviceToHost, s);
        } else {
            ws_launch(s, in + (size_t)r0 * sy, (long long)st, (long long)sy, W, nser, count, datascale, dt, crossing == WASS_WS_DOWN, demean != 0,
                      fields + (size_t)r0 * W, HW, n_cross + (size_t)r0 * W, wh, wt, dhist, hist_bins, hist_width);
            e = hipGetLastError();
        }
    }
    if (host && hist_bins > 0 && e == hipSuccess) e = hipMemcpyAsync(hist, dhist, (size_t)hist_bins * 8, hipMemcpyDeviceToHost, s);
    return finish(c, WASS_OK, e, s, "wave statistics");
}

}  // namespace wass

using namespace wass;

extern "C" int wass_wavestats_scratch_bytes(int count, int H, int W, double dt, double datascale, int crossing, int hist_bins, double hist_width,
                                            int slab_rows, int host, size_t* bytes, int* rows_per_slab)
{
    if (!bytes) return WASS_ERR_INVALID_ARG;
    int rc = ws_args(dt, datascale, crossing, hist_bins, hist_width);
    if (rc) return rc;
    WsPlan p;
    rc = ws_plan(count, H, W, slab_rows, host != 0, hist_bins, p);
    if (rc) return rc;
    *bytes = p.total;
    if (rows_per_slab) *rows_per_slab = p.rows;
    return WASS_OK;
}

extern "C" int wass_wavestats(wass_ctx* c, const float* in, size_t stride_t, size_t stride_y, int count, int H, int W, double dt, double datascale,
                              int crossing, int demean, int hist_bins, double hist_width, int slab_rows, double* fields, int32_t* n_cross,
                              uint64_t* hist)
{
    return ws_run(c, true, in, stride_t, stride_y, count, H, W, dt, datascale, crossing, demean, hist_bins, hist_width, slab_rows, fields, n_cross,
                  (unsigned long long*)hist);
}

extern "C" int wass_wavestats_dev(wass_ctx* c, const float* d_in, size_t stride_t, size_t stride_y, int count, int H, int W, double dt,
                                  double datascale, int crossing, int demean, int hist_bins, double hist_width, int slab_rows, double* d_fields,
                                  int32_t* d_n_cross, uint64_t* d_hist)
{
    return ws_run(c, false, d_in, stride_t, stride_y, count, H, W, dt, datascale, crossing, demean, hist_bins, hist_width, slab_rows, d_fields,
                  d_n_cross, (unsigned long long*)d_hist);
}
