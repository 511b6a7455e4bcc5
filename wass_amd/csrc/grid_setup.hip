// grid_setup.hip -- the device side of the gridder's `--action setup` (gridding/wassgridsurface/wassgridsurface.py:57-231).
//
// setup() aligns the first frame's whole cloud on the mean sea plane and takes np.quantile of the heights at 0.02 and 0.98
// (:122-123); with 3 to 5 million points that sort is the one step of setup() with real work in it.  Here the heights are never
// sorted: each double becomes an order-preserving 64-bit key and an MSD radix select in 11-bit digits (5 x 11 + 9 bits) finds
// the order statistics numpy interpolates between.  Every q of a call runs through the same launches (blockIdx.y = query), the
// decisions of a pass (which bin holds the rank, the new prefix) are taken by k_qs_pick into a record in device memory, and only
// that record comes back: per q the two neighbouring order statistics a[lo] and a[hi], plus the counts.
//   a[lo]   six histogram passes (the first, which has no prefix, once for all queries); k_qs_hist counts the digit of the keys that match the prefix so far into an LDS histogram per
//           workgroup and adds it to one of QS_COPIES global copies (same-address atomics serialise), k_qs_pick folds the copies.
//   a[hi]   = a[lo] when hi == lo or when the ties of a[lo] reach past lo (more than lo + 1 - #{keys below a[lo]} keys equal it);
//           otherwise the smallest key above a[lo]: k_qs_next, a block minimum and one 64-bit atomicMin per workgroup.
// Integer atomics only: the result does not depend on the order of the elements or of the workgroups.
// numpy's rule (numpy 2.2.6, lib/_function_base_impl.py: method "linear" has get_virtual_index = (n - 1) * quantiles; _get_indexes,
// _get_gamma, _lerp) is restated in qs_indexes and qs_lerp, fp64, no contraction.
#include "common.h"

#include <math.h>

#pragma clang fp contract(off)

namespace wass {

constexpr int QS_BITS = 11, QS_BINS = 1 << QS_BITS, QS_PASSES = 6, QS_COPIES = 4, QS_MAXQ = 8;
// one workgroup takes QS_TILE elements per sweep (QS_ITEMS independent loads per lane), one launch QS_MAX_BLOCKS tiles per sweep
constexpr int QS_THREADS = 256, QS_ITEMS = 8, QS_TILE = QS_THREADS * QS_ITEMS, QS_MAX_BLOCKS = 1024;
constexpr unsigned long long QS_NONE = ~0ull;

struct QsQuery {
    double q;
    unsigned long long k, prefix;          // remaining rank among the keys that match the prefix
    unsigned long long lo_key, hi_key;
    unsigned int eq;                       // keys equal to a[lo]
    int hi_shift;
    int want_hi;                           // numpy's next index differs from the previous one
    int state;                             // 0 running, 1 a[hi] needs k_qs_next, 2 done, -1 no values, -2 rank lost (internal error)
};
struct QsState {
    unsigned long long total, nan_count;   // values that are not NaN / that are
    QsQuery qy[QS_MAXQ];
};
constexpr size_t QS_HIST_OFF = (sizeof(QsState) + 255) & ~(size_t)255;
// one set of histogram copies per query, and one more (index QS_MAXQ) for pass 0: its digit counts are the same for every query
constexpr size_t QS_BYTES = QS_HIST_OFF + (size_t)(QS_MAXQ + 1) * QS_COPIES * QS_BINS * 4;

// the keys are reduce.h's order_key / order_unkey: -0.0 < +0.0, NaN is kept out by the callers, so QS_NONE is no value's key

// numpy's "linear" method for n >= 1 values: virtual index (n - 1) * q, _get_indexes (previous = floor, next = previous + 1, both
// -1 = the last element at or above n - 1, both 0 below 0) and _get_gamma (virtual - previous, with previous as numpy's index: -1
// stays -1).  lo / hi are the resolved positions in the sorted array.
__host__ __device__ inline void qs_indexes(unsigned long long n, double q, unsigned long long* lo, unsigned long long* hi, double* gamma)
{
    const double v = (double)(n - 1) * q;
    double prev = floor(v), next = prev + 1.0;
    if (v >= (double)(n - 1)) { prev = -1.0; next = -1.0; }
    if (v < 0.0) { prev = 0.0; next = 0.0; }
    *lo = prev < 0.0 ? n - 1 : (unsigned long long)prev;
    *hi = next < 0.0 ? n - 1 : (unsigned long long)next;
    *gamma = v - prev;
}
// numpy's _lerp: a + (b - a) * t, and b - (b - a) * (1 - t) where t >= 0.5
static inline double qs_lerp(double a, double b, double t)
{
    const double diff = b - a;
    double r = a + diff * t;
    if (t >= 0.5) r = b - diff * (1.0 - t);
    return r;
}

__host__ __device__ inline int qs_shift(int pass) { return pass < QS_PASSES - 1 ? 64 - QS_BITS * (pass + 1) : 0; }   // 53, 42, 31, 20, 9, 0
__host__ __device__ inline int qs_nbits(int pass) { return pass < QS_PASSES - 1 ? QS_BITS : 64 - QS_BITS * (QS_PASSES - 1); }

// the third row of align_on_sea_plane_RT times the baseline, for the valid points; 0 elsewhere (the passes skip those by the mask)
__global__ void __launch_bounds__(256) k_qs_align(const uint8_t* __restrict__ valid, const double* __restrict__ X, const double* __restrict__ Y,
                                                  const double* __restrict__ Z, size_t n, double r20, double r21, double r22, double t2,
                                                  double baseline, double* __restrict__ out)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double z = 0.0;
    if (valid[i]) z = -(((r20 * X[i] + r21 * Y[i]) + r22 * Z[i]) + t2) * baseline;
    out[i] = z;
}

// one digit of the keys that match query blockIdx.y's prefix.  Pass 0 has no prefix: it is launched once for all queries
// (gridDim.y = 1), into the shared set of copies, and also counts the NaNs.
__global__ void __launch_bounds__(QS_THREADS) k_qs_hist(const double* __restrict__ vals, const uint8_t* __restrict__ valid, size_t n, int pass,
                                                        QsState* __restrict__ st, unsigned int* __restrict__ hist)
{
    __shared__ unsigned int lh[QS_BINS];
    __shared__ unsigned int lnan;
    for (int i = threadIdx.x; i < QS_BINS; i += QS_THREADS) lh[i] = 0;
    if (threadIdx.x == 0) lnan = 0;
    __syncthreads();
    const int j = blockIdx.y, shift = qs_shift(pass);
    const unsigned int mask = (1u << qs_nbits(pass)) - 1u;
    const int hi_shift = st->qy[j].hi_shift;
    const unsigned long long prefix = st->qy[j].prefix;
    if (pass == 0 || st->qy[j].state == 0)
        for (size_t base = (size_t)blockIdx.x * QS_TILE; base < n; base += (size_t)gridDim.x * QS_TILE) {
            double v[QS_ITEMS];
            bool ok[QS_ITEMS];
#pragma unroll
            for (int k = 0; k < QS_ITEMS; ++k) {
                const size_t i = base + (size_t)k * QS_THREADS + threadIdx.x;
                ok[k] = i < n;
                v[k] = ok[k] ? vals[i] : 0.0;
                if (valid) ok[k] = ok[k] && valid[i] != 0;
            }
#pragma unroll
            for (int k = 0; k < QS_ITEMS; ++k) {
                if (!ok[k]) continue;
                if (v[k] != v[k]) { if (pass == 0) atomicAdd(&lnan, 1u); continue; }
                const unsigned long long key = order_key(v[k]);
                if (pass > 0 && (key >> hi_shift) != prefix) continue;
                atomicAdd(&lh[(unsigned int)(key >> shift) & mask], 1u);
            }
        }
    __syncthreads();
    unsigned int* mine = hist + ((size_t)(pass == 0 ? QS_MAXQ : j) * QS_COPIES + blockIdx.x % QS_COPIES) * QS_BINS;
    for (int i = threadIdx.x; i < QS_BINS; i += QS_THREADS)
        if (lh[i]) atomicAdd(&mine[i], lh[i]);
    if (threadIdx.x == 0 && lnan) atomicAdd(&st->nan_count, (unsigned long long)lnan);
}

// one workgroup per query: fold the copies (pass 0: the shared set, which is only read) into LDS, pick the bin that holds the rank,
// extend the prefix; pass 0 derives the rank from q, the last pass decides where a[hi] comes from.  Leaves the query's own
// histograms zeroed for the next pass.
__global__ void __launch_bounds__(256) k_qs_pick(unsigned int* __restrict__ hist, int pass, QsState* __restrict__ st)
{
    __shared__ unsigned long long tot[256];
    __shared__ unsigned int h[QS_BINS];
    const int j = blockIdx.x, nbits = qs_nbits(pass), nb = 1 << nbits, per = (nb + 255) / 256;
    unsigned int* own = hist + (size_t)j * QS_COPIES * QS_BINS;
    const unsigned int* src = pass == 0 ? hist + (size_t)QS_MAXQ * QS_COPIES * QS_BINS : own;
    for (int i = threadIdx.x; i < QS_BINS; i += 256) {
        unsigned int t = src[i];
        for (int cpy = 1; cpy < QS_COPIES; ++cpy) t += src[(size_t)cpy * QS_BINS + i];
        h[i] = t;
    }
    __syncthreads();
    unsigned long long s = 0;
    for (int b = threadIdx.x * per; b < min(nb, (threadIdx.x + 1) * per); ++b) s += h[b];
    tot[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        QsQuery& Q = st->qy[j];
        if (pass == 0) {
            unsigned long long total = 0;
            for (int t = 0; t < 256; ++t) total += tot[t];
            if (j == 0) st->total = total;
            Q.prefix = 0;
            if (total == 0) Q.state = -1;
            else {
                unsigned long long lo, hi;
                double gamma;
                qs_indexes(total, Q.q, &lo, &hi, &gamma);
                Q.k = lo;
                Q.want_hi = hi != lo;
                Q.state = 0;
            }
        }
        if (Q.state == 0) {
            unsigned long long k = Q.k;
            int t = 0;
            for (; t < 256; ++t) { if (k < tot[t]) break; k -= tot[t]; }
            int b = t * per;
            const int be = min(nb, (t + 1) * per);
            if (t < 256) for (; b < be; ++b) { if (k < h[b]) break; k -= h[b]; }
            if (t >= 256 || b >= be) Q.state = -2;
            else {
                Q.k = k;
                Q.prefix = (Q.prefix << nbits) | (unsigned long long)b;
                Q.hi_shift = qs_shift(pass);
                if (pass == QS_PASSES - 1) {
                    Q.lo_key = Q.prefix;
                    Q.eq = h[b];
                    // k keys equal to a[lo] sit in front of rank lo: a[lo + 1] is another of them when k + 1 < eq
                    const bool next_is_tie = k + 1 < (unsigned long long)h[b];
                    if (Q.want_hi && !next_is_tie) { Q.hi_key = QS_NONE; Q.state = 1; }
                    else { Q.hi_key = Q.lo_key; Q.state = 2; }
                }
            }
        }
    }
    if (pass > 0)
        for (int i = threadIdx.x; i < QS_BINS * QS_COPIES; i += 256) own[i] = 0;
}

// the smallest key above a[lo], for the queries that asked for it
__global__ void __launch_bounds__(QS_THREADS) k_qs_next(const double* __restrict__ vals, const uint8_t* __restrict__ valid, size_t n,
                                                        QsState* __restrict__ st)
{
    __shared__ unsigned long long red[QS_THREADS];
    const int j = blockIdx.y;
    if (st->qy[j].state != 1) return;                                  // the same for the whole workgroup
    const unsigned long long lo = st->qy[j].lo_key;
    unsigned long long m = QS_NONE;
    for (size_t base = (size_t)blockIdx.x * QS_TILE; base < n; base += (size_t)gridDim.x * QS_TILE) {
        double v[QS_ITEMS];
        bool ok[QS_ITEMS];
#pragma unroll
        for (int k = 0; k < QS_ITEMS; ++k) {
            const size_t i = base + (size_t)k * QS_THREADS + threadIdx.x;
            ok[k] = i < n;
            v[k] = ok[k] ? vals[i] : 0.0;
            if (valid) ok[k] = ok[k] && valid[i] != 0;
        }
#pragma unroll
        for (int k = 0; k < QS_ITEMS; ++k) {
            if (!ok[k] || v[k] != v[k]) continue;
            const unsigned long long key = order_key(v[k]);
            if (key > lo && key < m) m = key;
        }
    }
    red[threadIdx.x] = m;
    __syncthreads();
    block_tree<QS_THREADS>([&](int t, int u) { if (red[u] < red[t]) red[t] = red[u]; });
    if (threadIdx.x == 0 && red[0] != QS_NONE) atomicMin(&st->qy[j].hi_key, red[0]);
}

// the selection over n doubles of device memory (valid: optional mask), already ordered on stream s; synchronises
static int quantiles_run(wass_ctx* c, const double* d_vals, const uint8_t* d_valid, size_t n, const double* q, int nq, double* out,
                         uint64_t* n_points, hipStream_t s)
{
    const double nan = __builtin_nan("");
    if (n_points) *n_points = 0;
    for (int i = 0; i < nq; ++i) out[i] = nan;
    if (n == 0) return WASS_OK;
    int rc = ensure(c, c->qsel, QS_BYTES);
    if (rc) return rc;
    QsState* st = (QsState*)c->qsel.p;
    unsigned int* hist = (unsigned int*)((char*)c->qsel.p + QS_HIST_OFF);
    QsState h;
    memset(&h, 0, sizeof h);
    // hi_shift = 64 says "no prefix yet"; a shift by 64 is undefined, so k_qs_hist compares prefixes only from pass 1 on, when
    // k_qs_pick has set it to the pass's shift
    for (int i = 0; i < nq; ++i) { h.qy[i].q = q[i]; h.qy[i].hi_shift = 64; }
    WASS_HIP(c, hipMemsetAsync(c->qsel.p, 0, QS_BYTES, s));
    WASS_HIP(c, hipMemcpyAsync(st, &h, sizeof h, hipMemcpyHostToDevice, s));      // pageable source: staged before the call returns
    const size_t tiles = (n + QS_TILE - 1) / QS_TILE;
    const dim3 grid((unsigned)(tiles < (size_t)QS_MAX_BLOCKS ? tiles : (size_t)QS_MAX_BLOCKS), (unsigned)nq);
    for (int pass = 0; pass < QS_PASSES; ++pass) {
        hipLaunchKernelGGL(k_qs_hist, pass == 0 ? dim3(grid.x) : grid, dim3(QS_THREADS), 0, s, d_vals, d_valid, n, pass, st, hist);
        hipLaunchKernelGGL(k_qs_pick, dim3(nq), dim3(256), 0, s, hist, pass, st);
    }
    hipLaunchKernelGGL(k_qs_next, grid, dim3(QS_THREADS), 0, s, d_vals, d_valid, n, st);
    WASS_HIP(c, hipGetLastError());
    WASS_HIP(c, hipMemcpyAsync(&h, st, sizeof h, hipMemcpyDeviceToHost, s));
    WASS_HIP(c, hipStreamSynchronize(s));
    const unsigned long long total = h.total + h.nan_count;
    if (n_points) *n_points = total;
    if (total == 0 || h.nan_count) return WASS_OK;                                 // no values, or a NaN among them: all NaN
    for (int i = 0; i < nq; ++i) {
        const QsQuery& Q = h.qy[i];
        if (Q.state != 1 && Q.state != 2) return set_err(c, WASS_ERR_DEVICE, "quantile select lost its rank (internal error, state %d)", Q.state);
        if (Q.hi_key == QS_NONE) return set_err(c, WASS_ERR_DEVICE, "quantile select found no value above a[lo] (internal error)");
        unsigned long long lo, hi;
        double gamma;
        qs_indexes(h.total, q[i], &lo, &hi, &gamma);
        out[i] = qs_lerp(order_unkey(Q.lo_key), order_unkey(Q.hi_key), gamma);
    }
    return WASS_OK;
}

static int quantiles_args(wass_ctx* c, const double* q, int nq, double* out)
{
    if (!c) return WASS_ERR_INVALID_ARG;
    if (!q || !out) return set_err(c, WASS_ERR_INVALID_ARG, "null argument");
    if (nq < 1 || nq > QS_MAXQ) return set_err(c, WASS_ERR_INVALID_ARG, "nq = %d: 1 .. %d quantiles per call", nq, QS_MAXQ);
    for (int i = 0; i < nq; ++i)
        if (!(q[i] >= 0.0 && q[i] <= 1.0)) return set_err(c, WASS_ERR_INVALID_ARG, "q[%d] = %g: quantiles must be in [0, 1]", i, q[i]);
    return WASS_OK;
}

}  // namespace wass

using namespace wass;

extern "C" {

void wass_quantiles_launch_shape(int* per_block, int* per_launch)
{
    if (per_block) *per_block = QS_TILE;
    if (per_launch) *per_launch = QS_TILE * QS_MAX_BLOCKS;
}

int wass_quantiles_f64_dev(wass_ctx* c, const double* d_values, size_t n, const double* q, int nq, double* out)
{
    int rc = quantiles_args(c, q, nq, out);
    if (rc) return rc;
    if (n && !d_values) return set_err(c, WASS_ERR_INVALID_ARG, "null argument");
    WASS_HIP(c, hipSetDevice(c->device));
    return quantiles_run(c, d_values, nullptr, n, q, nq, out, nullptr, c->ts());
}

int wass_mesh_aligned_z_quantiles(wass_ctx* c, const wass_mesh* m, const double R[9], const double T[3], double baseline, const double* q,
                                  int nq, double* out, uint64_t* n_points)
{
    int rc = quantiles_args(c, q, nq, out);
    if (rc) return rc;
    if (!m || !R || !T) return set_err(c, WASS_ERR_INVALID_ARG, "null argument");
    WASS_HIP(c, hipSetDevice(c->device));
    const size_t n = m->n();
    if ((rc = ensure(c, c->scratch, n * 8))) return rc;
    double* z = (double*)c->scratch.p;
    hipLaunchKernelGGL(k_qs_align, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->ts(), m->valid, m->x, m->y, m->z, n, R[6], R[7], R[8], T[2],
                       baseline, z);
    return quantiles_run(c, z, m->valid, n, q, nq, out, n_points, c->ts());
}

}  // extern "C"
