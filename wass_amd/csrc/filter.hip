// filter.hip -- the temporal Butterworth filter of the gridded cube: scipy.signal.sosfiltfilt(sos, Z, axis=0) as wasspost's
// `filter` / `filter_fast` run it (postproc/wasspost/wasspost.py:149-314), for every cell of a count x H x W float32 cube.  The
// host side (wass_amd/postproc.py) designs the sections and their steady state zi in fp64 and passes them in.
//
// One lane per series, consecutive lanes along x, so every time step of a wave is one coalesced row segment.  State and
// arithmetic are fp64, two doubles per section, in scipy's own order of operations (transposed direct form II, no contraction:
// the library is built with -ffp-contract=off); the coefficients are kernel arguments, i.e. wave-uniform.
//   k_sos_forward   reads the f32 series (4 B), builds the odd padding IN FLOAT32 as scipy does (2 x[0] - x[k] is rounded to f32
//                   before anything becomes fp64), starts from zi * (first padded sample), writes all count + 2 padlen outputs
//                   as fp64 (8 B): a float32 hand-over would cost the 1e-8 the padding quirk is about
//   k_sos_backward  reads them last to first (8 B), starts from zi * (last one), drops the pads, writes f32 (4 B) -- or, for
//                   remove_mean, fp64 in place, and
//   k_sos_demean    sums every series first frame to last (numpy's order for mean(axis=0)), subtracts, casts.
// A wave keeps FILT_U rows in flight ahead of the one it is filtering (the chain is sequential in t; the loads are not).
// Rows are filtered in slabs so that the fp64 hand-over, (count + 2 padlen) * rows * W * 8 bytes, and the staging of a host
// cube, count * rows * W * 4 bytes, stay under FILT_SCRATCH_CAP; a series never crosses a slab, so the result does not
// depend on the slab height.  No atomics: the same input gives the same bits.
// Host side: filt_plan keeps the byte formula; the slab rule, the scratch, the staging of a host slab and the end of the call
// are cube.h's.
#include "common.h"
#include "cube.h"

namespace wass {

constexpr size_t FILT_SCRATCH_CAP = (size_t)16 << 30;   // bytes one wass_sosfiltfilt call may allocate
constexpr int FILT_MAX_SECTIONS = 6;                    // order 12; with more the coefficients no longer fit the scalar registers
constexpr int FILT_U = 8;                               // time steps loaded ahead of the recurrence

struct SosArgs {
    double b0[FILT_MAX_SECTIONS], b1[FILT_MAX_SECTIONS], b2[FILT_MAX_SECTIONS], a1[FILT_MAX_SECTIONS], a2[FILT_MAX_SECTIONS];
    double zi0[FILT_MAX_SECTIONS], zi1[FILT_MAX_SECTIONS];
};

template <int NS>
__device__ __forceinline__ double sos_step(double x, double (&z0)[NS], double (&z1)[NS], const SosArgs& a)
{
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const double y = a.b0[s] * x + z0[s];
        z0[s] = (a.b1[s] * x - a.a1[s] * y) + z1[s];
        z1[s] = a.b2[s] * x - a.a2[s] * y;
        x = y;
    }
    return x;
}

// n samples through the sections: load(j) gives sample j as a double, store(j, y) takes its output.  Blocks of FILT_U samples,
// the next block's loads issued before the current block's chain.
template <int NS, class Load, class Store>
__device__ __forceinline__ void sos_run(int n, double (&z0)[NS], double (&z1)[NS], const SosArgs& a, Load load, Store store)
{
    double cur[FILT_U], nxt[FILT_U];
    int j = 0;
    if (n >= FILT_U) {
#pragma unroll
        for (int u = 0; u < FILT_U; ++u) cur[u] = load(u);
    }
    for (; j + FILT_U <= n; j += FILT_U) {
        const bool more = j + 2 * FILT_U <= n;
        if (more) {
#pragma unroll
            for (int u = 0; u < FILT_U; ++u) nxt[u] = load(j + FILT_U + u);
        }
#pragma unroll
        for (int u = 0; u < FILT_U; ++u) store(j + u, sos_step<NS>(cur[u], z0, z1, a));
        if (more) {
#pragma unroll
            for (int u = 0; u < FILT_U; ++u) cur[u] = nxt[u];
        }
    }
    for (; j < n; ++j) store(j, sos_step<NS>(load(j), z0, z1, a));
}

// series i of the slab: row i / W, column i % W of x (element strides st, sy).  ypad[q][i], q < count + 2 padlen.
template <int NS>
__global__ void __launch_bounds__(256) k_sos_forward(const float* __restrict__ x, long long st, long long sy, int W, unsigned nser, int count,
                                                     int padlen, const SosArgs a, double* __restrict__ ypad)
{
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= nser) return;
    const float* __restrict__ p = x + (long long)(i / (unsigned)W) * sy + (i % (unsigned)W);
    double* __restrict__ yo = ypad + i;
    const float x0 = p[0], xl = p[(long long)(count - 1) * st];
    // scipy's odd_ext in the input's dtype: 2 x[0] - x[padlen .. 1], x, 2 x[-1] - x[-2 .. -(padlen + 1)]
    const double first = padlen ? (double)(2.f * x0 - p[(long long)padlen * st]) : (double)x0;
    double z0[NS], z1[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        z0[s] = a.zi0[s] * first;
        z1[s] = a.zi1[s] * first;
    }
    size_t q0 = 0;
    auto store = [&](int j, double y) { yo[(q0 + (size_t)j) * nser] = y; };
    sos_run<NS>(padlen, z0, z1, a, [&](int j) { return (double)(2.f * x0 - p[(long long)(padlen - j) * st]); }, store);
    q0 = (size_t)padlen;
    sos_run<NS>(count, z0, z1, a, [&](int j) { return (double)p[(long long)j * st]; }, store);
    q0 = (size_t)padlen + (size_t)count;
    sos_run<NS>(padlen, z0, z1, a, [&](int j) { return (double)(2.f * xl - p[(long long)(count - 2 - j) * st]); }, store);
}

// DEMEAN: the outputs stay fp64, in place in ypad; else out[t][row][col] (element strides ot, oy) = (float) output
template <int NS, bool DEMEAN>
__global__ void __launch_bounds__(256) k_sos_backward(double* __restrict__ ypad, int W, unsigned nser, int count, int padlen, const SosArgs a,
                                                      float* __restrict__ out, long long ot, long long oy)
{
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= nser) return;
    double* __restrict__ yi = ypad + i;
    float* __restrict__ o = DEMEAN ? nullptr : out + (long long)(i / (unsigned)W) * oy + (i % (unsigned)W);
    const size_t last = (size_t)count + 2 * (size_t)padlen - 1;
    const double first = yi[last * nser];
    double z0[NS], z1[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        z0[s] = a.zi0[s] * first;
        z1[s] = a.zi1[s] * first;
    }
    size_t q0 = last;                                   // sample j of a run is padded index q0 - j
    auto load = [&](int j) { return yi[(q0 - (size_t)j) * nser]; };
    sos_run<NS>(padlen, z0, z1, a, load, [](int, double) {});
    q0 = last - (size_t)padlen;
    sos_run<NS>(count, z0, z1, a, load, [&](int j, double y) {
        if (DEMEAN) yi[(q0 - (size_t)j) * nser] = y;
        else o[(long long)(count - 1 - j) * ot] = (float)y;
    });
}

// out = (float)(y - mean over t of y), the sum first frame to last in fp64
__global__ void __launch_bounds__(256) k_sos_demean(const double* __restrict__ ypad, int W, unsigned nser, int count, int padlen,
                                                    float* __restrict__ out, long long ot, long long oy)
{
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= nser) return;
    const double* __restrict__ y = ypad + (size_t)padlen * nser + i;
    float* __restrict__ o = out + (long long)(i / (unsigned)W) * oy + (i % (unsigned)W);
    double s = 0.0;
#pragma unroll 8
    for (int t = 0; t < count; ++t) s += y[(size_t)t * nser];
    const double m = s / (double)count;
#pragma unroll 8
    for (int t = 0; t < count; ++t) o[(long long)t * ot] = (float)(y[(size_t)t * nser] - m);
}

template <int NS>
static void launch_slab(hipStream_t s, const float* x, long long st, long long sy, int W, unsigned nser, int count, int padlen, const SosArgs& a,
                        double* ypad, bool demean, float* out, long long ot, long long oy)
{
    const dim3 grid((nser + 255u) / 256u), block(256);
    hipLaunchKernelGGL((k_sos_forward<NS>), grid, block, 0, s, x, st, sy, W, nser, count, padlen, a, ypad);
    if (demean) {
        hipLaunchKernelGGL((k_sos_backward<NS, true>), grid, block, 0, s, ypad, W, nser, count, padlen, a, out, ot, oy);
        hipLaunchKernelGGL(k_sos_demean, grid, block, 0, s, (const double*)ypad, W, nser, count, padlen, out, ot, oy);
    } else {
        hipLaunchKernelGGL((k_sos_backward<NS, false>), grid, block, 0, s, ypad, W, nser, count, padlen, a, out, ot, oy);
    }
}

static int filter_slab(wass_ctx* c, hipStream_t s, int ns, const float* x, long long st, long long sy, int W, unsigned nser, int count, int padlen,
                       const SosArgs& a, double* ypad, bool demean, float* out, long long ot, long long oy)
{
    switch (ns) {
    case 1: launch_slab<1>(s, x, st, sy, W, nser, count, padlen, a, ypad, demean, out, ot, oy); break;
    case 2: launch_slab<2>(s, x, st, sy, W, nser, count, padlen, a, ypad, demean, out, ot, oy); break;
    case 3: launch_slab<3>(s, x, st, sy, W, nser, count, padlen, a, ypad, demean, out, ot, oy); break;
    case 4: launch_slab<4>(s, x, st, sy, W, nser, count, padlen, a, ypad, demean, out, ot, oy); break;
    case 5: launch_slab<5>(s, x, st, sy, W, nser, count, padlen, a, ypad, demean, out, ot, oy); break;
    default: launch_slab<6>(s, x, st, sy, W, nser, count, padlen, a, ypad, demean, out, ot, oy); break;
    }
    WASS_HIP(c, hipGetLastError());
    return WASS_OK;
}

struct FiltPlan {
    int rows = 0;                  // rows per slab
    size_t ypad_bytes = 0, stage_bytes = 0, total = 0;
};

// 0, or why the problem cannot be planned
static int filt_plan(int count, int H, int W, int padlen, int slab, bool host, FiltPlan& p)
{
    if (count < 1 || H < 1 || W < 1 || padlen < 0 || slab < 0 || count <= padlen) return WASS_ERR_INVALID_ARG;
    const size_t P = (size_t)count + 2 * (size_t)padlen;
    const size_t per_row = P * (size_t)W * 8 + (host ? (size_t)count * (size_t)W * 4 : 0);
    const int rc = slab_rows(FILT_SCRATCH_CAP - 512, per_row, H, W, slab, &p.rows);
    if (rc) return rc;
    p.ypad_bytes = align256(P * (size_t)p.rows * (size_t)W * 8);
    p.stage_bytes = host ? align256((size_t)count * (size_t)p.rows * (size_t)W * 4) : 0;
    p.total = p.ypad_bytes + p.stage_bytes;
    return WASS_OK;
}

static int filt_args(wass_ctx* c, const double* sos, int ns, const double* zi, SosArgs& a)
{
    if (!sos || !zi) return set_err(c, WASS_ERR_INVALID_ARG, "null argument");
    if (ns < 1 || ns > FILT_MAX_SECTIONS) return set_err(c, WASS_ERR_INVALID_ARG, "%d sections (1 .. %d)", ns, FILT_MAX_SECTIONS);
    memset(&a, 0, sizeof a);
    for (int s = 0; s < ns; ++s) {
        if (sos[6 * s + 3] != 1.0) return set_err(c, WASS_ERR_INVALID_ARG, "sos[%d][3] must be 1", s);
        a.b0[s] = sos[6 * s]; a.b1[s] = sos[6 * s + 1]; a.b2[s] = sos[6 * s + 2];
        a.a1[s] = sos[6 * s + 4]; a.a2[s] = sos[6 * s + 5];
        a.zi0[s] = zi[2 * s]; a.zi1[s] = zi[2 * s + 1];
    }
    return WASS_OK;
}

static int filt_run(wass_ctx* c, bool host, const float* in, size_t st, size_t sy, int count, int H, int W, const double* sos, int ns,
                    const double* zi, int padlen, int remove_mean, int slab_rows, float* out, size_t ost, size_t osy)
{
    if (!c) return WASS_ERR_INVALID_ARG;
    if (!in || !out) return set_err(c, WASS_ERR_INVALID_ARG, "null argument");
    SosArgs a;
    int rc = filt_args(c, sos, ns, zi, a);
    if (rc) return rc;
    if (count >= 1 && padlen >= 0 && count <= padlen)
        return set_err(c, WASS_ERR_INVALID_ARG, "%d frames: more than padlen = %d are needed", count, padlen);
    FiltPlan p;
    rc = filt_plan(count, H, W, padlen, slab_rows, host, p);
    if (rc) return set_err(c, rc, "cannot plan a %d x %d x %d filter with padlen %d under the scratch cap of %zu bytes", count, H, W, padlen,
                           FILT_SCRATCH_CAP);
    if (sy < (size_t)W || osy < (size_t)W || (count > 1 && (st < (size_t)W || ost < (size_t)W)))
        return set_err(c, WASS_ERR_INVALID_ARG, "bad strides");
    WASS_HIP(c, hipSetDevice(c->device));
    hipStream_t s = c->ts();
    Arena mem;
    if ((rc = mem.reserve(c, p.total, "the filter scratch"))) return rc;
    double* ypad = mem.take<double>(p.ypad_bytes);
    float* stage = mem.take<float>(p.stage_bytes);
    for (int r0 = 0; r0 < H && !rc; r0 += p.rows) {
        const int rows = H - r0 < p.rows ? H - r0 : p.rows;
        const unsigned nser = (unsigned)((size_t)rows * W);
        if (host) {
            const size_t plane = (size_t)rows * W;
            hipError_t e = upload_rows(stage, in, 4, count, r0, rows, W, st, sy, s);
            if (e != hipSuccess) { rc = set_err(c, WASS_ERR_DEVICE, "upload of a slab: %s", hipGetErrorString(e)); break; }
            // the backward pass reads the hand-over only: the result may take the staged input's place
            rc = filter_slab(c, s, ns, stage, (long long)plane, W, W, nser, count, padlen, a, ypad, remove_mean != 0, stage, (long long)plane, W);
            if (!rc) e = download_rows(out, stage, 4, count, r0, rows, W, ost, osy, s);
            if (!rc && e != hipSuccess) rc = set_err(c, WASS_ERR_DEVICE, "download of a slab: %s", hipGetErrorString(e));
        } else {
            rc = filter_slab(c, s, ns, in + (size_t)r0 * sy, (long long)st, (long long)sy, W, nser, count, padlen, a, ypad, remove_mean != 0,
                             out + (size_t)r0 * osy, (long long)ost, (long long)osy);
        }
    }
    return finish(c, rc, hipSuccess, s, "temporal filter");
}

}  // namespace wass

using namespace wass;

extern "C" int wass_sosfiltfilt_scratch_bytes(int count, int H, int W, int padlen, int slab_rows, int host, size_t* bytes, int* rows_per_slab)
{
    if (!bytes) return WASS_ERR_INVALID_ARG;
    FiltPlan p;
    const int rc = filt_plan(count, H, W, padlen, slab_rows, host != 0, p);
    if (rc) return rc;
    *bytes = p.total;
    if (rows_per_slab) *rows_per_slab = p.rows;
    return WASS_OK;
}

extern "C" int wass_sosfiltfilt(wass_ctx* c, const float* in, size_t stride_t, size_t stride_y, int count, int H, int W, const double* sos,
                                int n_sections, const double* zi, int padlen, int remove_mean, int slab_rows, float* out, size_t out_stride_t,
                                size_t out_stride_y)
{
    return filt_run(c, true, in, stride_t, stride_y, count, H, W, sos, n_sections, zi, padlen, remove_mean, slab_rows, out, out_stride_t, out_stride_y);
}

extern "C" int wass_sosfiltfilt_dev(wass_ctx* c, const float* d_in, size_t stride_t, size_t stride_y, int count, int H, int W, const double* sos,
                                    int n_sections, const double* zi, int padlen, int remove_mean, int slab_rows, float* d_out,
                                    size_t out_stride_t, size_t out_stride_y)
{
    return filt_run(c, false, d_in, stride_t, stride_y, count, H, W, sos, n_sections, zi, padlen, remove_mean, slab_rows, d_out, out_stride_t,
                    out_stride_y);
}
