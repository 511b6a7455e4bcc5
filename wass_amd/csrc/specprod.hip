// specprod.hip -- spectral products of the 3-D spectrum S(f, ky, kx) where it lies, in device memory: the sums behind the
// frequency-direction spectrum, the frequency-wavenumber spectrum, the wavenumber spectrum, the peak, and the weighted normal
// equations of the surface-current fit on the dispersion shell ("Spectral products", holds the definitions; they are the
// specification: the reference has no such tool).
//
// S is nt x ny x nx fp64, dense.  The host (wass_amd/postproc.py) evaluates every atan2, sqrt and tanh and hands over integer label
// maps and fp64 maps; the kernels only multiply, add and compare, in fp64, every product and sum a rounding of its own (the library
// is built with -ffp-contract=off) and every sum in ONE order that depends on the shape and the labels alone:
//   k_sp_label    T[p][b] = the sum of v = S[p][cell] * scale over the cells with label b.  The host lists every label's cells in
//                 raster order (a CSR); one workgroup per (b, p): thread t adds the label's cells t, t + 256, .. in that order from 0.0,
//                 then reduce.h's block_sum over the 256 threads.  An empty label gives 0.
//   k_sp_cells    one lane per cell, the frequencies ascending: E2[cell] = E2[cell] + v from 0.0 (so a cube that arrives in slabs of
//                 frequencies gives the same bits), a flag for a v that is negative or not finite, and the largest v over the cells
//                 with a label >= 0 and the frequencies [qa, qb), the lowest flat index (p ny + i) nx + j among equals: strict > in the
//                 lane, then (largest key, lowest index) over the wave, the waves and, in k_sp_best, the workgroups; no atomics.
//   k_sp_current  one lane per cell, the frequencies ascending: the seven sums of the current fit over the bins that pass the
//                 threshold and the gate, from 0.0, and their number; then per sum block_sum over the workgroup's 256 cells (raster order);
//   k_sp_fold     the workgroups' partials: thread t adds workgroups t, t + 256, .. from 0.0, then block_sum.  The bin count is an
//                 integer and is added with atomics.
// Host side: sp_plan keeps the byte formula; the slab rule (frequencies for rows), the scratch, the staging of a host slab and the
// end of the call are cube.h's.
#include "common.h"
#include "cube.h"

#include <float.h>
#include <math.h>
#include <vector>

namespace wass {

constexpr size_t SPP_SCRATCH_CAP = (size_t)16 << 30;    // bytes one wass_specprod call may allocate
constexpr int SPP_NSUM = WASS_SPECPROD_NSUMS;
constexpr unsigned long long SPP_NONE = ~0ull;

__global__ void __launch_bounds__(256) k_sp_label(const double* __restrict__ S, size_t plane, const int* __restrict__ off, const int* __restrict__ idx,
                                                  double scale, int nlab, double* __restrict__ T)
{
    __shared__ double sh[256];
    const int b = blockIdx.x, p = blockIdx.y;
    const double* __restrict__ Sp = S + (size_t)p * plane;
    const int hi = off[b + 1];
    double s = 0.0;
    for (int q = off[b] + (int)threadIdx.x; q < hi; q += 256) s += Sp[idx[q]] * scale;
    s = block_sum<256>(s, sh);
    if (threadIdx.x == 0) T[(size_t)p * nlab + b] = s;
}

// (largest key, lowest index among equals) of the workgroup's 256 threads, complete in thread 0; key 0 = nothing seen
__device__ __forceinline__ void sp_block_best(unsigned long long& key, unsigned long long& idx)
{
    __shared__ unsigned long long sk[4], si[4];
    const unsigned long long kmax = wave_max(key);
    idx = wave_all(key == kmax ? idx : SPP_NONE, [](unsigned long long a, unsigned long long b) { return b < a ? b : a; });
    key = kmax;
    __syncthreads();                                    // sk, si may still be read by an earlier call
    if ((threadIdx.x & 63) == 0) { sk[threadIdx.x >> 6] = key; si[threadIdx.x >> 6] = idx; }
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < 4; ++w)
            if (sk[w] > key || (sk[w] == key && si[w] < idx)) { key = sk[w]; idx = si[w]; }
}

// S: the first of np frequencies, which is frequency p0 of the cube.  best[2 * block], best[2 * block + 1]: the block's (key,
// index) so far, 0 before the first slab.
template <bool WITH_E2>
__global__ void __launch_bounds__(256) k_sp_cells(const double* __restrict__ S, unsigned cells, int np, int p0, int qa, int qb,
                                                  const int* __restrict__ lab, double scale, double* __restrict__ e2,
                                                  unsigned long long* __restrict__ best, int* __restrict__ flag)
{
    const unsigned c = blockIdx.x * 256u + threadIdx.x;
    unsigned long long key = 0, idx = SPP_NONE;
    if (c < cells) {
        const double* __restrict__ p = S + c;
        const bool used = lab[c] >= 0;
        double acc = WITH_E2 ? e2[c] : 0.0;
        bool bad = false;
#pragma unroll 4
        for (int q = 0; q < np; ++q) {
            const double v = p[(size_t)q * cells] * scale;
            bad = bad || !(v >= 0.0 && v <= DBL_MAX);
            acc += v;
            const unsigned long long k = order_key(v);
            if (used && p0 + q >= qa && p0 + q < qb && k > key) { key = k; idx = (unsigned long long)(p0 + q) * cells + c; }
        }
        if (WITH_E2) e2[c] = acc;
        if (bad) *flag = 1;
    }
    sp_block_best(key, idx);
    if (threadIdx.x == 0) {
        const unsigned long long k0 = best[2 * blockIdx.x], i0 = best[2 * blockIdx.x + 1];
        if (key > k0 || (key == k0 && idx < i0)) { best[2 * blockIdx.x] = key; best[2 * blockIdx.x + 1] = idx; }
    }
}

__global__ void __launch_bounds__(256) k_sp_best(const unsigned long long* __restrict__ best, int nblocks, unsigned long long* __restrict__ out)
{
    unsigned long long key = 0, idx = SPP_NONE;
    for (int b = threadIdx.x; b < nblocks; b += 256) {
        const unsigned long long k = best[2 * b], i = best[2 * b + 1];
        if (k > key || (k == key && i < idx)) { key = k; idx = i; }
    }
    sp_block_best(key, idx);
    if (threadIdx.x == 0) { out[0] = key; out[1] = idx; }
}

struct SpCurrent {
    const double* omega; const double* kapx; const double* kapy; const double* sig0;
    double U, V, thr, gate, scale;
};

// part[q * nblocks + block], q < SPP_NSUM, in the order of the WASS_SPECPROD_ enum; *count += the bins taken
__global__ void __launch_bounds__(256) k_sp_current(const double* __restrict__ S, unsigned cells, int nx, int pa, int pb, const int* __restrict__ lab,
                                                    const SpCurrent a, double* __restrict__ part, unsigned long long* __restrict__ count,
                                                    int* __restrict__ flag)
{
    __shared__ double sh[256];
    const unsigned c = blockIdx.x * 256u + threadIdx.x;
    double s[SPP_NSUM];
#pragma unroll
    for (int q = 0; q < SPP_NSUM; ++q) s[q] = 0.0;
    unsigned long long n = 0;
    if (c < cells && lab[c] >= 0) {
        const double kx = a.kapx[c % (unsigned)nx], ky = a.kapy[c / (unsigned)nx], s0 = a.sig0[c];
        const double uv = kx * a.U + ky * a.V;
        const double* __restrict__ p = S + c;
        bool bad = false;
#pragma unroll 4
        for (int q = pa; q < pb; ++q) {
            const double w = p[(size_t)q * cells] * a.scale;
            bad = bad || !(w >= 0.0 && w <= DBL_MAX);
            if (!(w >= a.thr)) continue;
            const double d = a.omega[q] - s0, r = d - uv;
            if (!(fabs(r) <= a.gate)) continue;
            const double wkx = w * kx, wky = w * ky;
            s[WASS_SPECPROD_AXX] += wkx * kx;
            s[WASS_SPECPROD_AXY] += wkx * ky;
            s[WASS_SPECPROD_AYY] += wky * ky;
            s[WASS_SPECPROD_BX] += wkx * d;
            s[WASS_SPECPROD_BY] += wky * d;
            s[WASS_SPECPROD_SW] += w;
            s[WASS_SPECPROD_SR2] += (w * r) * r;
            ++n;
        }
        if (bad) *flag = 1;
    }
#pragma unroll
    for (int q = 0; q < SPP_NSUM; ++q) {
        const double t = block_sum<256>(s[q], sh);
        if (threadIdx.x == 0) part[(size_t)q * gridDim.x + blockIdx.x] = t;
    }
    n = wave_fold(n, [](unsigned long long x, unsigned long long y) { return x + y; });
    if ((threadIdx.x & 63) == 0 && n) atomicAdd(count, n);
}

__global__ void __launch_bounds__(256) k_sp_fold(const double* __restrict__ part, int nblocks, double* __restrict__ out)
{
    __shared__ double sh[256];
    const double* __restrict__ p = part + (size_t)blockIdx.x * nblocks;
    double s = 0.0;
    for (int b = threadIdx.x; b < nblocks; b += 256) s += p[b];
    s = block_sum<256>(s, sh);
    if (threadIdx.x == 0) out[blockIdx.x] = s;
}

// ---- host -------------------------------------------------------------------------------------------------------------------
struct SpPlan {
    int nf = 0, freqs = 0, nblocks = 0;                 // frequencies of the positive half, per slab; workgroups of the cell kernels
    size_t cells = 0, total = 0;
};

struct SpMem {
    double* stage; int* lab; int* idx_d; int* off_d; int* idx_k; int* off_k; double* T_d; double* T_k; double* e2;
    unsigned long long* best; unsigned long long* res;  // res: key, index, then the flag as an int
};

static void sp_carve(Carve& a, const SpPlan& p, bool host, int n_dir, int n_k, SpMem& m)
{
    m.stage = a.take<double>(host ? (size_t)p.freqs * p.cells * 8 : 0);
    m.lab = a.take<int>(p.cells * 4);
    m.idx_d = a.take<int>(p.cells * 4);
    m.off_d = a.take<int>(((size_t)n_dir + 1) * 4);
    m.idx_k = a.take<int>(p.cells * 4);
    m.off_k = a.take<int>(((size_t)n_k + 1) * 4);
    m.T_d = a.take<double>((size_t)p.nf * n_dir * 8);
    m.T_k = a.take<double>((size_t)p.nf * n_k * 8);
    m.e2 = a.take<double>(p.cells * 8);
    m.best = a.take<unsigned long long>((size_t)p.nblocks * 16);
    m.res = a.take<unsigned long long>(256);
}

// 0, or why the problem cannot be planned.  p0: the first frequency of the positive half.
static int sp_plan(int nt, int ny, int nx, int p0, int n_dir, int n_k, int slab, bool host, SpPlan& p)
{
    if (nt < 1 || ny < 1 || nx < 1 || p0 < 0 || p0 >= nt || n_dir < 1 || n_k < 1 || slab < 0) return WASS_ERR_INVALID_ARG;
    p.cells = (size_t)ny * nx;
    if (p.cells > 0x7fffff00u) return WASS_ERR_UNSUPPORTED;     // a cell is indexed with 32 bits
    p.nf = nt - p0;
    p.nblocks = (int)((p.cells + 255) / 256);
    p.freqs = 1;
    SpMem m;
    const size_t fixed = measure([&](Carve& a) { sp_carve(a, p, false, n_dir, n_k, m); }) + 256;     // 256: the staging's own rounding
    if (fixed >= SPP_SCRATCH_CAP) return WASS_ERR_NO_MEMORY;
    const int rc = slab_rows(SPP_SCRATCH_CAP - fixed, host ? p.cells * 8 : 0, p.nf, 1, slab, &p.freqs);
    if (rc) return rc;
    p.total = measure([&](Carve& a) { sp_carve(a, p, host, n_dir, n_k, m); });
    return WASS_OK;
}

// the cells of every label in raster order: off[b] .. off[b + 1] of idx.  false: a label outside -1 .. nlab - 1
static bool sp_csr(const int32_t* lab, size_t cells, int nlab, std::vector<int>& off, std::vector<int>& idx)
{
    off.assign((size_t)nlab + 1, 0);
    idx.assign(cells, 0);
    for (size_t c = 0; c < cells; ++c) {
        if (lab[c] < -1 || lab[c] >= nlab) return false;
        if (lab[c] >= 0) ++off[(size_t)lab[c] + 1];
    }
    for (int b = 0; b < nlab; ++b) off[b + 1] += off[b];
    std::vector<int> at(off.begin(), off.end() - 1);
    for (size_t c = 0; c < cells; ++c)
        if (lab[c] >= 0) idx[at[lab[c]]++] = (int)c;
    return true;
}

// what k_sp_cells and k_sp_best left: res = key, index, flag.  The refusal, or the peak (NaN and -1 where no bin was used).
static int sp_peak_result(wass_ctx* c, const unsigned long long* res, double* peak_value, int64_t* peak_index)
{
    if ((int)res[2]) return set_err(c, WASS_ERR_INVALID_ARG, "the positive half of the spectrum holds a bin that is negative or not finite");
    *peak_value = res[0] ? order_unkey(res[0]) : NAN;
    *peak_index = res[0] ? (int64_t)res[1] : -1;
    return WASS_OK;
}

static void sp_label_launch(hipStream_t s, const double* S, size_t cells, int np, const int* off, const int* idx, double scale, int nlab, double* T)
{
    for (int q = 0; q < np; q += 65535) {               // gridDim.y
        const int n = np - q < 65535 ? np - q : 65535;
        hipLaunchKernelGGL(k_sp_label, dim3(nlab, n), dim3(256), 0, s, S + (size_t)q * cells, cells, off, idx, scale, nlab, T + (size_t)q * nlab);
    }
}

static int sp_tables(wass_ctx* c, bool host, const double* S, int nt, int ny, int nx, int p0, double scale, const int32_t* lab_dir, int n_dir,
                     const int32_t* lab_k, int n_k, int slab, double* T_dir, double* T_k, double* E2, double* peak_value, int64_t* peak_index)
{
    if (!c) return WASS_ERR_INVALID_ARG;
    if (!S || !lab_dir || !lab_k || !T_dir || !T_k || !E2 || !peak_value || !peak_index) return set_err(c, WASS_ERR_INVALID_ARG, "null argument");
    if (!(scale > 0.0) || !isfinite(scale)) return set_err(c, WASS_ERR_INVALID_ARG, "scale = %g (positive and finite)", scale);
    SpPlan p;
    int rc = sp_plan(nt, ny, nx, p0, n_dir, n_k, slab, host, p);
    if (rc) return set_err(c, rc, "cannot plan the products of a %d x %d x %d spectrum from frequency %d, %d and %d labels, slabs of %d", nt, ny, nx, p0,
                           n_dir, n_k, slab);
    std::vector<int> off_d, idx_d, off_k, idx_k;
    if (!sp_csr(lab_dir, p.cells, n_dir, off_d, idx_d) || !sp_csr(lab_k, p.cells, n_k, off_k, idx_k))
        return set_err(c, WASS_ERR_INVALID_ARG, "a label outside -1 .. n - 1");
    WASS_HIP(c, hipSetDevice(c->device));
    hipStream_t s = c->ts();
    Arena mem;
    if ((rc = mem.reserve(c, p.total, "the spectral products"))) return rc;
    SpMem m;
    sp_carve(mem, p, host, n_dir, n_k, m);
    const size_t cells = p.cells;
    unsigned long long res[3] = {0, 0, 0};
    hipError_t e = hipMemcpyAsync(m.lab, lab_dir, cells * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(m.idx_d, idx_d.data(), cells * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(m.off_d, off_d.data(), off_d.size() * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(m.idx_k, idx_k.data(), cells * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(m.off_k, off_k.data(), off_k.size() * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemsetAsync(m.e2, 0, cells * 8, s);
    if (e == hipSuccess) e = hipMemsetAsync(m.best, 0, (size_t)p.nblocks * 16, s);
    if (e == hipSuccess) e = hipMemsetAsync(m.res, 0, 256, s);
    for (int q0 = 0; q0 < p.nf && e == hipSuccess; q0 += p.freqs) {
        const int np = p.nf - q0 < p.freqs ? p.nf - q0 : p.freqs;
        const double* src = S + (size_t)(p0 + q0) * cells;
        if (host) {
            e = hipMemcpyAsync(m.stage, src, (size_t)np * cells * 8, hipMemcpyHostToDevice, s);
            if (e != hipSuccess) break;
            src = m.stage;
        }
        sp_label_launch(s, src, cells, np, m.off_d, m.idx_d, scale, n_dir, m.T_d + (size_t)q0 * n_dir);
        sp_label_launch(s, src, cells, np, m.off_k, m.idx_k, scale, n_k, m.T_k + (size_t)q0 * n_k);
        hipLaunchKernelGGL((k_sp_cells<true>), dim3(p.nblocks), dim3(256), 0, s, src, (unsigned)cells, np, p0 + q0, p0, nt, (const int*)m.lab, scale,
                           m.e2, m.best, (int*)(m.res + 2));
        e = hipGetLastError();
    }
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_sp_best, dim3(1), dim3(256), 0, s, (const unsigned long long*)m.best, p.nblocks, m.res);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(res, m.res, sizeof res, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(T_dir, m.T_d, (size_t)p.nf * n_dir * 8, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(T_k, m.T_k, (size_t)p.nf * n_k * 8, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(E2, m.e2, cells * 8, hipMemcpyDeviceToHost, s);
    rc = finish(c, WASS_OK, e, s, "spectral products");
    if (rc) return rc;
    return sp_peak_result(c, res, peak_value, peak_index);
}

}  // namespace wass

using namespace wass;

extern "C" int wass_specprod_scratch_bytes(int nt, int ny, int nx, int p0, int n_dir, int n_k, int slab, int host, size_t* bytes,
                                           int* freqs_per_slab)
{
    if (!bytes) return WASS_ERR_INVALID_ARG;
    SpPlan p;
    const int rc = sp_plan(nt, ny, nx, p0, n_dir, n_k, slab, host != 0, p);
    if (rc) return rc;
    *bytes = p.total;
    if (freqs_per_slab) *freqs_per_slab = p.freqs;
    return WASS_OK;
}

extern "C" int wass_specprod_tables(wass_ctx* c, const double* S, int nt, int ny, int nx, int p0, double scale, const int32_t* lab_dir, int n_dir,
                                    const int32_t* lab_k, int n_k, int slab, double* T_dir, double* T_k, double* E2, double* peak_value,
                                    int64_t* peak_index)
{
    return sp_tables(c, true, S, nt, ny, nx, p0, scale, lab_dir, n_dir, lab_k, n_k, slab, T_dir, T_k, E2, peak_value, peak_index);
}

extern "C" int wass_specprod_tables_dev(wass_ctx* c, const double* d_S, int nt, int ny, int nx, int p0, double scale, const int32_t* lab_dir,
                                        int n_dir, const int32_t* lab_k, int n_k, double* T_dir, double* T_k, double* E2, double* peak_value,
                                        int64_t* peak_index)
{
    return sp_tables(c, false, d_S, nt, ny, nx, p0, scale, lab_dir, n_dir, lab_k, n_k, 0, T_dir, T_k, E2, peak_value, peak_index);
}

extern "C" int wass_specprod_peak_dev(wass_ctx* c, const double* d_S, int nt, int ny, int nx, int p0, int pa, int pb, double scale,
                                      const int32_t* labels, double* peak_value, int64_t* peak_index)
{
    if (!c) return WASS_ERR_INVALID_ARG;
    if (!d_S || !labels || !peak_value || !peak_index) return set_err(c, WASS_ERR_INVALID_ARG, "null argument");
    const size_t cells = (size_t)(ny > 0 ? ny : 0) * (size_t)(nx > 0 ? nx : 0);
    if (nt < 1 || ny < 1 || nx < 1 || p0 < 0 || p0 >= nt || pa < p0 || pb > nt || pa > pb || cells > 0x7fffff00u || !(scale > 0.0) || !isfinite(scale))
        return set_err(c, WASS_ERR_INVALID_ARG, "a %d x %d x %d spectrum, frequencies %d .. %d of the half from %d, scale %g", nt, ny, nx, pa, pb, p0, scale);
    WASS_HIP(c, hipSetDevice(c->device));
    hipStream_t s = c->ts();
    const int nblocks = (int)((cells + 255) / 256);
    int* lab;
    unsigned long long *best, *dres;
    auto lay = [&](Carve& a) {
        lab = a.take<int>(cells * 4);
        best = a.take<unsigned long long>((size_t)nblocks * 16);
        dres = a.take<unsigned long long>(256);
    };
    Arena mem;
    int rc = mem.reserve(c, measure(lay), "the peak of the spectrum");
    if (rc) return rc;
    lay(mem);
    unsigned long long res[3] = {0, 0, 0};
    hipError_t e = hipMemcpyAsync(lab, labels, cells * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemsetAsync(best, 0, (size_t)nblocks * 16, s);
    if (e == hipSuccess) e = hipMemsetAsync(dres, 0, 256, s);
    if (e == hipSuccess) {
        hipLaunchKernelGGL((k_sp_cells<false>), dim3(nblocks), dim3(256), 0, s, d_S + (size_t)p0 * cells, (unsigned)cells, nt - p0, p0, pa, pb,
                           (const int*)lab, scale, (double*)nullptr, best, (int*)(dres + 2));
        hipLaunchKernelGGL(k_sp_best, dim3(1), dim3(256), 0, s, (const unsigned long long*)best, nblocks, dres);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(res, dres, sizeof res, hipMemcpyDeviceToHost, s);
    rc = finish(c, WASS_OK, e, s, "peak of the spectrum");
    if (rc) return rc;
    return sp_peak_result(c, res, peak_value, peak_index);
}

extern "C" int wass_specprod_current_sums_dev(wass_ctx* c, const double* d_S, int nt, int ny, int nx, int pa, int pb, double scale,
                                              const int32_t* labels, const double* omega, const double* kappa_x, const double* kappa_y,
                                              const double* sigma0, double U, double V, double threshold_value, double gate_value, double* sums,
                                              int64_t* n_bins)
{
    if (!c) return WASS_ERR_INVALID_ARG;
    if (!d_S || !labels || !omega || !kappa_x || !kappa_y || !sigma0 || !sums || !n_bins) return set_err(c, WASS_ERR_INVALID_ARG, "null argument");
    const size_t cells = (size_t)(ny > 0 ? ny : 0) * (size_t)(nx > 0 ? nx : 0);
    if (nt < 1 || ny < 1 || nx < 1 || pa < 0 || pb > nt || pa > pb || cells > 0x7fffff00u || !(scale > 0.0) || !isfinite(scale) || !isfinite(U) ||
        !isfinite(V) || isnan(threshold_value) || isnan(gate_value))
        return set_err(c, WASS_ERR_INVALID_ARG, "a %d x %d x %d spectrum, frequencies %d .. %d, scale %g, current (%g, %g), threshold %g, gate %g", nt, ny,
                       nx, pa, pb, scale, U, V, threshold_value, gate_value);
    WASS_HIP(c, hipSetDevice(c->device));
    hipStream_t s = c->ts();
    const int nblocks = (int)((cells + 255) / 256);
    int* lab;
    double *maps, *part, *out;
    const size_t nmap = (size_t)nt + nx + ny + cells;
    auto lay = [&](Carve& a) {
        lab = a.take<int>(cells * 4);
        maps = a.take<double>(nmap * 8);                // omega, kappa_x, kappa_y, sigma0
        part = a.take<double>((size_t)SPP_NSUM * nblocks * 8);
        out = a.take<double>(256);                      // the sums, the count, the flag
    };
    Arena mem;
    int rc = mem.reserve(c, measure(lay), "the current sums");
    if (rc) return rc;
    lay(mem);
    double res[SPP_NSUM + 2];
    hipError_t e = hipMemcpyAsync(lab, labels, cells * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(maps, omega, (size_t)nt * 8, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(maps + nt, kappa_x, (size_t)nx * 8, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(maps + nt + nx, kappa_y, (size_t)ny * 8, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(maps + nt + nx + ny, sigma0, cells * 8, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemsetAsync(out, 0, 256, s);
    if (e == hipSuccess) {
        const SpCurrent a = {maps, maps + nt, maps + nt + nx, maps + nt + nx + ny, U, V, threshold_value, gate_value, scale};
        hipLaunchKernelGGL(k_sp_current, dim3(nblocks), dim3(256), 0, s, d_S, (unsigned)cells, nx, pa, pb, (const int*)lab, a, part,
                           (unsigned long long*)(out + SPP_NSUM), (int*)(out + SPP_NSUM + 1));
        hipLaunchKernelGGL(k_sp_fold, dim3(SPP_NSUM), dim3(256), 0, s, (const double*)part, nblocks, out);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(res, out, sizeof res, hipMemcpyDeviceToHost, s);
    rc = finish(c, WASS_OK, e, s, "current sums");
    if (rc) return rc;
    if (*(const int*)&res[SPP_NSUM + 1]) return set_err(c, WASS_ERR_INVALID_ARG, "a bin of the fit is negative or not finite");
    for (int q = 0; q < SPP_NSUM; ++q) sums[q] = res[q];
    *n_bins = *(const int64_t*)&res[SPP_NSUM];
    return WASS_OK;
}
