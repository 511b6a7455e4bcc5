// reduce_check.hip -- every primitive of wass_amd/csrc/reduce.h on one workgroup, bit for bit against host loops that fold in the order
// the header's comments state.  `reduce_check host` runs the host-side checks alone (no device needed): the probes must not be blind,
// that is, the documented trees must give other bits than a plain left-to-right sum of the same doubles.  Prints "ok" and exits 0.
#include "../../wass_amd/csrc/reduce.h"

#include <float.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

using namespace wass;
typedef unsigned long long u64;

static int fails = 0;
static void check(bool good, const char* what)
{
    if (!good) { printf("FAIL %s\n", what); ++fails; }
}
static void hip_ok(hipError_t e, const char* what)
{
    if (e != hipSuccess) { printf("FAIL %s: %s\n", what, hipGetErrorString(e)); exit(2); }
}
template <class T> static bool same_bits(const T* a, const T* b, size_t n) { return memcmp(a, b, n * sizeof(T)) == 0; }

// ---------------------------------------------------------------- the host's statement of each order
// wave_fold: for o = 32 .. 1: v = op(v, v of lane + o); a lane without a partner is handed its own value
template <class T, class F> static void h_fold(T* v, F op)
{
    for (int o = 32; o > 0; o >>= 1) {
        T n[64];
        for (int l = 0; l < 64; ++l) n[l] = op(v[l], l + o < 64 ? v[l + o] : v[l]);
        memcpy(v, n, sizeof n);
    }
}
// wave_all: for o = 32 .. 1: v = op(v, v of lane ^ o)
template <class T, class F> static void h_all(T* v, F op)
{
    for (int o = 32; o > 0; o >>= 1) {
        T n[64];
        for (int l = 0; l < 64; ++l) n[l] = op(v[l], v[l ^ o]);
        memcpy(v, n, sizeof n);
    }
}
// wave_scan: for o = 1 .. 32: lanes >= o take v = op(v, v of lane - o)
template <class T, class F> static void h_scan(T* v, F op)
{
    for (int o = 1; o < 64; o <<= 1) {
        T n[64];
        for (int l = 0; l < 64; ++l) n[l] = l >= o ? op(v[l], v[l - o]) : v[l];
        memcpy(v, n, sizeof n);
    }
}
// block_scan over nw waves: wave_scan, part[w] = lane 63 of wave w, then op(.. op(own, part[0]) .., part[w - 1])
template <class T, class F> static void h_block_scan(T* v, int nw, T* part, F op)
{
    for (int w = 0; w < nw; ++w) { h_scan(v + 64 * w, op); part[w] = v[64 * w + 63]; }
    for (int w = 0; w < nw; ++w)
        for (int l = 0; l < 64; ++l)
            for (int k = 0; k < w; ++k) v[64 * w + l] = op(v[64 * w + l], part[k]);
}
// block_tree: for o = N/2 .. 1: elements t < o take e[t] = e[t] . e[t + o]
static double h_tree(const double* e, int n)
{
    double a[1024];
    memcpy(a, e, n * sizeof(double));
    for (int o = n / 2; o > 0; o >>= 1)
        for (int t = 0; t < o; ++t) a[t] += a[t + o];
    return a[0];
}
// lds_scan: for o = 1 .. N/2: a[t] += a[t - o] of the round before (0 for t < o)
template <class T> static void h_lds_scan(T* a, int n)
{
    T* b = (T*)malloc(n * sizeof(T));
    for (int o = 1; o < n; o <<= 1) {
        for (int t = 0; t < n; ++t) b[t] = a[t] + (t >= o ? a[t - o] : T(0));
        memcpy(a, b, n * sizeof(T));
    }
    free(b);
}
static double h_seq(const double* e, int n)
{
    double s = e[0];
    for (int i = 1; i < n; ++i) s += e[i];
    return s;
}

// ---------------------------------------------------------------- inputs
static unsigned rng_state = 12345u;
static unsigned rng() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

// doubles whose sum depends on the order: magnitudes 2^53 apart, alternating signs.  A huge value and its negative are neighbours, so
// a left-to-right sum cancels them at once and keeps the small terms; a tree pairs them with small terms first and loses those.
static void order_probe(double* d, int n)
{
    for (int i = 0; i < n; i += 2) {
        if (rng() % 4 == 0) { d[i] = 0x1p53; d[i + 1] = -0x1p53; }
        else { d[i] = 1.0 + (double)(rng() % 1000) * 0x1p-10; d[i + 1] = -(0x1p26 + (double)(rng() % 7)); }
    }
}
// counts with zeros among them; wave `zero_wave` is all zero
static void counts(unsigned* c, int n, int zero_wave)
{
    for (int i = 0; i < n; ++i) c[i] = (i / 64 == zero_wave || rng() % 3 == 0) ? 0u : rng() % 41;
}

// ---------------------------------------------------------------- kernels
struct WaveOut {
    double fold_sum, all_sum[64];
    u64 fold_max, max64[64];
    unsigned max32[64], scan_add[64];
    int scan_max[64];
};
__global__ void __launch_bounds__(64) k_wave(const double* d, const u64* k, const unsigned* c, const int* m, WaveOut* o)
{
    const int l = threadIdx.x;
    const double f = wave_fold(d[l], [](double a, double b) { return a + b; });
    const u64 kf = wave_fold(k[l], [](u64 a, u64 b) { return b > a ? b : a; });
    if (l == 0) { o->fold_sum = f; o->fold_max = kf; }
    o->all_sum[l] = wave_all(d[l], [](double a, double b) { return a + b; });
    o->max64[l] = wave_max(k[l]);
    o->max32[l] = wave_max((unsigned)(k[l] >> 32));
    o->scan_add[l] = wave_scan(c[l], [](unsigned a, unsigned b) { return a + b; });
    o->scan_max[l] = wave_scan(m[l], [](int a, int b) { return max(a, b); });
}

struct BlockOut {
    unsigned scan_add[256], part[4];
    int scan_max[256];
    double tree_a, tree_b;
};
__global__ void __launch_bounds__(256) k_block(const unsigned* c, const int* m, const double* d, BlockOut* o)
{
    __shared__ unsigned pu[4];
    __shared__ int pi[4];
    __shared__ double a[256], b[256];
    const int t = threadIdx.x;
    o->scan_add[t] = block_scan(c[t], pu, [](unsigned x, unsigned y) { return x + y; });
    if (t < 4) o->part[t] = pu[t];
    o->scan_max[t] = block_scan(m[t], pi, [](int x, int y) { return max(x, y); });
    a[t] = d[t];
    b[t] = d[255 - t];
    __syncthreads();
    block_tree<256>([&](int i, int j) { a[i] += a[j]; b[i] += b[j]; });
    if (t == 0) { o->tree_a = a[0]; o->tree_b = b[0]; }
}

template <int N, class T> __global__ void __launch_bounds__(N) k_lds_scan(const T* in, T* out)
{
    __shared__ T a[N];
    a[threadIdx.x] = in[threadIdx.x];
    __syncthreads();
    lds_scan<N>(a);
    out[threadIdx.x] = a[threadIdx.x];
}

// two calls in one kernel: the second may only store into block_max's LDS once thread (0, 0) has read the first call's entries
template <int BY, class K> __global__ void __launch_bounds__(64 * BY) k_bmax(const K* ka, const K* kb, K* dst)
{
    const int t = threadIdx.y * 64 + threadIdx.x;
    block_max<BY>(ka[t], dst);
    block_max<BY>(kb[t], dst + 1);
    block_max<BY>(K(0), dst + 2);                       // nothing seen: nothing written
}

__global__ void k_keys(const float* f, const double* d, int n, unsigned* kf, u64* kd, float* rf, double* rd)
{
    const int i = threadIdx.x;
    if (i >= n) return;
    kf[i] = order_key(f[i]);
    kd[i] = order_key(d[i]);
    rf[i] = order_unkey(kf[i]);
    rd[i] = order_unkey(kd[i]);
}

// ---------------------------------------------------------------- driver
template <class T> static T* to_dev(const T* h, size_t n)
{
    T* d;
    hip_ok(hipMalloc((void**)&d, n * sizeof(T)), "hipMalloc");
    hip_ok(hipMemcpy(d, h, n * sizeof(T), hipMemcpyHostToDevice), "upload");
    return d;
}
template <class T> static void to_host(T* h, const T* d, size_t n)
{
    hip_ok(hipDeviceSynchronize(), "kernel");
    hip_ok(hipMemcpy(h, d, n * sizeof(T), hipMemcpyDeviceToHost), "download");
}

template <int BY, class K> static void run_bmax(const char* what)
{
    K ka[64 * BY], kb[64 * BY], want[3] = { 0, 0, 0 }, got[3] = { 0, 0, 0 };
    for (int i = 0; i < 64 * BY; ++i) {
        ka[i] = (K)(rng() % 1000 + 1);
        kb[i] = (K)(rng() % 1000 + 2000);               // every later key beats every earlier one: an early store would show in dst[0]
        want[0] = ka[i] > want[0] ? ka[i] : want[0];
        want[1] = kb[i] > want[1] ? kb[i] : want[1];
    }
    K *da = to_dev(ka, 64 * BY), *db = to_dev(kb, 64 * BY), *dd = to_dev(got, 3);
    hipLaunchKernelGGL((k_bmax<BY, K>), dim3(1), dim3(64, BY), 0, 0, da, db, dd);
    to_host(got, dd, 3);
    check(same_bits(got, want, 3), what);
    (void)hipFree(da); (void)hipFree(db); (void)hipFree(dd);
}

template <int N, class T> static void run_lds_scan(const char* what)
{
    static T in[N], want[N], got[N];
    for (int i = 0; i < N; ++i) in[i] = (T)((i / 64 == 5 || rng() % 3 == 0) ? 0 : rng() % 41);
    memcpy(want, in, sizeof in);
    h_lds_scan(want, N);
    T *di = to_dev(in, N), *dout = to_dev(in, N);
    hipLaunchKernelGGL((k_lds_scan<N, T>), dim3(1), dim3(N), 0, 0, di, dout);
    to_host(got, dout, N);
    check(same_bits(got, want, N), what);
    (void)hipFree(di); (void)hipFree(dout);
}

int main(int argc, char** argv)
{
    const auto add = [](double a, double b) { return a + b; };
    const auto uadd = [](unsigned a, unsigned b) { return a + b; };
    const auto imax = [](int a, int b) { return a > b ? a : b; };
    const auto kmax = [](u64 a, u64 b) { return b > a ? b : a; };

    // inputs, and the host's answers
    double d64[64], d256[256], fold[64], all[64];
    order_probe(d64, 64);
    order_probe(d256, 256);
    memcpy(fold, d64, sizeof fold); h_fold(fold, add);
    memcpy(all, d64, sizeof all); h_all(all, add);
    double rev[256];
    for (int i = 0; i < 256; ++i) rev[i] = d256[255 - i];
    const double tree_a = h_tree(d256, 256), tree_b = h_tree(rev, 256);
    // a probe whose tree gives the bits of the plain sum could not tell the orders apart
    const double seq64 = h_seq(d64, 64), seq256 = h_seq(d256, 256), seqrev = h_seq(rev, 256);
    check(!same_bits(&seq64, &fold[0], 1), "blind probe: wave tree == sequential sum");
    check(same_bits(&all[0], &fold[0], 1), "host: butterfly lane 0 != fold lane 0");
    check(!same_bits(&seq256, &tree_a, 1) && !same_bits(&seqrev, &tree_b, 1), "blind probe: block tree == sequential sum");
    if (fails) return 1;
    if (argc > 1 && !strcmp(argv[1], "host")) { printf("ok\n"); return 0; }

    // ---- one wave
    u64 keys[64], kfold[64], kall[64];
    unsigned c64[64], cscan[64], k32[64];
    int m64[64], mscan[64];
    for (int i = 0; i < 64; ++i) {
        keys[i] = ((u64)rng() << 40) ^ ((u64)rng() << 16) ^ rng();
        k32[i] = (unsigned)(keys[i] >> 32);
        m64[i] = rng() % 5 == 0 ? (int)(rng() % 100000) : -1;
    }
    counts(c64, 64, -1);
    memcpy(kfold, keys, sizeof keys); h_fold(kfold, kmax);
    memcpy(kall, keys, sizeof keys); h_all(kall, kmax);
    h_all(k32, [](unsigned a, unsigned b) { return b > a ? b : a; });
    memcpy(cscan, c64, sizeof c64); h_scan(cscan, uadd);
    memcpy(mscan, m64, sizeof m64); h_scan(mscan, imax);
    {
        WaveOut zero, got;
        memset(&zero, 0, sizeof zero);
        double* dd = to_dev(d64, 64);
        u64* dk = to_dev(keys, 64);
        unsigned* dc = to_dev(c64, 64);
        int* dm = to_dev(m64, 64);
        WaveOut* dout = to_dev(&zero, 1);
        hipLaunchKernelGGL(k_wave, dim3(1), dim3(64), 0, 0, dd, dk, dc, dm, dout);
        to_host(&got, dout, 1);
        check(same_bits(&got.fold_sum, &fold[0], 1), "wave_fold sum of doubles, lane 0");
        check(same_bits(got.all_sum, all, 64), "wave_all sum of doubles, every lane");
        check(got.fold_max == kfold[0], "wave_fold max of keys, lane 0");
        check(same_bits(got.max64, kall, 64), "wave_max of 64-bit keys");
        check(same_bits(got.max32, k32, 64), "wave_max of 32-bit keys");
        check(same_bits(got.scan_add, cscan, 64), "wave_scan +");
        check(same_bits(got.scan_max, mscan, 64), "wave_scan max");
        (void)hipFree(dd); (void)hipFree(dk); (void)hipFree(dc); (void)hipFree(dm); (void)hipFree(dout);
    }

    // ---- one workgroup of four waves
    {
        unsigned c[256], want_add[256], part[4];
        int m[256], want_max[256], parti[4];
        counts(c, 256, 2);
        for (int i = 0; i < 256; ++i) m[i] = rng() % 7 == 0 ? i : -1;      // k_ccl_init's use: the last break at or before me
        memcpy(want_add, c, sizeof c); h_block_scan(want_add, 4, part, uadd);
        memcpy(want_max, m, sizeof m); h_block_scan(want_max, 4, parti, imax);
        BlockOut zero, got;
        memset(&zero, 0, sizeof zero);
        unsigned* dc = to_dev(c, 256);
        int* dm = to_dev(m, 256);
        double* dd = to_dev(d256, 256);
        BlockOut* dout = to_dev(&zero, 1);
        hipLaunchKernelGGL(k_block, dim3(1), dim3(256), 0, 0, dc, dm, dd, dout);
        to_host(&got, dout, 1);
        check(same_bits(got.scan_add, want_add, 256), "block_scan +");
        check(same_bits(got.part, part, 4), "block_scan's wave totals");
        check(same_bits(got.scan_max, want_max, 256), "block_scan max");
        check(same_bits(&got.tree_a, &tree_a, 1) && same_bits(&got.tree_b, &tree_b, 1), "block_tree, two arrays");
        (void)hipFree(dc); (void)hipFree(dm); (void)hipFree(dd); (void)hipFree(dout);
    }
    run_lds_scan<1024, unsigned>("lds_scan<1024>");
    run_lds_scan<256, int>("lds_scan<256>");
    run_bmax<1, unsigned>("block_max<1>, twice");
    run_bmax<4, u64>("block_max<4>, twice");

    // ---- keys: round trip, order, and the two reserved keys
    {
        const int n = 10;
        const float f[n] = { -INFINITY, -FLT_MAX, -FLT_MIN, -0x1p-149f, -0.0f, 0.0f, 0x1p-149f, FLT_MIN, FLT_MAX, INFINITY };
        const double d[n] = { -INFINITY, -DBL_MAX, -DBL_MIN, -0x1p-1074, -0.0, 0.0, 0x1p-1074, DBL_MIN, DBL_MAX, INFINITY };
        unsigned kf[n];
        u64 kd[n];
        float rf[n];
        double rd[n];
        float* df = to_dev(f, n);
        double* dd = to_dev(d, n);
        unsigned* dkf = to_dev(kf, n);
        u64* dkd = to_dev(kd, n);
        float* drf = to_dev(rf, n);
        double* drd = to_dev(rd, n);
        hipLaunchKernelGGL(k_keys, dim3(1), dim3(64), 0, 0, df, dd, n, dkf, dkd, drf, drd);
        to_host(kf, dkf, n); to_host(kd, dkd, n); to_host(rf, drf, n); to_host(rd, drd, n);
        check(same_bits(rf, f, n) && same_bits(rd, d, n), "order_unkey(order_key(v)) on the device");
        for (int i = 0; i < n; ++i) {
            const float hf = order_unkey(kf[i]);
            const double hd = order_unkey(kd[i]);
            check(same_bits(&hf, &f[i], 1) && same_bits(&hd, &d[i], 1), "order_unkey on the host");
            check(kf[i] != 0u && kf[i] != ~0u && kd[i] != 0ull && kd[i] != ~0ull, "a finite value or infinity has a reserved key");
            if (i) check(kf[i] > kf[i - 1] && kd[i] > kd[i - 1], "keys do not order like their values");
        }
        (void)hipFree(df); (void)hipFree(dd); (void)hipFree(dkf); (void)hipFree(dkd); (void)hipFree(drf); (void)hipFree(drd);
    }
    if (fails) return 1;
    printf("ok\n");
    return 0;
}
