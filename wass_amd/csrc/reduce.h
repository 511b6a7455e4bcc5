// reduce.h -- the reductions and scans of the kernels, each shape written once.  Nearly every kernel here is tested bit for bit against
// an oracle that folds in the same order, so the order stated below is part of every caller's specification; the oracles in tests/
// cite it.  Device code only: no state, no macros, nothing of common.h (which includes this file).  A wave is 64 lanes, and every
// form indexes by threadIdx.x alone.
// What stays outside on purpose, and is no unfinished work:
//   - wave_min_u32 / wave_min2_u32 (common.h): the DPP forms of the SGM chain kernels;
//   - sgm_step.h, sgm_cost.hip, sgm_select.hip and the chain kernels of sgm_aggregate.hip: their dpp_mov calls move data inside the
//     recurrence and reduce nothing;
//   - the sequential branch of match.hip's wave_sum_f64: lane by lane is the reference's own order;
//   - the __ballot / __popcll compaction of mesh.hip (xyzc_pack_body, k_inlier_pack), __syncthreads_count, and k_ccl_count's
//     __shfl_up(r, 1), which reads the neighbour lane and scans nothing;
//   - the fixed sums across four waves (block_sum_store's ((s0+s1)+s2)+s3, k_dct_recon's part[0]+..+part[3]): written out where they
//     stand, the parenthesisation is the specification;
//   - loops of these very shapes that keep their own text because the kernel compiled to other instructions when it called this
//     header (other registers and schedule, the same values), and the kernels of the frame tail are held to the instruction:
//     in mesh.hip k_ransac_score (a butterfly over six values), k_ransac_pick, block_sum_store's wave sums (k_refine_cov_dev),
//     k_inl_text_format's scan, k_scan_blocks, the key folds of k_crop_limits_counts_dev and k_frame_header;
//     epipolar.hip's k_epi_best (block_tree cost it a register and six instructions); match.hip's arg-max butterfly in
//     k_match_iidyn (two (value, index) pairs folded at once: no operation on one value); and the carry of jpeg.hip's
//     block_excl_scan, which takes prefix and total in one pass over the waves (block_scan cost its kernels thirty instructions).
#pragma once

#include <hip/hip_runtime.h>

namespace wass {

// ---------------------------------------------------------------- keys
// An unsigned key that orders like the number it was made from (-0 below +0).  No finite number or infinity has key 0 or ~0: the
// callers keep those for "nothing seen".  Only NaNs with every mantissa bit set land there, and the callers keep NaN out.
__device__ __forceinline__ unsigned order_key(float v)
{
    const unsigned b = __float_as_uint(v);
    return (b >> 31) ? ~b : (b | 0x80000000u);
}

__device__ __forceinline__ unsigned long long order_key(double v)
{
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

__host__ __device__ __forceinline__ float order_unkey(unsigned k)
{
    return __builtin_bit_cast(float, (k >> 31) ? (k & 0x7fffffffu) : ~k);
}

__host__ __device__ __forceinline__ double order_unkey(unsigned long long k)
{
    return __builtin_bit_cast(double, (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k);
}

// ---------------------------------------------------------------- one wave
// No barrier, no LDS; all 64 lanes must be active.  op(own, other) takes the calling lane's value first.

// Fold towards lane 0: for o = 32, 16, .. 1: v = op(v, v of lane + o).  With S32(l) = v_l . v_(l+32) and So(l) = S2o(l) . S2o(l + o),
// lane 0 returns S1(0) = ((((S32(0) . S32(16)) . (S32(8) . S32(24))) . ..) . (.. S32(1) ..)): a balanced tree, larger strides inside.
// Only lane 0's result is complete (a lane whose partner lies past lane 63 is handed its own value).
template <class T, class F> __device__ __forceinline__ T wave_fold(T v, F op)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = op(v, __shfl_down(v, o));
    return v;
}

// Butterfly: for o = 32, 16, .. 1: v = op(v, v of lane ^ o).  The tree of wave_fold seen from every lane: with an operation that
// commutes bit for bit (+, min, max of numbers) all 64 lanes return what lane 0 of wave_fold returns.
template <class T, class F> __device__ __forceinline__ T wave_all(T v, F op)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = op(v, __shfl_xor(v, o));
    return v;
}

// Inclusive scan (Kogge-Stone): for o = 1, 2, .. 32: lanes >= o take v = op(v, value of lane - o).  Lane l returns the fold of lanes
// 0 .. l, associated as that doubling makes it; lane 63 returns the wave's total.
template <class T, class F> __device__ __forceinline__ T wave_scan(T v, F op)
{
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const T t = __shfl_up(v, o);
        if (lane >= o) v = op(v, t);
    }
    return v;
}

// The largest key in every lane.
template <class K> __device__ __forceinline__ K wave_max(K k)
{
    return wave_all(k, [](K a, K b) { return b > a ? b : a; });
}

// ---------------------------------------------------------------- one workgroup
// Inclusive scan over a block of whole waves (at most as many as `part` has entries): wave_scan, lane 63 of wave w stores its value
// in part[w], ONE barrier, then thread t of wave w returns op(.. op(op(own, part[0]), part[1]) .., part[w - 1]).  After the call
// part[] holds the waves' totals for the caller to read; the barrier before part[] is written again is the caller's.
template <class T, class F> __device__ __forceinline__ T block_scan(T v, T* part, F op)
{
    v = wave_scan(v, op);
    const int wv = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 63) part[wv] = v;
    __syncthreads();
    for (int k = 0; k < wv; ++k) v = op(v, part[k]);
    return v;
}

// Tree over N threads (N a power of two, the block's size): for o = N/2, N/4, .. 1: threads t < o call merge(t, t + o), then ONE
// barrier per level, the last level included.  merge folds the caller's LDS element(s) t + o into t, so element 0 ends as
// ((e0 . eN/2) . (eN/4 . e3N/4)) . ..., the order of wave_fold widened to N.  The caller fills its arrays and barriers before the
// call; any thread may read element 0 right after it.  A caller that fills the arrays again needs a barrier of its own first.
template <int N, class F> __device__ __forceinline__ void block_tree(F merge)
{
    for (int o = N / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) merge((int)threadIdx.x, (int)threadIdx.x + o);
        __syncthreads();
    }
}

// The sum of a block of N doubles in every thread: sh[t] = v, a barrier, block_tree with +=, and a barrier after the read so that sh
// can be filled again at once.
template <int N> __device__ __forceinline__ double block_sum(double v, double* sh)
{
    sh[threadIdx.x] = v;
    __syncthreads();
    block_tree<N>([&](int t, int u) { sh[t] += sh[u]; });
    const double r = sh[0];
    __syncthreads();
    return r;
}

// Inclusive prefix sum of a[0 .. N) in LDS by N threads (Hillis-Steele): for o = 1, 2, .. N/2: thread t reads a[t - o] (0 for t < o),
// barrier, a[t] += that, barrier.  Element t ends as the doubling order makes it (integers here: the order cannot show).  The
// caller barriers between filling a[] and the call; the call ends with a barrier, so any thread may read any element after it.
template <int N, class T> __device__ __forceinline__ void lds_scan(T* a)
{
    const int t = threadIdx.x;
    for (int o = 1; o < N; o <<= 1) {
        const T v = t >= o ? a[t - o] : T(0);
        __syncthreads();
        a[t] += v;
        __syncthreads();
    }
}

// The largest key of a block of 64 x BY threads into *dst (0 = nothing seen, and nothing is written): wave_max, a barrier FIRST
// (`part` may still be read by an earlier call: a kernel may call this more than once), lane 0 of each wave stores, a barrier, then
// thread (0, 0) takes the waves in order and makes one atomicMax.  Every thread of the block calls it.
template <int BY, class K> __device__ __forceinline__ void block_max(K k, K* dst)
{
    __shared__ K part[BY];
    k = wave_max(k);
    __syncthreads();
    if (threadIdx.x == 0) part[threadIdx.y] = k;
    __syncthreads();
    if (threadIdx.x == 0 && threadIdx.y == 0) {
#pragma unroll
        for (int w = 1; w < BY; ++w) k = part[w] > k ? part[w] : k;
        if (k) atomicMax(dst, k);
    }
}

}  // namespace wass
