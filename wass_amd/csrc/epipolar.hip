// epipolar.hip -- the essential-matrix filter of wass_match (src/wass_match/wass_match.cpp:250-358): cv::findEssentialMat's RANSAC as
// one chain of launches over every hypothesis of every pair of pictures.  See include/wass_gpu.h ("Essential-matrix filter").
//
//   k_epi_solve5   one sample of five matches -> up to ten essential matrices (Nister 2004, the degree-10 polynomial in z), one
//                  hypothesis per thread, workgroups of 64, the 10 x 20 constraint matrix in LDS with the lane as the minor index
//   k_epi_score    squared Sampson distance of every model to every match, exact int32 inlier counts (integer atomics)
//   k_epi_best     the largest count of a pair, ties to the lowest model index
//   k_epi_mask     inlier mask and err of one model per pair
//
// All fp64, compiled without contraction.  A lane of k_epi_solve5 touches only its own column of the LDS array, so the kernel
// has no barrier.  The solver's arithmetic is one __host__ __device__ function: the same source can be run on a CPU.
#include "common.h"

#include <math.h>
#include <utility>
#include <vector>

#define EPI_HD __host__ __device__ __forceinline__

namespace wass {

constexpr int EPI_LANES = 64;
constexpr int EPI_SOL = WASS_EPI_MAX_SOL;
constexpr int EPI_LDS_DOUBLES = 200;         // per lane: the 10 x 20 matrix; everything else the solver keeps in LDS reuses it
constexpr int EPI_BISECT = 100;              // halvings of an interval inside [-1, 1]: below 2^-100, or until no double lies between
constexpr int EPI_POLISH = 3;                // Gauss-Newton steps on the ten cubic constraints
constexpr int SCORE_THREADS = 256;           // models per workgroup of k_epi_score
constexpr int SCORE_TILE = 256;              // matches per workgroup of k_epi_score

enum : int { EPI_BAD_INDEX = 1 };

// ------------------------------------------------------------------------------------------------------------ monomial tables
// E = x X + y Y + z Z + W: an entry of E is a polynomial of degree 1 in (x, y, z), products of two and three entries have 10 and
// 20 coefficients.  The degree-3 order is the column order of the 10 x 20 matrix (Nister 2004, section 3.2): the first ten are
// eliminated, the last ten are x, y and 1 times powers of z.
struct Mono { int x, y, z; };
constexpr Mono EPI_M1[4] = { {1, 0, 0}, {0, 1, 0}, {0, 0, 1}, {0, 0, 0} };
constexpr Mono EPI_M2[10] = { {2, 0, 0}, {1, 1, 0}, {1, 0, 1}, {0, 2, 0}, {0, 1, 1}, {0, 0, 2}, {1, 0, 0}, {0, 1, 0}, {0, 0, 1}, {0, 0, 0} };
constexpr Mono EPI_M3[20] = { {3, 0, 0}, {0, 3, 0}, {2, 1, 0}, {1, 2, 0}, {2, 0, 1}, {2, 0, 0}, {0, 2, 1}, {0, 2, 0}, {1, 1, 1}, {1, 1, 0},
                              {1, 0, 2}, {1, 0, 1}, {1, 0, 0}, {0, 1, 2}, {0, 1, 1}, {0, 1, 0}, {0, 0, 3}, {0, 0, 2}, {0, 0, 1}, {0, 0, 0} };

constexpr int mono_find(const Mono* list, int n, Mono a, Mono b)
{
    for (int k = 0; k < n; ++k)
        if (list[k].x == a.x + b.x && list[k].y == a.y + b.y && list[k].z == a.z + b.z) return k;
    return -1;
}
template <int I, int J> constexpr int EPI_T2 = mono_find(EPI_M2, 10, EPI_M1[I], EPI_M1[J]);     // degree 1 x degree 1
template <int I, int J> constexpr int EPI_T3 = mono_find(EPI_M3, 20, EPI_M2[I], EPI_M1[J]);     // degree 2 x degree 1

// out += a * b (or -=), every index a compile-time constant: the arrays stay in registers
template <bool NEG, int... K>
EPI_HD void pmul11_seq(const double* a, const double* b, double* out, std::integer_sequence<int, K...>)
{
    static_assert(((EPI_T2<K / 4, K % 4> >= 0) && ...), "monomial table");
    if (NEG) ((out[EPI_T2<K / 4, K % 4>] -= a[K / 4] * b[K % 4]), ...);
    else ((out[EPI_T2<K / 4, K % 4>] += a[K / 4] * b[K % 4]), ...);
}
template <bool NEG> EPI_HD void pmul11(const double* a, const double* b, double* out) { pmul11_seq<NEG>(a, b, out, std::make_integer_sequence<int, 16>{}); }

template <bool NEG, int... K>
EPI_HD void pmul21_seq(const double* a, const double* b, double* out, std::integer_sequence<int, K...>)
{
    static_assert(((EPI_T3<K / 4, K % 4> >= 0) && ...), "monomial table");
    if (NEG) ((out[EPI_T3<K / 4, K % 4>] -= a[K / 4] * b[K % 4]), ...);
    else ((out[EPI_T3<K / 4, K % 4>] += a[K / 4] * b[K % 4]), ...);
}
template <bool NEG> EPI_HD void pmul21(const double* a, const double* b, double* out) { pmul21_seq<NEG>(a, b, out, std::make_integer_sequence<int, 40>{}); }

// ------------------------------------------------------------------------------------------------------------------- scoring
// The squared Sampson distance of one match to one model, in the operation order include/wass_gpu.h states; E is row-major.
EPI_HD float epi_err(const double* E, double ax, double ay, double bx, double by)
{
    const double l0 = (E[0] * ax + E[1] * ay) + E[2];        // E x0
    const double l1 = (E[3] * ax + E[4] * ay) + E[5];
    const double l2 = (E[6] * ax + E[7] * ay) + E[8];
    const double r0 = (E[0] * bx + E[3] * by) + E[6];        // E' x1
    const double r1 = (E[1] * bx + E[4] * by) + E[7];
    const double num = (bx * l0 + by * l1) + l2;
    const double den = ((l0 * l0 + l1 * l1) + r0 * r0) + r1 * r1;
    return (float)((num * num) / den);
}

// --------------------------------------------------------------------------------------------------------------- small 3 x 3
EPI_HD void m3_mul(const double* A, const double* B, double* C)          // C = A B
{
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) C[3 * i + j] = (A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j]) + A[3 * i + 2] * B[6 + j];
}
EPI_HD void m3_mul_t(const double* A, const double* B, double* C)        // C = A B'
{
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) C[3 * i + j] = (A[3 * i] * B[3 * j] + A[3 * i + 1] * B[3 * j + 1]) + A[3 * i + 2] * B[3 * j + 2];
}
EPI_HD void m3_cof(const double* E, double* Cf)                          // cofactors: det E = sum_j E[0][j] Cf[0][j]
{
    Cf[0] = E[4] * E[8] - E[5] * E[7]; Cf[1] = E[5] * E[6] - E[3] * E[8]; Cf[2] = E[3] * E[7] - E[4] * E[6];
    Cf[3] = E[2] * E[7] - E[1] * E[8]; Cf[4] = E[0] * E[8] - E[2] * E[6]; Cf[5] = E[1] * E[6] - E[0] * E[7];
    Cf[6] = E[1] * E[5] - E[2] * E[4]; Cf[7] = E[2] * E[3] - E[0] * E[5]; Cf[8] = E[0] * E[4] - E[1] * E[3];
}

// the ten cubic constraints at E: r[0..8] = 2 E E' E - tr(E E') E, r[9] = det E; A = E E' and the cofactors are handed back
EPI_HD void epi_residual(const double* E, double* r, double* A, double* Cf)
{
    m3_mul_t(E, E, A);
    double AE[9];
    m3_mul(A, E, AE);
    const double tr = (A[0] + A[4]) + A[8];
#pragma unroll
    for (int k = 0; k < 9; ++k) r[k] = 2.0 * AE[k] - tr * E[k];
    m3_cof(E, Cf);
    r[9] = (E[0] * Cf[0] + E[1] * Cf[1]) + E[2] * Cf[2];
}

EPI_HD void epi_compose(const double (&b)[4][9], double x, double y, double z, double* E)
{
#pragma unroll
    for (int k = 0; k < 9; ++k) E[k] = ((x * b[0][k] + y * b[1][k]) + z * b[2][k]) + b[3][k];
}

EPI_HD double sumsq10(const double* r)
{
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < 10; ++k) s += r[k] * r[k];
    return s;
}

// Gauss-Newton on the ten constraints in (x, y, z), from a root of the degree-10 polynomial: the polynomial's own conditioning
// (an elimination and a determinant of polynomials) is left behind, what remains is the conditioning of the solution itself.
// A step is kept only where it is finite and does not raise the residual.
EPI_HD void epi_polish(const double (&b)[4][9], double& x, double& y, double& z)
{
    double E[9], r[10], A[9], Cf[9];
    epi_compose(b, x, y, z, E);
    epi_residual(E, r, A, Cf);
    double cost = sumsq10(r);
    for (int it = 0; it < EPI_POLISH; ++it) {
        double J[3][10];
        const double tr = (A[0] + A[4]) + A[8];
#pragma unroll
        for (int v = 0; v < 3; ++v) {
            const double* D = b[v];
            double DEt[9], dA[9], t1[9], t2[9];
            m3_mul_t(D, E, DEt);
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 3; ++j) dA[3 * i + j] = DEt[3 * i + j] + DEt[3 * j + i];
            m3_mul(dA, E, t1);
            m3_mul(A, D, t2);
            const double dtr = (dA[0] + dA[4]) + dA[8];
            double dd = 0.0;
#pragma unroll
            for (int k = 0; k < 9; ++k) {
                J[v][k] = (2.0 * (t1[k] + t2[k]) - dtr * E[k]) - tr * D[k];
                dd += Cf[k] * D[k];
            }
            J[v][9] = dd;
        }
        double N[3][3], g[3];
#pragma unroll
        for (int u = 0; u < 3; ++u) {
#pragma unroll
            for (int v = 0; v < 3; ++v) {
                double s = 0.0;
#pragma unroll
                for (int k = 0; k < 10; ++k) s += J[u][k] * J[v][k];
                N[u][v] = s;
            }
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < 10; ++k) s += J[u][k] * r[k];
            g[u] = s;
        }
        const double c00 = N[1][1] * N[2][2] - N[1][2] * N[2][1], c01 = N[1][2] * N[2][0] - N[1][0] * N[2][2],
                     c02 = N[1][0] * N[2][1] - N[1][1] * N[2][0];
        const double det = (N[0][0] * c00 + N[0][1] * c01) + N[0][2] * c02;
        const double c11 = N[0][0] * N[2][2] - N[0][2] * N[2][0], c12 = N[0][1] * N[2][0] - N[0][0] * N[2][1],
                     c22 = N[0][0] * N[1][1] - N[0][1] * N[1][0];
        const double dx = ((c00 * g[0] + c01 * g[1]) + c02 * g[2]) / det;      // N is symmetric: its inverse is the cofactors over det
        const double dy = ((c01 * g[0] + c11 * g[1]) + c12 * g[2]) / det;
        const double dz = ((c02 * g[0] + c12 * g[1]) + c22 * g[2]) / det;
        const double nx = x - dx, ny = y - dy, nz = z - dz;
        double E2[9], r2[10], A2[9], Cf2[9];
        epi_compose(b, nx, ny, nz, E2);
        epi_residual(E2, r2, A2, Cf2);
        const double cost2 = sumsq10(r2);
        if (!(cost2 <= cost)) break;                         // NaN included
        x = nx; y = ny; z = nz; cost = cost2;
#pragma unroll
        for (int k = 0; k < 9; ++k) { E[k] = E2[k]; A[k] = A2[k]; Cf[k] = Cf2[k]; }
#pragma unroll
        for (int k = 0; k < 10; ++k) r[k] = r2[k];
    }
}

// ---------------------------------------------------------------------------------------------------------------- real roots
constexpr double epi_binom(int n, int k)
{
    double r = 1.0;
    for (int i = 1; i <= k; ++i) r = r * (double)(n - k + i) / (double)i;
    return r;
}
template <int N, int K> constexpr double EPI_BINOM = epi_binom(N, K);

// q = p^(10 - D) / (10 - D)!: coefficient k is C(k + 10 - D, k) c[k + 10 - D]
template <int D, int... K> EPI_HD void epi_derivative(const double (&c)[11], double (&q)[D + 1], std::integer_sequence<int, K...>)
{
    ((q[K] = EPI_BINOM<K + 10 - D, K> * c[K + 10 - D]), ...);
}

template <int D> EPI_HD double horner(const double (&q)[D + 1], double t)
{
    double s = q[D];
#pragma unroll
    for (int k = D - 1; k >= 0; --k) s = s * t + q[k];
    return s;
}

// The real roots in [-1, 1] of q = p^(10 - D) / (10 - D)!, a polynomial of degree D, from those of its derivative (`prev`, ascending):
// between two neighbouring critical points q is monotonic, so a change of sign brackets exactly one root, found by bisection.
template <int D, int LS> EPI_HD int epi_level(const double (&c)[11], const double* prev, int nprev, double* next)
{
    double q[D + 1];
    epi_derivative<D>(c, q, std::make_integer_sequence<int, D + 1>{});
    double lo = -1.0, flo = horner<D>(q, lo);
    int n = 0;
    for (int i = 0; i <= nprev; ++i) {
        const double hi = i < nprev ? prev[i * LS] : 1.0;
        const double fhi = horner<D>(q, hi);
        if ((flo < 0.0) != (fhi < 0.0)) {
            double a = lo, bb = hi;
            const bool neg = flo < 0.0;
            for (int it = 0; it < EPI_BISECT; ++it) {
                const double m = 0.5 * (a + bb);
                if (!(m > a && m < bb)) break;
                if ((horner<D>(q, m) < 0.0) == neg) a = m;
                else bb = m;
            }
            next[n * LS] = 0.5 * (a + bb);
            ++n;
        }
        lo = hi;
        flo = fhi;
    }
    return n;
}

// the real roots of c[0] + c[1] t + ... + c[10] t^10 in [-1, 1], ascending, into A (A and B: ten slots each); returns their number
template <int LS> EPI_HD int epi_roots_unit(const double (&c)[11], double* A, double* B)
{
    int n = epi_level<1, LS>(c, A, 0, B);
    n = epi_level<2, LS>(c, B, n, A);
    n = epi_level<3, LS>(c, A, n, B);
    n = epi_level<4, LS>(c, B, n, A);
    n = epi_level<5, LS>(c, A, n, B);
    n = epi_level<6, LS>(c, B, n, A);
    n = epi_level<7, LS>(c, A, n, B);
    n = epi_level<8, LS>(c, B, n, A);
    n = epi_level<9, LS>(c, A, n, B);
    return epi_level<10, LS>(c, B, n, A);
}

template <int NA, int NB> EPI_HD void pmul_z(const double (&a)[NA], const double (&b)[NB], double (&out)[NA + NB - 1], bool neg)
{
#pragma unroll
    for (int i = 0; i < NA; ++i)
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            const double t = a[i] * b[j];
            out[i + j] = neg ? out[i + j] - t : out[i + j] + t;
        }
}

// ------------------------------------------------------------------------------------------------------------------- solver
// The five-point problem of one sample.  q0, q1: the five matches (normalised coordinates, x1' E x0 = 0).  sm: this lane's 200
// doubles, element i at sm[i * LS].  Eout: ten row-major 3 x 3 slots; the first `return value` hold the solutions, scaled to
// Frobenius norm 1, by ascending z; the others are zero.
template <int LS> EPI_HD int epi_solve5_core(const double (&q0)[5][2], const double (&q1)[5][2], double* sm, double* Eout)
{
#pragma unroll 1
    for (int k = 0; k < EPI_SOL * 9; ++k) Eout[k] = 0.0;
    // ---- the 5 x 9 constraint matrix: row i = x1_i (x) x0_i over the row-major entries of E; columns tracked in 45..53
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        const double a[3] = { q0[i][0], q0[i][1], 1.0 }, bq[3] = { q1[i][0], q1[i][1], 1.0 };
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int cc = 0; cc < 3; ++cc) sm[(i * 9 + 3 * r + cc) * LS] = bq[r] * a[cc];
    }
    for (int k = 0; k < 9; ++k) sm[(45 + k) * LS] = (double)k;
    // ---- its null space: Gauss-Jordan with complete pivoting leaves [I | N], the basis is (-N; I) in the permuted columns
    for (int cc = 0; cc < 5; ++cc) {
        int pr = cc, pc = cc;
        double best = -1.0;
        for (int r = cc; r < 5; ++r)
            for (int k = cc; k < 9; ++k) {
                const double v = fabs(sm[(r * 9 + k) * LS]);
                if (v > best) { best = v; pr = r; pc = k; }
            }
        if (!(best > 0.0) || !isfinite(best)) return 0;
        if (pr != cc)
            for (int k = 0; k < 9; ++k) {
                const double t = sm[(cc * 9 + k) * LS];
                sm[(cc * 9 + k) * LS] = sm[(pr * 9 + k) * LS];
                sm[(pr * 9 + k) * LS] = t;
            }
        if (pc != cc)
            for (int r = 0; r < 6; ++r) {                    // row 5 is the column record
                const double t = sm[(r * 9 + cc) * LS];
                sm[(r * 9 + cc) * LS] = sm[(r * 9 + pc) * LS];
                sm[(r * 9 + pc) * LS] = t;
            }
        const double piv = sm[(cc * 9 + cc) * LS];
        for (int k = cc; k < 9; ++k) sm[(cc * 9 + k) * LS] /= piv;
        for (int r = 0; r < 5; ++r) {
            if (r == cc) continue;
            const double f = sm[(r * 9 + cc) * LS];
            for (int k = cc; k < 9; ++k) sm[(r * 9 + k) * LS] -= f * sm[(cc * 9 + k) * LS];
        }
    }
    for (int k = 0; k < 36; ++k) sm[(60 + k) * LS] = 0.0;
    for (int j = 0; j < 4; ++j) {
        for (int i = 0; i < 5; ++i) sm[(60 + j * 9 + (int)sm[(45 + i) * LS]) * LS] = -sm[(i * 9 + 5 + j) * LS];
        sm[(60 + j * 9 + (int)sm[(45 + 5 + j) * LS]) * LS] = 1.0;
    }
    double b[4][9];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int k = 0; k < 9; ++k) b[j][k] = sm[(60 + j * 9 + k) * LS];
    // modified Gram-Schmidt, twice: an orthonormal X, Y, Z, W
#pragma unroll
    for (int pass = 0; pass < 2; ++pass)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
#pragma unroll
            for (int i = 0; i < j; ++i) {
                double d = 0.0;
#pragma unroll
                for (int k = 0; k < 9; ++k) d += b[i][k] * b[j][k];
#pragma unroll
                for (int k = 0; k < 9; ++k) b[j][k] -= d * b[i][k];
            }
            double nn = 0.0;
#pragma unroll
            for (int k = 0; k < 9; ++k) nn += b[j][k] * b[j][k];
            nn = sqrt(nn);
            if (!(nn > 0.0) || !isfinite(nn)) return 0;
#pragma unroll
            for (int k = 0; k < 9; ++k) b[j][k] /= nn;
        }
    // ---- the ten cubic constraints on E = x X + y Y + z Z + W: 2 E E' E - tr(E E') E = 0 (rows 0..8) and det E = 0 (row 9)
    {
        double e[9][4];
#pragma unroll
        for (int k = 0; k < 9; ++k)
#pragma unroll
            for (int v = 0; v < 4; ++v) e[k][v] = b[v][k];
        double L[6][10];                                     // E E' - tr(E E') / 2 I: 00 01 02 11 12 22
        constexpr int SI[6] = { 0, 0, 0, 1, 1, 2 }, SJ[6] = { 0, 1, 2, 1, 2, 2 };
#pragma unroll
        for (int s = 0; s < 6; ++s) {
#pragma unroll
            for (int m = 0; m < 10; ++m) L[s][m] = 0.0;
#pragma unroll
            for (int k = 0; k < 3; ++k) pmul11<false>(e[3 * SI[s] + k], e[3 * SJ[s] + k], L[s]);
        }
#pragma unroll
        for (int m = 0; m < 10; ++m) {
            const double h = 0.5 * ((L[0][m] + L[3][m]) + L[5][m]);
            L[0][m] -= h; L[3][m] -= h; L[5][m] -= h;
        }
        constexpr int SYM[3][3] = { { 0, 1, 2 }, { 1, 3, 4 }, { 2, 4, 5 } };
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                double row[20];
#pragma unroll
                for (int m = 0; m < 20; ++m) row[m] = 0.0;
#pragma unroll
                for (int k = 0; k < 3; ++k) pmul21<false>(L[SYM[i][k]], e[3 * k + j], row);
#pragma unroll
                for (int m = 0; m < 20; ++m) sm[((3 * i + j) * 20 + m) * LS] = row[m];
            }
        double row[20], mn[10];
#pragma unroll
        for (int m = 0; m < 20; ++m) row[m] = 0.0;
        constexpr int CA[3] = { 4, 5, 3 }, CB[3] = { 8, 6, 7 }, CC[3] = { 5, 3, 4 }, CD[3] = { 7, 8, 6 };       // cofactors of row 0
#pragma unroll
        for (int j = 0; j < 3; ++j) {
#pragma unroll
            for (int m = 0; m < 10; ++m) mn[m] = 0.0;
            pmul11<false>(e[CA[j]], e[CB[j]], mn);
            pmul11<true>(e[CC[j]], e[CD[j]], mn);
            pmul21<false>(mn, e[j], row);
        }
#pragma unroll
        for (int m = 0; m < 20; ++m) sm[(180 + m) * LS] = row[m];
    }
    // ---- Gauss-Jordan with partial pivoting on the first ten columns
    for (int cc = 0; cc < 10; ++cc) {
        int pr = cc;
        double best = -1.0;
        for (int r = cc; r < 10; ++r) {
            const double v = fabs(sm[(r * 20 + cc) * LS]);
            if (v > best) { best = v; pr = r; }
        }
        if (!(best > 0.0) || !isfinite(best)) return 0;
        if (pr != cc)
            for (int k = cc; k < 20; ++k) {
                const double t = sm[(cc * 20 + k) * LS];
                sm[(cc * 20 + k) * LS] = sm[(pr * 20 + k) * LS];
                sm[(pr * 20 + k) * LS] = t;
            }
        const double piv = sm[(cc * 20 + cc) * LS];
        for (int k = cc + 1; k < 20; ++k) sm[(cc * 20 + k) * LS] /= piv;
        for (int r = 0; r < 10; ++r) {
            if (r == cc) continue;
            const double f = sm[(r * 20 + cc) * LS];
            for (int k = cc + 1; k < 20; ++k) sm[(r * 20 + k) * LS] -= f * sm[(cc * 20 + k) * LS];
        }
    }
    // ---- rows e..j (leading x^2 z, x^2, y^2 z, y^2, x y z, x y): e - z f, g - z h, i - z j are [x y 1] times polynomials in z
    double Bx[3][4], By[3][4], Bc[3][5];
#pragma unroll
    for (int t = 0; t < 3; ++t) {
        double er[10], fr[10];
#pragma unroll
        for (int k = 0; k < 10; ++k) {
            er[k] = sm[((4 + 2 * t) * 20 + 10 + k) * LS];
            fr[k] = sm[((5 + 2 * t) * 20 + 10 + k) * LS];
        }
        Bx[t][0] = er[2]; Bx[t][1] = er[1] - fr[2]; Bx[t][2] = er[0] - fr[1]; Bx[t][3] = -fr[0];
        By[t][0] = er[5]; By[t][1] = er[4] - fr[5]; By[t][2] = er[3] - fr[4]; By[t][3] = -fr[3];
        Bc[t][0] = er[9]; Bc[t][1] = er[8] - fr[9]; Bc[t][2] = er[7] - fr[8]; Bc[t][3] = er[6] - fr[7]; Bc[t][4] = -fr[6];
    }
    double c[11];
    {
#pragma unroll
        for (int k = 0; k < 11; ++k) c[k] = 0.0;
        constexpr int R1[3] = { 1, 0, 0 }, R2[3] = { 2, 2, 1 };
#pragma unroll
        for (int t = 0; t < 3; ++t) {
            double mnr[7];
#pragma unroll
            for (int k = 0; k < 7; ++k) mnr[k] = 0.0;
            pmul_z<4, 4>(Bx[R1[t]], By[R2[t]], mnr, false);
            pmul_z<4, 4>(Bx[R2[t]], By[R1[t]], mnr, true);
            pmul_z<5, 7>(Bc[t], mnr, c, t == 1);
        }
        double big = 0.0;
#pragma unroll
        for (int k = 0; k < 11; ++k) big = fabs(c[k]) > big ? fabs(c[k]) : big;
        if (!(big > 0.0) || !isfinite(big)) return 0;
#pragma unroll
        for (int k = 0; k < 11; ++k) c[k] /= big;
    }
    // ---- real roots: z in [-1, 1] from the polynomial, |z| > 1 as 1 / u from the reversed polynomial; sorted by z into 20..39
    double* zl = sm + 20 * LS;
    int nz = 0;
#pragma unroll 1
    for (int pass = 0; pass < 2; ++pass) {
        const int n = epi_roots_unit<LS>(c, sm, sm + 10 * LS);
        for (int i = 0; i < n; ++i) {
            double z = sm[i * LS];
            if (pass) {
                if (z == 0.0) continue;
                z = 1.0 / z;
            }
            int at = nz;
            while (at > 0 && zl[(at - 1) * LS] > z) {
                zl[at * LS] = zl[(at - 1) * LS];
                --at;
            }
            zl[at * LS] = z;
            ++nz;
        }
#pragma unroll
        for (int k = 0; k < 5; ++k) { const double t = c[k]; c[k] = c[10 - k]; c[10 - k] = t; }
    }
    // ---- back-substitution: [x y 1] spans the null space of B(z); the cross product of the two rows that give the longest one
    int nsol = 0;
    for (int i = 0; i < nz && nsol < EPI_SOL; ++i) {
        const double z = zl[i * LS];
        double Bz[3][3];
#pragma unroll
        for (int t = 0; t < 3; ++t) {
            Bz[t][0] = horner<3>(Bx[t], z);
            Bz[t][1] = horner<3>(By[t], z);
            Bz[t][2] = horner<4>(Bc[t], z);
        }
        double v[3] = { 0.0, 0.0, 0.0 }, vn = -1.0;
        constexpr int PA[3] = { 0, 0, 1 }, PB[3] = { 1, 2, 2 };
#pragma unroll
        for (int t = 0; t < 3; ++t) {
            const double* r = Bz[PA[t]];
            const double* s = Bz[PB[t]];
            const double w0 = r[1] * s[2] - r[2] * s[1], w1 = r[2] * s[0] - r[0] * s[2], w2 = r[0] * s[1] - r[1] * s[0];
            const double wn = (w0 * w0 + w1 * w1) + w2 * w2;
            if (wn > vn) { vn = wn; v[0] = w0; v[1] = w1; v[2] = w2; }
        }
        double x = v[0] / v[2], y = v[1] / v[2], zz = z;
        if (!(isfinite(x) && isfinite(y) && isfinite(zz))) continue;
        epi_polish(b, x, y, zz);
        double E[9];
        epi_compose(b, x, y, zz, E);
        double nn = 0.0;
#pragma unroll
        for (int k = 0; k < 9; ++k) nn += E[k] * E[k];
        nn = sqrt(nn);
        bool ok = nn > 0.0 && isfinite(nn);
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            E[k] /= nn;
            ok = ok && isfinite(E[k]);
        }
        if (!ok) continue;
#pragma unroll
        for (int k = 0; k < 9; ++k) Eout[nsol * 9 + k] = E[k];
        ++nsol;
    }
    return nsol;
}

// ------------------------------------------------------------------------------------------------------------------ kernels
__global__ void __launch_bounds__(EPI_LANES) k_epi_solve5(const double* __restrict__ x0, const double* __restrict__ x1, size_t pt_stride,
                                                          const int* __restrict__ samples, size_t sample_stride, const int* __restrict__ dims,
                                                          int rounds, double* __restrict__ E, int* __restrict__ nsol, int* __restrict__ flag)
{
    __shared__ double sm[EPI_LDS_DOUBLES * EPI_LANES];
    const int p = blockIdx.y, lane = threadIdx.x;
    const int r = blockIdx.x * EPI_LANES + lane;
    if (r >= rounds) return;                                 // no barrier below: a lane works in its own column of sm
    const int m = dims[2 * p];
    const int* sp = samples + p * sample_stride + (size_t)r * 5;
    double* Eo = E + ((size_t)p * rounds + r) * (EPI_SOL * 9);
    double q0[5][2], q1[5][2];
    bool bad = false;
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        int j = sp[i];
        if (j < 0 || j >= m) { bad = true; j = 0; }
        q0[i][0] = x0[p * pt_stride + 2 * (size_t)j];
        q0[i][1] = x0[p * pt_stride + 2 * (size_t)j + 1];
        q1[i][0] = x1[p * pt_stride + 2 * (size_t)j];
        q1[i][1] = x1[p * pt_stride + 2 * (size_t)j + 1];
    }
    int n = 0;
    if (bad) {
        atomicOr(flag, EPI_BAD_INDEX);
        for (int k = 0; k < EPI_SOL * 9; ++k) Eo[k] = 0.0;
    } else {
        n = epi_solve5_core<EPI_LANES>(q0, q1, sm + lane, Eo);
    }
    nsol[(size_t)p * rounds + r] = n;
}

// dims: per pair its number of matches and the bits of its float32 threshold (float)(t * t).
// One thread per model, one tile of matches per workgroup (blockIdx.y), one pair per blockIdx.z.  counts is zero on entry; a slot
// the solver left empty (nsol given) gets -1 from the workgroup of the first tile and nothing from the others.
__global__ void __launch_bounds__(SCORE_THREADS) k_epi_score(const double* __restrict__ E, int nmodels, const int* __restrict__ nsol,
                                                             const double* __restrict__ x0, const double* __restrict__ x1, size_t pt_stride,
                                                             const int* __restrict__ dims, int* __restrict__ counts)
{
    __shared__ double sx[SCORE_TILE][4];
    const int p = blockIdx.z, m = dims[2 * p];
    const float thr = __int_as_float(dims[2 * p + 1]);
    const int j0 = blockIdx.y * SCORE_TILE;
    if (j0 >= m) return;                                     // uniform over the workgroup
    const int nj = min(SCORE_TILE, m - j0);
    for (int t = threadIdx.x; t < nj; t += SCORE_THREADS) {
        const size_t o = p * pt_stride + 2 * (size_t)(j0 + t);
        sx[t][0] = x0[o]; sx[t][1] = x0[o + 1]; sx[t][2] = x1[o]; sx[t][3] = x1[o + 1];
    }
    __syncthreads();
    const int k = blockIdx.x * SCORE_THREADS + threadIdx.x;
    if (k >= nmodels) return;
    int* out = counts + (size_t)p * nmodels + k;
    if (nsol && (k % EPI_SOL) >= nsol[(size_t)p * (nmodels / EPI_SOL) + k / EPI_SOL]) {
        if (blockIdx.y == 0) *out = -1;
        return;
    }
    double e[9];
    const double* Ek = E + ((size_t)p * nmodels + k) * 9;
#pragma unroll
    for (int q = 0; q < 9; ++q) e[q] = Ek[q];
    int cnt = 0;
    for (int t = 0; t < nj; ++t) cnt += epi_err(e, sx[t][0], sx[t][1], sx[t][2], sx[t][3]) <= thr ? 1 : 0;       // NaN: never
    if (cnt) atomicAdd(out, cnt);
}

struct EpiBest {
    int index, count;
};

// the largest count of a pair; of equal counts the lowest index (the reference's strict >)
__global__ void __launch_bounds__(256) k_epi_best(const int* __restrict__ counts, int nmodels, const double* __restrict__ E,
                                                  EpiBest* __restrict__ best, double* __restrict__ Ebest)
{
    __shared__ int s_cnt[256], s_idx[256];
    const int p = blockIdx.x, t = threadIdx.x;
    int bc = -1, bi = -1;
    for (int k = t; k < nmodels; k += 256) {
        const int v = counts[(size_t)p * nmodels + k];
        if (v > bc) { bc = v; bi = k; }
    }
    s_cnt[t] = bc;
    s_idx[t] = bi;
    __syncthreads();
    for (int s = 128; s >= 1; s >>= 1) {
        if (t < s) {
            const int oc = s_cnt[t + s], oi = s_idx[t + s];
            if (oi >= 0 && (oc > s_cnt[t] || (oc == s_cnt[t] && (s_idx[t] < 0 || oi < s_idx[t])))) { s_cnt[t] = oc; s_idx[t] = oi; }
        }
        __syncthreads();
    }
    const int idx = s_idx[0];
    if (t == 0) { best[p].index = idx; best[p].count = idx >= 0 ? s_cnt[0] : 0; }
    if (t < 9) Ebest[(size_t)p * 9 + t] = idx >= 0 ? E[((size_t)p * nmodels + idx) * 9 + t] : 0.0;
}

__global__ void __launch_bounds__(256) k_epi_mask(const double* __restrict__ E, const double* __restrict__ x0, const double* __restrict__ x1,
                                                  size_t pt_stride, const int* __restrict__ dims, uint8_t* __restrict__ mask,
                                                  float* __restrict__ err, size_t out_stride)
{
    const int p = blockIdx.y, m = dims[2 * p];
    const float thr = __int_as_float(dims[2 * p + 1]);
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= m) return;
    double e[9];
#pragma unroll
    for (int q = 0; q < 9; ++q) e[q] = E[(size_t)p * 9 + q];
    const size_t o = p * pt_stride + 2 * (size_t)j;
    const float v = epi_err(e, x0[o], x0[o + 1], x1[o], x1[o + 1]);
    err[p * out_stride + j] = v;
    mask[p * out_stride + j] = v <= thr ? 1 : 0;
}

// ---------------------------------------------------------------------------------------------------------------- host side
struct EpiPlan {
    int batch = 0, mmax = 0;
    int* d_flag = nullptr;
    int* d_dims = nullptr;
    EpiBest* d_best = nullptr;
    double* d_Ebest = nullptr;
    int* d_nsol = nullptr;
    int* d_counts = nullptr;
    double* d_E = nullptr;
    std::vector<int> dims;                                   // the upload's source: lives until the call's last synchronisation
};

// the layout of c->epi for a batch and its rounds (rounds == 0: the flag, the sizes, the best and its model alone)
static void epi_carve(EpiPlan& pl, int batch, int rounds, Carve& a)
{
    const size_t b = (size_t)batch, k = (size_t)rounds * EPI_SOL;
    pl.batch = batch;
    pl.d_flag = a.take<int>(256);
    pl.d_dims = a.take<int>(2 * b * sizeof(int));
    pl.d_best = a.take<EpiBest>(b * sizeof(EpiBest));
    pl.d_Ebest = a.take<double>(b * 9 * sizeof(double));
    pl.d_nsol = a.take<int>(b * rounds * sizeof(int));
    pl.d_counts = a.take<int>(b * k * sizeof(int));
    pl.d_E = a.take<double>(b * k * 9 * sizeof(double));
}

static size_t epi_ctx_bytes(int batch, int rounds) { EpiPlan pl; return measure([&](Carve& a) { epi_carve(pl, batch, rounds, a); }); }

// checks the sizes of a batch, lays the context's scratch out (rounds == 0: the sizes and the flag alone) and enqueues the upload
static int epi_plan(wass_ctx* c, const int* m, const double* t, int batch, int rounds, size_t pt_stride, size_t out_stride, bool outputs, EpiPlan* pl,
                    hipStream_t s)
{
    if (!m || batch < 1 || batch > 65535) return set_err(c, WASS_ERR_INVALID_ARG, "batch = %d: 1 .. 65535 pairs with their sizes", batch);
    if (rounds < 0 || rounds > WASS_EPI_MAX_ROUNDS) return set_err(c, WASS_ERR_INVALID_ARG, "rounds = %d: 1 .. %d", rounds, WASS_EPI_MAX_ROUNDS);
    int mmax = 0;
    for (int p = 0; p < batch; ++p) {
        if (m[p] < 5 || m[p] > WASS_EPI_MAX_M) return set_err(c, WASS_ERR_INVALID_ARG, "pair %d has %d matches: 5 .. %d", p, m[p], WASS_EPI_MAX_M);
        if (t && !(t[p] >= 0.0)) return set_err(c, WASS_ERR_INVALID_ARG, "pair %d: threshold = %g: a distance, not negative", p, t[p]);
        mmax = m[p] > mmax ? m[p] : mmax;
    }
    if (batch > 1 && pt_stride < 2 * (size_t)mmax) return set_err(c, WASS_ERR_INVALID_ARG, "pt_stride is shorter than the largest pair (%d matches)", mmax);
    if (outputs && batch > 1 && out_stride < (size_t)mmax) return set_err(c, WASS_ERR_INVALID_ARG, "out_stride is shorter than the largest pair (%d matches)", mmax);
    int rc = carve_buf(c, c->epi, [&](Carve& a) { epi_carve(*pl, batch, rounds, a); });
    if (rc) return rc;
    const size_t b = (size_t)batch;
    pl->mmax = mmax;
    pl->dims.assign(2 * b, 0);
    for (int p = 0; p < batch; ++p) {
        const float thr = t ? (float)(t[p] * t[p]) : 0.0f;
        pl->dims[2 * (size_t)p] = m[p];
        memcpy(&pl->dims[2 * (size_t)p + 1], &thr, sizeof thr);
    }
    WASS_HIP(c, hipMemsetAsync(pl->d_flag, 0, 256, s));
    WASS_HIP(c, hipMemcpyAsync(pl->d_dims, pl->dims.data(), 2 * b * sizeof(int), hipMemcpyHostToDevice, s));
    return WASS_OK;
}

static int epi_solve_enqueue(wass_ctx* c, const EpiPlan& pl, const double* d_x0, const double* d_x1, size_t pt_stride, const int32_t* d_samples,
                             size_t sample_stride, int rounds, double* d_E, int32_t* d_nsol, hipStream_t s)
{
    hipLaunchKernelGGL(k_epi_solve5, dim3((unsigned)((rounds + EPI_LANES - 1) / EPI_LANES), (unsigned)pl.batch), dim3(EPI_LANES), 0, s, d_x0, d_x1,
                       pt_stride, d_samples, sample_stride, pl.d_dims, rounds, d_E, d_nsol, pl.d_flag);
    WASS_HIP(c, hipGetLastError());
    return WASS_OK;
}

static int epi_score_enqueue(wass_ctx* c, const EpiPlan& pl, const double* d_E, int nmodels, const int32_t* d_nsol, const double* d_x0,
                             const double* d_x1, size_t pt_stride, int32_t* d_counts, hipStream_t s)
{
    WASS_HIP(c, hipMemsetAsync(d_counts, 0, (size_t)pl.batch * nmodels * sizeof(int32_t), s));
    hipLaunchKernelGGL(k_epi_score, dim3((unsigned)((nmodels + SCORE_THREADS - 1) / SCORE_THREADS), (unsigned)((pl.mmax + SCORE_TILE - 1) / SCORE_TILE),
                                         (unsigned)pl.batch),
                       dim3(SCORE_THREADS), 0, s, d_E, nmodels, d_nsol, d_x0, d_x1, pt_stride, pl.d_dims, d_counts);
    WASS_HIP(c, hipGetLastError());
    return WASS_OK;
}

static int epi_mask_enqueue(wass_ctx* c, const EpiPlan& pl, const double* d_E, const double* d_x0, const double* d_x1, size_t pt_stride,
                            uint8_t* d_mask, float* d_err, size_t out_stride, hipStream_t s)
{
    hipLaunchKernelGGL(k_epi_mask, dim3((unsigned)((pl.mmax + 255) / 256), (unsigned)pl.batch), dim3(256), 0, s, d_E, d_x0, d_x1, pt_stride, pl.d_dims,
                       d_mask, d_err, out_stride);
    WASS_HIP(c, hipGetLastError());
    return WASS_OK;
}

static int epi_finish(wass_ctx* c, const EpiPlan& pl, hipStream_t s)
{
    int flag = 0;
    WASS_HIP(c, hipMemcpyAsync(&flag, pl.d_flag, sizeof flag, hipMemcpyDeviceToHost, s));
    WASS_HIP(c, hipStreamSynchronize(s));
    if (flag & EPI_BAD_INDEX) return set_err(c, WASS_ERR_INVALID_ARG, "a sample names a match outside its pair");
    return WASS_OK;
}

}  // namespace wass

using namespace wass;

extern "C" {

int wass_epi_scratch_bytes(int batch, int rounds, size_t* bytes)
{
    if (!bytes || batch < 1 || batch > 65535 || rounds < 1 || rounds > WASS_EPI_MAX_ROUNDS) return WASS_ERR_INVALID_ARG;
    *bytes = epi_ctx_bytes(batch, rounds);
    return WASS_OK;
}

int wass_epi_solve5_dev(wass_ctx* c, const double* d_x0, const double* d_x1, size_t pt_stride, const int32_t* d_samples, size_t sample_stride,
                        const int* m, int rounds, int batch, double* d_E, int32_t* d_nsol)
{
    if (!c) return WASS_ERR_INVALID_ARG;
    if (!d_x0 || !d_x1 || !d_samples || !d_E || !d_nsol) return set_err(c, WASS_ERR_INVALID_ARG, "null argument");
    if (rounds < 1 || rounds > WASS_EPI_MAX_ROUNDS) return set_err(c, WASS_ERR_INVALID_ARG, "rounds = %d: 1 .. %d", rounds, WASS_EPI_MAX_ROUNDS);
    if (batch > 1 && sample_stride < 5 * (size_t)rounds) return set_err(c, WASS_ERR_INVALID_ARG, "sample_stride is shorter than %d samples", rounds);
    WASS_HIP(c, hipSetDevice(c->device));
    EpiPlan pl;
    hipStream_t s = c->ts();
    int rc = epi_plan(c, m, nullptr, batch, 0, pt_stride, 0, false, &pl, s);
    if (rc) return rc;
    if ((rc = epi_solve_enqueue(c, pl, d_x0, d_x1, pt_stride, d_samples, sample_stride, rounds, d_E, d_nsol, s))) return rc;
    return epi_finish(c, pl, s);
}

int wass_epi_score_dev(wass_ctx* c, const double* d_E, int nmodels, const int32_t* d_nsol, const double* d_x0, const double* d_x1, size_t pt_stride,
                       const int* m, const double* t, int batch, int32_t* d_counts)
{
    if (!c) return WASS_ERR_INVALID_ARG;
    if (!d_E || !d_x0 || !d_x1 || !d_counts || !t) return set_err(c, WASS_ERR_INVALID_ARG, "null argument");
    if (nmodels < 1 || nmodels > WASS_EPI_MAX_ROUNDS * WASS_EPI_MAX_SOL)
        return set_err(c, WASS_ERR_INVALID_ARG, "%d models: 1 .. %d", nmodels, WASS_EPI_MAX_ROUNDS * WASS_EPI_MAX_SOL);
    if (d_nsol && nmodels % WASS_EPI_MAX_SOL) return set_err(c, WASS_ERR_INVALID_ARG, "with solution counts the models come in tens");
    WASS_HIP(c, hipSetDevice(c->device));
    EpiPlan pl;
    hipStream_t s = c->ts();
    int rc = epi_plan(c, m, t, batch, 0, pt_stride, 0, false, &pl, s);
    if (rc) return rc;
    if ((rc = epi_score_enqueue(c, pl, d_E, nmodels, d_nsol, d_x0, d_x1, pt_stride, d_counts, s))) return rc;
    return epi_finish(c, pl, s);
}

int wass_epi_mask_dev(wass_ctx* c, const double* d_E, const double* d_x0, const double* d_x1, size_t pt_stride, const int* m, const double* t, int batch,
                      uint8_t* d_mask, float* d_err, size_t out_stride)
{
    if (!c) return WASS_ERR_INVALID_ARG;
    if (!d_E || !d_x0 || !d_x1 || !d_mask || !d_err || !t) return set_err(c, WASS_ERR_INVALID_ARG, "null argument");
    WASS_HIP(c, hipSetDevice(c->device));
    EpiPlan pl;
    hipStream_t s = c->ts();
    int rc = epi_plan(c, m, t, batch, 0, pt_stride, out_stride, true, &pl, s);
    if (rc) return rc;
    if ((rc = epi_mask_enqueue(c, pl, d_E, d_x0, d_x1, pt_stride, d_mask, d_err, out_stride, s))) return rc;
    return epi_finish(c, pl, s);
}

int wass_epi_find_dev(wass_ctx* c, const double* d_x0, const double* d_x1, size_t pt_stride, const int32_t* d_samples, size_t sample_stride,
                      const int* m, const double* t, int rounds, int batch, double* E, int* best_index, int* best_count, uint8_t* d_mask, float* d_err,
                      size_t out_stride)
{
    if (!c) return WASS_ERR_INVALID_ARG;
    if (!d_x0 || !d_x1 || !d_samples || !E || !best_index || !best_count || !d_mask || !d_err || !t) return set_err(c, WASS_ERR_INVALID_ARG, "null argument");
    if (rounds < 1 || rounds > WASS_EPI_MAX_ROUNDS) return set_err(c, WASS_ERR_INVALID_ARG, "rounds = %d: 1 .. %d", rounds, WASS_EPI_MAX_ROUNDS);
    if (batch > 1 && sample_stride < 5 * (size_t)rounds) return set_err(c, WASS_ERR_INVALID_ARG, "sample_stride is shorter than %d samples", rounds);
    WASS_HIP(c, hipSetDevice(c->device));
    EpiPlan pl;
    hipStream_t s = c->ts();
    int rc = epi_plan(c, m, t, batch, rounds, pt_stride, out_stride, true, &pl, s);
    if (rc) return rc;
    const int nmodels = rounds * EPI_SOL;
    if ((rc = epi_solve_enqueue(c, pl, d_x0, d_x1, pt_stride, d_samples, sample_stride, rounds, pl.d_E, pl.d_nsol, s))) return rc;
    if ((rc = epi_score_enqueue(c, pl, pl.d_E, nmodels, pl.d_nsol, d_x0, d_x1, pt_stride, pl.d_counts, s))) return rc;
    hipLaunchKernelGGL(k_epi_best, dim3((unsigned)batch), dim3(256), 0, s, pl.d_counts, nmodels, pl.d_E, pl.d_best, pl.d_Ebest);
    WASS_HIP(c, hipGetLastError());
    if ((rc = epi_mask_enqueue(c, pl, pl.d_Ebest, d_x0, d_x1, pt_stride, d_mask, d_err, out_stride, s))) return rc;
    std::vector<EpiBest> best((size_t)batch);
    WASS_HIP(c, hipMemcpyAsync(best.data(), pl.d_best, best.size() * sizeof(EpiBest), hipMemcpyDeviceToHost, s));
    WASS_HIP(c, hipMemcpyAsync(E, pl.d_Ebest, (size_t)batch * 9 * sizeof(double), hipMemcpyDeviceToHost, s));
    if ((rc = epi_finish(c, pl, s))) return rc;
    for (int p = 0; p < batch; ++p) {
        best_index[p] = best[(size_t)p].index;
        best_count[p] = best[(size_t)p].count;
    }
    return WASS_OK;
}

}  // extern "C"
