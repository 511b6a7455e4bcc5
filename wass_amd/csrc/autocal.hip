// autocal.hip -- the device side of wass_autocalibrate (src/wass_autocalibrate/wass_autocalibrate.cpp, sba_driver.cpp): the choice
// among the four poses of an essential matrix and the two-camera bundle adjustment.  See include/wass_gpu.h ("Autocalibration").
//
//   k_ac_triangulate   one thread per (candidate, match): the least-squares point of the two rays and the count of z > 1
//   k_ac_linearize     one thread per point: residuals, V_i, e_b,i, W_i0, W_i1; per workgroup U_0, U_1, e_a, |e|^2 and two maxima
//   k_ac_schur         one thread per point: (V_i + mu I)^-1 and the point's share of the 12 x 12 reduced system
//   k_ac_backsub       one thread per point: db_i, the candidate point, its residuals, the four sums of the step test
//   k_ac_error         one thread per point: the residuals alone
//   k_ac_reduce        the workgroups' partial results, in ascending order of the workgroup
//
// All fp64, compiled without contraction.  A workgroup is one wave of 64; a sum over the wave is the fixed tree
// v += lane(l + 32), (l + 16), (l + 8), (l + 4), (l + 2), (l + 1), a lane past the points adding 0.0; k_ac_reduce then adds the
// workgroups one after another.  No result depends on launch timing.  The Levenberg-Marquardt loop is host code (wass_ac_bundle_dev): it is
// bounded by max_iters and by the damping counter, and no kernel waits for anything.
#include "common.h"

#include <math.h>
#include <string.h>

#include <cmath>

namespace wass {

constexpr int AC_WG = 64;
constexpr int AC_LIN = WASS_AC_LIN_ROWS;     // rows of the per-point record
constexpr int AC_LSUM = WASS_AC_LIN_SUMS;    // the linearisation's reduced record: 55 sums and 2 maxima
constexpr int AC_LADD = 55;
constexpr int AC_SSUM = 90;                  // 78 entries of the lower triangle and 12 of the right-hand side
constexpr int AC_BSUM = 4;
constexpr int AC_PART = 96;                  // doubles per workgroup in the partial array

// one camera as the kernels take it: the fixed initial rotation, the local rotation v (vector part of a unit quaternion), the
// translation, and what the host derives from v: w = sqrt(1 - |v|^2), 1 / w and Rj = R(w, v) R0
struct AcCam {
    double R0[9], v[3], t[3], w, iw, Rj[9];
};
struct AcCams {
    AcCam c[2];
};

// s = (v0 v0 + v1 v1) + v2 v2, w = sqrt(1 - s), Rl = I + 2 (w [v]x + (v v' - s I)), Rj = Rl R0 with (a b + c d) + e f per entry
static void ac_cam(const double* p, AcCam* c)
{
    memcpy(c->R0, p, 9 * sizeof(double));
    memcpy(c->v, p + 9, 3 * sizeof(double));
    memcpy(c->t, p + 12, 3 * sizeof(double));
    const double* v = c->v;
    const double s = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2];
    c->w = sqrt(1.0 - s);
    c->iw = 1.0 / c->w;
    const double vx[9] = { 0.0, -v[2], v[1], v[2], 0.0, -v[0], -v[1], v[0], 0.0 };
    double Rl[9];
    for (int r = 0; r < 3; ++r)
        for (int k = 0; k < 3; ++k) {
            const double d = r == k ? 1.0 : 0.0;
            Rl[3 * r + k] = d + 2.0 * (c->w * vx[3 * r + k] + (v[r] * v[k] - s * d));
        }
    for (int r = 0; r < 3; ++r)
        for (int k = 0; k < 3; ++k) c->Rj[3 * r + k] = (Rl[3 * r] * c->R0[k] + Rl[3 * r + 1] * c->R0[3 + k]) + Rl[3 * r + 2] * c->R0[6 + k];
}

// sum and maximum of a wave in lane 0
__device__ __forceinline__ double ac_sum(double v) { return wave_fold(v, [](double a, double b) { return a + b; }); }
__device__ __forceinline__ double ac_max(double v) { return wave_fold(v, [](double a, double b) { return fmax(a, b); }); }

// the projection of one point by one camera: X = Rj M + t, iz = 1 / X2, (px, py) = (X0 iz, X1 iz)
__device__ __forceinline__ void ac_project(const AcCam& c, double m0, double m1, double m2, double& iz, double& px, double& py)
{
    const double X0 = ((c.Rj[0] * m0 + c.Rj[1] * m1) + c.Rj[2] * m2) + c.t[0];
    const double X1 = ((c.Rj[3] * m0 + c.Rj[4] * m1) + c.Rj[5] * m2) + c.t[1];
    const double X2 = ((c.Rj[6] * m0 + c.Rj[7] * m1) + c.Rj[8] * m2) + c.t[2];
    iz = 1.0 / X2;
    px = X0 * iz;
    py = X1 * iz;
}

// the two rows of A = d proj / d (v, t) (2 x 6) and of B = d proj / d M (2 x 3) of one camera at one point, and the residual
__device__ __forceinline__ void ac_cam_lin(const AcCam& c, double m0, double m1, double m2, double u, double w, double* ax, double* ay, double* bx,
                                           double* by, double& ex, double& ey)
{
    double iz, px, py;
    ac_project(c, m0, m1, m2, iz, px, py);
    ex = u - px;
    ey = w - py;
    const double Y0 = (c.R0[0] * m0 + c.R0[1] * m1) + c.R0[2] * m2;
    const double Y1 = (c.R0[3] * m0 + c.R0[4] * m1) + c.R0[5] * m2;
    const double Y2 = (c.R0[6] * m0 + c.R0[7] * m1) + c.R0[8] * m2;
    const double v0 = c.v[0], v1 = c.v[1], v2 = c.v[2];
    const double c0 = v1 * Y2 - v2 * Y1, c1 = v2 * Y0 - v0 * Y2, c2 = v0 * Y1 - v1 * Y0;
    const double h = (v0 * Y0 + v1 * Y1) + v2 * Y2;
    const double g0 = c.w * Y0 + c0, g1 = c.w * Y1 + c1, g2 = c.w * Y2 + c2;
    const double G0 = c.iw * c0 + Y0, G1 = c.iw * c1 + Y1, G2 = c.iw * c2 + Y2;
    // D = dX / dv = 2 ((h I - G v') - [g]x)
    const double D00 = 2.0 * ((h - G0 * v0) - 0.0), D01 = 2.0 * ((0.0 - G0 * v1) - (-g2)), D02 = 2.0 * ((0.0 - G0 * v2) - g1);
    const double D10 = 2.0 * ((0.0 - G1 * v0) - g2), D11 = 2.0 * ((h - G1 * v1) - 0.0), D12 = 2.0 * ((0.0 - G1 * v2) - (-g0));
    const double D20 = 2.0 * ((0.0 - G2 * v0) - (-g1)), D21 = 2.0 * ((0.0 - G2 * v1) - g0), D22 = 2.0 * ((h - G2 * v2) - 0.0);
    ax[0] = iz * (D00 - px * D20); ax[1] = iz * (D01 - px * D21); ax[2] = iz * (D02 - px * D22);
    ay[0] = iz * (D10 - py * D20); ay[1] = iz * (D11 - py * D21); ay[2] = iz * (D12 - py * D22);
    ax[3] = iz; ax[4] = 0.0; ax[5] = -(px * iz);
    ay[3] = 0.0; ay[4] = iz; ay[5] = -(py * iz);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        bx[k] = iz * (c.Rj[k] - px * c.Rj[6 + k]);
        by[k] = iz * (c.Rj[3 + k] - py * c.Rj[6 + k]);
    }
}

// --------------------------------------------------------------------------------------------------------------- triangulation
// grid (ceil(m / 256), 4).  counts is zero on entry.
__global__ void __launch_bounds__(256) k_ac_triangulate(const double* __restrict__ x0, const double* __restrict__ x1, const uint8_t* __restrict__ mask,
                                                        int m, const double* __restrict__ RT, double* __restrict__ pts, int* __restrict__ counts)
{
    const int k = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    const double* R = RT + 12 * k;           // candidate k: R (9) and T (3)
    const double* T = R + 9;
    int good = 0;
    if (i < m) {
        const double p0 = x0[2 * (size_t)i], p1 = x0[2 * (size_t)i + 1], q0 = x1[2 * (size_t)i], q1 = x1[2 * (size_t)i + 1];
        const double r20 = q0 * R[6] - R[0], r21 = q0 * R[7] - R[1], r22 = q0 * R[8] - R[2];
        const double r30 = q1 * R[6] - R[3], r31 = q1 * R[7] - R[4], r32 = q1 * R[8] - R[5];
        const double b2 = T[0] - T[2] * q0, b3 = T[1] - T[2] * q1;
        const double a = (1.0 + r20 * r20) + r30 * r30, b = r20 * r21 + r30 * r31, cc = (r20 * r22 - p0) + r30 * r32;
        const double d = (1.0 + r21 * r21) + r31 * r31, e = (r21 * r22 - p1) + r31 * r32;
        const double f = ((p0 * p0 + p1 * p1) + r22 * r22) + r32 * r32;
        const double y0 = r20 * b2 + r30 * b3, y1 = r21 * b2 + r31 * b3, y2 = r22 * b2 + r32 * b3;
        const double C00 = d * f - e * e, C01 = cc * e - b * f, C02 = b * e - cc * d;
        const double C11 = a * f - cc * cc, C12 = b * cc - a * e, C22 = a * d - b * b;
        const double det = (a * C00 + b * C01) + cc * C02;
        double X = ((C00 * y0 + C01 * y1) + C02 * y2) / det;
        double Y = ((C01 * y0 + C11 * y1) + C12 * y2) / det;
        double Z = ((C02 * y0 + C12 * y1) + C22 * y2) / det;
        if (!(det != 0.0) || !isfinite(det)) X = Y = Z = __longlong_as_double(0x7ff8000000000000LL);
        double* o = pts + ((size_t)k * m + i) * 3;
        o[0] = X; o[1] = Y; o[2] = Z;
        good = (mask[i] != 0 && Z > 1.0) ? 1 : 0;
    }
    const int n = __syncthreads_count(good);
    if (threadIdx.x == 0 && n) atomicAdd(counts + k, n);
}

// --------------------------------------------------------------------------------------------------------------- linearisation
// lin: AC_LIN rows of n (row r of point i at lin[r * n + i]); part: AC_PART doubles per workgroup
__global__ void __launch_bounds__(AC_WG) k_ac_linearize(AcCams cams, const double* __restrict__ pts, const double* __restrict__ obs, int n,
                                                        double* __restrict__ lin, double* __restrict__ part)
{
    const int i = blockIdx.x * AC_WG + threadIdx.x;
    const bool in = i < n;
    const size_t j = in ? (size_t)i : (size_t)(n - 1);
    const double m0 = pts[3 * j], m1 = pts[3 * j + 1], m2 = pts[3 * j + 2];
    double* out = part + (size_t)blockIdx.x * AC_PART;
    double V[6] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 }, eb[3] = { 0.0, 0.0, 0.0 }, err = 0.0;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        double ax[6], ay[6], bx[3], by[3], ex, ey;
        ac_cam_lin(cams.c[q], m0, m1, m2, obs[4 * j + 2 * q], obs[4 * j + 2 * q + 1], ax, ay, bx, by, ex, ey);
        const double vq[6] = { bx[0] * bx[0] + by[0] * by[0], bx[0] * bx[1] + by[0] * by[1], bx[0] * bx[2] + by[0] * by[2],
                               bx[1] * bx[1] + by[1] * by[1], bx[1] * bx[2] + by[1] * by[2], bx[2] * bx[2] + by[2] * by[2] };
        const double e2 = ex * ex + ey * ey;
        if (q == 0) {
#pragma unroll
            for (int k = 0; k < 6; ++k) V[k] = vq[k];
#pragma unroll
            for (int k = 0; k < 3; ++k) eb[k] = bx[k] * ex + by[k] * ey;
            err = e2;
        } else {
#pragma unroll
            for (int k = 0; k < 6; ++k) V[k] = V[k] + vq[k];
#pragma unroll
            for (int k = 0; k < 3; ++k) eb[k] = eb[k] + (bx[k] * ex + by[k] * ey);
            err = err + e2;
        }
        if (in) {
            lin[(size_t)(2 * q) * n + i] = ex;
            lin[(size_t)(2 * q + 1) * n + i] = ey;
#pragma unroll
            for (int a = 0; a < 6; ++a)
#pragma unroll
                for (int k = 0; k < 3; ++k) lin[(size_t)(13 + 18 * q + 3 * a + k) * n + i] = ax[a] * bx[k] + ay[a] * by[k];
        }
        // U_q (lower triangle by rows) and e_a,q over the wave
        int s = 0;
#pragma unroll
        for (int a = 0; a < 6; ++a)
#pragma unroll
            for (int b = 0; b <= a; ++b, ++s) {
                const double r = ac_sum(in ? ax[a] * ax[b] + ay[a] * ay[b] : 0.0);
                if (threadIdx.x == 0) out[21 * q + s] = r;
            }
#pragma unroll
        for (int a = 0; a < 6; ++a) {
            const double r = ac_sum(in ? ax[a] * ex + ay[a] * ey : 0.0);
            if (threadIdx.x == 0) out[42 + 6 * q + a] = r;
        }
    }
    if (in) {
#pragma unroll
        for (int k = 0; k < 6; ++k) lin[(size_t)(4 + k) * n + i] = V[k];
#pragma unroll
        for (int k = 0; k < 3; ++k) lin[(size_t)(10 + k) * n + i] = eb[k];
    }
    const double se = ac_sum(in ? err : 0.0);
    const double mg = ac_max(in ? fmax(fmax(fabs(eb[0]), fabs(eb[1])), fabs(eb[2])) : 0.0);
    const double md = ac_max(in ? fmax(fmax(V[0], V[3]), V[5]) : 0.0);
    if (threadIdx.x == 0) { out[54] = se; out[55] = mg; out[56] = md; }
}

// one thread per entry of the record: the workgroups in ascending order; entries at or above nadd are maxima
__global__ void __launch_bounds__(128) k_ac_reduce(const double* __restrict__ part, int nblocks, int nval, int nadd, double* __restrict__ out)
{
    const int t = threadIdx.x;
    if (t >= nval) return;
    double v = part[t];
    for (int b = 1; b < nblocks; ++b) {
        const double x = part[(size_t)b * AC_PART + t];
        v = t < nadd ? v + x : fmax(v, x);
    }
    out[t] = v;
}

// ------------------------------------------------------------------------------------------------------------------ Schur step
__global__ void __launch_bounds__(AC_WG) k_ac_schur(const double* __restrict__ lin, int n, double mu, double* __restrict__ vinv, double* __restrict__ part)
{
    const int i = blockIdx.x * AC_WG + threadIdx.x;
    const bool in = i < n;
    const size_t j = in ? (size_t)i : (size_t)(n - 1);
    double* out = part + (size_t)blockIdx.x * AC_PART;
    const double a = lin[(size_t)4 * n + j] + mu, b = lin[(size_t)5 * n + j], c = lin[(size_t)6 * n + j];
    const double d = lin[(size_t)7 * n + j] + mu, e = lin[(size_t)8 * n + j], f = lin[(size_t)9 * n + j] + mu;
    const double C00 = d * f - e * e, C01 = c * e - b * f, C02 = b * e - c * d;
    const double C11 = a * f - c * c, C12 = b * c - a * e, C22 = a * d - b * b;
    const double det = (a * C00 + b * C01) + c * C02;
    const double id = 1.0 / det;
    const double Vi[9] = { C00 * id, C01 * id, C02 * id, C01 * id, C11 * id, C12 * id, C02 * id, C12 * id, C22 * id };
    if (in) {
        vinv[i] = Vi[0]; vinv[(size_t)n + i] = Vi[1]; vinv[(size_t)2 * n + i] = Vi[2];
        vinv[(size_t)3 * n + i] = Vi[4]; vinv[(size_t)4 * n + i] = Vi[5]; vinv[(size_t)5 * n + i] = Vi[8];
    }
    const double eb0 = lin[(size_t)10 * n + j], eb1 = lin[(size_t)11 * n + j], eb2 = lin[(size_t)12 * n + j];
    double W[36];
#pragma unroll
    for (int p = 0; p < 36; ++p) W[p] = lin[(size_t)(13 + p) * n + j];
    int s = 0;
#pragma unroll
    for (int p = 0; p < 12; ++p) {
        const double y0 = (W[3 * p] * Vi[0] + W[3 * p + 1] * Vi[3]) + W[3 * p + 2] * Vi[6];
        const double y1 = (W[3 * p] * Vi[1] + W[3 * p + 1] * Vi[4]) + W[3 * p + 2] * Vi[7];
        const double y2 = (W[3 * p] * Vi[2] + W[3 * p + 1] * Vi[5]) + W[3 * p + 2] * Vi[8];
#pragma unroll
        for (int q = 0; q <= p; ++q, ++s) {
            const double r = ac_sum(in ? (y0 * W[3 * q] + y1 * W[3 * q + 1]) + y2 * W[3 * q + 2] : 0.0);
            if (threadIdx.x == 0) out[s] = r;
        }
        const double r = ac_sum(in ? (y0 * eb0 + y1 * eb1) + y2 * eb2 : 0.0);
        if (threadIdx.x == 0) out[78 + p] = r;
    }
}

// ----------------------------------------------------------------------------------------------------------- back-substitution
struct AcStep {
    double da[12], mu;
};

__global__ void __launch_bounds__(AC_WG) k_ac_backsub(AcCams cnew, AcStep st, const double* __restrict__ pts, const double* __restrict__ obs,
                                                      const double* __restrict__ lin, const double* __restrict__ vinv, int n, double* __restrict__ db,
                                                      double* __restrict__ ptsn, double* __restrict__ part)
{
    const int i = blockIdx.x * AC_WG + threadIdx.x;
    const bool in = i < n;
    const size_t j = in ? (size_t)i : (size_t)(n - 1);
    double* out = part + (size_t)blockIdx.x * AC_PART;
    double g[3], eb[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        double acc = lin[(size_t)(13 + k) * n + j] * st.da[0];
#pragma unroll
        for (int p = 1; p < 12; ++p) acc = acc + lin[(size_t)(13 + 3 * p + k) * n + j] * st.da[p];
        eb[k] = lin[(size_t)(10 + k) * n + j];
        g[k] = eb[k] - acc;
    }
    const double i00 = vinv[j], i01 = vinv[(size_t)n + j], i02 = vinv[(size_t)2 * n + j];
    const double i11 = vinv[(size_t)3 * n + j], i12 = vinv[(size_t)4 * n + j], i22 = vinv[(size_t)5 * n + j];
    const double d0 = (i00 * g[0] + i01 * g[1]) + i02 * g[2];
    const double d1 = (i01 * g[0] + i11 * g[1]) + i12 * g[2];
    const double d2 = (i02 * g[0] + i12 * g[1]) + i22 * g[2];
    const double m0 = pts[3 * j], m1 = pts[3 * j + 1], m2 = pts[3 * j + 2];
    const double n0 = m0 + d0, n1 = m1 + d1, n2 = m2 + d2;
    if (in) {
        db[3 * j] = d0; db[3 * j + 1] = d1; db[3 * j + 2] = d2;
        ptsn[3 * j] = n0; ptsn[3 * j + 1] = n1; ptsn[3 * j + 2] = n2;
    }
    double iz, px, py;
    ac_project(cnew.c[0], n0, n1, n2, iz, px, py);
    const double ex0 = obs[4 * j] - px, ey0 = obs[4 * j + 1] - py;
    ac_project(cnew.c[1], n0, n1, n2, iz, px, py);
    const double ex1 = obs[4 * j + 2] - px, ey1 = obs[4 * j + 3] - py;
    const double s0 = ac_sum(in ? (ex0 * ex0 + ey0 * ey0) + (ex1 * ex1 + ey1 * ey1) : 0.0);
    const double s1 = ac_sum(in ? (d0 * d0 + d1 * d1) + d2 * d2 : 0.0);
    const double s2 = ac_sum(in ? (m0 * m0 + m1 * m1) + m2 * m2 : 0.0);
    const double s3 = ac_sum(in ? (d0 * (st.mu * d0 + eb[0]) + d1 * (st.mu * d1 + eb[1])) + d2 * (st.mu * d2 + eb[2]) : 0.0);
    if (threadIdx.x == 0) { out[0] = s0; out[1] = s1; out[2] = s2; out[3] = s3; }
}

// res (may be null): 4 x n, the residuals
__global__ void __launch_bounds__(AC_WG) k_ac_error(AcCams cams, const double* __restrict__ pts, const double* __restrict__ obs, int n,
                                                    double* __restrict__ res, double* __restrict__ part)
{
    const int i = blockIdx.x * AC_WG + threadIdx.x;
    const bool in = i < n;
    const size_t j = in ? (size_t)i : (size_t)(n - 1);
    const double m0 = pts[3 * j], m1 = pts[3 * j + 1], m2 = pts[3 * j + 2];
    double iz, px, py;
    ac_project(cams.c[0], m0, m1, m2, iz, px, py);
    const double ex0 = obs[4 * j] - px, ey0 = obs[4 * j + 1] - py;
    ac_project(cams.c[1], m0, m1, m2, iz, px, py);
    const double ex1 = obs[4 * j + 2] - px, ey1 = obs[4 * j + 3] - py;
    if (in && res) { res[i] = ex0; res[(size_t)n + i] = ey0; res[(size_t)2 * n + i] = ex1; res[(size_t)3 * n + i] = ey1; }
    const double s0 = ac_sum(in ? (ex0 * ex0 + ey0 * ey0) + (ex1 * ex1 + ey1 * ey1) : 0.0);
    if (threadIdx.x == 0) part[(size_t)blockIdx.x * AC_PART] = s0;
}

// ---------------------------------------------------------------------------------------------------------------- host side
struct AcPlan {
    int n = 0, nb = 0;
    double *d_part = nullptr, *d_rec = nullptr, *d_lin = nullptr, *d_vinv = nullptr, *d_db = nullptr, *d_ptsn = nullptr;
    int* d_counts = nullptr;
};

static size_t ac_blocks(int n) { return ((size_t)n + AC_WG - 1) / AC_WG; }

// the layout of c->ac for n points: the counts, then six arrays of doubles
static void ac_carve(AcPlan& pl, int n, Carve& a)
{
    const size_t N = (size_t)n, d = sizeof(double);
    pl.n = n; pl.nb = (int)ac_blocks(n);
    pl.d_counts = a.take<int>(256);
    pl.d_rec = a.take<double>(AC_PART * d);
    pl.d_part = a.take<double>(pl.nb * AC_PART * d);
    pl.d_lin = a.take<double>(AC_LIN * N * d);
    pl.d_vinv = a.take<double>(6 * N * d);
    pl.d_db = a.take<double>(3 * N * d);
    pl.d_ptsn = a.take<double>(3 * N * d);
}

static size_t ac_ctx_bytes(int n) { AcPlan pl; return measure([&](Carve& a) { ac_carve(pl, n, a); }); }

static int ac_plan(wass_ctx* c, int n, AcPlan* pl)
{
    if (n < 1 || n > WASS_AC_MAX_N) return set_err(c, WASS_ERR_INVALID_ARG, "n = %d: 1 .. %d points", n, WASS_AC_MAX_N);
    return carve_buf(c, c->ac, [&](Carve& a) { ac_carve(*pl, n, a); });
}

// the partial results of the last kernel to one record on the host; returns after a synchronisation
static int ac_collect(wass_ctx* c, const AcPlan& pl, int nval, int nadd, double* rec, hipStream_t s)
{
    hipLaunchKernelGGL(k_ac_reduce, dim3(1), dim3(128), 0, s, pl.d_part, pl.nb, nval, nadd, pl.d_rec);
    WASS_HIP(c, hipGetLastError());
    WASS_HIP(c, hipMemcpyAsync(rec, pl.d_rec, (size_t)nval * sizeof(double), hipMemcpyDeviceToHost, s));
    WASS_HIP(c, hipStreamSynchronize(s));
    return WASS_OK;
}

static int ac_linearize(wass_ctx* c, const AcPlan& pl, const double* cams, const double* d_pts, const double* d_obs, double* sums, hipStream_t s)
{
    AcCams k;
    ac_cam(cams, &k.c[0]);
    ac_cam(cams + 15, &k.c[1]);
    hipLaunchKernelGGL(k_ac_linearize, dim3((unsigned)pl.nb), dim3(AC_WG), 0, s, k, d_pts, d_obs, pl.n, pl.d_lin, pl.d_part);
    WASS_HIP(c, hipGetLastError());
    return ac_collect(c, pl, AC_LSUM, AC_LADD, sums, s);
}

static int ac_tri(int a, int b) { return a * (a + 1) / 2 + b; }

// S = diag(U_0 + mu I, U_1 + mu I) - sum_i W_i V_i*^-1 W_i' (12 x 12, both triangles) and rhs = e_a - sum_i W_i V_i*^-1 e_b,i
static int ac_schur(wass_ctx* c, const AcPlan& pl, const double* sums, double mu, double* S, double* rhs, hipStream_t s)
{
    double rec[AC_SSUM];
    hipLaunchKernelGGL(k_ac_schur, dim3((unsigned)pl.nb), dim3(AC_WG), 0, s, pl.d_lin, pl.n, mu, pl.d_vinv, pl.d_part);
    WASS_HIP(c, hipGetLastError());
    int rc = ac_collect(c, pl, AC_SSUM, AC_SSUM, rec, s);
    if (rc) return rc;
    for (int p = 0; p < 12; ++p) {
        for (int q = 0; q <= p; ++q) {
            double u = 0.0;
            if (p / 6 == q / 6) {
                u = sums[21 * (p / 6) + ac_tri(p % 6, q % 6)];
                if (p == q) u = u + mu;
            }
            S[12 * p + q] = S[12 * q + p] = u - rec[ac_tri(p, q)];
        }
        rhs[p] = sums[42 + p] - rec[78 + p];
    }
    return WASS_OK;
}

// Cholesky S = L L' by rows and the two triangular solves; false when a pivot is not positive or not finite
static bool ac_cholesky_solve(const double* S, const double* rhs, double* x)
{
    double L[144];
    for (int p = 0; p < 12; ++p)
        for (int q = 0; q <= p; ++q) {
            double v = S[12 * p + q];
            for (int k = 0; k < q; ++k) v = v - L[12 * p + k] * L[12 * q + k];
            if (p == q) {
                if (!(v > 0.0) || !std::isfinite(v)) return false;
                L[12 * p + p] = sqrt(v);
            } else {
                L[12 * p + q] = v / L[12 * q + q];
            }
        }
    double y[12];
    for (int p = 0; p < 12; ++p) {
        double v = rhs[p];
        for (int k = 0; k < p; ++k) v = v - L[12 * p + k] * y[k];
        y[p] = v / L[12 * p + p];
    }
    for (int p = 11; p >= 0; --p) {
        double v = y[p];
        for (int k = p + 1; k < 12; ++k) v = v - L[12 * k + p] * x[k];
        x[p] = v / L[12 * p + p];
    }
    for (int p = 0; p < 12; ++p)
        if (!std::isfinite(x[p])) return false;
    return true;
}

static void ac_moved(const double* cams, const double* da, double* out)
{
    memcpy(out, cams, 30 * sizeof(double));
    for (int q = 0; q < 2; ++q)
        for (int k = 0; k < 6; ++k) out[15 * q + 9 + k] = cams[15 * q + 9 + k] + da[6 * q + k];
}

// scal: |e_new|^2, |dp|^2, |p|^2 and dL = dp' (mu dp + J'e), the cameras' share added after the points'
static int ac_backsub(wass_ctx* c, const AcPlan& pl, const double* cams, const double* sums, const double* da, double mu, const double* d_pts,
                      const double* d_obs, double* d_db, double* d_ptsn, double* cams_new, double* scal, hipStream_t s)
{
    ac_moved(cams, da, cams_new);
    AcCams k;
    ac_cam(cams_new, &k.c[0]);
    ac_cam(cams_new + 15, &k.c[1]);
    AcStep st;
    memcpy(st.da, da, sizeof st.da);
    st.mu = mu;
    hipLaunchKernelGGL(k_ac_backsub, dim3((unsigned)pl.nb), dim3(AC_WG), 0, s, k, st, d_pts, d_obs, pl.d_lin, pl.d_vinv, pl.n, d_db, d_ptsn, pl.d_part);
    WASS_HIP(c, hipGetLastError());
    int rc = ac_collect(c, pl, AC_BSUM, AC_BSUM, scal, s);
    if (rc) return rc;
    for (int q = 0; q < 2; ++q)
        for (int k2 = 0; k2 < 6; ++k2) {
            const double d = da[6 * q + k2], p = cams[15 * q + 9 + k2];
            scal[1] = scal[1] + d * d;
            scal[2] = scal[2] + p * p;
            scal[3] = scal[3] + d * (mu * d + sums[42 + 6 * q + k2]);
        }
    return WASS_OK;
}

static int ac_check(wass_ctx* c, const double* cams, const void* d_pts, const void* d_obs)
{
    if (!cams || !d_pts || !d_obs) return set_err(c, WASS_ERR_INVALID_ARG, "null argument");
    return WASS_OK;
}

}  // namespace wass

using namespace wass;

extern "C" {

int wass_ac_scratch_bytes(int n, size_t* bytes)
{
    if (!bytes || n < 1 || n > WASS_AC_MAX_N) return WASS_ERR_INVALID_ARG;
    *bytes = ac_ctx_bytes(n);
    return WASS_OK;
}

int wass_ac_triangulate_dev(wass_ctx* c, const double* d_x0, const double* d_x1, const uint8_t* d_mask, int m, const double* R4, const double* T4,
                            double* d_pts, int32_t* counts)
{
    if (!c) return WASS_ERR_INVALID_ARG;
    if (!d_x0 || !d_x1 || !d_mask || !R4 || !T4 || !d_pts || !counts) return set_err(c, WASS_ERR_INVALID_ARG, "null argument");
    if (m < 1 || m > WASS_AC_MAX_N) return set_err(c, WASS_ERR_INVALID_ARG, "m = %d: 1 .. %d matches", m, WASS_AC_MAX_N);
    WASS_HIP(c, hipSetDevice(c->device));
    AcPlan pl;
    int rc = ac_plan(c, 1, &pl);
    if (rc) return rc;
    double rt[48];
    for (int q = 0; q < 4; ++q) {
        memcpy(rt + 12 * q, R4 + 9 * q, 9 * sizeof(double));
        memcpy(rt + 12 * q + 9, T4 + 3 * q, 3 * sizeof(double));
    }
    hipStream_t s = c->ts();
    WASS_HIP(c, hipMemcpyAsync(pl.d_rec, rt, sizeof rt, hipMemcpyHostToDevice, s));
    WASS_HIP(c, hipMemsetAsync(pl.d_counts, 0, 4 * sizeof(int), s));
    hipLaunchKernelGGL(k_ac_triangulate, dim3((unsigned)((m + 255) / 256), 4), dim3(256), 0, s, d_x0, d_x1, d_mask, m, pl.d_rec, d_pts, pl.d_counts);
    WASS_HIP(c, hipGetLastError());
    WASS_HIP(c, hipMemcpyAsync(counts, pl.d_counts, 4 * sizeof(int), hipMemcpyDeviceToHost, s));
    WASS_HIP(c, hipStreamSynchronize(s));
    return WASS_OK;
}

int wass_ac_linearize_dev(wass_ctx* c, const double* cams, const double* d_pts, const double* d_obs, int n, double* d_lin, double* sums)
{
    if (!c) return WASS_ERR_INVALID_ARG;
    int rc = ac_check(c, cams, d_pts, d_obs);
    if (rc) return rc;
    if (!sums) return set_err(c, WASS_ERR_INVALID_ARG, "null argument");
    WASS_HIP(c, hipSetDevice(c->device));
    AcPlan pl;
    if ((rc = ac_plan(c, n, &pl))) return rc;
    hipStream_t s = c->ts();
    if ((rc = ac_linearize(c, pl, cams, d_pts, d_obs, sums, s))) return rc;
    if (d_lin) {
        WASS_HIP(c, hipMemcpyAsync(d_lin, pl.d_lin, (size_t)AC_LIN * n * sizeof(double), hipMemcpyDeviceToDevice, s));
        WASS_HIP(c, hipStreamSynchronize(s));
    }
    return WASS_OK;
}

int wass_ac_step_dev(wass_ctx* c, const double* cams, const double* d_pts, const double* d_obs, int n, double mu, double* S, double* rhs, double* da,
                     double* d_db, double* d_pts_new, double* cams_new, double* scal, int* ok)
{
    if (!c) return WASS_ERR_INVALID_ARG;
    int rc = ac_check(c, cams, d_pts, d_obs);
    if (rc) return rc;
    if (!S || !rhs || !da || !cams_new || !scal || !ok) return set_err(c, WASS_ERR_INVALID_ARG, "null argument");
    if (!(mu >= 0.0)) return set_err(c, WASS_ERR_INVALID_ARG, "mu = %g: not negative", mu);
    WASS_HIP(c, hipSetDevice(c->device));
    AcPlan pl;
    if ((rc = ac_plan(c, n, &pl))) return rc;
    hipStream_t s = c->ts();
    double sums[AC_LSUM];
    if ((rc = ac_linearize(c, pl, cams, d_pts, d_obs, sums, s))) return rc;
    if ((rc = ac_schur(c, pl, sums, mu, S, rhs, s))) return rc;
    *ok = ac_cholesky_solve(S, rhs, da) ? 1 : 0;
    if (!*ok) {
        for (int p = 0; p < 12; ++p) da[p] = 0.0;
        for (int p = 0; p < 4; ++p) scal[p] = 0.0;
        memcpy(cams_new, cams, 30 * sizeof(double));
        return WASS_OK;
    }
    if ((rc = ac_backsub(c, pl, cams, sums, da, mu, d_pts, d_obs, pl.d_db, pl.d_ptsn, cams_new, scal, s))) return rc;
    if (d_db) WASS_HIP(c, hipMemcpyAsync(d_db, pl.d_db, (size_t)3 * n * sizeof(double), hipMemcpyDeviceToDevice, s));
    if (d_pts_new) WASS_HIP(c, hipMemcpyAsync(d_pts_new, pl.d_ptsn, (size_t)3 * n * sizeof(double), hipMemcpyDeviceToDevice, s));
    WASS_HIP(c, hipStreamSynchronize(s));
    return WASS_OK;
}

int wass_ac_error_dev(wass_ctx* c, const double* cams, const double* d_pts, const double* d_obs, int n, double* d_res, double* err)
{
    if (!c) return WASS_ERR_INVALID_ARG;
    int rc = ac_check(c, cams, d_pts, d_obs);
    if (rc) return rc;
    if (!err) return set_err(c, WASS_ERR_INVALID_ARG, "null argument");
    WASS_HIP(c, hipSetDevice(c->device));
    AcPlan pl;
    if ((rc = ac_plan(c, n, &pl))) return rc;
    hipStream_t s = c->ts();
    AcCams k;
    ac_cam(cams, &k.c[0]);
    ac_cam(cams + 15, &k.c[1]);
    hipLaunchKernelGGL(k_ac_error, dim3((unsigned)pl.nb), dim3(AC_WG), 0, s, k, d_pts, d_obs, n, d_res, pl.d_part);
    WASS_HIP(c, hipGetLastError());
    return ac_collect(c, pl, 1, 1, err, s);
}

int wass_ac_bundle_dev(wass_ctx* c, double* cams, double* d_pts, const double* d_obs, int n, int max_iters, double* info)
{
    if (!c) return WASS_ERR_INVALID_ARG;
    int rc = ac_check(c, cams, d_pts, d_obs);
    if (rc) return rc;
    if (!info) return set_err(c, WASS_ERR_INVALID_ARG, "null argument");
    if (max_iters < 0) return set_err(c, WASS_ERR_INVALID_ARG, "max_iters = %d: not negative", max_iters);
    WASS_HIP(c, hipSetDevice(c->device));
    AcPlan pl;
    if ((rc = ac_plan(c, n, &pl))) return rc;
    hipStream_t s = c->ts();
    const double tau = 1e-3, eps1 = 1e-12, eps2 = 1e-12, eps2_sq = eps2 * eps2, eps3_sq = 1e-12 * 1e-12, tiny_sq = 1e-12 * 1e-12;
    double sums[AC_LSUM], S[144], rhs[12], da[12], scal[4], cnew[30];
    double mu = 0.0, err = 0.0, err0 = 0.0, ginf = 0.0, dp2 = 0.0;
    unsigned nu = 2;
    int stop = 0, it = 0, solves = 0;
    for (it = 0; it < max_iters && !stop; ++it) {
        if ((rc = ac_linearize(c, pl, cams, d_pts, d_obs, sums, s))) return rc;
        err = sums[54];
        if (it == 0) err0 = err;
        if (!std::isfinite(err)) { stop = 7; break; }
        ginf = sums[55];
        for (int p = 0; p < 12; ++p) ginf = fmax(ginf, fabs(sums[42 + p]));
        if (ginf <= eps1) { stop = 1; break; }
        if (err <= eps3_sq) { stop = 6; break; }
        if (it == 0) {
            double md = sums[56];
            for (int q = 0; q < 2; ++q)
                for (int a = 0; a < 6; ++a) md = fmax(md, sums[21 * q + ac_tri(a, a)]);
            mu = tau * md;
        }
        for (;;) {
            if ((rc = ac_schur(c, pl, sums, mu, S, rhs, s))) return rc;
            ++solves;
            if (ac_cholesky_solve(S, rhs, da)) {
                if ((rc = ac_backsub(c, pl, cams, sums, da, mu, d_pts, d_obs, pl.d_db, pl.d_ptsn, cnew, scal, s))) return rc;
                dp2 = scal[1];
                if (dp2 <= eps2_sq * scal[2]) { stop = 2; break; }
                if (dp2 >= (scal[2] + eps2) / tiny_sq) { stop = 4; break; }
                if (!std::isfinite(scal[0])) { stop = 7; break; }
                const double dF = err - scal[0], dL = scal[3];
                if (dL > 0.0 && dF > 0.0) {
                    double t = 2.0 * dF / dL - 1.0;
                    t = 1.0 - t * t * t;
                    mu = mu * fmax(t, 1.0 / 3.0);
                    nu = 2;
                    memcpy(cams, cnew, sizeof cnew);
                    WASS_HIP(c, hipMemcpyAsync(d_pts, pl.d_ptsn, (size_t)3 * n * sizeof(double), hipMemcpyDeviceToDevice, s));
                    err = scal[0];
                    break;
                }
            }
            mu = mu * (double)nu;
            const unsigned nu2 = nu << 1;
            if (nu2 <= nu || !std::isfinite(mu)) { stop = 5; break; }
            nu = nu2;
        }
    }
    if (!stop) stop = 3;
    WASS_HIP(c, hipStreamSynchronize(s));
    info[0] = err0; info[1] = err; info[2] = (double)it; info[3] = (double)stop; info[4] = mu; info[5] = ginf; info[6] = dp2; info[7] = (double)solves;
    return WASS_OK;
}

}  // extern "C"
