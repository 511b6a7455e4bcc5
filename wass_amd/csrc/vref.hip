// vref.hip -- variational (photometric) refinement of the gridded surface: gridding/wassgridsurface/TFVariationalRefinement.py.
//
// A half-resolution height field Zc [Hc = Ny / 2][Wc = Nx / 2] is moved by Adam so that the two pictures, sampled where the grid nodes
// of Z = resize(Zc) project, agree; a derivative-of-Gaussian term keeps Z regular.  The reference leaves the gradient to TensorFlow;
// here it is written out, and every value is ONE stated sequence of float32 operations (no contraction, division and square root
// correctly rounded), so that it does not depend on the launch shape and a whole trajectory can be reproduced bit for bit
// (tests/vref_oracle.py restates the same sequence in numpy).  Only the two loss sums are reductions; they are fp64.
//
// Per node i = (y, x) of the Ny x Nx grid, X = XX / b, Y = YY / b (float32 of the fp64 quotient), Z:
//   projection  c_r = ((R[r][0] X + R[r][1] Y) + R[r][2] Z) + T[r]                        r = 0, 1, 2
//               s_kr = ((Pk[r][0] c_0 + Pk[r][1] c_1) + Pk[r][2] c_2) + Pk[r][3]           k = 0, 1 (camera)
//               u_k = s_k0 / s_k2, v_k = s_k1 / s_k2
//               a node is DEGENERATE when, in either camera, s_k2 <= 0 or u_k or v_k is not finite: both of its samples are 0 and
//               so is its part of the data term and of the gradient; its coordinates are written as computed
//   sampling    tfa.image.interpolate_bilinear(indexing = "xy") per axis of extent `size`: f = min(max(0, floor(q)), size - 2),
//               a = min(max(0, q - f), 1); tl = I[fy][fx], tr = I[fy][fx + 1], bl = I[fy + 1][fx], br = I[fy + 1][fx + 1];
//               top = a_x (tr - tl) + tl, bot = a_x (br - bl) + bl, val = a_y (bot - top) + top, Iks = val * mask
//   slopes      Zdx, Zdy: cross-correlation of Z with the two 7 x 7 kernels, zero padding; acc = acc + K[a][b] * Z[y + a - 3][x + b - 3]
//               over the taps in row-major order from acc = 0, a tap outside the grid reading 0
//   losses      d = (I0s - I1s) / 255; data = sum(d * d) / N, smooth = sum(Zdx * Zdx + Zdy * Zdy) / N: the terms float32, the sums
//               and the division fp64 (block partials folded in a fixed order); energy = data + alpha * smooth in fp64
//   resize      tf.image.resize, bilinear, half-pixel centres, no antialiasing, per axis: src = (dst + 0.5) * (in / out) - 0.5 with
//               in / out one float32 quotient, lo = max(floor(src), 0), hi = min(ceil(src), in - 1), t = src - floor(src);
//               top = tl + (tr - tl) * tx, bot = bl + (br - bl) * tx, Z = top + (bot - top) * ty.  The per-axis tables are made on
//               the host with these float32 operations.
// The gradient of the energy:
//   sampler     dval/du = a_y (dbot - dtop) + dtop with dtop = tr - tl, dbot = br - bl, where 0 <= u - f_x <= 1 and 0 elsewhere;
//               dval/dv = bot - top where 0 <= v - f_y <= 1 and 0 elsewhere.  At the ties (u an integer, u = size - 1) this is
//               the slope of the cell the sampler reads, i.e. the right-hand derivative at an interior integer and the left-hand
//               one at size - 1.
//   projection  q_kr = (Pk[r][0] R[0][2] + Pk[r][1] R[1][2]) + Pk[r][2] R[2][2] (float32, on the host);
//               du_k/dZ = (q_k0 - u_k q_k2) / s_k2, dv_k/dZ = (q_k1 - v_k q_k2) / s_k2
//               dIk = (gx_k * du_k/dZ + gy_k * dv_k/dZ) * mask
//   data        gd = (d * (dI0 - dI1)) * cD, cD = float32(2 / (255 N))
//   smoothness  the adjoint of the two correlations = correlation with the flipped kernels: sx = sum Kx[6 - a][6 - b] * Zdx[y + a - 3][x + b - 3],
//               sy alike from Ky and Zdy, each over the taps in row-major order from 0, zero outside; gs = (sx + sy) * cS,
//               cS = float32(2 alpha / N);  gZ = gd + gs
//   resize      adjoint as a gather: coarse node (cy, cx) is read by the fine rows y in [ry0, ry1) and columns x in [rx0, rx1)
//               (host tables).  wy(y) = (lo_y == cy ? 1 - ty : 0) + (hi_y == cy ? ty : 0), wx alike;
//               row(y) = sum over x ascending of wx(x) * gZ[y][x] from 0; gC = sum over y ascending of wy(y) * row(y) from 0
//   Adam        Keras: m = m + (g - m) * c1, v = v + (g * g - v) * c2, Zc = Zc - (m * lr_t) / (sqrt(v) + eps), with
//               c1 = float32(1 - 0.9), c2 = float32(1 - 0.999), lr_t = float32(lr sqrt(1 - 0.999^t) / (1 - 0.9^t)) from fp64 on the host
//
// Launch plan of one iteration (plain launches on the context's stream, no host synchronisation):
//   k_vref_forward   64 x 16 nodes per workgroup: Z of the tile and its 3-node halo from Zc into LDS (resize), the two slopes from
//                    LDS, projection, the two picture gathers, gd                      -> Zdx, Zdy, gd
//   k_vref_smooth    the same tile: Zdx, Zdy with halo into LDS, gZ = gd + gs          -> gZ
//   k_vref_step      one coarse node per lane: the gather over gZ, then Adam in place  -> Zc, m, v
// Every report_every iterations k_vref_forward also leaves fp64 block partials of the two sums and k_vref_loss folds them into a
// row of the trace on the device; the trace is read once, after the last iteration.
#include "common.h"

#include <math.h>

#include <new>
#include <vector>

#pragma clang fp contract(off)

namespace wass {

constexpr int VR_TW = 64, VR_TH = 16, VR_THREADS = 256, VR_ROWS = VR_TH / (VR_THREADS / VR_TW);   // 4 nodes per lane
constexpr int VR_HALO = 3, VR_LW = VR_TW + 2 * VR_HALO, VR_LH = VR_TH + 2 * VR_HALO;
constexpr double VR_B1 = 0.9, VR_B2 = 0.999;

struct VrefCam {
    float R[9], T[3], P[2][12], q[2][3];
};
struct VrefKer {
    float kx[49], ky[49];
};
// per-axis tables of the resize, device pointers
struct VrefAxis {
    const int* lo; const int* hi; const float* t;     // per fine index
    const int* r0; const int* r1;                     // per coarse index: the fine indices [r0, r1) that read it
};

__device__ __forceinline__ float vref_resize_at(const float* __restrict__ Zc, int Wc, const VrefAxis& ay, const VrefAxis& ax, int y, int x)
{
    const int yl = ay.lo[y], yh = ay.hi[y], xl = ax.lo[x], xh = ax.hi[x];
    const float ty = ay.t[y], tx = ax.t[x];
    const float tl = Zc[(size_t)yl * Wc + xl], tr = Zc[(size_t)yl * Wc + xh], bl = Zc[(size_t)yh * Wc + xl], br = Zc[(size_t)yh * Wc + xh];
    const float top = tl + (tr - tl) * tx, bot = bl + (br - bl) * tx;
    return top + (bot - top) * ty;
}

struct VrefSample {
    float val, gx, gy;
};
// q inside the picture's clamps: see the header.  u, v finite.
__device__ __forceinline__ VrefSample vref_bilinear(const float* __restrict__ I, int H, int W, float u, float v)
{
    const float fxf = fminf(fmaxf(0.0f, floorf(u)), (float)(W - 2)), fyf = fminf(fmaxf(0.0f, floorf(v)), (float)(H - 2));
    const float rx = u - fxf, ry = v - fyf;
    const float ax = fminf(fmaxf(0.0f, rx), 1.0f), ay = fminf(fmaxf(0.0f, ry), 1.0f);
    const int fx = (int)fxf, fy = (int)fyf;
    const float* p = I + (size_t)fy * W + fx;
    const float tl = p[0], tr = p[1], bl = p[W], br = p[W + 1];
    const float dtop = tr - tl, dbot = br - bl;
    const float top = ax * dtop + tl, bot = ax * dbot + bl;
    VrefSample s;
    s.val = ay * (bot - top) + top;
    s.gx = (rx >= 0.0f && rx <= 1.0f) ? ay * (dbot - dtop) + dtop : 0.0f;
    s.gy = (ry >= 0.0f && ry <= 1.0f) ? bot - top : 0.0f;
    return s;
}

struct VrefFwd {
    const float* Z;            // full-resolution input (COARSE = false)
    const float* Zc;           // the variable (COARSE = true)
    int Ny, Nx, Wc;
    const float* Xb; const float* Yb; const float* mask;
    const float* I0; int H0, W0;
    const float* I1; int H1, W1;
    float cD;
    // outputs, each optional
    float* Zdx; float* Zdy; float* gd; float* I0s; float* I1s; float* uv; float* Zmasked;
    double* partial;           // [blocks][2]: sum of d * d, sum of Zdx * Zdx + Zdy * Zdy
};

template <bool COARSE>
__global__ void __launch_bounds__(VR_THREADS) k_vref_forward(VrefFwd a, VrefAxis ay, VrefAxis ax, VrefCam cam, VrefKer ker)
{
    __shared__ float zt[VR_LH][VR_LW];
    __shared__ double red[2][VR_THREADS];
    const int x0 = blockIdx.x * VR_TW, y0 = blockIdx.y * VR_TH;
    for (int i = threadIdx.x; i < VR_LH * VR_LW; i += VR_THREADS) {
        const int r = i / VR_LW, c = i - r * VR_LW, gy = y0 + r - VR_HALO, gx = x0 + c - VR_HALO;
        float z = 0.0f;
        if (gy >= 0 && gy < a.Ny && gx >= 0 && gx < a.Nx) z = COARSE ? vref_resize_at(a.Zc, a.Wc, ay, ax, gy, gx) : a.Z[(size_t)gy * a.Nx + gx];
        zt[r][c] = z;
    }
    __syncthreads();
    const int lx = threadIdx.x & (VR_TW - 1), ly0 = threadIdx.x / VR_TW;
    const size_t N = (size_t)a.Ny * a.Nx;
    double sd = 0.0, ss = 0.0;
    const bool want_data = a.gd || a.I0s || a.I1s || a.uv || a.partial;
#pragma unroll 1
    for (int k = 0; k < VR_ROWS; ++k) {
        const int ly = ly0 + k * (VR_THREADS / VR_TW), y = y0 + ly, x = x0 + lx;
        if (y >= a.Ny || x >= a.Nx) continue;
        const size_t i = (size_t)y * a.Nx + x;
        const float Z = zt[ly + VR_HALO][lx + VR_HALO];
        if (a.Zdx || a.Zdy || a.partial) {
            float sx = 0.0f, sy = 0.0f;
#pragma unroll
            for (int r = 0; r < 7; ++r)
#pragma unroll
                for (int c = 0; c < 7; ++c) {
                    const float z = zt[ly + r][lx + c];
                    sx = sx + ker.kx[r * 7 + c] * z;
                    sy = sy + ker.ky[r * 7 + c] * z;
                }
            if (a.Zdx) a.Zdx[i] = sx;
            if (a.Zdy) a.Zdy[i] = sy;
            ss += (double)(sx * sx + sy * sy);
        }
        const float m = a.mask[i];
        if (a.Zmasked) a.Zmasked[i] = Z * m;
        if (!want_data) continue;
        const float X = a.Xb[i], Y = a.Yb[i];
        float c[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) c[r] = ((cam.R[3 * r] * X + cam.R[3 * r + 1] * Y) + cam.R[3 * r + 2] * Z) + cam.T[r];
        float u[2], v[2], s2[2];
        bool ok = true;
#pragma unroll
        for (int kc = 0; kc < 2; ++kc) {
            const float* P = cam.P[kc];
            const float s0 = ((P[0] * c[0] + P[1] * c[1]) + P[2] * c[2]) + P[3];
            const float s1 = ((P[4] * c[0] + P[5] * c[1]) + P[6] * c[2]) + P[7];
            s2[kc] = ((P[8] * c[0] + P[9] * c[1]) + P[10] * c[2]) + P[11];
            u[kc] = s0 / s2[kc];
            v[kc] = s1 / s2[kc];
            ok = ok && s2[kc] > 0.0f && isfinite(u[kc]) && isfinite(v[kc]);
        }
        if (a.uv) {
            a.uv[i] = u[0]; a.uv[N + i] = v[0]; a.uv[2 * N + i] = u[1]; a.uv[3 * N + i] = v[1];
        }
        float i0 = 0.0f, i1 = 0.0f, g = 0.0f, d = 0.0f;
        if (ok) {
            const VrefSample A = vref_bilinear(a.I0, a.H0, a.W0, u[0], v[0]), B = vref_bilinear(a.I1, a.H1, a.W1, u[1], v[1]);
            i0 = A.val * m;
            i1 = B.val * m;
            d = (i0 - i1) / 255.0f;
            const float du0 = (cam.q[0][0] - u[0] * cam.q[0][2]) / s2[0], dv0 = (cam.q[0][1] - v[0] * cam.q[0][2]) / s2[0];
            const float du1 = (cam.q[1][0] - u[1] * cam.q[1][2]) / s2[1], dv1 = (cam.q[1][1] - v[1] * cam.q[1][2]) / s2[1];
            const float dI0 = (A.gx * du0 + A.gy * dv0) * m, dI1 = (B.gx * du1 + B.gy * dv1) * m;
            g = (d * (dI0 - dI1)) * a.cD;
        }
        if (a.I0s) a.I0s[i] = i0;
        if (a.I1s) a.I1s[i] = i1;
        if (a.gd) a.gd[i] = g;
        sd += (double)(d * d);
    }
    if (a.partial) {                                    // uniform for the launch
        red[0][threadIdx.x] = sd;
        red[1][threadIdx.x] = ss;
        __syncthreads();
        for (int o = VR_THREADS / 2; o > 0; o >>= 1) {
            if ((int)threadIdx.x < o) {
                red[0][threadIdx.x] += red[0][threadIdx.x + o];
                red[1][threadIdx.x] += red[1][threadIdx.x + o];
            }
            __syncthreads();
        }
        if (threadIdx.x == 0) {
            const size_t b = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
            a.partial[2 * b] = red[0][0];
            a.partial[2 * b + 1] = red[1][0];
        }
    }
}

// one workgroup: the block partials folded in a fixed order into row [steps, data, smooth, energy] of the trace
__global__ void __launch_bounds__(VR_THREADS) k_vref_loss(const double* __restrict__ partial, int nblocks, double n_nodes, double alpha,
                                                          double steps, double* __restrict__ row)
{
    __shared__ double red[2][VR_THREADS];
    double sd = 0.0, ss = 0.0;
    for (int b = threadIdx.x; b < nblocks; b += VR_THREADS) { sd += partial[2 * b]; ss += partial[2 * b + 1]; }
    red[0][threadIdx.x] = sd;
    red[1][threadIdx.x] = ss;
    __syncthreads();
    for (int o = VR_THREADS / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            red[0][threadIdx.x] += red[0][threadIdx.x + o];
            red[1][threadIdx.x] += red[1][threadIdx.x + o];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double data = red[0][0] / n_nodes, smooth = red[1][0] / n_nodes;
        row[0] = steps; row[1] = data; row[2] = smooth; row[3] = data + alpha * smooth;
    }
}

// gZ = gd + (sx + sy) * cS, the correlations with the flipped kernels (kf: already flipped by the host)
__global__ void __launch_bounds__(VR_THREADS) k_vref_smooth(const float* __restrict__ Zdx, const float* __restrict__ Zdy, const float* __restrict__ gd,
                                                            int Ny, int Nx, float cS, VrefKer kf, float* __restrict__ gZ)
{
    __shared__ float dxt[VR_LH][VR_LW], dyt[VR_LH][VR_LW];
    const int x0 = blockIdx.x * VR_TW, y0 = blockIdx.y * VR_TH;
    for (int i = threadIdx.x; i < VR_LH * VR_LW; i += VR_THREADS) {
        const int r = i / VR_LW, c = i - r * VR_LW, gy = y0 + r - VR_HALO, gx = x0 + c - VR_HALO;
        const bool in = gy >= 0 && gy < Ny && gx >= 0 && gx < Nx;
        dxt[r][c] = in ? Zdx[(size_t)gy * Nx + gx] : 0.0f;
        dyt[r][c] = in ? Zdy[(size_t)gy * Nx + gx] : 0.0f;
    }
    __syncthreads();
    const int lx = threadIdx.x & (VR_TW - 1), ly0 = threadIdx.x / VR_TW;
#pragma unroll 1
    for (int k = 0; k < VR_ROWS; ++k) {
        const int ly = ly0 + k * (VR_THREADS / VR_TW), y = y0 + ly, x = x0 + lx;
        if (y >= Ny || x >= Nx) continue;
        float sx = 0.0f, sy = 0.0f;
#pragma unroll
        for (int r = 0; r < 7; ++r)
#pragma unroll
            for (int c = 0; c < 7; ++c) {
                sx = sx + kf.kx[r * 7 + c] * dxt[ly + r][lx + c];
                sy = sy + kf.ky[r * 7 + c] * dyt[ly + r][lx + c];
            }
        const size_t i = (size_t)y * Nx + x;
        gZ[i] = gd[i] + (sx + sy) * cS;
    }
}

struct VrefAdam {
    float* m; float* v; float c1, c2, lr_t, eps;
};
// the adjoint of the resize as a gather, then (ADAM) the update in place
template <bool ADAM>
__global__ void __launch_bounds__(VR_THREADS) k_vref_step(const float* __restrict__ gZ, int Nx, int Hc, int Wc, VrefAxis ay, VrefAxis ax,
                                                          float* __restrict__ gC, float* __restrict__ Zc, VrefAdam ad)
{
    const int cx = blockIdx.x * 64 + (threadIdx.x & 63), cy = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (cx >= Wc || cy >= Hc) return;
    const int ya = ay.r0[cy], yb = ay.r1[cy], xa = ax.r0[cx], xb = ax.r1[cx];
    float g = 0.0f;
    for (int y = ya; y < yb; ++y) {
        const float ty = ay.t[y];
        const float wy = (ay.lo[y] == cy ? 1.0f - ty : 0.0f) + (ay.hi[y] == cy ? ty : 0.0f);
        float row = 0.0f;
        for (int x = xa; x < xb; ++x) {
            const float tx = ax.t[x];
            const float wx = (ax.lo[x] == cx ? 1.0f - tx : 0.0f) + (ax.hi[x] == cx ? tx : 0.0f);
            row = row + wx * gZ[(size_t)y * Nx + x];
        }
        g = g + wy * row;
    }
    const size_t i = (size_t)cy * Wc + cx;
    if (gC) gC[i] = g;
    if (ADAM) {
        float m = ad.m[i], v = ad.v[i];
        m = m + (g - m) * ad.c1;
        v = v + (g * g - v) * ad.c2;
        ad.m[i] = m;
        ad.v[i] = v;
        Zc[i] = Zc[i] - (m * ad.lr_t) / (sqrtf(v) + ad.eps);
    }
}

__global__ void __launch_bounds__(256) k_vref_finite(const float* __restrict__ a, size_t n, int* __restrict__ bad)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n && !isfinite(a[i])) atomicOr(bad, 1);
}

static inline size_t vr_align(size_t v) { return (v + 255) & ~(size_t)255; }

struct VrefLayout {
    size_t N, Nc, off_x, off_y, off_mask, off_I0, off_I1, off_z, off_zdx, off_zdy, off_gd, off_gz, off_partial, off_flag, off_tab, total;
    int bx, by, nblocks;
};

static bool vref_dims_ok(int ny, int nx, int ih0, int iw0, int ih1, int iw1)
{
    return ny >= 2 && nx >= 2 && ny <= 32768 && nx <= 32768 && ih0 >= 2 && iw0 >= 2 && ih1 >= 2 && iw1 >= 2 && ih0 <= 32768 && iw0 <= 32768 &&
           ih1 <= 32768 && iw1 <= 32768;
}

static VrefLayout vref_layout(int ny, int nx, int ih0, int iw0, int ih1, int iw1)
{
    VrefLayout L;
    L.N = (size_t)ny * nx;
    L.Nc = (size_t)(ny / 2) * (nx / 2);
    L.bx = (nx + VR_TW - 1) / VR_TW;
    L.by = (ny + VR_TH - 1) / VR_TH;
    L.nblocks = L.bx * L.by;
    size_t o = 0;
    const size_t plane = vr_align(L.N * 4);
    L.off_x = o; o += plane;
    L.off_y = o; o += plane;
    L.off_mask = o; o += plane;
    L.off_I0 = o; o += vr_align((size_t)ih0 * iw0 * 4);
    L.off_I1 = o; o += vr_align((size_t)ih1 * iw1 * 4);
    L.off_z = o; o += plane;
    L.off_zdx = o; o += plane;
    L.off_zdy = o; o += plane;
    L.off_gd = o; o += plane;
    L.off_gz = o; o += plane;
    L.off_partial = o; o += vr_align((size_t)L.nblocks * 16);
    L.off_flag = o; o += 256;
    L.off_tab = o; o += vr_align((size_t)(ny + nx) * 12 + (size_t)(ny / 2 + nx / 2) * 8);
    L.total = o;
    return L;
}

// tf.image.resize's per-axis rule (see the header) and, per coarse index, the fine indices that read it
static void vref_axis_tables(int in, int out, std::vector<int>& lo, std::vector<int>& hi, std::vector<float>& t, std::vector<int>& r0,
                             std::vector<int>& r1)
{
    lo.resize(out); hi.resize(out); t.resize(out);
    r0.assign(in, 0); r1.assign(in, 0);
    const float scale = (float)in / (float)out;
    for (int d = 0; d < out; ++d) {
        const float src = ((float)d + 0.5f) * scale - 0.5f, fl = floorf(src);
        lo[d] = (int)fl > 0 ? (int)fl : 0;
        const int ce = (int)ceilf(src);
        hi[d] = ce < in - 1 ? ce : in - 1;
        if (lo[d] > in - 1) lo[d] = in - 1;
        if (hi[d] < lo[d]) hi[d] = lo[d];
        t[d] = src - fl;
    }
    for (int c = 0; c < in; ++c) {
        bool any = false;
        for (int d = 0; d < out; ++d)
            if (lo[d] == c || hi[d] == c) {
                if (!any) { r0[c] = d; any = true; }
                r1[c] = d + 1;
            }
    }
}

}  // namespace wass

using namespace wass;

struct wass_vref {
    wass_ctx* c = nullptr;
    int ny = 0, nx = 0, hc = 0, wc = 0, ih0 = 0, iw0 = 0, ih1 = 0, iw1 = 0;
    VrefLayout L = {};
    char* mem = nullptr;
    double* trace = nullptr;     // device rows of the loss trace, grown on demand
    int trace_cap = 0;
    VrefCam cam = {};
    VrefKer ker = {}, kerf = {};
    VrefAxis ay = {}, ax = {};
    float* p(size_t off) const { return (float*)(mem + off); }
};

namespace {

VrefFwd vref_fwd_args(const wass_vref* h)
{
    VrefFwd a;
    memset(&a, 0, sizeof a);
    a.Ny = h->ny; a.Nx = h->nx; a.Wc = h->wc;
    a.Xb = h->p(h->L.off_x); a.Yb = h->p(h->L.off_y); a.mask = h->p(h->L.off_mask);
    a.I0 = h->p(h->L.off_I0); a.H0 = h->ih0; a.W0 = h->iw0;
    a.I1 = h->p(h->L.off_I1); a.H1 = h->ih1; a.W1 = h->iw1;
    a.cD = (float)(2.0 / (255.0 * (double)h->L.N));
    return a;
}

void vref_launch_forward(const wass_vref* h, const VrefFwd& a, bool coarse, hipStream_t s)
{
    const dim3 grid((unsigned)h->L.bx, (unsigned)h->L.by);
    if (coarse) hipLaunchKernelGGL(k_vref_forward<true>, grid, dim3(VR_THREADS), 0, s, a, h->ay, h->ax, h->cam, h->ker);
    else hipLaunchKernelGGL(k_vref_forward<false>, grid, dim3(VR_THREADS), 0, s, a, h->ay, h->ax, h->cam, h->ker);
}

void vref_launch_loss(const wass_vref* h, double alpha, double steps, double* d_row, hipStream_t s)
{
    hipLaunchKernelGGL(k_vref_loss, dim3(1), dim3(VR_THREADS), 0, s, (const double*)(h->mem + h->L.off_partial), h->L.nblocks, (double)h->L.N, alpha,
                       steps, d_row);
}

// gd, Zdx, Zdy of the handle -> gZ of the handle -> gC and / or the Adam step
void vref_launch_backward(const wass_vref* h, double alpha, float* d_gC, float* d_Zc, const VrefAdam* ad, hipStream_t s)
{
    const float cS = (float)(2.0 * alpha / (double)h->L.N);
    hipLaunchKernelGGL(k_vref_smooth, dim3((unsigned)h->L.bx, (unsigned)h->L.by), dim3(VR_THREADS), 0, s, (const float*)h->p(h->L.off_zdx),
                       (const float*)h->p(h->L.off_zdy), (const float*)h->p(h->L.off_gd), h->ny, h->nx, cS, h->kerf, h->p(h->L.off_gz));
    const dim3 grid((unsigned)((h->wc + 63) / 64), (unsigned)((h->hc + 3) / 4));
    VrefAdam none = {};
    if (ad) hipLaunchKernelGGL(k_vref_step<true>, grid, dim3(VR_THREADS), 0, s, (const float*)h->p(h->L.off_gz), h->nx, h->hc, h->wc, h->ay, h->ax, d_gC, d_Zc, *ad);
    else hipLaunchKernelGGL(k_vref_step<false>, grid, dim3(VR_THREADS), 0, s, (const float*)h->p(h->L.off_gz), h->nx, h->hc, h->wc, h->ay, h->ax, d_gC, d_Zc, none);
}

// every one of the `count` planes of n floats finite?  synchronises
int vref_all_finite(wass_vref* h, const float* const* planes, int count, size_t n, const char* what)
{
    wass_ctx* c = h->c;
    hipStream_t s = c->ts();
    int* flag = (int*)(h->mem + h->L.off_flag);
    WASS_HIP(c, hipMemsetAsync(flag, 0, 4, s));
    for (int k = 0; k < count; ++k)
        hipLaunchKernelGGL(k_vref_finite, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, planes[k], n, flag);
    WASS_HIP(c, hipGetLastError());
    int bad = 0;
    WASS_HIP(c, hipMemcpyAsync(&bad, flag, 4, hipMemcpyDeviceToHost, s));
    WASS_HIP(c, hipStreamSynchronize(s));
    if (bad) return set_err(c, WASS_ERR_INVALID_ARG, "%s holds a value that is not finite", what);
    return WASS_OK;
}

int vref_trace_rows(wass_vref* h, int rows)
{
    if (rows <= h->trace_cap) return WASS_OK;
    wass_ctx* c = h->c;
    if (h->trace) {
        WASS_HIP(c, hipStreamSynchronize(c->ts()));
        (void)hipFree(h->trace);
        h->trace = nullptr;
        h->trace_cap = 0;
    }
    if (hipMalloc((void**)&h->trace, (size_t)rows * 32) != hipSuccess) {
        h->trace = nullptr;
        return set_err(c, WASS_ERR_NO_MEMORY, "hipMalloc of %d rows of the loss trace failed", rows);
    }
    h->trace_cap = rows;
    return WASS_OK;
}

}  // namespace

extern "C" {

int wass_vref_scratch_bytes(int ny, int nx, int ih0, int iw0, int ih1, int iw1, size_t* bytes)
{
    if (!bytes || !vref_dims_ok(ny, nx, ih0, iw0, ih1, iw1)) return WASS_ERR_INVALID_ARG;
    *bytes = vref_layout(ny, nx, ih0, iw0, ih1, iw1).total;
    return WASS_OK;
}

void wass_vref_destroy(wass_vref* h)
{
    if (!h) return;
    if (h->c) (void)hipSetDevice(h->c->device);
    if (h->mem || h->trace) (void)hipDeviceSynchronize();
    if (h->mem) (void)hipFree(h->mem);
    if (h->trace) (void)hipFree(h->trace);
    delete h;
}

int wass_vref_create(wass_ctx* c, int ny, int nx, const float* d_xb, const float* d_yb, const float* d_mask, const double Rp2c[9],
                     const double Tp2c[3], const double P0cam[12], const double P1cam[12], const float* d_I0, int ih0, int iw0,
                     const float* d_I1, int ih1, int iw1, const float* kernels, wass_vref** out)
{
    if (!c) return WASS_ERR_INVALID_ARG;
    if (!out) return set_err(c, WASS_ERR_INVALID_ARG, "null argument");
    *out = nullptr;
    if (!d_xb || !d_yb || !d_mask || !Rp2c || !Tp2c || !P0cam || !P1cam || !d_I0 || !d_I1 || !kernels)
        return set_err(c, WASS_ERR_INVALID_ARG, "null argument");
    if (ny < 2 || nx < 2 || ny > 32768 || nx > 32768) return set_err(c, WASS_ERR_INVALID_ARG, "grid of %d x %d: 2 .. 32768 nodes per axis", ny, nx);
    if (!vref_dims_ok(ny, nx, ih0, iw0, ih1, iw1))
        return set_err(c, WASS_ERR_INVALID_ARG, "pictures of %d x %d and %d x %d: 2 .. 32768 pixels per side", ih0, iw0, ih1, iw1);
    for (int i = 0; i < 12; ++i)
        if (!isfinite(P0cam[i]) || !isfinite(P1cam[i]) || (i < 9 && !isfinite(Rp2c[i])) || (i < 3 && !isfinite(Tp2c[i])))
            return set_err(c, WASS_ERR_INVALID_ARG, "a matrix holds a value that is not finite");
    for (int i = 0; i < 98; ++i)
        if (!isfinite(kernels[i])) return set_err(c, WASS_ERR_INVALID_ARG, "a kernel holds a value that is not finite");
    WASS_HIP(c, hipSetDevice(c->device));
    wass_vref* h = new (std::nothrow) wass_vref;
    if (!h) return set_err(c, WASS_ERR_NO_MEMORY, "out of host memory");
    h->c = c; h->ny = ny; h->nx = nx; h->hc = ny / 2; h->wc = nx / 2;
    h->ih0 = ih0; h->iw0 = iw0; h->ih1 = ih1; h->iw1 = iw1;
    h->L = vref_layout(ny, nx, ih0, iw0, ih1, iw1);
    const VrefLayout& L = h->L;
    hipError_t e = hipMalloc((void**)&h->mem, L.total);
    if (e != hipSuccess) {
        h->mem = nullptr;
        wass_vref_destroy(h);
        return set_err(c, WASS_ERR_NO_MEMORY, "hipMalloc(%zu) for the refinement's set-up: %s", L.total, hipGetErrorString(e));
    }
    for (int i = 0; i < 9; ++i) h->cam.R[i] = (float)Rp2c[i];
    for (int i = 0; i < 3; ++i) h->cam.T[i] = (float)Tp2c[i];
    for (int i = 0; i < 12; ++i) { h->cam.P[0][i] = (float)P0cam[i]; h->cam.P[1][i] = (float)P1cam[i]; }
    for (int k = 0; k < 2; ++k)
        for (int r = 0; r < 3; ++r) {
            const float* P = h->cam.P[k] + 4 * r;
            h->cam.q[k][r] = (P[0] * h->cam.R[2] + P[1] * h->cam.R[5]) + P[2] * h->cam.R[8];
        }
    for (int i = 0; i < 49; ++i) {
        h->ker.kx[i] = kernels[i]; h->ker.ky[i] = kernels[49 + i];
        h->kerf.kx[i] = kernels[48 - i]; h->kerf.ky[i] = kernels[49 + 48 - i];
    }
    // the resize tables: per fine index lo, hi, t; per coarse index the range of fine indices
    std::vector<int> lo[2], hi[2], r0[2], r1[2];
    std::vector<float> t[2];
    vref_axis_tables(h->hc, ny, lo[0], hi[0], t[0], r0[0], r1[0]);
    vref_axis_tables(h->wc, nx, lo[1], hi[1], t[1], r0[1], r1[1]);
    hipStream_t s = c->ts();
    char* tab = h->mem + L.off_tab;
    bool ok = true;
    VrefAxis* axes[2] = {&h->ay, &h->ax};
    for (int k = 0; k < 2 && ok; ++k) {
        const size_t nf = lo[k].size(), nc = r0[k].size();
        VrefAxis& A = *axes[k];
        A.lo = (const int*)tab; ok = ok && hipMemcpyAsync(tab, lo[k].data(), nf * 4, hipMemcpyHostToDevice, s) == hipSuccess; tab += nf * 4;
        A.hi = (const int*)tab; ok = ok && hipMemcpyAsync(tab, hi[k].data(), nf * 4, hipMemcpyHostToDevice, s) == hipSuccess; tab += nf * 4;
        A.t = (const float*)tab; ok = ok && hipMemcpyAsync(tab, t[k].data(), nf * 4, hipMemcpyHostToDevice, s) == hipSuccess; tab += nf * 4;
        A.r0 = (const int*)tab; ok = ok && hipMemcpyAsync(tab, r0[k].data(), nc * 4, hipMemcpyHostToDevice, s) == hipSuccess; tab += nc * 4;
        A.r1 = (const int*)tab; ok = ok && hipMemcpyAsync(tab, r1[k].data(), nc * 4, hipMemcpyHostToDevice, s) == hipSuccess; tab += nc * 4;
    }
    const hipMemcpyKind dd = hipMemcpyDeviceToDevice;
    ok = ok && hipMemcpyAsync(h->mem + L.off_x, d_xb, L.N * 4, dd, s) == hipSuccess;
    ok = ok && hipMemcpyAsync(h->mem + L.off_y, d_yb, L.N * 4, dd, s) == hipSuccess;
    ok = ok && hipMemcpyAsync(h->mem + L.off_mask, d_mask, L.N * 4, dd, s) == hipSuccess;
    ok = ok && hipMemcpyAsync(h->mem + L.off_I0, d_I0, (size_t)ih0 * iw0 * 4, dd, s) == hipSuccess;
    ok = ok && hipMemcpyAsync(h->mem + L.off_I1, d_I1, (size_t)ih1 * iw1 * 4, dd, s) == hipSuccess;
    ok = ok && hipStreamSynchronize(s) == hipSuccess;                              // the host tables leave scope
    int rc = ok ? WASS_OK : set_err(c, WASS_ERR_DEVICE, "refinement set-up failed: %s", hipGetErrorString(hipGetLastError()));
    if (!rc) {
        const float* planes[3] = {h->p(L.off_x), h->p(L.off_y), h->p(L.off_mask)};
        rc = vref_all_finite(h, planes, 3, L.N, "XX / b, YY / b or the mask");
    }
    if (!rc) {
        const float* p0[1] = {h->p(L.off_I0)};
        const float* p1[1] = {h->p(L.off_I1)};
        rc = vref_all_finite(h, p0, 1, (size_t)ih0 * iw0, "picture 0");
        if (!rc) rc = vref_all_finite(h, p1, 1, (size_t)ih1 * iw1, "picture 1");
    }
    if (rc) {
        wass_vref_destroy(h);
        return rc;
    }
    *out = h;
    return WASS_OK;
}

int wass_vref_sample(wass_vref* h, const float* d_Z, float* d_I0s, float* d_I1s, float* d_uv)
{
    if (!h) return WASS_ERR_INVALID_ARG;
    wass_ctx* c = h->c;
    if (!d_Z || !d_I0s || !d_I1s || !d_uv) return set_err(c, WASS_ERR_INVALID_ARG, "null argument");
    WASS_HIP(c, hipSetDevice(c->device));
    const float* planes[1] = {d_Z};
    int rc = vref_all_finite(h, planes, 1, h->L.N, "Z");
    if (rc) return rc;
    VrefFwd a = vref_fwd_args(h);
    a.Z = d_Z; a.I0s = d_I0s; a.I1s = d_I1s; a.uv = d_uv;
    vref_launch_forward(h, a, false, c->ts());
    WASS_HIP(c, hipGetLastError());
    WASS_HIP(c, hipStreamSynchronize(c->ts()));
    return WASS_OK;
}

int wass_vref_zgrad(wass_vref* h, const float* d_Z, float* d_Zdx, float* d_Zdy)
{
    if (!h) return WASS_ERR_INVALID_ARG;
    wass_ctx* c = h->c;
    if (!d_Z || !d_Zdx || !d_Zdy) return set_err(c, WASS_ERR_INVALID_ARG, "null argument");
    WASS_HIP(c, hipSetDevice(c->device));
    const float* planes[1] = {d_Z};
    int rc = vref_all_finite(h, planes, 1, h->L.N, "Z");
    if (rc) return rc;
    VrefFwd a = vref_fwd_args(h);
    a.Z = d_Z; a.Zdx = d_Zdx; a.Zdy = d_Zdy;
    vref_launch_forward(h, a, false, c->ts());
    WASS_HIP(c, hipGetLastError());
    WASS_HIP(c, hipStreamSynchronize(c->ts()));
    return WASS_OK;
}

int wass_vref_loss(wass_vref* h, const float* d_Z, double* data_loss, double* smoothness_loss)
{
    if (!h) return WASS_ERR_INVALID_ARG;
    wass_ctx* c = h->c;
    if (!d_Z || !data_loss || !smoothness_loss) return set_err(c, WASS_ERR_INVALID_ARG, "null argument");
    WASS_HIP(c, hipSetDevice(c->device));
    const float* planes[1] = {d_Z};
    int rc = vref_all_finite(h, planes, 1, h->L.N, "Z");
    if (rc) return rc;
    if ((rc = vref_trace_rows(h, 1))) return rc;
    hipStream_t s = c->ts();
    VrefFwd a = vref_fwd_args(h);
    a.Z = d_Z; a.partial = (double*)(h->mem + h->L.off_partial);
    vref_launch_forward(h, a, false, s);
    vref_launch_loss(h, 0.0, 0.0, h->trace, s);
    WASS_HIP(c, hipGetLastError());
    double row[4];
    WASS_HIP(c, hipMemcpyAsync(row, h->trace, sizeof row, hipMemcpyDeviceToHost, s));
    WASS_HIP(c, hipStreamSynchronize(s));
    *data_loss = row[1];
    *smoothness_loss = row[2];
    return WASS_OK;
}

int wass_vref_gradient(wass_vref* h, const float* d_Zc, double alpha, float* d_gC, float* d_gZ)
{
    if (!h) return WASS_ERR_INVALID_ARG;
    wass_ctx* c = h->c;
    if (!d_Zc || !d_gC) return set_err(c, WASS_ERR_INVALID_ARG, "null argument");
    if (!isfinite(alpha)) return set_err(c, WASS_ERR_INVALID_ARG, "alpha is not finite");
    WASS_HIP(c, hipSetDevice(c->device));
    const float* planes[1] = {d_Zc};
    int rc = vref_all_finite(h, planes, 1, h->L.Nc, "Zc");
    if (rc) return rc;
    hipStream_t s = c->ts();
    VrefFwd a = vref_fwd_args(h);
    a.Zc = d_Zc; a.Zdx = h->p(h->L.off_zdx); a.Zdy = h->p(h->L.off_zdy); a.gd = h->p(h->L.off_gd);
    vref_launch_forward(h, a, true, s);
    vref_launch_backward(h, alpha, d_gC, nullptr, nullptr, s);
    WASS_HIP(c, hipGetLastError());
    if (d_gZ) WASS_HIP(c, hipMemcpyAsync(d_gZ, h->p(h->L.off_gz), h->L.N * 4, hipMemcpyDeviceToDevice, s));
    WASS_HIP(c, hipStreamSynchronize(s));
    return WASS_OK;
}

int wass_vref_adjoint(wass_vref* h, const float* d_Zdx, const float* d_Zdy, const float* d_gd, double alpha, float* d_gC, float* d_gZ)
{
    if (!h) return WASS_ERR_INVALID_ARG;
    wass_ctx* c = h->c;
    if (!d_Zdx || !d_Zdy || !d_gd || !d_gC) return set_err(c, WASS_ERR_INVALID_ARG, "null argument");
    if (!isfinite(alpha)) return set_err(c, WASS_ERR_INVALID_ARG, "alpha is not finite");
    WASS_HIP(c, hipSetDevice(c->device));
    const float* planes[3] = {d_Zdx, d_Zdy, d_gd};
    int rc = vref_all_finite(h, planes, 3, h->L.N, "Zdx, Zdy or gd");
    if (rc) return rc;
    hipStream_t s = c->ts();
    const hipMemcpyKind dd = hipMemcpyDeviceToDevice;
    WASS_HIP(c, hipMemcpyAsync(h->p(h->L.off_zdx), d_Zdx, h->L.N * 4, dd, s));
    WASS_HIP(c, hipMemcpyAsync(h->p(h->L.off_zdy), d_Zdy, h->L.N * 4, dd, s));
    WASS_HIP(c, hipMemcpyAsync(h->p(h->L.off_gd), d_gd, h->L.N * 4, dd, s));
    vref_launch_backward(h, alpha, d_gC, nullptr, nullptr, s);
    WASS_HIP(c, hipGetLastError());
    if (d_gZ) WASS_HIP(c, hipMemcpyAsync(d_gZ, h->p(h->L.off_gz), h->L.N * 4, dd, s));
    WASS_HIP(c, hipStreamSynchronize(s));
    return WASS_OK;
}

int wass_vref_optimize(wass_vref* h, float* d_Zc, float* d_m, float* d_v, int64_t* step, int iters, double alpha, double lr, double eps,
                       int report_every, double* trace, int trace_cap, int* n_trace, float* d_Zout)
{
    if (!h) return WASS_ERR_INVALID_ARG;
    wass_ctx* c = h->c;
    if (n_trace) *n_trace = 0;
    if (!d_Zc || !d_m || !d_v || !step) return set_err(c, WASS_ERR_INVALID_ARG, "null argument");
    if (iters < 0) return set_err(c, WASS_ERR_INVALID_ARG, "iters = %d: not negative", iters);
    if (*step < 0) return set_err(c, WASS_ERR_INVALID_ARG, "the Adam state's step count is negative");
    if (!isfinite(alpha) || !isfinite(lr) || !isfinite(eps)) return set_err(c, WASS_ERR_INVALID_ARG, "alpha, lr or eps is not finite");
    if (trace_cap < 0 || (trace_cap > 0 && !trace) || (trace && !n_trace)) return set_err(c, WASS_ERR_INVALID_ARG, "bad trace arguments");
    WASS_HIP(c, hipSetDevice(c->device));
    const float* planes[3] = {d_Zc, d_m, d_v};
    int rc = vref_all_finite(h, planes, 3, h->L.Nc, "Zc or the Adam state");
    if (rc) return rc;
    // the rows of the trace: before the first step, after step ii (from 0) where ii % report_every == 0, after the last
    const int every = report_every > 0 ? report_every : 0;
    const int rows_max = 2 + (every ? (iters + every - 1) / every : 0);
    const bool want = trace && trace_cap > 0;
    if (want && (rc = vref_trace_rows(h, rows_max))) return rc;
    hipStream_t s = c->ts();
    const VrefLayout& L = h->L;
    VrefFwd base = vref_fwd_args(h);
    base.Zc = d_Zc;
    int rows = 0;
    for (int it = 0; it < iters; ++it) {
        VrefFwd a = base;
        a.Zdx = h->p(L.off_zdx); a.Zdy = h->p(L.off_zdy); a.gd = h->p(L.off_gd);
        const bool report = want && rows < trace_cap && (it == 0 || (every && (it - 1) % every == 0));
        if (report) a.partial = (double*)(h->mem + L.off_partial);
        vref_launch_forward(h, a, true, s);
        if (report) vref_launch_loss(h, alpha, (double)it, h->trace + 4 * (size_t)rows++, s);
        const double t = (double)(*step + it + 1);
        VrefAdam ad;
        ad.m = d_m; ad.v = d_v;
        ad.c1 = (float)(1.0 - VR_B1); ad.c2 = (float)(1.0 - VR_B2);
        ad.lr_t = (float)(lr * sqrt(1.0 - pow(VR_B2, t)) / (1.0 - pow(VR_B1, t)));
        ad.eps = (float)eps;
        vref_launch_backward(h, alpha, nullptr, d_Zc, &ad, s);
    }
    const bool last_row = want && rows < trace_cap && (iters > 0 || rows == 0);
    if (last_row || d_Zout) {
        VrefFwd a = base;
        a.Zmasked = d_Zout;
        if (last_row) a.partial = (double*)(h->mem + L.off_partial);
        vref_launch_forward(h, a, true, s);
        if (last_row) vref_launch_loss(h, alpha, (double)iters, h->trace + 4 * (size_t)rows++, s);
    }
    WASS_HIP(c, hipGetLastError());
    if (rows) WASS_HIP(c, hipMemcpyAsync(trace, h->trace, (size_t)rows * 32, hipMemcpyDeviceToHost, s));
    WASS_HIP(c, hipStreamSynchronize(s));
    *step += iters;
    if (n_trace) *n_trace = rows;
    return WASS_OK;
}

}  // extern "C"
