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
//
// Batches: every kernel of the loop takes its frame from blockIdx.z (k_vref_loss: from its workgroup index) and offsets what belongs
// to a frame -- mask, pictures, Zc, m, v, Zdx, Zdy, gd, gZ, the block partials, the trace rows -- by the frame's stride `fs`; XX / b,
// YY / b, the cameras, the kernels, the axis tables and lr_t are shared (all frames of a batch are at the same Adam step).  Bounds are
// tested on the frame's own (y, x) before the offset is added, so a halo or a gather never reaches the next frame's plane.  A value
// is the same sequence of operations whatever the frame index and the partials of frame f are folded with frame f's only, in the
// order of the single run: frame f of a batch IS the single run of frame f, bit for bit, and the single entry points are a batch of one.
//   k_vref_ingest    per fine node: mask = caller's mask != 0, or !isnan(Zi); zin = mask ? (float)(-(double)Zi / baseline) : 0
//   k_vref_down      per coarse node: cv.resize's INTER_LINEAR rule (refinement.downsample_linear) from host tables s, s + 1, f:
//                    row = S[s] * (1 - f) + S[s + 1] * f in float32, the two rows combined by the same rule; m = v = 0
//   k_vref_finish    per fine node: Z = resize(Zc) * mask, out = mask ? (float)(-(double)Z * baseline) : NaN
#include "cube.h"

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
    size_t fs;                 // the frame's stride in floats: frame blockIdx.z of every per-frame pointer below starts at blockIdx.z * fs
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
    {                                                   // this frame's planes: every per-frame pointer moves once, in scalar registers
        const size_t fo = (size_t)blockIdx.z * a.fs;
        if (COARSE) a.Zc += fo; else a.Z += fo;
        a.mask += fo; a.I0 += fo; a.I1 += fo;
        if (a.Zdx) a.Zdx += fo;
        if (a.Zdy) a.Zdy += fo;
        if (a.gd) a.gd += fo;
        if (a.I0s) a.I0s += fo;
        if (a.I1s) a.I1s += fo;
        if (a.uv) a.uv += fo;
        if (a.Zmasked) a.Zmasked += fo;
        if (a.partial) a.partial += fo / 2;             // fs is even: a frame is a multiple of 256 bytes
    }
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
        block_tree<VR_THREADS>([&](int t, int u) { red[0][t] += red[0][u]; red[1][t] += red[1][u]; });
        if (threadIdx.x == 0) {
            const size_t b = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
            a.partial[2 * b] = red[0][0];
            a.partial[2 * b + 1] = red[1][0];
        }
    }
}

// one workgroup per frame: the frame's block partials folded in a fixed order into row [steps, data, smooth, energy] of its trace
__global__ void __launch_bounds__(VR_THREADS) k_vref_loss(const double* __restrict__ partial, size_t fs, int nblocks, double n_nodes, double alpha,
                                                          double steps, double* __restrict__ row, size_t row_stride)
{
    __shared__ double red[2][VR_THREADS];
    partial += (size_t)blockIdx.x * (fs / 2);
    row += (size_t)blockIdx.x * row_stride;
    double sd = 0.0, ss = 0.0;
    for (int b = threadIdx.x; b < nblocks; b += VR_THREADS) { sd += partial[2 * b]; ss += partial[2 * b + 1]; }
    red[0][threadIdx.x] = sd;
    red[1][threadIdx.x] = ss;
    __syncthreads();
    block_tree<VR_THREADS>([&](int t, int u) { red[0][t] += red[0][u]; red[1][t] += red[1][u]; });
    if (threadIdx.x == 0) {
        const double data = red[0][0] / n_nodes, smooth = red[1][0] / n_nodes;
        row[0] = steps; row[1] = data; row[2] = smooth; row[3] = data + alpha * smooth;
    }
}

// gZ = gd + (sx + sy) * cS, the correlations with the flipped kernels (kf: already flipped by the host)
__global__ void __launch_bounds__(VR_THREADS) k_vref_smooth(const float* __restrict__ Zdx, const float* __restrict__ Zdy, const float* __restrict__ gd,
                                                            size_t fs, int Ny, int Nx, float cS, VrefKer kf, float* __restrict__ gZ)
{
    __shared__ float dxt[VR_LH][VR_LW], dyt[VR_LH][VR_LW];
    const int x0 = blockIdx.x * VR_TW, y0 = blockIdx.y * VR_TH;
    const size_t fo = (size_t)blockIdx.z * fs;
    Zdx += fo; Zdy += fo; gd += fo; gZ += fo;
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
__global__ void __launch_bounds__(VR_THREADS) k_vref_step(const float* __restrict__ gZ, size_t fs, int Nx, int Hc, int Wc, VrefAxis ay, VrefAxis ax,
                                                          float* __restrict__ gC, float* __restrict__ Zc, VrefAdam ad)
{
    const size_t fo = (size_t)blockIdx.z * fs;
    gZ += fo;
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
    const size_t i = fo + (size_t)cy * Wc + cx;
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

// flag = min(flag, index of the frame) over the values that are not finite; `per` values per frame
__global__ void __launch_bounds__(256) k_vref_finite(const float* __restrict__ a, size_t n, size_t per, int* __restrict__ flag)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n && !isfinite(a[i])) atomicMin(flag, (int)(i / per));
}

// `count` floats per frame from src (frame stride ss) to dst (frame stride ds); blockIdx.z: the frame
__global__ void __launch_bounds__(256) k_vref_copy(float* __restrict__ dst, size_t ds, const float* __restrict__ src, size_t ss, size_t count)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < count) dst[(size_t)blockIdx.z * ds + i] = src[(size_t)blockIdx.z * ss + i];
}

// Zi [n][N] metres, z up, NaN outside; mask_in [n][N] or null -> the frame's mask (1 / 0) and zin in the plane's frame; a value inside
// the mask that is not finite (after the division as well) leaves its frame's index in flag
__global__ void __launch_bounds__(256) k_vref_ingest(const float* __restrict__ Zi, const float* __restrict__ mask_in, size_t N, double baseline,
                                                     size_t fs, float* __restrict__ mask, float* __restrict__ zin, int* __restrict__ flag)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const size_t f = blockIdx.z;
    const float z = Zi[f * N + i];
    const bool in = mask_in ? mask_in[f * N + i] != 0.0f : !isnan(z);
    float v = 0.0f;
    if (in) {
        v = (float)(-(double)z / baseline);
        if (!isfinite(v)) atomicMin(flag, (int)f);
    }
    mask[f * fs + i] = in ? 1.0f : 0.0f;
    zin[f * fs + i] = v;
}

// per-axis tables of cv.resize's INTER_LINEAR rule, device pointers, per coarse index
struct VrefDown {
    const int* s; const int* s1; const float* f;
};

__global__ void __launch_bounds__(VR_THREADS) k_vref_down(const float* __restrict__ zin, size_t fs, int Nx, int Hc, int Wc, VrefDown dy, VrefDown dx,
                                                          float* __restrict__ Zc, float* __restrict__ m, float* __restrict__ v)
{
    const int cx = blockIdx.x * 64 + (threadIdx.x & 63), cy = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (cx >= Wc || cy >= Hc) return;
    const size_t fo = (size_t)blockIdx.z * fs;
    const float* S0 = zin + fo + (size_t)dy.s[cy] * Nx;
    const float* S1 = zin + fo + (size_t)dy.s1[cy] * Nx;
    const int xa = dx.s[cx], xb = dx.s1[cx];
    const float fx = dx.f[cx], fy = dy.f[cy], gx = 1.0f - fx, gy = 1.0f - fy;
    const float r0 = S0[xa] * gx + S0[xb] * fx, r1 = S1[xa] * gx + S1[xb] * fx;
    const size_t i = fo + (size_t)cy * Wc + cx;
    Zc[i] = r0 * gy + r1 * fy;
    m[i] = 0.0f;
    v[i] = 0.0f;
}

// out [n][N] metres, NaN outside the mask; Zm [n][N] (may be null) = resize(Zc) * mask
__global__ void __launch_bounds__(256) k_vref_finish(const float* __restrict__ Zc, const float* __restrict__ mask, size_t fs, int Ny, int Nx, int Wc,
                                                     VrefAxis ay, VrefAxis ax, double baseline, float* __restrict__ out, float* __restrict__ Zm)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= Nx || y >= Ny) return;
    const size_t fo = (size_t)blockIdx.z * fs, i = (size_t)y * Nx + x, o = (size_t)blockIdx.z * Ny * Nx + i;
    const float mk = mask[fo + i];
    const float z = vref_resize_at(Zc + fo, Wc, ay, ax, y, x) * mk;
    if (Zm) Zm[o] = z;
    out[o] = mk != 0.0f ? (float)(-(double)z * baseline) : __builtin_nanf("");
}

// One allocation: what every frame shares, then nb frames of `frame` bytes each.  The f_ offsets count from a frame's start.
struct VrefLayout {
    size_t N, Nc, off_x, off_y, off_flag, off_tab, shared;
    size_t f_mask, f_zin, f_zdx, f_zdy, f_gd, f_gz, f_I0, f_I1, f_zc, f_m, f_v, f_partial, frame, total;
    int bx, by, nblocks;
};

constexpr int VR_MAX_BATCH = 4096;
constexpr int VR_NO_FRAME = 0x7f7f7f7f;      // what hipMemset(0x7f) leaves in the flag

static bool vref_dims_ok(int ny, int nx, int ih0, int iw0, int ih1, int iw1)
{
    return ny >= 2 && nx >= 2 && ny <= 32768 && nx <= 32768 && ih0 >= 2 && iw0 >= 2 && ih1 >= 2 && iw1 >= 2 && ih0 <= 32768 && iw0 <= 32768 &&
           ih1 <= 32768 && iw1 <= 32768;
}

static VrefLayout vref_layout(int nb, int ny, int nx, int ih0, int iw0, int ih1, int iw1)
{
    VrefLayout L;
    L.N = (size_t)ny * nx;
    L.Nc = (size_t)(ny / 2) * (nx / 2);
    L.bx = (nx + VR_TW - 1) / VR_TW;
    L.by = (ny + VR_TH - 1) / VR_TH;
    L.nblocks = L.bx * L.by;
    const size_t plane = align256(L.N * 4), coarse = align256(L.Nc * 4);
    size_t o = 0;
    L.off_x = o; o += plane;
    L.off_y = o; o += plane;
    L.off_flag = o; o += 256;
    // resize: lo, hi, t per fine index, r0, r1 per coarse index; down-sampling: s, s1, f per coarse index
    L.off_tab = o; o += align256((size_t)(ny + nx) * 12 + (size_t)(ny / 2 + nx / 2) * 20);
    L.shared = o;
    o = 0;
    L.f_mask = o; o += plane;
    L.f_zin = o; o += plane;
    L.f_zdx = o; o += plane;
    L.f_zdy = o; o += plane;
    L.f_gd = o; o += plane;
    L.f_gz = o; o += plane;
    L.f_I0 = o; o += align256((size_t)ih0 * iw0 * 4);
    L.f_I1 = o; o += align256((size_t)ih1 * iw1 * 4);
    L.f_zc = o; o += coarse;
    L.f_m = o; o += coarse;
    L.f_v = o; o += coarse;
    L.f_partial = o; o += align256((size_t)L.nblocks * 16);
    L.frame = o;
    L.total = L.shared + (size_t)nb * L.frame;
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

// cv.resize's INTER_LINEAR rule per axis (refinement.downsample_linear): f = (float)((d + 0.5) * (in / out) - 0.5) from fp64,
// s = floor(f), f -= s; s < 0: s = 0, f = 0; s >= in - 1: s = in - 1, f = 0; s1 = min(s + 1, in - 1)
static void vref_down_tables(int in, int out, std::vector<int>& s, std::vector<int>& s1, std::vector<float>& f)
{
    s.resize(out); s1.resize(out); f.resize(out);
    const double scale = (double)in / (double)out;
    for (int d = 0; d < out; ++d) {
        float fv = (float)(((double)d + 0.5) * scale - 0.5);
        int sv = (int)floorf(fv);
        fv = fv - (float)sv;
        if (sv < 0) { sv = 0; fv = 0.0f; }
        if (sv >= in - 1) { sv = in - 1; fv = 0.0f; }
        s[d] = sv;
        s1[d] = sv + 1 < in - 1 ? sv + 1 : in - 1;
        f[d] = fv;
    }
}

}  // namespace wass

using namespace wass;

struct wass_vref {
    wass_ctx* c = nullptr;
    bool batch = false;          // made by wass_vref_batch_create: owns mask, pictures, Zc, m, v of nb frames
    int nb = 1, n = 0;           // frames allocated, frames loaded
    int64_t step = 0;            // Adam steps the loaded frames have taken (batch)
    double baseline = 1.0;       // of the last load (batch)
    int ny = 0, nx = 0, hc = 0, wc = 0, ih0 = 0, iw0 = 0, ih1 = 0, iw1 = 0;
    VrefLayout L = {};
    char* mem = nullptr;
    double* trace = nullptr;     // device rows of the loss trace [nb][trace_cap][4], grown on demand
    int trace_cap = 0;
    VrefCam cam = {};
    VrefKer ker = {}, kerf = {};
    VrefAxis ay = {}, ax = {};
    VrefDown dy = {}, dx = {};
    float* p(size_t off) const { return (float*)(mem + off); }                 // shared
    float* fp(size_t off) const { return (float*)(mem + L.shared + off); }     // frame 0; frame f: + f * fs()
    size_t fs() const { return L.frame / 4; }
    int* flag() const { return (int*)(mem + L.off_flag); }
};

namespace {

VrefFwd vref_fwd_args(const wass_vref* h)
{
    VrefFwd a;
    memset(&a, 0, sizeof a);
    a.fs = h->fs();
    a.Ny = h->ny; a.Nx = h->nx; a.Wc = h->wc;
    a.Xb = h->p(h->L.off_x); a.Yb = h->p(h->L.off_y); a.mask = h->fp(h->L.f_mask);
    a.I0 = h->fp(h->L.f_I0); a.H0 = h->ih0; a.W0 = h->iw0;
    a.I1 = h->fp(h->L.f_I1); a.H1 = h->ih1; a.W1 = h->iw1;
    a.cD = (float)(2.0 / (255.0 * (double)h->L.N));
    return a;
}

// n: the frames of the launch (grid z).  A pointer of the caller's (n = 1 only) needs no stride.
void vref_launch_forward(const wass_vref* h, const VrefFwd& a, bool coarse, int n, hipStream_t s)
{
    const dim3 grid((unsigned)h->L.bx, (unsigned)h->L.by, (unsigned)n);
    if (coarse) hipLaunchKernelGGL(k_vref_forward<true>, grid, dim3(VR_THREADS), 0, s, a, h->ay, h->ax, h->cam, h->ker);
    else hipLaunchKernelGGL(k_vref_forward<false>, grid, dim3(VR_THREADS), 0, s, a, h->ay, h->ax, h->cam, h->ker);
}

// row `row` of every frame's trace
void vref_launch_loss(const wass_vref* h, double alpha, double steps, int row, int n, hipStream_t s)
{
    hipLaunchKernelGGL(k_vref_loss, dim3((unsigned)n), dim3(VR_THREADS), 0, s, (const double*)h->fp(h->L.f_partial), h->fs(), h->L.nblocks,
                       (double)h->L.N, alpha, steps, h->trace + 4 * (size_t)row, 4 * (size_t)h->trace_cap);
}

// gd, Zdx, Zdy of the handle -> gZ of the handle -> gC and / or the Adam step
void vref_launch_backward(const wass_vref* h, double alpha, float* d_gC, float* d_Zc, const VrefAdam* ad, int n, hipStream_t s)
{
    const float cS = (float)(2.0 * alpha / (double)h->L.N);
    const VrefLayout& L = h->L;
    hipLaunchKernelGGL(k_vref_smooth, dim3((unsigned)L.bx, (unsigned)L.by, (unsigned)n), dim3(VR_THREADS), 0, s, (const float*)h->fp(L.f_zdx),
                       (const float*)h->fp(L.f_zdy), (const float*)h->fp(L.f_gd), h->fs(), h->ny, h->nx, cS, h->kerf, h->fp(L.f_gz));
    const dim3 grid((unsigned)((h->wc + 63) / 64), (unsigned)((h->hc + 3) / 4), (unsigned)n);
    VrefAdam none = {};
    if (ad) hipLaunchKernelGGL(k_vref_step<true>, grid, dim3(VR_THREADS), 0, s, (const float*)h->fp(L.f_gz), h->fs(), h->nx, h->hc, h->wc, h->ay, h->ax, d_gC, d_Zc, *ad);
    else hipLaunchKernelGGL(k_vref_step<false>, grid, dim3(VR_THREADS), 0, s, (const float*)h->fp(L.f_gz), h->fs(), h->nx, h->hc, h->wc, h->ay, h->ax, d_gC, d_Zc, none);
}

int vref_flag_reset(wass_vref* h, hipStream_t s)
{
    WASS_HIP(h->c, hipMemsetAsync(h->flag(), 0x7f, 4, s));
    return WASS_OK;
}

// the flag after everything enqueued so far: the first frame that left its index there, or -1.  synchronises
int vref_flag_read(wass_vref* h, hipStream_t s, int* frame)
{
    int v = VR_NO_FRAME;
    WASS_HIP(h->c, hipGetLastError());
    WASS_HIP(h->c, hipMemcpyAsync(&v, h->flag(), 4, hipMemcpyDeviceToHost, s));
    WASS_HIP(h->c, hipStreamSynchronize(s));
    *frame = v == VR_NO_FRAME ? -1 : v;
    return WASS_OK;
}

void vref_launch_finite(wass_vref* h, const float* a, size_t total, size_t per, hipStream_t s)
{
    hipLaunchKernelGGL(k_vref_finite, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, a, total, per, h->flag());
}

// every one of the `count` planes of n floats finite?  synchronises
int vref_all_finite(wass_vref* h, const float* const* planes, int count, size_t n, const char* what)
{
    wass_ctx* c = h->c;
    hipStream_t s = c->ts();
    int rc = vref_flag_reset(h, s), bad = -1;
    if (rc) return rc;
    for (int k = 0; k < count; ++k) vref_launch_finite(h, planes[k], n, n, s);
    if ((rc = vref_flag_read(h, s, &bad))) return rc;
    if (bad >= 0) return set_err(c, WASS_ERR_INVALID_ARG, "%s holds a value that is not finite", what);
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
    if (hipMalloc((void**)&h->trace, (size_t)h->nb * rows * 32) != hipSuccess) {
        h->trace = nullptr;
        return set_err(c, WASS_ERR_NO_MEMORY, "hipMalloc of %d x %d rows of the loss trace failed", h->nb, rows);
    }
    h->trace_cap = rows;
    return WASS_OK;
}

void vref_copy_frames(float* dst, size_t ds, const float* src, size_t ss, size_t count, int n, hipStream_t s)
{
    hipLaunchKernelGGL(k_vref_copy, dim3((unsigned)((count + 255) / 256), 1, (unsigned)n), dim3(256), 0, s, dst, ds, src, ss, count);
}

// The loop of both optimize entries: `iters` steps of n frames whose Zc, m, v start at the given pointers with the handle's frame
// stride (the caller's own planes when n = 1), from Adam step `step`.  trace: host [n][trace_cap][4].  Synchronises.
int vref_run(wass_vref* h, int n, float* d_Zc, float* d_m, float* d_v, int64_t step, int iters, double alpha, double lr, double eps,
             int report_every, double* trace, int trace_cap, int* n_trace, float* d_Zout)
{
    wass_ctx* c = h->c;
    // the rows of the trace: before the first step, after step ii (from 0) where ii % report_every == 0, after the last
    const int every = report_every > 0 ? report_every : 0;
    const int rows_max = 2 + (every ? (iters + every - 1) / every : 0);
    const bool want = trace && trace_cap > 0;
    int rc;
    if (want && (rc = vref_trace_rows(h, rows_max))) return rc;
    hipStream_t s = c->ts();
    const VrefLayout& L = h->L;
    VrefFwd base = vref_fwd_args(h);
    base.Zc = d_Zc;
    int rows = 0;
    for (int it = 0; it < iters; ++it) {
        VrefFwd a = base;
        a.Zdx = h->fp(L.f_zdx); a.Zdy = h->fp(L.f_zdy); a.gd = h->fp(L.f_gd);
        const bool report = want && rows < trace_cap && (it == 0 || (every && (it - 1) % every == 0));
        if (report) a.partial = (double*)h->fp(L.f_partial);
        vref_launch_forward(h, a, true, n, s);
        if (report) vref_launch_loss(h, alpha, (double)it, rows++, n, s);
        const double t = (double)(step + it + 1);
        VrefAdam ad;
        ad.m = d_m; ad.v = d_v;
        ad.c1 = (float)(1.0 - VR_B1); ad.c2 = (float)(1.0 - VR_B2);
        ad.lr_t = (float)(lr * sqrt(1.0 - pow(VR_B2, t)) / (1.0 - pow(VR_B1, t)));
        ad.eps = (float)eps;
        vref_launch_backward(h, alpha, nullptr, d_Zc, &ad, n, s);
    }
    const bool last_row = want && rows < trace_cap && (iters > 0 || rows == 0);
    if (last_row || d_Zout) {
        VrefFwd a = base;
        a.Zmasked = d_Zout;
        if (last_row) a.partial = (double*)h->fp(L.f_partial);
        vref_launch_forward(h, a, true, n, s);
        if (last_row) vref_launch_loss(h, alpha, (double)iters, rows++, n, s);
    }
    WASS_HIP(c, hipGetLastError());
    if (rows)
        for (int f = 0; f < n; ++f)
            WASS_HIP(c, hipMemcpyAsync(trace + 4 * (size_t)f * trace_cap, h->trace + 4 * (size_t)f * h->trace_cap, (size_t)rows * 32,
                                       hipMemcpyDeviceToHost, s));
    WASS_HIP(c, hipStreamSynchronize(s));
    if (n_trace) *n_trace = rows;
    return WASS_OK;
}

// the handle with everything the frames share: XX / b, YY / b, the cameras, the kernels, the axis tables.  Synchronises.
int vref_new(wass_ctx* c, int nb, int ny, int nx, const float* d_xb, const float* d_yb, const double Rp2c[9], const double Tp2c[3],
             const double P0cam[12], const double P1cam[12], int ih0, int iw0, int ih1, int iw1, const float* kernels, wass_vref** out)
{
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
    h->c = c; h->nb = nb; h->ny = ny; h->nx = nx; h->hc = ny / 2; h->wc = nx / 2;
    h->ih0 = ih0; h->iw0 = iw0; h->ih1 = ih1; h->iw1 = iw1;
    h->L = vref_layout(nb, ny, nx, ih0, iw0, ih1, iw1);
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
    // the resize tables: per fine index lo, hi, t; per coarse index the range of fine indices; then the down-sampling's s, s1, f
    std::vector<int> lo[2], hi[2], r0[2], r1[2], ds[2], ds1[2];
    std::vector<float> t[2], df[2];
    vref_axis_tables(h->hc, ny, lo[0], hi[0], t[0], r0[0], r1[0]);
    vref_axis_tables(h->wc, nx, lo[1], hi[1], t[1], r0[1], r1[1]);
    vref_down_tables(ny, h->hc, ds[0], ds1[0], df[0]);
    vref_down_tables(nx, h->wc, ds[1], ds1[1], df[1]);
    hipStream_t s = c->ts();
    char* tab = h->mem + L.off_tab;
    bool ok = true;
    auto put = [&](const void* src, size_t count) {
        const void* at = tab;
        ok = ok && hipMemcpyAsync(tab, src, count * 4, hipMemcpyHostToDevice, s) == hipSuccess;
        tab += count * 4;
        return at;
    };
    VrefAxis* axes[2] = {&h->ay, &h->ax};
    VrefDown* downs[2] = {&h->dy, &h->dx};
    for (int k = 0; k < 2; ++k) {
        const size_t nf = lo[k].size(), nc = r0[k].size();
        VrefAxis& A = *axes[k];
        A.lo = (const int*)put(lo[k].data(), nf);
        A.hi = (const int*)put(hi[k].data(), nf);
        A.t = (const float*)put(t[k].data(), nf);
        A.r0 = (const int*)put(r0[k].data(), nc);
        A.r1 = (const int*)put(r1[k].data(), nc);
        VrefDown& D = *downs[k];
        D.s = (const int*)put(ds[k].data(), nc);
        D.s1 = (const int*)put(ds1[k].data(), nc);
        D.f = (const float*)put(df[k].data(), nc);
    }
    const hipMemcpyKind dd = hipMemcpyDeviceToDevice;
    ok = ok && hipMemcpyAsync(h->mem + L.off_x, d_xb, L.N * 4, dd, s) == hipSuccess;
    ok = ok && hipMemcpyAsync(h->mem + L.off_y, d_yb, L.N * 4, dd, s) == hipSuccess;
    ok = ok && hipStreamSynchronize(s) == hipSuccess;                              // the host tables leave scope
    int rc = ok ? WASS_OK : set_err(c, WASS_ERR_DEVICE, "refinement set-up failed: %s", hipGetErrorString(hipGetLastError()));
    if (rc) {
        wass_vref_destroy(h);
        return rc;
    }
    *out = h;
    return WASS_OK;
}

}  // namespace

extern "C" {

int wass_vref_scratch_bytes(int ny, int nx, int ih0, int iw0, int ih1, int iw1, size_t* bytes)
{
    return wass_vref_batch_scratch_bytes(1, ny, nx, ih0, iw0, ih1, iw1, bytes);
}

int wass_vref_batch_scratch_bytes(int nb, int ny, int nx, int ih0, int iw0, int ih1, int iw1, size_t* bytes)
{
    if (!bytes || nb < 1 || nb > VR_MAX_BATCH || !vref_dims_ok(ny, nx, ih0, iw0, ih1, iw1)) return WASS_ERR_INVALID_ARG;
    *bytes = vref_layout(nb, ny, nx, ih0, iw0, ih1, iw1).total;
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

void wass_vref_batch_destroy(wass_vref* h) { wass_vref_destroy(h); }

int wass_vref_create(wass_ctx* c, int ny, int nx, const float* d_xb, const float* d_yb, const float* d_mask, const double Rp2c[9],
                     const double Tp2c[3], const double P0cam[12], const double P1cam[12], const float* d_I0, int ih0, int iw0,
                     const float* d_I1, int ih1, int iw1, const float* kernels, wass_vref** out)
{
    if (!c) return WASS_ERR_INVALID_ARG;
    if (!out) return set_err(c, WASS_ERR_INVALID_ARG, "null argument");
    *out = nullptr;
    if (!d_xb || !d_yb || !d_mask || !Rp2c || !Tp2c || !P0cam || !P1cam || !d_I0 || !d_I1 || !kernels)
        return set_err(c, WASS_ERR_INVALID_ARG, "null argument");
    wass_vref* h = nullptr;
    int rc = vref_new(c, 1, ny, nx, d_xb, d_yb, Rp2c, Tp2c, P0cam, P1cam, ih0, iw0, ih1, iw1, kernels, &h);
    if (rc) return rc;
    const VrefLayout& L = h->L;
    hipStream_t s = c->ts();
    const hipMemcpyKind dd = hipMemcpyDeviceToDevice;
    bool ok = hipMemcpyAsync(h->fp(L.f_mask), d_mask, L.N * 4, dd, s) == hipSuccess;
    ok = ok && hipMemcpyAsync(h->fp(L.f_I0), d_I0, (size_t)ih0 * iw0 * 4, dd, s) == hipSuccess;
    ok = ok && hipMemcpyAsync(h->fp(L.f_I1), d_I1, (size_t)ih1 * iw1 * 4, dd, s) == hipSuccess;
    rc = ok ? WASS_OK : set_err(c, WASS_ERR_DEVICE, "refinement set-up failed: %s", hipGetErrorString(hipGetLastError()));
    if (!rc) {
        const float* planes[3] = {h->p(L.off_x), h->p(L.off_y), h->fp(L.f_mask)};
        rc = vref_all_finite(h, planes, 3, L.N, "XX / b, YY / b or the mask");
    }
    if (!rc) {
        const float* p0[1] = {h->fp(L.f_I0)};
        const float* p1[1] = {h->fp(L.f_I1)};
        rc = vref_all_finite(h, p0, 1, (size_t)ih0 * iw0, "picture 0");
        if (!rc) rc = vref_all_finite(h, p1, 1, (size_t)ih1 * iw1, "picture 1");
    }
    if (rc) {
        wass_vref_destroy(h);
        return rc;
    }
    h->n = 1;
    *out = h;
    return WASS_OK;
}

// the single entries take a handle of wass_vref_create only: a batch handle's frames are loaded, not passed in
#define VREF_SINGLE(h)                                                                                             \
    do {                                                                                                           \
        if (!(h)) return WASS_ERR_INVALID_ARG;                                                                     \
        if ((h)->batch) return set_err((h)->c, WASS_ERR_INVALID_ARG, "a handle of wass_vref_batch_create: use the wass_vref_batch_ entries"); \
    } while (0)
#define VREF_BATCH(h)                                                                                              \
    do {                                                                                                           \
        if (!(h)) return WASS_ERR_INVALID_ARG;                                                                     \
        if (!(h)->batch) return set_err((h)->c, WASS_ERR_INVALID_ARG, "a handle of wass_vref_create: use the wass_vref_ entries"); \
    } while (0)

int wass_vref_sample(wass_vref* h, const float* d_Z, float* d_I0s, float* d_I1s, float* d_uv)
{
    VREF_SINGLE(h);
    wass_ctx* c = h->c;
    if (!d_Z || !d_I0s || !d_I1s || !d_uv) return set_err(c, WASS_ERR_INVALID_ARG, "null argument");
    WASS_HIP(c, hipSetDevice(c->device));
    const float* planes[1] = {d_Z};
    int rc = vref_all_finite(h, planes, 1, h->L.N, "Z");
    if (rc) return rc;
    VrefFwd a = vref_fwd_args(h);
    a.Z = d_Z; a.I0s = d_I0s; a.I1s = d_I1s; a.uv = d_uv;
    vref_launch_forward(h, a, false, 1, c->ts());
    WASS_HIP(c, hipGetLastError());
    WASS_HIP(c, hipStreamSynchronize(c->ts()));
    return WASS_OK;
}

int wass_vref_zgrad(wass_vref* h, const float* d_Z, float* d_Zdx, float* d_Zdy)
{
    VREF_SINGLE(h);
    wass_ctx* c = h->c;
    if (!d_Z || !d_Zdx || !d_Zdy) return set_err(c, WASS_ERR_INVALID_ARG, "null argument");
    WASS_HIP(c, hipSetDevice(c->device));
    const float* planes[1] = {d_Z};
    int rc = vref_all_finite(h, planes, 1, h->L.N, "Z");
    if (rc) return rc;
    VrefFwd a = vref_fwd_args(h);
    a.Z = d_Z; a.Zdx = d_Zdx; a.Zdy = d_Zdy;
    vref_launch_forward(h, a, false, 1, c->ts());
    WASS_HIP(c, hipGetLastError());
    WASS_HIP(c, hipStreamSynchronize(c->ts()));
    return WASS_OK;
}

int wass_vref_loss(wass_vref* h, const float* d_Z, double* data_loss, double* smoothness_loss)
{
    VREF_SINGLE(h);
    wass_ctx* c = h->c;
    if (!d_Z || !data_loss || !smoothness_loss) return set_err(c, WASS_ERR_INVALID_ARG, "null argument");
    WASS_HIP(c, hipSetDevice(c->device));
    const float* planes[1] = {d_Z};
    int rc = vref_all_finite(h, planes, 1, h->L.N, "Z");
    if (rc) return rc;
    if ((rc = vref_trace_rows(h, 1))) return rc;
    hipStream_t s = c->ts();
    VrefFwd a = vref_fwd_args(h);
    a.Z = d_Z; a.partial = (double*)h->fp(h->L.f_partial);
    vref_launch_forward(h, a, false, 1, s);
    vref_launch_loss(h, 0.0, 0.0, 0, 1, s);
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
    VREF_SINGLE(h);
    wass_ctx* c = h->c;
    if (!d_Zc || !d_gC) return set_err(c, WASS_ERR_INVALID_ARG, "null argument");
    if (!isfinite(alpha)) return set_err(c, WASS_ERR_INVALID_ARG, "alpha is not finite");
    WASS_HIP(c, hipSetDevice(c->device));
    const float* planes[1] = {d_Zc};
    int rc = vref_all_finite(h, planes, 1, h->L.Nc, "Zc");
    if (rc) return rc;
    hipStream_t s = c->ts();
    VrefFwd a = vref_fwd_args(h);
    a.Zc = d_Zc; a.Zdx = h->fp(h->L.f_zdx); a.Zdy = h->fp(h->L.f_zdy); a.gd = h->fp(h->L.f_gd);
    vref_launch_forward(h, a, true, 1, s);
    vref_launch_backward(h, alpha, d_gC, nullptr, nullptr, 1, s);
    WASS_HIP(c, hipGetLastError());
    if (d_gZ) WASS_HIP(c, hipMemcpyAsync(d_gZ, h->fp(h->L.f_gz), h->L.N * 4, hipMemcpyDeviceToDevice, s));
    WASS_HIP(c, hipStreamSynchronize(s));
    return WASS_OK;
}

int wass_vref_adjoint(wass_vref* h, const float* d_Zdx, const float* d_Zdy, const float* d_gd, double alpha, float* d_gC, float* d_gZ)
{
    VREF_SINGLE(h);
    wass_ctx* c = h->c;
    if (!d_Zdx || !d_Zdy || !d_gd || !d_gC) return set_err(c, WASS_ERR_INVALID_ARG, "null argument");
    if (!isfinite(alpha)) return set_err(c, WASS_ERR_INVALID_ARG, "alpha is not finite");
    WASS_HIP(c, hipSetDevice(c->device));
    const float* planes[3] = {d_Zdx, d_Zdy, d_gd};
    int rc = vref_all_finite(h, planes, 3, h->L.N, "Zdx, Zdy or gd");
    if (rc) return rc;
    hipStream_t s = c->ts();
    const hipMemcpyKind dd = hipMemcpyDeviceToDevice;
    WASS_HIP(c, hipMemcpyAsync(h->fp(h->L.f_zdx), d_Zdx, h->L.N * 4, dd, s));
    WASS_HIP(c, hipMemcpyAsync(h->fp(h->L.f_zdy), d_Zdy, h->L.N * 4, dd, s));
    WASS_HIP(c, hipMemcpyAsync(h->fp(h->L.f_gd), d_gd, h->L.N * 4, dd, s));
    vref_launch_backward(h, alpha, d_gC, nullptr, nullptr, 1, s);
    WASS_HIP(c, hipGetLastError());
    if (d_gZ) WASS_HIP(c, hipMemcpyAsync(d_gZ, h->fp(h->L.f_gz), h->L.N * 4, dd, s));
    WASS_HIP(c, hipStreamSynchronize(s));
    return WASS_OK;
}

int wass_vref_optimize(wass_vref* h, float* d_Zc, float* d_m, float* d_v, int64_t* step, int iters, double alpha, double lr, double eps,
                       int report_every, double* trace, int trace_cap, int* n_trace, float* d_Zout)
{
    VREF_SINGLE(h);
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
    if ((rc = vref_run(h, 1, d_Zc, d_m, d_v, *step, iters, alpha, lr, eps, report_every, trace, trace_cap, n_trace, d_Zout))) return rc;
    *step += iters;
    return WASS_OK;
}

// ---- batches
int wass_vref_batch_create(wass_ctx* c, int nb, int ny, int nx, const float* d_xb, const float* d_yb, const double Rp2c[9], const double Tp2c[3],
                           const double P0cam[12], const double P1cam[12], int ih0, int iw0, int ih1, int iw1, const float* kernels,
                           wass_vref** out)
{
    if (!c) return WASS_ERR_INVALID_ARG;
    if (!out) return set_err(c, WASS_ERR_INVALID_ARG, "null argument");
    *out = nullptr;
    if (!d_xb || !d_yb || !Rp2c || !Tp2c || !P0cam || !P1cam || !kernels) return set_err(c, WASS_ERR_INVALID_ARG, "null argument");
    if (nb < 1 || nb > VR_MAX_BATCH) return set_err(c, WASS_ERR_INVALID_ARG, "a batch of %d frames: 1 .. %d", nb, VR_MAX_BATCH);
    wass_vref* h = nullptr;
    int rc = vref_new(c, nb, ny, nx, d_xb, d_yb, Rp2c, Tp2c, P0cam, P1cam, ih0, iw0, ih1, iw1, kernels, &h);
    if (rc) return rc;
    const float* planes[2] = {h->p(h->L.off_x), h->p(h->L.off_y)};
    if ((rc = vref_all_finite(h, planes, 2, h->L.N, "XX / b or YY / b"))) {
        wass_vref_destroy(h);
        return rc;
    }
    h->batch = true;
    *out = h;
    return WASS_OK;
}

int wass_vref_batch_load(wass_vref* h, int n, const float* d_Zi, const float* d_mask, const float* d_I0, const float* d_I1, double baseline)
{
    VREF_BATCH(h);
    wass_ctx* c = h->c;
    if (!d_Zi || !d_I0 || !d_I1) return set_err(c, WASS_ERR_INVALID_ARG, "null argument");
    if (n < 1 || n > h->nb) return set_err(c, WASS_ERR_INVALID_ARG, "%d frames into a handle of %d", n, h->nb);
    if (!isfinite(baseline) || baseline == 0.0) return set_err(c, WASS_ERR_INVALID_ARG, "the baseline must be finite and not 0");
    WASS_HIP(c, hipSetDevice(c->device));
    h->n = 0;                                            // nothing is loaded until this call has gone through
    hipStream_t s = c->ts();
    const VrefLayout& L = h->L;
    const size_t fs = h->fs(), n0 = (size_t)h->ih0 * h->iw0, n1 = (size_t)h->ih1 * h->iw1;
    int rc, bad = -1;
    const float* pics[2] = {d_I0, d_I1};
    const size_t counts[2] = {n0, n1};
    for (int k = 0; k < 2; ++k) {
        if ((rc = vref_flag_reset(h, s))) return rc;
        vref_launch_finite(h, pics[k], (size_t)n * counts[k], counts[k], s);
        if ((rc = vref_flag_read(h, s, &bad))) return rc;
        if (bad >= 0) return set_err(c, WASS_ERR_INVALID_ARG, "picture %d of frame %d holds a value that is not finite", k, bad);
    }
    if ((rc = vref_flag_reset(h, s))) return rc;
    hipLaunchKernelGGL(k_vref_ingest, dim3((unsigned)((L.N + 255) / 256), 1, (unsigned)n), dim3(256), 0, s, d_Zi, d_mask, L.N, baseline, fs,
                       h->fp(L.f_mask), h->fp(L.f_zin), h->flag());
    vref_copy_frames(h->fp(L.f_I0), fs, d_I0, n0, n0, n, s);
    vref_copy_frames(h->fp(L.f_I1), fs, d_I1, n1, n1, n, s);
    hipLaunchKernelGGL(k_vref_down, dim3((unsigned)((h->wc + 63) / 64), (unsigned)((h->hc + 3) / 4), (unsigned)n), dim3(VR_THREADS), 0, s,
                       (const float*)h->fp(L.f_zin), fs, h->nx, h->hc, h->wc, h->dy, h->dx, h->fp(L.f_zc), h->fp(L.f_m), h->fp(L.f_v));
    if ((rc = vref_flag_read(h, s, &bad))) return rc;
    if (bad >= 0) return set_err(c, WASS_ERR_INVALID_ARG, "frame %d holds a value inside its mask that is not finite", bad);
    h->n = n;
    h->step = 0;
    h->baseline = baseline;
    return WASS_OK;
}

int wass_vref_batch_set_state(wass_vref* h, const float* d_Zc, const float* d_m, const float* d_v, int64_t step)
{
    VREF_BATCH(h);
    wass_ctx* c = h->c;
    if (h->n < 1) return set_err(c, WASS_ERR_INVALID_ARG, "no frames are loaded");
    if (!d_Zc || !d_m || !d_v) return set_err(c, WASS_ERR_INVALID_ARG, "null argument");
    if (step < 0) return set_err(c, WASS_ERR_INVALID_ARG, "the Adam state's step count is negative");
    WASS_HIP(c, hipSetDevice(c->device));
    hipStream_t s = c->ts();
    const VrefLayout& L = h->L;
    int rc = vref_flag_reset(h, s), bad = -1;
    if (rc) return rc;
    const float* src[3] = {d_Zc, d_m, d_v};
    for (int k = 0; k < 3; ++k) vref_launch_finite(h, src[k], (size_t)h->n * L.Nc, L.Nc, s);
    if ((rc = vref_flag_read(h, s, &bad))) return rc;
    if (bad >= 0) return set_err(c, WASS_ERR_INVALID_ARG, "Zc or the Adam state of frame %d holds a value that is not finite", bad);
    const size_t dst[3] = {L.f_zc, L.f_m, L.f_v};
    for (int k = 0; k < 3; ++k) vref_copy_frames(h->fp(dst[k]), h->fs(), src[k], L.Nc, L.Nc, h->n, s);
    WASS_HIP(c, hipGetLastError());
    WASS_HIP(c, hipStreamSynchronize(s));
    h->step = step;
    return WASS_OK;
}

int wass_vref_batch_get_state(wass_vref* h, float* d_Zc, float* d_m, float* d_v, int64_t* step)
{
    VREF_BATCH(h);
    wass_ctx* c = h->c;
    if (h->n < 1) return set_err(c, WASS_ERR_INVALID_ARG, "no frames are loaded");
    if (!d_Zc || !d_m || !d_v || !step) return set_err(c, WASS_ERR_INVALID_ARG, "null argument");
    WASS_HIP(c, hipSetDevice(c->device));
    hipStream_t s = c->ts();
    const VrefLayout& L = h->L;
    float* dst[3] = {d_Zc, d_m, d_v};
    const size_t src[3] = {L.f_zc, L.f_m, L.f_v};
    for (int k = 0; k < 3; ++k) vref_copy_frames(dst[k], L.Nc, h->fp(src[k]), h->fs(), L.Nc, h->n, s);
    WASS_HIP(c, hipGetLastError());
    WASS_HIP(c, hipStreamSynchronize(s));
    *step = h->step;
    return WASS_OK;
}

int wass_vref_batch_optimize(wass_vref* h, int iters, double alpha, double lr, double eps, int report_every, double* trace, int trace_cap,
                             int* n_trace)
{
    VREF_BATCH(h);
    wass_ctx* c = h->c;
    if (n_trace) *n_trace = 0;
    if (h->n < 1) return set_err(c, WASS_ERR_INVALID_ARG, "no frames are loaded");
    if (iters < 0) return set_err(c, WASS_ERR_INVALID_ARG, "iters = %d: not negative", iters);
    if (!isfinite(alpha) || !isfinite(lr) || !isfinite(eps)) return set_err(c, WASS_ERR_INVALID_ARG, "alpha, lr or eps is not finite");
    if (trace_cap < 0 || (trace_cap > 0 && !trace) || (trace && !n_trace)) return set_err(c, WASS_ERR_INVALID_ARG, "bad trace arguments");
    WASS_HIP(c, hipSetDevice(c->device));
    const VrefLayout& L = h->L;
    int rc = vref_run(h, h->n, h->fp(L.f_zc), h->fp(L.f_m), h->fp(L.f_v), h->step, iters, alpha, lr, eps, report_every, trace, trace_cap, n_trace,
                      nullptr);
    if (rc) return rc;
    h->step += iters;
    return WASS_OK;
}

int wass_vref_batch_result(wass_vref* h, float* d_out, float* d_Z)
{
    VREF_BATCH(h);
    wass_ctx* c = h->c;
    if (h->n < 1) return set_err(c, WASS_ERR_INVALID_ARG, "no frames are loaded");
    if (!d_out) return set_err(c, WASS_ERR_INVALID_ARG, "null argument");
    WASS_HIP(c, hipSetDevice(c->device));
    hipStream_t s = c->ts();
    const VrefLayout& L = h->L;
    hipLaunchKernelGGL(k_vref_finish, dim3((unsigned)((h->nx + 63) / 64), (unsigned)((h->ny + 3) / 4), (unsigned)h->n), dim3(256), 0, s,
                       (const float*)h->fp(L.f_zc), (const float*)h->fp(L.f_mask), h->fs(), h->ny, h->nx, h->wc, h->ay, h->ax, h->baseline, d_out, d_Z);
    WASS_HIP(c, hipGetLastError());
    WASS_HIP(c, hipStreamSynchronize(s));
    return WASS_OK;
}

}  // extern "C"
