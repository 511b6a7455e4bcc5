// grid_linear.hip -- wassgridsurface --ia LinearND (gridding/wassgridsurface/wassgridsurface.py:437-482): the value at a node of
// the lattice is the plane through the three cloud points of the Delaunay triangle that holds it.  The reference asks scipy's
// LinearNDInterpolator (Qhull) for it; here no triangulation is built.  Every node walks the implicit triangulation (DESIGN.md
// "LinearND"): nearest point a, its nearest point b (a Delaunay edge), the apex of that edge on the node's side, and across
// the edge that separates the node from the triangle until it is inside.  What makes the result a definition and not a
// procedure is the certificate at the end: the node lies in the triangle and no other point lies in its circumcircle, both
// decided by fp64 determinants whose magnitudes exceed their rounding bounds (LIN_EO, LIN_EI below).  A certified triangle is the
// Delaunay triangle whatever path found it; everything else is flagged.
//
// Stages, all on c->ts(): bucket (cell of an acceleration grid per point: count, the scan of grid.hip, fill, duplicates out),
// hull (extremes in 32 directions, their polygon, the points not certainly inside it to the host, monotone chain there, the hull
// back), walk (one lane per node, a wave is an 8 x 8 patch of nodes).  Nothing depends on the order inside a bucket: every tie
// goes to the lower index.  The walk's helpers are __host__ __device__: tests/native/linearnd_host.hip runs the same source on the
// CPU under the host's sanitizers.
#include <algorithm>
#include <math.h>
#include <vector>

#include "common.h"
#include "grid_align.h"

namespace wass {

constexpr unsigned int LIN_NONE = 0xFFFFFFFFu;        // no point / a duplicate that does not exist / outside the area
constexpr double LIN_EPS = 1.1102230246251565e-16;    // 2^-53, the unit roundoff of fp64
// Rounding bounds of the two determinants (derived in DESIGN.md "LinearND"): |orient - exact| <= LIN_EO * S with S the sum of
// the magnitudes of its two products, |incircle - exact| <= LIN_EI * P with P its permanent, both as computed.
constexpr double LIN_EO = 5.0 * LIN_EPS;
constexpr double LIN_EI = 12.0 * LIN_EPS;
constexpr int LIN_NDIR = 32;                          // directions of the extreme-point reduction
constexpr int LIN_DEFAULT_STEPS = 256;                // walk steps before flag 3
constexpr size_t LIN_HANDOVER = 4096;                 // hull candidates that come to the host with their count, in one copy

struct LinPt { double x, y; unsigned int i, s; };     // a cloud point: coordinates, original index, slot in the bucketed arrays

// The acceleration grid and the bucketed cloud.  cell_x / cell_y are monotone in the coordinate (a subtraction, a product with a
// positive constant, floor, two clamps), so the cells f(lo) .. f(hi) hold every point with lo <= x <= hi whatever the roundings.
struct LinAccel {
    double xmin, ymin, xmax, ymax, ipx, ipy, hy;      // hy = 1 / ipy, the height of a row of cells (0: the extent has no height)
    int gw, gh;
    const unsigned int* off;                          // gw * gh + 1 entries: the slots of cell c are off[c] .. off[c + 1]
    const double *bx, *by, *bz;
    const unsigned int* bidx;                         // original index per slot, LIN_NONE for a duplicate
    __host__ __device__ __forceinline__ int cell_x(double x) const { return (int)fmin(fmax(floor((x - xmin) * ipx), 0.0), (double)(gw - 1)); }
    __host__ __device__ __forceinline__ int cell_y(double y) const { return (int)fmin(fmax(floor((y - ymin) * ipy), 0.0), (double)(gh - 1)); }
};

struct LinWalkArgs {
    LinAccel A;
    const double *hx, *hy;                            // the convex hull, counter-clockwise, strict turns only
    int nh;
    int W, H, npx;                                    // node lattice; patches of 8 x 8 nodes per row of patches
    double xmin, xmax, ymin, ymax, stepx, stepy;      // numpy's linspace: i * step + start, the last node is stop itself
    int max_steps;
    double* out;
    uint8_t* flags;
    unsigned int* counts;                             // [4] nodes per flag
};

struct LinDirs { double dx[LIN_NDIR], dy[LIN_NDIR]; };

// orient(A, B, C) = (A - C) x (B - C), the local origin is the LAST argument: > 0 when A, B, C turn counter-clockwise.
// S receives |(ax - cx)(by - cy)| + |(ay - cy)(bx - cx)|.  Swapping A and B negates the result exactly.
__host__ __device__ __forceinline__ double lin_orient(double ax, double ay, double bx, double by, double cx, double cy, double& S)
{
    const double acx = ax - cx, acy = ay - cy, bcx = bx - cx, bcy = by - cy;
    const double t1 = acx * bcy, t2 = acy * bcx;
    S = fabs(t1) + fabs(t2);
    return t1 - t2;
}

// incircle(A, B, C, D), the local origin is D: > 0 when D lies inside the circle through the counter-clockwise A, B, C.
// P receives the permanent.  The order of operations is the one written here, nowhere contracted.
__host__ __device__ __forceinline__ double lin_incircle(double ax, double ay, double bx, double by, double cx, double cy, double dx, double dy, double& P)
{
    const double adx = ax - dx, ady = ay - dy, bdx = bx - dx, bdy = by - dy, cdx = cx - dx, cdy = cy - dy;
    const double bdxcdy = bdx * cdy, cdxbdy = cdx * bdy, alift = adx * adx + ady * ady;
    const double cdxady = cdx * ady, adxcdy = adx * cdy, blift = bdx * bdx + bdy * bdy;
    const double adxbdy = adx * bdy, bdxady = bdx * ady, clift = cdx * cdx + cdy * cdy;
    P = ((fabs(bdxcdy) + fabs(cdxbdy)) * alift + (fabs(cdxady) + fabs(adxcdy)) * blift) + (fabs(adxbdy) + fabs(bdxady)) * clift;
    return (alift * (bdxcdy - cdxbdy) + blift * (cdxady - adxcdy)) + clift * (adxbdy - bdxady);
}

// ---------------------------------------------------------------------------------------------------------------- bucket
// the aligned cloud of a resident mesh (grid_align's expressions); an invalid point becomes NaN and is dropped by the area mask
__global__ void __launch_bounds__(256) k_lin_align(const uint8_t* __restrict__ valid, const double* __restrict__ X, const double* __restrict__ Y,
                                                   const double* __restrict__ Z, size_t n, GridDev g, double* __restrict__ ax,
                                                   double* __restrict__ ay, double* __restrict__ az)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double x = __builtin_nan(""), y = x, z = x;
    if (valid[i]) grid_align(g, X[i], Y[i], Z[i], x, y, z);
    ax[i] = x; ay[i] = y; az[i] = z;
}

// the reference's area_mask, closed on every side; NaN and infinities fail it
__global__ void __launch_bounds__(256) k_lin_count(const double* __restrict__ X, const double* __restrict__ Y, size_t n, LinAccel A,
                                                   unsigned int* __restrict__ pcell, unsigned int* __restrict__ cnt)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double x = X[i], y = Y[i];
    unsigned int cell = LIN_NONE;
    if (x >= A.xmin && x <= A.xmax && y >= A.ymin && y <= A.ymax) {
        cell = (unsigned int)A.cell_y(y) * (unsigned int)A.gw + (unsigned int)A.cell_x(x);
        atomicAdd(&cnt[cell], 1u);
    }
    pcell[i] = cell;
}

__global__ void __launch_bounds__(256) k_lin_fill(const double* __restrict__ X, const double* __restrict__ Y, const double* __restrict__ Z,
                                                  const unsigned int* __restrict__ pcell, size_t n, const unsigned int* __restrict__ off,
                                                  unsigned int* __restrict__ fill, double* __restrict__ bx, double* __restrict__ by,
                                                  double* __restrict__ bz, unsigned int* __restrict__ braw)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const unsigned int c = pcell[i];
    if (c == LIN_NONE) return;
    const unsigned int s = off[c] + atomicAdd(&fill[c], 1u);
    bx[s] = X[i]; by[s] = Y[i]; bz[s] = Z[i]; braw[s] = (unsigned int)i;
}

// Of several points with exactly the same (x, y) the lowest index stands: every point looks through its own cell (equal
// coordinates share a cell) and writes its index, or LIN_NONE, into its slot of bidx.  braw is only read, bidx only written.
__global__ void __launch_bounds__(256) k_lin_dedupe(const double* __restrict__ X, const double* __restrict__ Y, const unsigned int* __restrict__ pcell,
                                                    size_t n, const unsigned int* __restrict__ off, const double* __restrict__ bx,
                                                    const double* __restrict__ by, const unsigned int* __restrict__ braw,
                                                    unsigned int* __restrict__ bidx, unsigned int* __restrict__ counters)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const unsigned int c = pcell[i];
    if (c == LIN_NONE) return;
    const double x = X[i], y = Y[i];
    const unsigned int s1 = off[c + 1];
    unsigned int mine = LIN_NONE;
    bool dup = false;
    for (unsigned int s = off[c]; s < s1; ++s) {
        const unsigned int j = braw[s];
        if (j == (unsigned int)i) mine = s;
        else if (j < (unsigned int)i && bx[s] == x && by[s] == y) dup = true;
    }
    if (mine == LIN_NONE) return;                     // cannot happen: the fill put this point into its cell
    bidx[mine] = dup ? LIN_NONE : (unsigned int)i;
    if (!dup) atomicAdd(&counters[4], 1u);
}

// ---------------------------------------------------------------------------------------------------------------- hull
// pass 1: the largest d . p per direction (order keys; 0 = nothing seen).  Which point wins a rounding tie does not matter: any
// 32 cloud points span a polygon inside the hull.
__global__ void __launch_bounds__(256) k_hull_max(const double* __restrict__ bx, const double* __restrict__ by, const unsigned int* __restrict__ bidx,
                                                  const unsigned int* __restrict__ off, size_t ng, LinDirs D, unsigned long long* __restrict__ maxkey)
{
    const size_t s = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= off[ng] || bidx[s] == LIN_NONE) return;
    const double x = bx[s], y = by[s];
    for (int k = 0; k < LIN_NDIR; ++k) {
        const unsigned long long key = order_key(D.dx[k] * x + D.dy[k] * y);
        if (key > maxkey[k]) atomicMax(&maxkey[k], key);
    }
}
// pass 2: who reached it, the lowest index first: (index << 32 | slot)
__global__ void __launch_bounds__(256) k_hull_arg(const double* __restrict__ bx, const double* __restrict__ by, const unsigned int* __restrict__ bidx,
                                                  const unsigned int* __restrict__ off, size_t ng, LinDirs D,
                                                  const unsigned long long* __restrict__ maxkey, unsigned long long* __restrict__ arg)
{
    const size_t s = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= off[ng] || bidx[s] == LIN_NONE) return;
    const double x = bx[s], y = by[s];
    for (int k = 0; k < LIN_NDIR; ++k)
        if (order_key(D.dx[k] * x + D.dy[k] * y) == maxkey[k]) atomicMin(&arg[k], ((unsigned long long)bidx[s] << 32) | (unsigned long long)s);
}
// pass 3, one thread: the convex polygon of the (at most 32) extreme points, counter-clockwise with strict turns, by the
// monotone chain.  poly: [0] the vertex count as a double (0 when fewer than 3 remain), then x[33], then y[33].
__global__ void k_hull_poly(const double* __restrict__ bx, const double* __restrict__ by, const unsigned long long* __restrict__ arg, double* __restrict__ poly)
{
    double px[LIN_NDIR], py[LIN_NDIR], hx[2 * LIN_NDIR], hy[2 * LIN_NDIR], S;
    int m = 0;
    for (int k = 0; k < LIN_NDIR; ++k) {
        if (arg[k] == ~0ull) continue;
        const unsigned int s = (unsigned int)arg[k];
        const double x = bx[s], y = by[s];
        int j = m;                                    // insertion in (x, y) order, equal points once
        bool seen = false;
        for (int t = 0; t < m; ++t) seen = seen || (px[t] == x && py[t] == y);
        if (seen) continue;
        while (j > 0 && (px[j - 1] > x || (px[j - 1] == x && py[j - 1] > y))) { px[j] = px[j - 1]; py[j] = py[j - 1]; --j; }
        px[j] = x; py[j] = y; ++m;
    }
    int h = 0;
    for (int t = 0; t < m; ++t) {                     // lower chain
        while (h >= 2 && lin_orient(hx[h - 2], hy[h - 2], hx[h - 1], hy[h - 1], px[t], py[t], S) <= 0.0) --h;
        hx[h] = px[t]; hy[h] = py[t]; ++h;
    }
    const int low = h + 1;
    for (int t = m - 2; t >= 0; --t) {                // upper chain
        while (h >= low && lin_orient(hx[h - 2], hy[h - 2], hx[h - 1], hy[h - 1], px[t], py[t], S) <= 0.0) --h;
        hx[h] = px[t]; hy[h] = py[t]; ++h;
    }
    --h;                                              // the first point came back as the last
    if (h < 3) h = 0;
    poly[0] = (double)h;
    for (int t = 0; t < h; ++t) { poly[1 + t] = hx[t]; poly[1 + 2 * LIN_NDIR + t] = hy[t]; }
}
// pass 4: a point certainly inside that polygon (left of every edge by more than the bound) is no hull vertex; the others go
// to the host, in the order the atomics hand out (the host sorts them)
__global__ void __launch_bounds__(256) k_hull_filter(const double* __restrict__ bx, const double* __restrict__ by, const unsigned int* __restrict__ bidx,
                                                     const unsigned int* __restrict__ off, size_t ng, const double* __restrict__ poly,
                                                     double* __restrict__ sx, double* __restrict__ sy, unsigned int* __restrict__ si,
                                                     unsigned int* __restrict__ counters)
{
    const size_t s = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= off[ng] || bidx[s] == LIN_NONE) return;
    const double x = bx[s], y = by[s];
    const int h = (int)poly[0];
    bool inside = h >= 3;
    for (int t = 0; t < h && inside; ++t) {
        const int u = t + 1 < h ? t + 1 : 0;
        double S;
        const double o = lin_orient(poly[1 + t], poly[1 + 2 * LIN_NDIR + t], poly[1 + u], poly[1 + 2 * LIN_NDIR + u], x, y, S);
        inside = o > LIN_EO * S;
    }
    if (inside) return;
    const unsigned int j = atomicAdd(&counters[5], 1u);
    sx[j] = x; sy[j] = y; si[j] = bidx[s];
}

// ---------------------------------------------------------------------------------------------------------------- walk
// Rings of cells around the cell of (cx, cy): after a step the square of cells within k of it has been looked at.  k grows by
// one up to 4 and by a quarter of itself from there (a search through an empty region would otherwise spend its time on the two
// side cells of every row of every ring), so a step takes the shell between two squares: whole runs of cells above and below,
// a run on either side in the rows between.  visit(y, xa, xb) sees the cells xa .. xb of row y; covered(x0, x1, y0, y1)
// says, after each step, whether the square looked at so far suffices.  The growth ends at the latest with the square that
// reaches the far side of the grid.
template <class Visit, class Covered>
__host__ __device__ __forceinline__ void lin_rings(const LinAccel& A, double cx, double cy, Visit visit, Covered covered)
{
    const int mx = A.cell_x(cx), my = A.cell_y(cy);
    const int kmax = max(max(mx, A.gw - 1 - mx), max(my, A.gh - 1 - my));
    for (int kp = -1, k = 0; kp < kmax; kp = k, k = min(k + 1 + k / 4, kmax)) {
        const int x0 = max(mx - k, 0), x1 = min(mx + k, A.gw - 1), y0 = max(my - k, 0), y1 = min(my + k, A.gh - 1);
        for (int y = y0; y <= y1; ++y) {
            if (y < my - kp || y > my + kp) { visit(y, x0, x1); continue; }
            if (mx - kp - 1 >= x0) visit(y, x0, mx - kp - 1);
            if (mx + kp + 1 <= x1) visit(y, mx + kp + 1, x1);
        }
        if (covered(mx - k, mx + k, my - k, my + k)) break;
    }
}

// A circle that bounds a search: centre and radius as computed, and whether they may be trusted (otherwise: the whole grid).
struct LinCirc { double x, y, r; bool bounded; };

// the radius widened by 2^-20 of itself and by the rounding of the sums it enters
__host__ __device__ __forceinline__ double lin_wide(const LinCirc& C) { return C.r + C.r * 0x1p-20 + (C.r + fabs(C.x) + fabs(C.y)) * 0x1p-40; }

// the cells under the box of the circle
__host__ __device__ __forceinline__ void lin_box(const LinAccel& A, const LinCirc& C, int& cx0, int& cx1, int& cy0, int& cy1)
{
    if (!C.bounded) { cx0 = 0; cx1 = A.gw - 1; cy0 = 0; cy1 = A.gh - 1; return; }
    const double R = lin_wide(C);
    cx0 = A.cell_x(C.x - R); cx1 = A.cell_x(C.x + R); cy0 = A.cell_y(C.y - R); cy1 = A.cell_y(C.y + R);
}

// The cells xa .. xb of row y cut down to those the circle reaches; false when none is left.  The points of row y have their y
// in [ymin + y hy, ymin + (y + 1) hy] up to the roundings of cell_y, which the slack (2^-20 of a row, 2^-40 of the coordinates)
// covers for any grid of at most 2048 rows; dy is the least distance of the centre from that band, and the chord at that distance
// is widened like the radius.  A box without corners: in a region of uneven density the corners hold most of a box's points.
__host__ __device__ __forceinline__ bool lin_row_clip(const LinAccel& A, const LinCirc& C, int y, int& xa, int& xb)
{
    if (!C.bounded || !(A.hy > 0.0)) return true;
    const double lo = A.ymin + (double)y * A.hy, hi = A.ymin + (double)(y + 1) * A.hy;
    const double slack = A.hy * 0x1p-20 + (fabs(lo) + fabs(hi)) * 0x1p-40;
    const double dy = fmax(fmax(lo - C.y, C.y - hi) - slack, 0.0), R = lin_wide(C);
    if (dy > R) return false;
    double half = sqrt(R * R - dy * dy);
    half = half + half * 0x1p-20 + (R + fabs(C.x)) * 0x1p-40;
    xa = max(xa, A.cell_x(C.x - half)); xb = min(xb, A.cell_x(C.x + half));
    return xa <= xb;
}

// The circle through a, b, c.  Centre and radius are computed relative to a; they are trusted (to 2^-23 of the radius)
// only when the cross product is far above its own rounding bound and the triangle's shortest side is not vanishingly short.
__host__ __device__ __forceinline__ LinCirc lin_circle(const LinPt& a, const LinPt& b, const LinPt& c)
{
    const double bx = b.x - a.x, by = b.y - a.y, cx = c.x - a.x, cy = c.y - a.y, ex = c.x - b.x, ey = c.y - b.y;
    const double t1 = bx * cy, t2 = by * cx, cross = t1 - t2, S = fabs(t1) + fabs(t2);
    const double lb = bx * bx + by * by, lc = cx * cx + cy * cy, le = ex * ex + ey * ey;
    const double shortest = fmin(le, fmin(lb, lc)), longest = fmax(le, fmax(lb, lc));
    LinCirc C = { 0.0, 0.0, 0.0, false };
    if (!(fabs(cross) >= S * 0x1p-26) || !(shortest * 0x1p40 >= longest) || !(S > 0.0)) return C;
    const double d = 2.0 * cross, ux = (cy * lb - by * lc) / d, uy = (bx * lc - cx * lb) / d;
    C.r = sqrt(ux * ux + uy * uy);
    C.x = a.x + ux; C.y = a.y + uy;
    C.bounded = C.r < 1.0e300;
    return C;
}

// the point nearest to (px, py), not counting index `skip`; ties to the lower index
__host__ __device__ __forceinline__ LinPt lin_nearest(const LinAccel& A, double px, double py, unsigned int skip)
{
    LinPt best = { 0.0, 0.0, LIN_NONE, 0u };
    double bd = 0.0;
    LinCirc C = { px, py, 0.0, false };               // the circle about (px, py) through the best so far
    lin_rings(A, px, py,
        [&](int row, int xa, int xb) {
            if (!lin_row_clip(A, C, row, xa, xb)) return;
            const unsigned int s1 = A.off[(size_t)row * A.gw + xb + 1];
            for (unsigned int s = A.off[(size_t)row * A.gw + xa]; s < s1; ++s) {
                const unsigned int i = A.bidx[s];
                if (i == LIN_NONE || i == skip) continue;
                const double x = A.bx[s], y = A.by[s], dx = x - px, dy = y - py, d = dx * dx + dy * dy;
                if (best.i == LIN_NONE || d < bd || (d == bd && i < best.i)) {
                    best.x = x; best.y = y; best.i = i; best.s = s; bd = d;
                    C.r = sqrt(d); C.bounded = true;
                }
            }
        },
        [&](int x0, int x1, int y0, int y1) {
            if (best.i == LIN_NONE) return false;
            int cx0, cx1, cy0, cy1;
            lin_box(A, C, cx0, cx1, cy0, cy1);
            return cx0 >= x0 && cx1 <= x1 && cy0 >= y0 && cy1 <= y1;
        });
    return best;
}

// The apex of the edge a -> b: among the points strictly left of it the one whose circle through a and b holds no other of
// them.  The running best is replaced on incircle > 0, or == 0 with a lower index.
__host__ __device__ __forceinline__ LinPt lin_apex(const LinAccel& A, const LinPt& a, const LinPt& b)
{
    LinPt best = { 0.0, 0.0, LIN_NONE, 0u };
    LinCirc C = { 0.0, 0.0, 0.0, false };             // the circle through a, b and the best so far: nothing outside it can replace the best
    lin_rings(A, 0.5 * (a.x + b.x), 0.5 * (a.y + b.y),
        [&](int row, int xa, int xb) {
            if (!lin_row_clip(A, C, row, xa, xb)) return;
            const unsigned int s1 = A.off[(size_t)row * A.gw + xb + 1];
            for (unsigned int s = A.off[(size_t)row * A.gw + xa]; s < s1; ++s) {
                const unsigned int i = A.bidx[s];
                if (i == LIN_NONE || i == a.i || i == b.i) continue;
                const double x = A.bx[s], y = A.by[s];
                double S;
                if (!(lin_orient(a.x, a.y, b.x, b.y, x, y, S) > 0.0)) continue;
                bool take = best.i == LIN_NONE;
                if (!take) {
                    const double ic = lin_incircle(a.x, a.y, b.x, b.y, best.x, best.y, x, y, S);
                    take = ic > 0.0 || (ic == 0.0 && i < best.i);
                }
                if (take) { best.x = x; best.y = y; best.i = i; best.s = s; C = lin_circle(a, b, best); }
            }
        },
        [&](int x0, int x1, int y0, int y1) {
            if (best.i == LIN_NONE) return false;
            int cx0, cx1, cy0, cy1;
            lin_box(A, C, cx0, cx1, cy0, cy1);
            return cx0 >= x0 && cx1 <= x1 && cy0 >= y0 && cy1 <= y1;
        });
    return best;
}

__host__ __device__ __forceinline__ void lin_swap(LinPt& a, LinPt& b) { const LinPt t = a; a = b; b = t; }

// The certificate and the value of the triangle (a, b, c) for the node q, in the canonical form: vertices by index i < j < k,
// sign of the triangle from orient(Pi, Pj, Pk), containment from the three orient(.., q), every other point of the cells under
// the circle strictly outside by more than the bound.  Returns flag 0 or 2.
__host__ __device__ __forceinline__ int lin_certify(const LinAccel& A, LinPt a, LinPt b, LinPt c, double qx, double qy, double& val)
{
    if (a.i > b.i) lin_swap(a, b);
    if (b.i > c.i) lin_swap(b, c);
    if (a.i > b.i) lin_swap(a, b);
    double S, Si, Sj, Sk;
    const double o3 = lin_orient(a.x, a.y, b.x, b.y, c.x, c.y, S);
    bool ok = fabs(o3) > LIN_EO * S;
    const double sg = o3 > 0.0 ? 1.0 : -1.0;
    const double oi = lin_orient(b.x, b.y, c.x, c.y, qx, qy, Si), oj = lin_orient(c.x, c.y, a.x, a.y, qx, qy, Sj),
                 ok3 = lin_orient(a.x, a.y, b.x, b.y, qx, qy, Sk);
    ok = ok && sg * oi >= LIN_EO * Si && sg * oj >= LIN_EO * Sj && sg * ok3 >= LIN_EO * Sk;
    val = ((oi * A.bz[a.s] + oj * A.bz[b.s]) + ok3 * A.bz[c.s]) / ((oi + oj) + ok3);
    if (!isfinite(val)) { val = __builtin_nan(""); ok = false; }
    if (!ok) return 2;
    int cx0, cx1, cy0, cy1;
    const LinCirc C = lin_circle(a, b, c);
    lin_box(A, C, cx0, cx1, cy0, cy1);
    for (int y = cy0; y <= cy1 && ok; ++y) {
        int xa = cx0, xb = cx1;
        if (!lin_row_clip(A, C, y, xa, xb)) continue;
        const unsigned int s1 = A.off[(size_t)y * A.gw + xb + 1];
        for (unsigned int s = A.off[(size_t)y * A.gw + xa]; s < s1; ++s) {
            const unsigned int i = A.bidx[s];
            if (i == LIN_NONE || i == a.i || i == b.i || i == c.i) continue;
            double P;
            const double ic = lin_incircle(a.x, a.y, b.x, b.y, c.x, c.y, A.bx[s], A.by[s], P);
            if (!(sg * ic < -(LIN_EI * P))) { ok = false; break; }
        }
    }
    return ok ? 0 : 2;
}

__host__ __device__ __forceinline__ int lin_node(const LinWalkArgs& P, double qx, double qy, double& val)
{
    val = __builtin_nan("");
    double S;
    // 1. certainly beyond a hull edge
    for (int e = 0; e < P.nh; ++e) {
        const int f = e + 1 < P.nh ? e + 1 : 0;
        const double o = lin_orient(P.hx[e], P.hy[e], P.hx[f], P.hy[f], qx, qy, S);
        if (o < -(LIN_EO * S)) return 1;
    }
    // 2. a Delaunay edge next to the node, the node on its left
    LinPt a = lin_nearest(P.A, qx, qy, LIN_NONE);
    if (a.i == LIN_NONE) return 2;
    LinPt b = lin_nearest(P.A, a.x, a.y, a.i);
    if (b.i == LIN_NONE) return 2;
    double o = lin_orient(a.x, a.y, b.x, b.y, qx, qy, S);
    if (o < 0.0) lin_swap(a, b);
    // 3, 4. apex, and across the edge that separates the node from the triangle
    for (int step = 0; step < P.max_steps; ++step) {
        const LinPt c = lin_apex(P.A, a, b);
        if (c.i == LIN_NONE) {
            if (step == 0 && o == 0.0) { lin_swap(a, b); o = 1.0; continue; }   // the node is on the line of the first edge: the other side
            return 2;                                 // inside the hull as far as step 1 can tell, and nothing left of the edge: a rounding case
        }
        const double obc = lin_orient(b.x, b.y, c.x, c.y, qx, qy, S), oca = lin_orient(c.x, c.y, a.x, a.y, qx, qy, S);
        if (obc >= 0.0 && oca >= 0.0) return lin_certify(P.A, a, b, c, qx, qy, val);   // 5.
        if (obc < 0.0) a = c;                         // the node is left of c -> b
        else b = c;                                   // ... of a -> c
        o = 1.0;
    }
    return 3;
}

// One lane per node.  A wave takes an 8 x 8 patch of the lattice (not 64 nodes of a row): neighbouring nodes walk through the same
// cells, so the lanes of a wave share cache lines and their trip counts stay close.
__global__ void __launch_bounds__(256) k_lin_walk(LinWalkArgs P)
{
    const int lane = threadIdx.x & 63, patch = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int nx = (patch % P.npx) * 8 + (lane & 7), ny = (patch / P.npx) * 8 + (lane >> 3);
    int flag = 255;
    if (nx < P.W && ny < P.H) {
        const double qx = (nx == P.W - 1 && P.W > 1) ? P.xmax : (double)nx * P.stepx + P.xmin;
        const double qy = (ny == P.H - 1 && P.H > 1) ? P.ymax : (double)ny * P.stepy + P.ymin;
        double val;
        flag = lin_node(P, qx, qy, val);
        if (flag == 3) val = __builtin_nan("");
        P.out[(size_t)ny * P.W + nx] = val;
        P.flags[(size_t)ny * P.W + nx] = (uint8_t)flag;
    }
    for (int f = 0; f < 4; ++f) {
        const unsigned long long m = __ballot(flag == f);
        if (lane == 0 && m) atomicAdd(&P.counts[f], (unsigned int)__popcll(m));
    }
}

__global__ void __launch_bounds__(256) k_lin_nothing(double* __restrict__ out, uint8_t* __restrict__ flags, size_t nn)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nn) return;
    out[i] = __builtin_nan("");
    flags[i] = 1;
}

// ---------------------------------------------------------------------------------------------------------------- host
struct LinLayout {
    unsigned int *cnt, *off, *fill, *pcell, *braw, *bidx, *si, *counters;
    double *bx, *by, *bz, *sx, *sy, *hx, *hy, *poly, *in_x, *in_y, *in_z, *st_out;
    unsigned long long *maxkey, *arg;
    uint8_t* st_flags;
};

// the acceleration grid of n points: a square of cells, about two points per cell, at most 2048 a side
static int lin_accel_side(size_t n)
{
    const double s = ceil(sqrt((double)n / 2.0));
    return (int)std::min(2048.0, std::max(1.0, s));
}

// ONE layout for the three entries: the bucketed cloud, the hull's survivors and vertices, the aligned or staged input cloud
// (mesh and host entries) and the staged result (host entry).
static void lin_lay(Carve& a, LinLayout& L, size_t n, size_t nn, size_t ng)
{
    L.counters = a.take<unsigned int>(8 * 4);         // [0..3] nodes per flag, [4] points taken, [5] hull survivors
    L.maxkey = a.take<unsigned long long>(LIN_NDIR * 8); L.arg = a.take<unsigned long long>(LIN_NDIR * 8);
    L.poly = a.take<double>((1 + 4 * LIN_NDIR) * 8);
    L.cnt = a.take<unsigned int>((ng + 1) * 4); L.off = a.take<unsigned int>((ng + 1) * 4); L.fill = a.take<unsigned int>(ng * 4);
    L.pcell = a.take<unsigned int>(n * 4); L.braw = a.take<unsigned int>(n * 4); L.bidx = a.take<unsigned int>(n * 4);
    L.bx = a.take<double>(n * 8); L.by = a.take<double>(n * 8); L.bz = a.take<double>(n * 8);
    L.sx = a.take<double>(n * 8); L.sy = a.take<double>(n * 8); L.si = a.take<unsigned int>(n * 4);
    L.hx = a.take<double>(n * 8); L.hy = a.take<double>(n * 8);
    L.in_x = a.take<double>(n * 8); L.in_y = a.take<double>(n * 8); L.in_z = a.take<double>(n * 8);
    L.st_out = a.take<double>(nn * 8); L.st_flags = a.take<uint8_t>(nn);
}

static int lin_check(wass_ctx* c, size_t n, const wass_grid_setup* gs, const wass_linear_opts* o)
{
    if (!c || !gs) return set_err(c, WASS_ERR_INVALID_ARG, "null argument");
    if (gs->width < 1 || gs->height < 1) return set_err(c, WASS_ERR_INVALID_ARG, "bad grid: width and height must be at least 1");
    if ((gs->width > 1 && !(gs->xmax > gs->xmin)) || (gs->height > 1 && !(gs->ymax > gs->ymin)))
        return set_err(c, WASS_ERR_INVALID_ARG, "bad grid: xmax <= xmin or ymax <= ymin");
    if (!(gs->xmax >= gs->xmin) || !(gs->ymax >= gs->ymin) || !isfinite(gs->xmin) || !isfinite(gs->xmax) || !isfinite(gs->ymin) || !isfinite(gs->ymax))
        return set_err(c, WASS_ERR_INVALID_ARG, "bad grid extent");
    if (n > 0x7FFFFFF0ull || (size_t)gs->width * gs->height > 0x7FFFFFF0ull) return set_err(c, WASS_ERR_UNSUPPORTED, "cloud or grid too large");
    if (o && (o->max_walk_steps < 0 || o->accel_w < 0 || o->accel_h < 0 || o->accel_w > 2048 || o->accel_h > 2048))
        return set_err(c, WASS_ERR_INVALID_ARG, "bad linear options");
    return WASS_OK;
}

static void lin_dims(size_t n, const wass_linear_opts* o, int& gw, int& gh)
{
    gw = o && o->accel_w ? o->accel_w : lin_accel_side(n);
    gh = o && o->accel_h ? o->accel_h : lin_accel_side(n);
}

// the hull of the survivors: sorted by (x, y, index), monotone chain with the sign of lin_orient, strict turns only
static void lin_hull_host(std::vector<double>& sx, std::vector<double>& sy, std::vector<unsigned int>& si, std::vector<double>& hx,
                          std::vector<double>& hy)
{
    const size_t m = sx.size();
    std::vector<unsigned int> ord(m);
    for (size_t t = 0; t < m; ++t) ord[t] = (unsigned int)t;
    std::sort(ord.begin(), ord.end(), [&](unsigned int p, unsigned int q) {
        if (sx[p] != sx[q]) return sx[p] < sx[q];
        if (sy[p] != sy[q]) return sy[p] < sy[q];
        return si[p] < si[q];
    });
    hx.clear(); hy.clear();
    double S;
    auto push = [&](unsigned int t, size_t low) {
        while (hx.size() >= low && lin_orient(hx[hx.size() - 2], hy[hx.size() - 2], hx.back(), hy.back(), sx[t], sy[t], S) <= 0.0) {
            hx.pop_back(); hy.pop_back();
        }
        hx.push_back(sx[t]); hy.push_back(sy[t]);
    };
    for (size_t t = 0; t < m; ++t) push(ord[t], 2);
    const size_t low = hx.size() + 1;
    for (size_t t = m - 1; t-- > 0;) push(ord[t], low);
    if (!hx.empty()) { hx.pop_back(); hy.pop_back(); }
    if (hx.size() < 3) { hx.clear(); hy.clear(); }
}

// Everything after the layout is carved: d_x, d_y, d_z are device memory (the caller's or L.in_*).  Returns after the stream has
// run (the counts come back with the call); WASS_ERR_TOO_FEW_POINTS with an all-NaN surface, every flag 1.
static int lin_core(wass_ctx* c, const LinLayout& L, const double* d_x, const double* d_y, const double* d_z, size_t n,
                    const wass_grid_setup* gs, const wass_linear_opts* o, int gw, int gh, double* d_out, uint8_t* d_flags, wass_linear_info* info)
{
    hipStream_t s = c->ts();
    const size_t nn = (size_t)gs->width * gs->height, ng = (size_t)gw * gh;
    const dim3 blk(256), gp((unsigned)((n + 255) / 256)), gn((unsigned)((nn + 255) / 256));
    const bool timing = o && o->timing;
    struct Events {                                   // released on every way out
        hipEvent_t e[4] = {};
        ~Events() { for (auto& v : e) if (v) (void)hipEventDestroy(v); }
    } evs;
    hipEvent_t* ev = evs.e;
    if (timing)
        for (int k = 0; k < 4; ++k) WASS_HIP(c, hipEventCreate(&ev[k]));
    auto stamp = [&](int k) { if (timing) (void)hipEventRecord(ev[k], s); };
    if (info) memset(info, 0, sizeof *info);
    unsigned int h_counters[8] = {};
    std::vector<double> sx, sy, hx, hy;
    std::vector<unsigned int> si;
    size_t nh = 0;
    WASS_HIP(c, hipMemsetAsync(L.counters, 0, 8 * 4, s));
    stamp(0);
    if (n > 0) {
        LinAccel A;
        A.xmin = gs->xmin; A.ymin = gs->ymin; A.xmax = gs->xmax; A.ymax = gs->ymax;
        A.ipx = gs->xmax > gs->xmin ? (double)gw / (gs->xmax - gs->xmin) : 0.0;
        A.ipy = gs->ymax > gs->ymin ? (double)gh / (gs->ymax - gs->ymin) : 0.0;
        A.hy = A.ipy > 0.0 ? 1.0 / A.ipy : 0.0;
        A.gw = gw; A.gh = gh; A.off = L.off; A.bx = L.bx; A.by = L.by; A.bz = L.bz; A.bidx = L.bidx;
        WASS_HIP(c, hipMemsetAsync(L.cnt, 0, (ng + 1) * 4, s));
        WASS_HIP(c, hipMemsetAsync(L.fill, 0, ng * 4, s));
        hipLaunchKernelGGL(k_lin_count, gp, blk, 0, s, d_x, d_y, n, A, L.pcell, L.cnt);
        grid_scan_enqueue(L.cnt, ng + 1, L.off, s);   // one entry more: off[ng] is the number of points in the area
        hipLaunchKernelGGL(k_lin_fill, gp, blk, 0, s, d_x, d_y, d_z, (const unsigned int*)L.pcell, n, (const unsigned int*)L.off, L.fill, L.bx,
                           L.by, L.bz, L.braw);
        hipLaunchKernelGGL(k_lin_dedupe, gp, blk, 0, s, d_x, d_y, (const unsigned int*)L.pcell, n, (const unsigned int*)L.off, (const double*)L.bx,
                           (const double*)L.by, (const unsigned int*)L.braw, L.bidx, L.counters);
        stamp(1);
        LinDirs D;
        for (int k = 0; k < LIN_NDIR; ++k) { D.dx[k] = cos(2.0 * M_PI * k / LIN_NDIR); D.dy[k] = sin(2.0 * M_PI * k / LIN_NDIR); }
        WASS_HIP(c, hipMemsetAsync(L.maxkey, 0, LIN_NDIR * 8, s));
        WASS_HIP(c, hipMemsetAsync(L.arg, 0xFF, LIN_NDIR * 8, s));
        hipLaunchKernelGGL(k_hull_max, gp, blk, 0, s, (const double*)L.bx, (const double*)L.by, (const unsigned int*)L.bidx,
                           (const unsigned int*)L.off, ng, D, L.maxkey);
        hipLaunchKernelGGL(k_hull_arg, gp, blk, 0, s, (const double*)L.bx, (const double*)L.by, (const unsigned int*)L.bidx,
                           (const unsigned int*)L.off, ng, D, (const unsigned long long*)L.maxkey, L.arg);
        hipLaunchKernelGGL(k_hull_poly, dim3(1), dim3(1), 0, s, (const double*)L.bx, (const double*)L.by, (const unsigned long long*)L.arg, L.poly);
        hipLaunchKernelGGL(k_hull_filter, gp, blk, 0, s, (const double*)L.bx, (const double*)L.by, (const unsigned int*)L.bidx,
                           (const unsigned int*)L.off, ng, (const double*)L.poly, L.sx, L.sy, L.si, L.counters);
        WASS_HIP(c, hipGetLastError());
        // The hull hand-over, one synchronisation: the count and the first LIN_HANDOVER survivors together (1120 survived of the
        // 4 M points of DESIGN.md's measurement); only a cloud that leaves more, one on a circle say, comes back for the rest.
        const size_t first = std::min(n, LIN_HANDOVER);
        sx.resize(first); sy.resize(first); si.resize(first);
        WASS_HIP(c, hipMemcpyAsync(h_counters, L.counters, sizeof h_counters, hipMemcpyDeviceToHost, s));
        WASS_HIP(c, hipMemcpyAsync(sx.data(), L.sx, first * 8, hipMemcpyDeviceToHost, s));
        WASS_HIP(c, hipMemcpyAsync(sy.data(), L.sy, first * 8, hipMemcpyDeviceToHost, s));
        WASS_HIP(c, hipMemcpyAsync(si.data(), L.si, first * 4, hipMemcpyDeviceToHost, s));
        WASS_HIP(c, hipStreamSynchronize(s));
        const size_t m = h_counters[5];
        if (m > n) return set_err(c, WASS_ERR_DEVICE, "hull survivors out of range");
        sx.resize(m); sy.resize(m); si.resize(m);
        if (m > first) {
            WASS_HIP(c, hipMemcpyAsync(sx.data() + first, L.sx + first, (m - first) * 8, hipMemcpyDeviceToHost, s));
            WASS_HIP(c, hipMemcpyAsync(sy.data() + first, L.sy + first, (m - first) * 8, hipMemcpyDeviceToHost, s));
            WASS_HIP(c, hipMemcpyAsync(si.data() + first, L.si + first, (m - first) * 4, hipMemcpyDeviceToHost, s));
            WASS_HIP(c, hipStreamSynchronize(s));
        }
        if (m >= 3) {
            lin_hull_host(sx, sy, si, hx, hy);
            nh = hx.size();
        }
        if (nh >= 3) {
            WASS_HIP(c, hipMemcpyAsync(L.hx, hx.data(), nh * 8, hipMemcpyHostToDevice, s));
            WASS_HIP(c, hipMemcpyAsync(L.hy, hy.data(), nh * 8, hipMemcpyHostToDevice, s));
            stamp(2);
            LinWalkArgs P;
            P.A = A; P.hx = L.hx; P.hy = L.hy; P.nh = (int)nh;
            P.W = gs->width; P.H = gs->height; P.npx = (gs->width + 7) / 8;
            P.xmin = gs->xmin; P.xmax = gs->xmax; P.ymin = gs->ymin; P.ymax = gs->ymax;
            P.stepx = gs->width > 1 ? (gs->xmax - gs->xmin) / (double)(gs->width - 1) : 0.0;
            P.stepy = gs->height > 1 ? (gs->ymax - gs->ymin) / (double)(gs->height - 1) : 0.0;
            P.max_steps = o && o->max_walk_steps ? o->max_walk_steps : LIN_DEFAULT_STEPS;
            P.out = d_out; P.flags = d_flags; P.counts = L.counters;
            const size_t patches = (size_t)P.npx * ((gs->height + 7) / 8);
            hipLaunchKernelGGL(k_lin_walk, dim3((unsigned)((patches + 3) / 4)), blk, 0, s, P);
            stamp(3);
        }
    }
    if (nh < 3) {
        hipLaunchKernelGGL(k_lin_nothing, gn, blk, 0, s, d_out, d_flags, nn);
        h_counters[1] = (unsigned int)nn;
    }
    WASS_HIP(c, hipGetLastError());
    if (nh >= 3) WASS_HIP(c, hipMemcpyAsync(h_counters, L.counters, sizeof h_counters, hipMemcpyDeviceToHost, s));
    WASS_HIP(c, hipStreamSynchronize(s));
    if (info) {
        for (int f = 0; f < 4; ++f) info->counts[f] = h_counters[f];
        info->n_taken = h_counters[4];
        info->hull_vertices = (int)nh; info->hull_candidates = (int)h_counters[5];
        info->accel_w = gw; info->accel_h = gh;
        if (timing && nh >= 3) {
            (void)hipEventElapsedTime(&info->ms_bucket, ev[0], ev[1]);
            (void)hipEventElapsedTime(&info->ms_hull, ev[1], ev[2]);
            (void)hipEventElapsedTime(&info->ms_walk, ev[2], ev[3]);
        }
    }
    if (nh < 3) return set_err(c, WASS_ERR_TOO_FEW_POINTS, "fewer than three points in the area, or all of them collinear");
    return WASS_OK;
}

static void lin_counts_out(const wass_linear_info& info, uint64_t* counts)
{
    if (counts)
        for (int f = 0; f < 4; ++f) counts[f] = info.counts[f];
}

}  // namespace wass

using namespace wass;

extern "C" int wass_grid_linear_scratch_bytes(size_t n, int width, int height, size_t* bytes)
{
    if (!bytes || width < 1 || height < 1 || n > 0x7FFFFFF0ull) return WASS_ERR_INVALID_ARG;
    const size_t side = (size_t)lin_accel_side(n);
    *bytes = measure([&](Carve& a) { LinLayout L; lin_lay(a, L, n, (size_t)width * height, side * side); });
    return WASS_OK;
}

extern "C" int wass_grid_linear_dev_ex(wass_ctx* c, const double* d_x, const double* d_y, const double* d_z, size_t n, const wass_grid_setup* gs,
                                       const wass_linear_opts* opts, double* d_out, uint8_t* d_flags, wass_linear_info* info)
{
    int rc, gw, gh;
    if ((rc = lin_check(c, n, gs, opts))) return rc;
    if (!d_out || !d_flags || (n && (!d_x || !d_y || !d_z))) return set_err(c, WASS_ERR_INVALID_ARG, "null argument");
    WASS_HIP(c, hipSetDevice(c->device));
    lin_dims(n, opts, gw, gh);
    LinLayout L;
    if ((rc = carve_buf(c, c->linear, [&](Carve& a) { lin_lay(a, L, n, (size_t)gs->width * gs->height, (size_t)gw * gh); }))) return rc;
    return lin_core(c, L, d_x, d_y, d_z, n, gs, opts, gw, gh, d_out, d_flags, info);
}

extern "C" int wass_grid_linear_dev(wass_ctx* c, const double* d_x, const double* d_y, const double* d_z, size_t n, const wass_grid_setup* gs,
                                    double* d_out, uint8_t* d_flags, uint64_t* counts)
{
    wass_linear_info info;
    memset(&info, 0, sizeof info);
    const int rc = wass_grid_linear_dev_ex(c, d_x, d_y, d_z, n, gs, nullptr, d_out, d_flags, &info);
    lin_counts_out(info, counts);
    return rc;
}

extern "C" int wass_grid_linear(wass_ctx* c, const double* x, const double* y, const double* z, size_t n, const wass_grid_setup* gs, double* out,
                                uint8_t* flags, uint64_t* counts)
{
    int rc, gw, gh;
    if ((rc = lin_check(c, n, gs, nullptr))) return rc;
    if (!out || !flags || (n && (!x || !y || !z))) return set_err(c, WASS_ERR_INVALID_ARG, "null argument");
    WASS_HIP(c, hipSetDevice(c->device));
    lin_dims(n, nullptr, gw, gh);
    const size_t nn = (size_t)gs->width * gs->height;
    LinLayout L;
    if ((rc = carve_buf(c, c->linear, [&](Carve& a) { lin_lay(a, L, n, nn, (size_t)gw * gh); }))) return rc;
    hipStream_t s = c->ts();
    if (n) {
        WASS_HIP(c, hipMemcpyAsync(L.in_x, x, n * 8, hipMemcpyHostToDevice, s));
        WASS_HIP(c, hipMemcpyAsync(L.in_y, y, n * 8, hipMemcpyHostToDevice, s));
        WASS_HIP(c, hipMemcpyAsync(L.in_z, z, n * 8, hipMemcpyHostToDevice, s));
    }
    wass_linear_info info;
    memset(&info, 0, sizeof info);
    rc = lin_core(c, L, L.in_x, L.in_y, L.in_z, n, gs, nullptr, gw, gh, L.st_out, L.st_flags, &info);
    lin_counts_out(info, counts);
    if (rc != WASS_OK && rc != WASS_ERR_TOO_FEW_POINTS) return rc;
    WASS_HIP(c, hipMemcpyAsync(out, L.st_out, nn * 8, hipMemcpyDeviceToHost, s));
    WASS_HIP(c, hipMemcpyAsync(flags, L.st_flags, nn, hipMemcpyDeviceToHost, s));
    WASS_HIP(c, hipStreamSynchronize(s));
    return rc;
}

extern "C" int wass_mesh_grid_linear_ex(wass_ctx* c, const wass_mesh* m, const wass_grid_setup* gs, const wass_linear_opts* opts, double* d_out,
                                        uint8_t* d_flags, wass_linear_info* info)
{
    if (!m) return set_err(c, WASS_ERR_INVALID_ARG, "null argument");
    const size_t n = m->n();
    int rc, gw, gh;
    if ((rc = lin_check(c, n, gs, opts))) return rc;
    if (!d_out || !d_flags) return set_err(c, WASS_ERR_INVALID_ARG, "null argument");
    WASS_HIP(c, hipSetDevice(c->device));
    lin_dims(n, opts, gw, gh);
    LinLayout L;
    if ((rc = carve_buf(c, c->linear, [&](Carve& a) { lin_lay(a, L, n, (size_t)gs->width * gs->height, (size_t)gw * gh); }))) return rc;
    if (n) {
        GridDev g;
        memset(&g, 0, sizeof g);
        memcpy(g.R, gs->R, sizeof g.R); memcpy(g.T, gs->T, sizeof g.T);
        g.baseline = gs->baseline;
        hipLaunchKernelGGL(k_lin_align, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->ts(), (const uint8_t*)m->valid, (const double*)m->x,
                           (const double*)m->y, (const double*)m->z, n, g, L.in_x, L.in_y, L.in_z);
    }
    return lin_core(c, L, L.in_x, L.in_y, L.in_z, n, gs, opts, gw, gh, d_out, d_flags, info);
}

extern "C" int wass_mesh_grid_linear(wass_ctx* c, const wass_mesh* m, const wass_grid_setup* gs, double* d_out, uint8_t* d_flags, uint64_t* counts)
{
    wass_linear_info info;
    memset(&info, 0, sizeof info);
    const int rc = wass_mesh_grid_linear_ex(c, m, gs, nullptr, d_out, d_flags, &info);
    lin_counts_out(info, counts);
    return rc;
}
