// linearnd_host.hip -- the walk of wass_amd/csrc/grid_linear.hip on the CPU: the same source (its helpers are __host__ __device__),
// a plain counting sort in place of the bucket kernels, filled in REVERSE index order so that no result can lean on the order
// inside a bucket, and the monotone chain over every existing point in place of the device's pre-filter.
//   linearnd_host IN OUT    IN: int64 n, W, H, accel_w, accel_h, max_steps; double xmin, xmax, ymin, ymax; x[n], y[n], z[n]
//                           OUT: double out[H][W]; uint8 flags[H][W]; stderr: "taken T hull V"
#include "../../wass_amd/csrc/grid_linear.hip"
#include <cstdio>
#include <cstdlib>

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    long long hd[6];
    double ext[4];
    if (fread(hd, 8, 6, f) != 6 || fread(ext, 8, 4, f) != 4) return 2;
    const size_t n = (size_t)hd[0];
    const int W = (int)hd[1], H = (int)hd[2], gw = (int)hd[3], gh = (int)hd[4], steps = (int)hd[5];
    std::vector<double> x(n), y(n), z(n);
    if (fread(x.data(), 8, n, f) != n || fread(y.data(), 8, n, f) != n || fread(z.data(), 8, n, f) != n) return 2;
    fclose(f);
    LinAccel A;
    A.xmin = ext[0]; A.xmax = ext[1]; A.ymin = ext[2]; A.ymax = ext[3];
    A.ipx = ext[1] > ext[0] ? (double)gw / (ext[1] - ext[0]) : 0.0;
    A.ipy = ext[3] > ext[2] ? (double)gh / (ext[3] - ext[2]) : 0.0;
    A.hy = A.ipy > 0.0 ? 1.0 / A.ipy : 0.0;
    A.gw = gw; A.gh = gh;
    const size_t ng = (size_t)gw * gh;
    std::vector<unsigned int> off(ng + 2, 0), pcell(n), braw(n), fill(ng, 0);
    std::vector<double> bx(n), by(n), bz(n);
    for (size_t i = 0; i < n; ++i) {
        unsigned int c = LIN_NONE;
        if (x[i] >= A.xmin && x[i] <= A.xmax && y[i] >= A.ymin && y[i] <= A.ymax) {
            c = (unsigned int)A.cell_y(y[i]) * gw + A.cell_x(x[i]);
            off[c + 1]++;
        }
        pcell[i] = c;
    }
    for (size_t c = 0; c < ng; ++c) off[c + 1] += off[c];
    for (size_t i = n; i-- > 0;) {
        const unsigned int c = pcell[i];
        if (c == LIN_NONE) continue;
        const unsigned int s = off[c] + fill[c]++;
        bx[s] = x[i]; by[s] = y[i]; bz[s] = z[i]; braw[s] = (unsigned int)i;
    }
    std::vector<unsigned int> bidx(braw);
    for (size_t c = 0; c < ng; ++c)
        for (unsigned int s = off[c]; s < off[c + 1]; ++s)
            for (unsigned int t = off[c]; t < off[c + 1]; ++t)
                if (braw[t] < braw[s] && bx[t] == bx[s] && by[t] == by[s]) bidx[s] = LIN_NONE;
    A.off = off.data(); A.bx = bx.data(); A.by = by.data(); A.bz = bz.data(); A.bidx = bidx.data();
    std::vector<double> sx, sy, hx, hy;
    std::vector<unsigned int> si;
    for (unsigned int s = 0; s < off[ng]; ++s)
        if (bidx[s] != LIN_NONE) { sx.push_back(bx[s]); sy.push_back(by[s]); si.push_back(bidx[s]); }
    if (sx.size() >= 3) lin_hull_host(sx, sy, si, hx, hy);
    fprintf(stderr, "taken %zu hull %zu\n", sx.size(), hx.size());
    LinWalkArgs P;
    P.A = A; P.hx = hx.data(); P.hy = hy.data(); P.nh = (int)hx.size(); P.W = W; P.H = H; P.max_steps = steps;
    P.xmin = ext[0]; P.xmax = ext[1]; P.ymin = ext[2]; P.ymax = ext[3];
    P.stepx = W > 1 ? (ext[1] - ext[0]) / (double)(W - 1) : 0.0;
    P.stepy = H > 1 ? (ext[3] - ext[2]) / (double)(H - 1) : 0.0;
    std::vector<double> out((size_t)W * H);
    std::vector<unsigned char> fl((size_t)W * H);
    for (int ny = 0; ny < H; ++ny)
        for (int nx = 0; nx < W; ++nx) {
            const double qx = (nx == W - 1 && W > 1) ? P.xmax : (double)nx * P.stepx + P.xmin;
            const double qy = (ny == H - 1 && H > 1) ? P.ymax : (double)ny * P.stepy + P.ymin;
            double v = __builtin_nan("");
            int g = 1;
            if (P.nh >= 3) {
                g = lin_node(P, qx, qy, v);
                if (g == 3) v = __builtin_nan("");
            }
            out[(size_t)ny * W + nx] = v; fl[(size_t)ny * W + nx] = (unsigned char)g;
        }
    f = fopen(argv[2], "wb");
    if (!f) return 2;
    fwrite(out.data(), 8, out.size(), f); fwrite(fl.data(), 1, fl.size(), f);
    fclose(f);
    return 0;
}
