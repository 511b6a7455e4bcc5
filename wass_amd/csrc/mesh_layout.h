// mesh_layout.h -- the plain records of the mesh stages (mesh.hip) and every layout of the frame tail's memory, each stated ONCE
// as a function that takes its pieces from a Carve (scratch.h).  No HIP header: tests/native/mesh_layout_check.cpp compiles this
// with the host compiler and checks alignment, bounds and overlap of every layout.
#pragma once
#include <stdint.h>
#include "scratch.h"

namespace wass {

// Counters are striped over NSLOT addresses (summed on the host): tens of thousands of waves hitting one
// address serialise at ~12 ns per atomic, which would dominate these otherwise trivial kernels.
constexpr int NSLOT = 64;
// z-gap percentile: GAP_HIST_COPIES copies of the global histogram (same-address atomics serialise), which k_radix_pick adds up.
constexpr int GAP_HIST_COPIES = 4;
// 5 x 11 + 9 bits = 64.  (13-bit digits, five passes: measured SLOWER -- 42 + 23 us per pass against 26 + 11: the 32 KB
// histogram per workgroup costs occupancy and the pick kernel scans four times the bins.)
constexpr int GAP_BITS = 11, GAP_BINS = 1 << GAP_BITS, GAP_PASSES = 6;
constexpr int REFINE_BLOCKS = 1024;                           // per-block partial sums of the refinement
constexpr int INL_LINE_MAX = 40;                              // a line of plane_refinement_inliers.xyz: at most 3 x 12 + 3 = 39 bytes
constexpr int RANSAC_MAX_ROUNDS = 1800;                       // PLANE_RANSAC_ROUNDS: k_ransac_score keeps 36 bytes of LDS per round (64 KB)
static_assert((size_t)RANSAC_MAX_ROUNDS * (32 + 4) <= 64 * 1024, "k_ransac_score: a plane and a counter per round in LDS");
constexpr size_t XYZC_HEADER = 148;                           // u32 n, f64 scale[3], min[3], Rinv[9], Tinv[3] (PovMesh.cpp:417-436)
inline size_t xyzc_bytes(size_t npoints) { return XYZC_HEADER + npoints * 6; }   // mesh_cam.xyzC: the header, a u16 triple per point
inline size_t nblocks256(size_t n) { return (n + 255) / 256; }
// every n-th of ninl refinement inliers, in raster order, starting with the first
inline size_t points_selected(size_t ninl, size_t every) { return (ninl + every - 1) / every; }

// Decisions that only need a few numbers (the digit of a radix-select pass, the best RANSAC candidate, a 3x3
// eigenvector) are taken by single-workgroup kernels writing into this record, so that a whole stage chain runs
// without host round trips; the host reads the record once at the end.
struct DevState {
    unsigned long long sel_k, sel_prefix, sel_total;      // radix select: remaining rank, key prefix, number of keys
    int sel_hi_shift, sel_fail;
    double zgap;
    unsigned long long ccl_best;                          // (size << 32) | ~mincm of the winning component
    int ransac_found, zero;                               // zero: the crop switch of a refinement without a crop (wass_mesh_refine_plane)
    unsigned long long ransac_best;
    double ransac_plane[4];
    double wsum, centroid[3], ninl;
    double plane[4];                                      // refined plane
    int refine_ok, pad1;
    // host-sync-free frame tail (wass_mesh_finish_frame_async): everything the xyzC encoder needs, decided on the device
    double rtR[9], rtT[3], rtRinv[9], rtTinv[3];
    double mn[3], sc[3];
    unsigned int npts, have_plane;
    unsigned long long kept1, kept2;
    unsigned long long ntri;                              // valid points the triangulation produced
    unsigned int ninl_sel, inl_text_bad;                  // refinement inliers seen by the selection for plane_refinement_inliers.xyz;
    unsigned long long inl_text_bytes;                    // ... bytes of that file's text when the device formatted it, numbers it could not format
};

struct PlaneCand { double n[3]; double d; int ok; int pad; };   // RANSAC (PovMesh.cpp:665-777)

// a layout below carved over mem, carved<CclLay>(mem, n), and its size, lay_bytes<CclLay>(n)
template <class Lay, class... A> Lay carved(void* mem, A... args) { Lay l; Carve a{ (char*)mem }; l.carve(a, args...); return l; }
template <class Lay, class... A> size_t lay_bytes(A... args) { Lay l; return measure([&](Carve& a) { l.carve(a, args...); }); }

// ---- device memory.  A slot's record: the scalars, then the radix histograms (256-aligned: one fill, not three)
struct RecordLay {
    DevState* ds; unsigned int* hist;
    void carve(Carve& a) { ds = a.take<DevState>(sizeof(DevState)); hist = a.take<unsigned int>((size_t)GAP_HIST_COPIES * GAP_BINS * 4); }
};
// The three phases below time-share the context's scratch buffer in stream order, each carved from its start: an entry point
// measures the largest layout of the phases it runs and ensures the buffer once.  Connected components of n points:
struct CclLay {
    int* parent; unsigned int* size; unsigned int* mincm;
    void carve(Carve& a, size_t n) { parent = a.take<int>(n * 4); size = a.take<unsigned int>(n * 4); mincm = a.take<unsigned int>(n * 4); }
};
// the plane stages: candidates, their inlier counts, the sample triples of `rounds` RANSAC rounds; the per-block partial sums of the
// refinement (rounds = 0: the refinement alone).  The components' arrays are dead when k_ransac_planes starts.
struct PlaneLay {
    PlaneCand* cand; unsigned long long* counts; int32_t* uv; double* part;
    void carve(Carve& a, int rounds)
    {
        cand = a.take<PlaneCand>((size_t)rounds * sizeof(PlaneCand)); counts = a.take<unsigned long long>((size_t)rounds * 8);
        uv = a.take<int32_t>((size_t)rounds * 24); part = a.take<double>((size_t)REFINE_BLOCKS * 6 * 8);
    }
};
// a compaction of n points: the total, the per-block counts that k_scan_blocks turns into offsets.  They lie over the plane stages'
// pieces, all of which are dead after k_refine_finish.  `out` > 0: the compacted output behind them (wass_mesh_refinement_inliers).
struct PackLay {
    unsigned int* total; unsigned int* bcnt; double* out;
    void carve(Carve& a, size_t n, size_t out_bytes = 0) { total = a.take<unsigned int>(4); bcnt = a.take<unsigned int>(nblocks256(n) * 4); out = a.take<double>(out_bytes); }
};
// a slot's inlier selection of up to `cap` points: totals ([0] refinement inliers, [2] bytes of text, [3] numbers not formatted), the
// points; with text also the text blocks' byte counts, the text and its per-block staging
struct InlierLay {
    unsigned int* totals; double* pts; unsigned int* blockbytes; char* text; char* staging;
    void carve(Carve& a, size_t cap, bool with_text)
    {
        const size_t t = with_text ? 1 : 0, nb = nblocks256(cap);
        totals = a.take<unsigned int>(16); pts = a.take<double>(cap * 24);
        blockbytes = a.take<unsigned int>(t * nb * 4); text = a.take<char>(t * cap * INL_LINE_MAX);
        staging = a.take<char>(t * nb * 256 * INL_LINE_MAX);
    }
};
// striped counters: kept[0 .. NSLOT) survivors of the crop by the RANSAC plane (and wass_mesh_crop_plane's one counter),
// kept[NSLOT .. 2 NSLOT) of the final crop -- one piece: k_ransac_planes clears and k_frame_header folds both; lim: [NSLOT][6] keys
struct CountersLay {
    unsigned long long* kept; unsigned long long* lim;
    void carve(Carve& a) { kept = a.take<unsigned long long>((size_t)2 * NSLOT * 8); lim = a.take<unsigned long long>((size_t)NSLOT * 6 * 8); }
};
// the limits before any point: min keys all ones, max keys zero
inline void limits_init(unsigned long long* lim) { for (int i = 0; i < NSLOT * 6; ++i) lim[i] = i % 6 < 3 ? ~0ull : 0ull; }

// ---- pinned memory: the source images of the frame tail's small host-to-device copies.  The record's initial image, what a
// stage-by-stage call was given (record_put), the limits' initial image, and a slot's RANSAC samples (two areas: the host never
// waits for the previous frame's copy).
constexpr size_t STAGE_PARAM_BYTES = 256;
struct StageLay {
    DevState* init; unsigned char* param; unsigned long long* lim_init; int32_t* uv[2];
    void carve(Carve& a)
    {
        init = a.take<DevState>(sizeof(DevState)); param = a.take<unsigned char>(STAGE_PARAM_BYTES);
        lim_init = a.take<unsigned long long>((size_t)NSLOT * 6 * 8);
        for (auto& u : uv) u = a.take<int32_t>((size_t)RANSAC_MAX_ROUNDS * 24);
    }
};

}  // namespace wass
