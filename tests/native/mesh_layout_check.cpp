// mesh_layout_check.cpp -- every layout of the frame tail's memory (wass_amd/csrc/mesh_layout.h) on the host: each is carved over
// a block of exactly its measured size; every piece must be 256-aligned, lie inside the block and overlap no other piece of its
// layout.  Exit status 0 and "ok", or the first failed check.
#include "../../wass_amd/csrc/mesh_layout.h"

#include <stdio.h>
#include <stdlib.h>
#include <vector>

using namespace wass;

struct Piece { const char* name; const void* p; size_t bytes; };

// the pieces of one layout against the block [base, base + total)
static bool check(const char* lay, const char* base, size_t total, const std::vector<Piece>& pieces)
{
    for (size_t i = 0; i < pieces.size(); ++i) {
        const Piece& a = pieces[i];
        const char* p = (const char*)a.p;
        if (a.bytes == 0) continue;                            // takes no room, nobody may follow it
        if ((uintptr_t)p % 256) return printf("%s: %s is not 256-aligned\n", lay, a.name), false;
        if (p < base || p + a.bytes > base + total) return printf("%s: %s lies outside measure()\n", lay, a.name), false;
        for (size_t j = i + 1; j < pieces.size(); ++j) {
            const char* q = (const char*)pieces[j].p;
            if (pieces[j].bytes && p < q + pieces[j].bytes && q < p + a.bytes) return printf("%s: %s overlaps %s\n", lay, a.name, pieces[j].name), false;
        }
    }
    return true;
}

// carve a layout over a block of exactly measure() bytes and hand its pieces to check()
template <class Lay, class Pieces, class... A> static bool run(const char* name, Pieces pieces, A... args)
{
    const size_t total = lay_bytes<Lay>(args...);
    char* block = (char*)aligned_alloc(256, total ? total : 256);
    Lay l;
    Carve a{ block };
    l.carve(a, args...);
    const bool ok = a.used == total && check(name, block, total, pieces(l));
    if (a.used != total) printf("%s: carved %zu bytes, measured %zu\n", name, a.used, total);
    free(block);
    return ok;
}

int main()
{
    const size_t ns[] = { 1, 256, 257, (size_t)2456 * 2058 };
    const int rounds[] = { 0, 1, 1800 };
    const size_t everys[] = { 1, 10 };
    bool ok = true;
    ok = ok && run<RecordLay>("record", [](const RecordLay& l) {
        return std::vector<Piece>{ { "ds", l.ds, sizeof(DevState) }, { "hist", l.hist, (size_t)GAP_HIST_COPIES * GAP_BINS * 4 } }; });
    ok = ok && run<CountersLay>("counters", [](const CountersLay& l) {
        return std::vector<Piece>{ { "kept1", l.kept, (size_t)NSLOT * 8 }, { "kept2", l.kept + NSLOT, (size_t)NSLOT * 8 }, { "lim", l.lim, (size_t)NSLOT * 6 * 8 } }; });
    // the pinned stage holds the record's image, the largest parameter block and 1800 sample triples per area
    ok = ok && run<StageLay>("stage", [](const StageLay& l) {
        return std::vector<Piece>{ { "init", l.init, sizeof(DevState) }, { "param", l.param, STAGE_PARAM_BYTES }, { "lim_init", l.lim_init, (size_t)NSLOT * 6 * 8 },
                                   { "uv0", l.uv[0], (size_t)1800 * 24 }, { "uv1", l.uv[1], (size_t)1800 * 24 } }; });
    // (the largest block a stage-by-stage call puts: the encoder's switch word, its pad and R, T and their inverses)
    if (STAGE_PARAM_BYTES < 8 + 24 * sizeof(double) || RANSAC_MAX_ROUNDS != 1800) return puts("stage: parameter block or uv area too small"), 1;
    for (int r : rounds)
        ok = ok && run<PlaneLay>("plane", [r](const PlaneLay& l) {
            return std::vector<Piece>{ { "cand", l.cand, (size_t)r * sizeof(PlaneCand) }, { "counts", l.counts, (size_t)r * 8 }, { "uv", l.uv, (size_t)r * 24 },
                                       { "part", l.part, (size_t)REFINE_BLOCKS * 6 * 8 } }; }, r);
    for (size_t n : ns) {
        const size_t nb = (n + 255) / 256;
        ok = ok && run<CclLay>("ccl", [n](const CclLay& l) {
            return std::vector<Piece>{ { "parent", l.parent, n * 4 }, { "size", l.size, n * 4 }, { "mincm", l.mincm, n * 4 } }; }, n);
        ok = ok && run<PackLay>("pack", [nb](const PackLay& l) { return std::vector<Piece>{ { "total", l.total, 4 }, { "bcnt", l.bcnt, nb * 4 } }; }, n);
        for (size_t every : everys) {
            const size_t cap = points_selected(n, every), nb2 = (cap + 255) / 256;
            if (cap * every < n || (cap - 1) * every >= n) return puts("points_selected is not the ceiling"), 1;
            ok = ok && run<PackLay>("pack + output", [nb, cap](const PackLay& l) {
                return std::vector<Piece>{ { "total", l.total, 4 }, { "bcnt", l.bcnt, nb * 4 }, { "out", l.out, cap * 24 } }; }, n, cap * 24);
            for (bool text : { false, true })
                ok = ok && run<InlierLay>("inliers", [cap, nb2, text](const InlierLay& l) {
                    const size_t t = text ? 1 : 0;
                    return std::vector<Piece>{ { "totals", l.totals, 16 }, { "pts", l.pts, cap * 24 }, { "blockbytes", l.blockbytes, t * nb2 * 4 },
                                               { "text", l.text, t * cap * INL_LINE_MAX }, { "staging", l.staging, t * nb2 * 256 * INL_LINE_MAX } }; }, cap, text);
        }
    }
    if (xyzc_bytes(0) != 148 || xyzc_bytes(7) != 148 + 42) return puts("xyzc_bytes"), 1;
    unsigned long long lim[NSLOT * 6];
    limits_init(lim);
    for (int i = 0; i < NSLOT * 6; ++i)
        if (lim[i] != (i % 6 < 3 ? ~0ull : 0ull)) return puts("limits_init"), 1;
    return ok ? (puts("ok"), 0) : 1;
}
