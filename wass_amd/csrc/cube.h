// cube.h -- what the one-shot operators of the count x H x W cube share (filter, radiance, polarimetric, pyramid, visibility,
// wavestats, specprod): the host scaffolding of a call that allocates its scratch, runs and frees it.  Plain functions and one RAII struct;
// every operator keeps its own plan and byte formula.  (The ordered-key maxima of their kernels are reduce.h's.)
// A call makes ONE hipMalloc and one hipFree by design: the scratch of a cube is gigabytes and is not kept in the context.
// The handles of spectrum.hip (wass_spec3d, wass_spatial_filter) hold an Arena for their lifetime and stage through the same
// functions.  The piece-by-piece hand-out itself (Carve, align256) is scratch.h's, which the context's pool shares.
#pragma once

#include "common.h"

namespace wass {

// A Carve over ONE hipMalloc of `total` bytes, freed when the struct goes out of scope.  A total of 0 makes no call at all, and
// every piece of it is a pointer nobody may follow.  An Arena that has reserved nothing measures, as every Carve without memory.
struct Arena : Carve {
    Arena() = default;
    Arena(const Arena&) = delete;
    Arena& operator=(const Arena&) = delete;
    ~Arena() { if (mem) (void)hipFree(mem); }
    int reserve(wass_ctx* c, size_t total, const char* what)
    {
        if (total && hipMalloc((void**)&mem, total) != hipSuccess) return set_err(c, WASS_ERR_NO_MEMORY, "hipMalloc(%zu) for %s failed", total, what);
        return WASS_OK;
    }
};

// The end of an operator `what`: the pending error e becomes the call's, unless rc already holds one; with `sync` the stream is
// waited for, which a call that holds an Arena must do before it returns (the scratch is freed then).
inline int finish(wass_ctx* c, int rc, hipError_t e, hipStream_t s, const char* what, bool sync = true)
{
    if (!rc && e != hipSuccess) rc = set_err(c, WASS_ERR_DEVICE, "%s: %s", what, hipGetErrorString(e));
    if (sync) {
        e = hipStreamSynchronize(s);
        if (!rc && e != hipSuccess) rc = set_err(c, WASS_ERR_DEVICE, "%s: %s", what, hipGetErrorString(e));
    }
    return rc;
}

// Rows of H x W per slab: as many as `avail` bytes hold at per_row bytes each (per_row 0: nothing grows with the rows), then at
// most 0x7fffff00 / W, H and, where it is positive, `asked`.
inline int slab_rows(size_t avail, size_t per_row, int H, int W, int asked, int* rows_out)
{
    size_t rows = per_row ? avail / per_row : (size_t)H;
    if (rows < 1) return WASS_ERR_NO_MEMORY;
    const size_t most = 0x7fffff00u / (size_t)W;        // the series of a slab are indexed with 32 bits
    if (rows > most) rows = most;
    if (rows > (size_t)H) rows = (size_t)H;
    if (asked > 0 && rows > (size_t)asked) rows = (size_t)asked;
    if (rows < 1) return WASS_ERR_UNSUPPORTED;
    *rows_out = (int)rows;
    return WASS_OK;
}

// Frames per launch: `asked` (0: dflt), at most count and most, halved until total(b) is at most cap.  0: not even one frame fits.
// total(b) is called last with the batch returned, so it may fill in the plan as it goes.
template <class F> int fit_batch(int asked, int dflt, int most, int count, size_t cap, F total)
{
    int b = asked ? asked : dflt;
    if (b > count) b = count;
    if (b > most) b = most;
    while (b >= 1 && total(b) > cap) b /= 2;
    return b;
}

// `count` frames, rows r0 .. r0 + rows - 1 of each, between a host cube (elements of `elem` bytes, st and sy elements from frame
// to frame and row to row, the last axis dense) and a dense count x rows x W block on the device.  A whole batch is rows == H
// with `host` at its first frame.
inline hipError_t upload_rows(void* dev, const void* host, size_t elem, int count, int r0, int rows, int W, size_t st, size_t sy, hipStream_t s)
{
    const size_t rowb = (size_t)W * elem, plane = (size_t)rows * rowb;
    hipError_t e = hipSuccess;
    for (int t = 0; t < count && e == hipSuccess; ++t)
        e = hipMemcpy2DAsync((char*)dev + (size_t)t * plane, rowb, (const char*)host + ((size_t)t * st + (size_t)r0 * sy) * elem, sy * elem, rowb, rows,
                             hipMemcpyHostToDevice, s);
    return e;
}

// The way back; with kind = hipMemcpyDeviceToDevice `host` is a cube on the device.
inline hipError_t download_rows(void* host, const void* dev, size_t elem, int count, int r0, int rows, int W, size_t st, size_t sy, hipStream_t s,
                                hipMemcpyKind kind = hipMemcpyDeviceToHost)
{
    const size_t rowb = (size_t)W * elem, plane = (size_t)rows * rowb;
    hipError_t e = hipSuccess;
    for (int t = 0; t < count && e == hipSuccess; ++t)
        e = hipMemcpy2DAsync((char*)host + ((size_t)t * st + (size_t)r0 * sy) * elem, sy * elem, (const char*)dev + (size_t)t * plane, rowb, rowb, rows,
                             kind, s);
    return e;
}

}  // namespace wass
