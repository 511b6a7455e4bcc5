// mesh_tail.h -- FrameTail: the state of the frame tail (mesh.hip), the one chain that runs for every stereo pair, owned in one
// place.  wass_ctx holds it by value; its events, pinned blocks and buffers free themselves with the context (wass_ctx_destroy:
// the device is selected and the streams have been synchronised).
#pragma once
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include "mesh_layout.h"

namespace wass {

// an event / a block of pinned memory that is released with its owner; create() and alloc() do nothing the second time
struct NoCopy { NoCopy() = default; NoCopy(const NoCopy&) = delete; NoCopy& operator=(const NoCopy&) = delete; };
struct Event : NoCopy {
    hipEvent_t e = nullptr;
    ~Event() { if (e) (void)hipEventDestroy(e); }
    bool create(unsigned flags) { return e || hipEventCreateWithFlags(&e, flags) == hipSuccess; }
    operator hipEvent_t() const { return e; }
};
struct Pinned : NoCopy {
    void* p = nullptr;
    ~Pinned() { if (p) (void)hipHostFree(p); }
    bool alloc(size_t bytes) { return p || hipHostMalloc(&p, bytes, hipHostMallocDefault) == hipSuccess; }
};

struct FrameTail {
    // Up to TWO frames may be pending (round 5): a driver enqueues frame n's tail BEFORE it reads frame n-1's record, so that the tail
    // stream never waits for the previous frame's downloads plus a host round trip (with one record per context that chain, not the
    // SGM stage, set the C++ driver's frame period).  Everything a pending frame needs is per slot; frame k lives in slot(k).
    struct Slot {
        Buf rec_buf, inl;          // the device record with its radix histograms (rec) / every n-th refinement inlier (InlierLay)
        RecordLay rec = {};
        Pinned h_frame;            // the record as downloaded (created by the slot's first frame)
        int32_t* h_uv = nullptr;   // the slot's RANSAC samples in the pinned stage ...
        Event ev_uv;               // ... have been copied to the device
        bool uv_busy = false;
        Event ev_copy;             // the frame's downloads have finished
        int inl_every = 0;         // > 0: the frame also selected every n-th refinement inlier
        bool inl_text = false;     // ... and formatted plane_refinement_inliers.xyz on the device
        size_t inl_cap = 0;        // ... capacity (points) of the selection
        unsigned long long sgm_call = 0;   // 1-based index of the SGM call whose disparity the frame was built from
        int tail_set = 0;          // the timing-event set its tail was recorded into
    } slots[2];
    unsigned long long nframe_enq = 0, nframe_col = 0;   // frame tails enqueued / records read
    unsigned long long cur_frame = 0;                     // the frame whose slot the stage helpers (and the stage-by-stage calls) use
    Slot& slot(unsigned long long frame) { return slots[frame & 1]; }
    Slot& cur() { return slot(cur_frame); }
    Pinned h_stage;                // StageLay, created on first use (mesh.hip host_stage)
    StageLay stage = {};
    Event ev_pack;                 // the tail stream has finished the file image
    hipEvent_t ev_copy = nullptr;  // the most recently recorded download event: an alias of one of the slots'
    // stage times of the frame tail (wass_frame_result.stage_ms): [0] before k_triangulate, [1] entry of the mesh tail, [2] z-gap
    // percentile found, [3] biggest component kept, [4] RANSAC plane picked, [5] file image packed.  Created on first use.
    // Four sets, alternated by wass_triangulate[_dev]: a pipelined driver enqueues frame n+1's triangulation BEFORE it reads frame
    // n's record, and with two frames pending a record is read after two more triangulations.
    Event ev_sets[4][6];
    int tail_set = 0;              // set of the last triangulation
    bool timed[4] = {};
    Event* ev() { return ev_sets[tail_set]; }
    Buf counters;                  // striped counters and limit keys ...
    CountersLay cn = {};           // ... as laid out in it
    Buf tri_cnt;                   // striped count of the points the last triangulation produced
    Buf xyzc;                      // the file image of mesh_cam.xyzC (own buffer: downloaded asynchronously)
    Buf ccmask;                    // valid mask after the outlier removal, kept for graph_components.jpg when asked for (jpeg.hip)

    // what a context needs from its first call on: ev_copy blocks the waiting host thread unless WASS_SPIN_WAIT is set
    bool init()
    {
        const unsigned copy_flags = hipEventDisableTiming | (getenv("WASS_SPIN_WAIT") ? 0 : hipEventBlockingSync);
        if (!ev_pack.create(hipEventDisableTiming) || !slots[0].ev_copy.create(copy_flags) || !slots[1].ev_copy.create(copy_flags)) return false;
        ev_copy = slots[0].ev_copy;
        return true;
    }
};

}  // namespace wass
