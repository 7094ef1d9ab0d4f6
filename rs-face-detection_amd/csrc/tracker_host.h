// tracker_host.h -- rfd_tracker: what a tracker (include/rfd.h, "tracker") owns on the device, and what its kernel is told.
// tracker_host.hip holds every rfd_tracker_* entry; the kernel is kernels_track.hip; the host decisions are track_plan.h.
#pragma once
#include "ctx_access.h" // what a tracker needs of its context: ctx_stream, ctx_device
#include "host_resources.h"
#include "track_plan.h"
#include "track_identity_host.h" // TrackIdentityState: empty unless identities are enabled
#include "track_shots_host.h"    // TrackShotState: empty unless shots are enabled

namespace rfd {

// One slot of a stream in HBM: 32 bytes, read and written as two 16-byte halves.  serial 0 = free.
struct TrackSlot {
    int32_t serial;
    int32_t missed;
    int32_t hits;
    float shot_q;
    float box[4];
};
static_assert(sizeof(TrackSlot) == 32, "TrackSlot is two 16-byte halves");

struct TrackParams {
    // the call
    const int32_t *plan; // device copy of track_plan's array for n frames
    int n, max_det;
    const float *boxes;  // [n][max_det][5]
    const float *lmk;    // [n][max_det][10]
    const int *count;    // [n]
    const float *quality; // [n][max_det] or null
    // the config
    float iou_min, min_score, new_score, improve;
    int max_missed, min_hits, max_tracks;
    // the state
    TrackSlot *slots;     // [streams][max_tracks]
    int32_t *next_serial; // [streams]
    // the outputs (rfd_track_out)
    int32_t *track;
    uint32_t *flags;
    int32_t *stats, *ended;
    float *due_boxes, *due_lmk;
    int32_t *due_count, *due_total, *due_track;
};

// one workgroup (one wave) per group of the plan
int launch_track_update(const TrackParams &p, int groups, hipStream_t s);
inline size_t track_update_lds_bytes(int max_det) { return (size_t)max_det * 8; }

} // namespace rfd

// The tracks of `streams` cameras of one context in HBM.  Next to the context, which lends it its device and stream; the caller
// destroys it first.
struct rfd_tracker {
    rfd_ctx *ctx = nullptr;
    rfd_tracker_config cfg = {};
    int max_batch = 0, max_det = 0; // of the context, fixed at its creation
    rfd::DevBuf slots;              // [streams][max_tracks] TrackSlot, zero = every slot free
    rfd::DevBuf next_serial;        // [streams] int32, 1 at creation
    // the stream list of a call travels as its plan through a ring of page-locked slots, so an update enqueues without waiting
    // for the stream
    static constexpr int kRing = 4;
    rfd::PinnedRing<kRing> plan_ring;
    rfd::DevBuf plan;
    // host form, allocated by its first call: the device twins of the caller's arrays
    rfd::DevBuf h_boxes, h_lmk, h_count, h_quality, h_track, h_flags, h_stats, h_ended, h_due_boxes, h_due_lmk, h_due_count,
        h_due_total, h_due_track;
    // the track identities (track_identity_host.hip): nothing is allocated before rfd_tracker_identity_enable
    rfd::TrackIdentityState ident;
    // the track shots (track_shots_host.hip): nothing is allocated before rfd_tracker_shots_enable
    rfd::TrackShotState shots;
};
