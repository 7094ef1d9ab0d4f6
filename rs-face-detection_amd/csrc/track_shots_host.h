// track_shots_host.h -- what the track shots (include/rfd.h, "track shots") own on the device beside a tracker's slots, and what
// their kernels are told.  track_shots_host.hip holds the entries; the kernels are kernels_track_shots.hip; the host decisions
// are track_shots_plan.h.  rfd_tracker (tracker_host.h) holds one TrackShotState, empty until rfd_tracker_shots_enable.
#pragma once
#include "ctx_access.h"
#include "host_resources.h"
#include "track_shots_plan.h"

namespace rfd {

struct TrackSlot;   // tracker_host.h
struct TrackIdHead; // track_identity_host.h

// The head of one entry in HBM: 32 bytes, read and written as two 16-byte halves.  It belongs to the track in its slot only
// while serial equals the slot's.
struct TrackShotHead {
    int32_t serial;
    int32_t shots;
    int32_t kept;
    float q;
    int64_t first_stamp;
    int64_t best_stamp;
};
static_assert(sizeof(TrackShotHead) == 32, "TrackShotHead is two 16-byte halves");

// One row copy: row `src` of the source rows to row `dst` of the destination rows.
struct ShotCopyItem {
    int32_t src, dst;
};

struct TrackShotState {
    bool enabled = false;
    rfd_track_shot_config cfg = {};
    size_t row_bytes = 0;
    DevBuf heads; // [streams][max_tracks] TrackShotHead, zero at enable
    DevBuf bank;  // [streams][max_tracks][crop_h][crop_w][3] u8
    // the stream list and the stamps of a call travel through a ring of this state's own, so the tracker's ring stays as it is
    static constexpr int kRing = 4;
    PinnedRing<kRing> ring;
    DevBuf call;  // device copy of a ring slot (track_shot_ring_bytes(max_batch))
    // the work list between the deciding kernel of a call and its copy: segments of max_tracks items, one per group (keep) or
    // one in all (collect), each with its count
    DevBuf items;     // [max_batch][max_tracks] ShotCopyItem
    DevBuf seg_count; // [max_batch] int32
    DevBuf scratch;   // collect: [max_batch] counts, [max_batch + 1] prefix, [max_batch][max_tracks] found entries
    // host forms, allocated by their first call: the device twins of the caller's arrays
    DevBuf h_total, h_first, h_row, h_serial, h_crops, h_face_status, h_q, h_status, h_stats, h_ended, h_rtotal, h_rfirst, h_rec,
        h_rcrops;
};

// what the kernels are told about the tracker
struct TrackShotCommon {
    const int32_t *plan;  // keep: track_plan's array for n frames; collect: stream[n]
    const int64_t *stamp; // [n]
    int n, max_det, max_tracks;
    const TrackSlot *slots; // [streams][max_tracks], read only
    TrackShotHead *heads;
    ShotCopyItem *items;
    int32_t *seg_count;
};

struct TrackShotDecideParams {
    TrackShotCommon c;
    const int32_t *total, *first, *row, *serial; // rfd_track_obs
    int m;
    const int32_t *face_status;
    const float *q;
    int32_t *status;
};

struct TrackRecordListParams {
    TrackShotCommon c;
    const int32_t *stats, *ended;
    int cap;
    const TrackIdHead *id_heads; // null: identities are not enabled
    int32_t *scratch;
    int32_t *total, *first;
    rfd_track_record *rec;
};

struct ShotCopyParams {
    const uint8_t *src;
    uint8_t *dst;
    uint32_t row_bytes;
    const ShotCopyItem *items;
    const int32_t *seg_count;
    int segments, seg_stride;
};

// one workgroup of one wave per group of the plan
int launch_track_shot_decide(const TrackShotDecideParams &p, int groups, hipStream_t s);
// one workgroup
int launch_track_record_list(const TrackRecordListParams &p, hipStream_t s);
// `bound` items (the host-known most) times the chunks of a row
int launch_shot_copy(const ShotCopyParams &p, int bound, hipStream_t s);

} // namespace rfd
