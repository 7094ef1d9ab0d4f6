// track_identity_host.h -- what the track identities (include/rfd.h, "track identities") own on the device beside a tracker's
// slots, and what their kernels are told.  track_identity_host.hip holds the entries; the kernels are kernels_track_identity.hip;
// the host decisions are track_identity_plan.h.  rfd_tracker (tracker_host.h) holds one TrackIdentityState, empty until
// rfd_tracker_identity_enable.
#pragma once
#include "ctx_access.h"
#include "host_resources.h"
#include "track_identity_plan.h"

namespace rfd {

struct TrackSlot; // tracker_host.h

// The head of one entry in HBM: 32 bytes, read and written as two 16-byte halves.  It belongs to the track in its slot only
// while serial equals the slot's.
struct TrackIdHead {
    int32_t serial;
    int32_t identity;
    int32_t row;
    float score;
    int32_t named;
    int32_t shots;
    float weight;
    int32_t pad;
};
static_assert(sizeof(TrackIdHead) == 32, "TrackIdHead is two 16-byte halves");

struct TrackIdentityState {
    bool enabled = false;
    rfd_track_identity_config cfg = {};
    DevBuf heads;     // [streams][max_tracks] TrackIdHead, zero at enable
    DevBuf templates; // [streams][max_tracks][dim] f32, zero at enable
    // host forms, allocated by their first call: the device twins of the caller's arrays
    DevBuf h_total, h_first, h_row, h_serial, h_emb, h_weight, h_query, h_status, h_scores, h_rows, h_ids, h_track, h_count,
        h_flags, h_who, h_identity, h_id_score;
};

// what every kernel of this file is told about the tracker
struct TrackIdCommon {
    const int32_t *plan; // fuse, label: track_plan's array for n frames; who: stream[n]
    int n, max_det, max_tracks, dim;
    const TrackSlot *slots; // [streams][max_tracks], read only
    TrackIdHead *heads;
    float *templates;
};

struct TrackFuseParams {
    TrackIdCommon c;
    const int32_t *total, *first, *row, *serial; // rfd_track_obs
    int m;
    const float *emb, *weight;
    float *query;
    int32_t *status;
};

struct TrackLabelParams {
    TrackIdCommon c;
    const int32_t *total, *first, *row, *serial;
    int m, k;
    const float *scores;
    const int32_t *rows, *ids, *status_in;
    float accept, release, margin;
};

struct TrackWhoParams {
    TrackIdCommon c;
    const int32_t *track, *count;
    const uint32_t *flags_in;
    uint32_t *who;
    int32_t *identity;
    float *id_score;
};

// one workgroup of one wave per group of the plan
int launch_track_fuse(const TrackFuseParams &p, int groups, hipStream_t s);
int launch_track_label(const TrackLabelParams &p, int groups, hipStream_t s);
// workgroups of 256 rows, ceil(max_det / 256) per frame
int launch_track_who(const TrackWhoParams &p, hipStream_t s);

} // namespace rfd
