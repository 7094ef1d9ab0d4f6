// track_identity_plan.h -- the host decisions of the track identities (include/rfd.h, "track identities"): which bounds a
// config must keep, how large the state may grow, how many template elements a lane holds, and how the stream list of a call
// becomes the work list of its launch.  Plain host code: nothing of the device runtime is included, so
// tests/cpp/track_identity_plan_check.cpp builds it with the host compiler alone.  track_identity_host.hip does what is decided
// here; kernels_track_identity.hip runs it.
//
// The plan of a fuse or label call IS the tracker's (track_plan.h): one workgroup walks the observations of one stream in
// time order, the face list is in (frame, row) order, so walking the stream's frames in call order and each frame's
// observations [first[b], first[b + 1]) in ascending t is that order.  A who call has no order to keep: its "plan" is the
// stream list as it stands, n ints.
#pragma once
#include "track_plan.h"

namespace rfd {

constexpr int kTrackIdentityMinDim = 32, kTrackIdentityMaxDim = 1024;
constexpr int kTrackIdentityMaxK = 32;
constexpr size_t kTrackIdentityMaxBytes = (size_t)1 << 30; // of the templates: streams * max_tracks * dim * 4

// The bounds of rfd_track_identity_config; a refusal names its field in msg.
inline bool track_identity_config_ok(const rfd_track_identity_config &c, char *msg, size_t cap)
{
    auto no = [&](const char *what) { snprintf(msg, cap, "%s", what); return false; };
    if (c.dim < kTrackIdentityMinDim || c.dim > kTrackIdentityMaxDim || c.dim % 32 != 0) return no("dim is not a multiple of 32 in 32..1024");
    if (!std::isfinite(c.accept)) return no("accept is not finite");
    if (!std::isfinite(c.release)) return no("release is not finite");
    if (!(c.release <= c.accept)) return no("release > accept");
    if (!(std::isfinite(c.margin) && c.margin >= 0.0f)) return no("margin is not finite and >= 0");
    return true;
}

// Bytes of the templates of a tracker; the heads beside them are 32 bytes per slot and not counted (rfd.h states the bound on
// streams * max_tracks * dim * 4).
inline size_t track_identity_template_bytes(int streams, int max_tracks, int dim)
{
    return (size_t)streams * (size_t)max_tracks * (size_t)dim * sizeof(float);
}
inline bool track_identity_fits(int streams, int max_tracks, int dim)
{
    return track_identity_template_bytes(streams, max_tracks, dim) <= kTrackIdentityMaxBytes;
}

// Lane l of the wave holds elements l, l + 64, ...: ceil(dim / 64) of them, rounded up to the kernel instantiations 1, 2, 4,
// 8, 16 (an element at or past dim is never touched).
inline int track_identity_lane_elems(int dim)
{
    const int need = (dim + 63) / 64;
    int j = 1;
    while (j < need) j *= 2;
    return j;
}

// The work list of a fuse or label call: track_plan's array and group count, under the name this layer uses.
inline size_t track_identity_plan_ints(int n) { return track_plan_ints(n); }
inline int track_identity_plan(const int32_t *stream, int n, int32_t *plan) { return track_plan(stream, n, plan); }

} // namespace rfd
