// track_plan.h -- the host decisions of the tracker (include/rfd.h, "tracker"): which bounds a config must keep, and how the
// stream list of one update call becomes the work list of its launch.  Plain host code: nothing of HIP is included, so
// tests/cpp/track_plan_check.cpp builds it with the host compiler alone.  tracker_host.hip does what is decided here;
// kernels_track.hip (track_update_kernel) runs it.
//
// The plan.  One workgroup walks the frames of one stream in call order, so the call's frames are grouped by stream: the
// distinct streams in ascending order, each with the indices of its frames in call order (a stable grouping).  The plan is one
// array of 3 n + 1 ints that travels to the device as it stands:
//     group_stream [n]      stream of group g             (g < groups)
//     group_first  [n + 1]  order[group_first[g] .. group_first[g + 1]) are the frames of group g
//     order        [n]      frame indices, grouped
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <cmath>

#include "../../include/rfd.h"

namespace rfd {

constexpr int kTrackMaxStreams = 4096;

inline size_t track_plan_ints(int n) { return 3 * (size_t)n + 1; }
inline int32_t *track_plan_group_stream(int32_t *plan, int) { return plan; }
inline int32_t *track_plan_group_first(int32_t *plan, int n) { return plan + n; }
inline int32_t *track_plan_order(int32_t *plan, int n) { return plan + 2 * (size_t)n + 1; }

// The first frame whose stream lies outside [0, streams), or -1.
inline int track_plan_bad_stream(const int32_t *stream, int n, int streams)
{
    for (int i = 0; i < n; ++i)
        if (stream[i] < 0 || stream[i] >= streams) return i;
    return -1;
}

// Fills plan (track_plan_ints(n) ints) for checked streams; returns the number of groups.
inline int track_plan(const int32_t *stream, int n, int32_t *plan)
{
    int32_t *gs = track_plan_group_stream(plan, n), *gf = track_plan_group_first(plan, n), *order = track_plan_order(plan, n);
    for (int i = 0; i < n; ++i) order[i] = i;
    std::stable_sort(order, order + n, [stream](int32_t a, int32_t b) { return stream[a] < stream[b]; });
    int groups = 0;
    for (int i = 0; i < n; ++i)
        if (i == 0 || stream[order[i]] != stream[order[i - 1]]) {
            gs[groups] = stream[order[i]];
            gf[groups] = i;
            ++groups;
        }
    gf[groups] = n;
    for (int g = groups; g < n; ++g) gs[g] = -1; // the unused tail is defined: the slot is copied whole
    for (int g = groups + 1; g <= n; ++g) gf[g] = n;
    return groups;
}

// The bounds of rfd_tracker_config; a refusal names its field in msg.
inline bool track_config_ok(const rfd_tracker_config &c, char *msg, size_t cap)
{
    auto no = [&](const char *what) { snprintf(msg, cap, "%s", what); return false; };
    if (c.streams < 1 || c.streams > kTrackMaxStreams) return no("streams outside 1..4096");
    if (c.max_tracks != 64 && c.max_tracks != 128 && c.max_tracks != 256) return no("max_tracks is not 64, 128 or 256");
    if (!(std::isfinite(c.iou_min) && c.iou_min > 0.0f)) return no("iou_min is not finite and > 0");
    if (c.max_missed < 0) return no("max_missed < 0");
    if (std::isnan(c.min_score)) return no("min_score is NaN");
    if (!(c.new_score >= c.min_score)) return no("new_score < min_score (or NaN)");
    if (c.min_hits < 1) return no("min_hits < 1");
    if (!(std::isfinite(c.improve) && c.improve >= 1.0f)) return no("improve is not finite and >= 1");
    return true;
}

} // namespace rfd
