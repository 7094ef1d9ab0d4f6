// view_plan.h -- the host decisions of "detection over overlapping views" (include/rfd.h, "views"): how a frame is cut into
// overlapping tiles (rfd_view_plan), and where each view of a call stands among the views of its frame (view_slots), which fixes
// the layout the device merge works on.  Plain host code: nothing of HIP is included, so tests/cpp/view_plan_check.cpp builds it
// with the host compiler alone.  detector.hip does what is decided here; kernels_post.hip (decode_views_kernel) runs it.
//
// Tiling along one axis.  W the frame extent, t the tile extent, o the overlap, 0 <= o < t.
//   W <= t : one tile [0, W).
//   else   : n = ceil((W - o) / (t - o)) tiles of extent exactly t, tile i at floor(i * (W - t) / (n - 1)).
// The last tile ends at W (i = n - 1 gives W - t).  Neighbouring starts differ by at most ceil((W - t) / (n - 1)), and
// n - 1 >= (W - t) / (t - o) makes that at most t - o: neighbours overlap by at least o, so every pixel is covered.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/rfd.h"

namespace rfd {

constexpr uint32_t kViewInnerLeft = 1u, kViewInnerTop = 2u, kViewInnerRight = 4u, kViewInnerBottom = 8u;

inline void view_config_default(rfd_view_config *cfg, int net_w, int net_h)
{
    cfg->tile_w = net_w;   // scale 1: a tile is read pixel for pixel
    cfg->tile_h = net_h;
    cfg->overlap = net_w / 5;
    cfg->full_view = 1;
    cfg->edge_margin = 4.0f; // network pixels; a chosen value, not tuned on data (rfd.h)
}

// tiles of one axis; 0: the arguments are outside the rule
inline int64_t view_axis_tiles(int64_t W, int64_t t, int64_t o)
{
    if (W < 1 || t < 1 || o < 0 || o >= t) return 0;
    if (W <= t) return 1;
    return (W - o + (t - o) - 1) / (t - o);
}

// start of tile i of n (view_axis_tiles) along an axis of extent W
inline int64_t view_axis_start(int64_t W, int64_t t, int64_t n, int64_t i) { return n <= 1 ? 0 : i * (W - t) / (n - 1); }

// The views of one frame: the whole frame first (full_view set and more than one tile; inner = 0), then the tiles row-major.
// *count is always written: the number of views the plan has, or 0 where the arguments are refused.  count > cap:
// RFD_ERR_CAPACITY and nothing else is written.
inline int view_plan(int frame, int frame_w, int frame_h, const rfd_view_config *cfg, rfd_view *out, int cap, int *count)
{
    if (!count) return RFD_ERR_INVALID_ARG;
    *count = 0;
    if (!cfg || frame < 0 || cap < 0 || (cap > 0 && !out)) return RFD_ERR_INVALID_ARG;
    const int64_t nx = view_axis_tiles(frame_w, cfg->tile_w, cfg->overlap), ny = view_axis_tiles(frame_h, cfg->tile_h, cfg->overlap);
    if (nx < 1 || ny < 1) return RFD_ERR_INVALID_ARG;
    const bool full = cfg->full_view != 0 && nx * ny > 1;
    const int64_t total = nx * ny + (full ? 1 : 0);
    *count = total > INT32_MAX ? INT32_MAX : (int)total;
    if (total > cap) return RFD_ERR_CAPACITY;
    int k = 0;
    if (full) out[k++] = rfd_view{frame, 0, 0, frame_w, frame_h, 0u};
    const int w = frame_w <= cfg->tile_w ? frame_w : cfg->tile_w, h = frame_h <= cfg->tile_h ? frame_h : cfg->tile_h;
    for (int64_t j = 0; j < ny; ++j)
        for (int64_t i = 0; i < nx; ++i) {
            const int x = (int)view_axis_start(frame_w, cfg->tile_w, nx, i), y = (int)view_axis_start(frame_h, cfg->tile_h, ny, j);
            const uint32_t inner = (x > 0 ? kViewInnerLeft : 0u) | (y > 0 ? kViewInnerTop : 0u) |
                                   ((int64_t)x + w < frame_w ? kViewInnerRight : 0u) | ((int64_t)y + h < frame_h ? kViewInnerBottom : 0u);
            out[k++] = rfd_view{frame, x, y, w, h, inner};
        }
    return RFD_OK;
}

// What is wrong with the views of a call, for the caller's message.
enum ViewFault : int { kViewOk = 0, kViewFrameRange, kViewFrameOrder, kViewEmpty, kViewOrigin, kViewInnerBits };

// slot[i] = the position of view i among the views of its frame; *vmax = the most views any frame has (0 for no views).
// The views are sorted by frame, each names a frame of [0, n_frames), is non-empty, starts at x, y >= 0 and sets no bit of
// `inner` above the four sides'.  Otherwise the fault is returned, *bad names the first offending view and slot / vmax are
// not to be used.
inline ViewFault view_slots(const rfd_view *views, int n_views, int n_frames, int32_t *slot, int *vmax, int *bad)
{
    *vmax = 0;
    int run = 0;
    for (int i = 0; i < n_views; ++i) {
        const rfd_view &v = views[i];
        *bad = i;
        if (v.frame < 0 || v.frame >= n_frames) return kViewFrameRange;
        if (i > 0 && v.frame < views[i - 1].frame) return kViewFrameOrder;
        if (v.w < 1 || v.h < 1) return kViewEmpty;
        if (v.x < 0 || v.y < 0) return kViewOrigin;
        if (v.inner > 15u) return kViewInnerBits;
        run = i > 0 && v.frame == views[i - 1].frame ? run + 1 : 0;
        slot[i] = run;
        if (run + 1 > *vmax) *vmax = run + 1;
    }
    *bad = -1;
    return kViewOk;
}

// view v lies inside a frame of frame_w x frame_h (64-bit: x + w of two int32 does not wrap)
inline bool view_inside(const rfd_view &v, int frame_w, int frame_h)
{
    return v.x >= 0 && v.y >= 0 && v.w >= 1 && v.h >= 1 && (int64_t)v.x + v.w <= frame_w && (int64_t)v.y + v.h <= frame_h;
}

} // namespace rfd
