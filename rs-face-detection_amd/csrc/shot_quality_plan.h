// shot_quality_plan.h -- the geometry and the argument checks of the shot quality (include/rfd.h, "shot quality"): the region of
// a box in its frame, the edges of the 32 x 32 cell grid, the inverse map from a pixel to its cell, which bounds a config and
// a frame must keep.  Plain code with nothing of HIP in it: tests/cpp/shot_quality_plan_check.cpp builds it with the host
// compiler alone, and kernels_shot_quality.hip compiles the very same functions for the device (SQ_HD), so what the check
// program proves of the inverse map holds for the kernel.  shot_quality_host.hip does the checks.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include <cmath>

#include "../../include/rfd.h"

#if defined(__HIPCC__)
#define SQ_HD __host__ __device__
#else
#define SQ_HD
#endif

namespace rfd {

constexpr int kSqGrid = 32;                            // cells per side
constexpr int kSqMaxSide = RFD_SHOT_QUALITY_MAX_SIDE;  // a cell of a 32768 x 32768 region sums to 255 * 2^20 < 2^31

// Rust's `as i32`: toward zero, saturating, NaN -> 0 (kernels_pre.hip has the same as rust_f32_as_i32).
SQ_HD inline int32_t sq_as_i32(float f)
{
    if (f != f) return 0;
    if (f >= 2147483648.0f) return 2147483647;
    if (f <= -2147483648.0f) return -2147483647 - 1;
    return (int32_t)f;
}

// The region of a box in an H x W frame.  x0, y0 lie in [0, INT32_MAX], x1 in [INT32_MIN, W - 1], y1 in [INT32_MIN, H - 1]; the
// sides are int64, so no box overflows them.  measured: both sides >= 32, and then the region lies inside the frame.
struct SqRegion {
    int32_t x0, y0, x1, y1;
    int64_t w, h;
    bool measured;
};

SQ_HD inline SqRegion sq_region(float bx1, float by1, float bx2, float by2, int32_t W, int32_t H)
{
    SqRegion g;
    const int32_t ax = sq_as_i32(bx1), ay = sq_as_i32(by1), cx = sq_as_i32(bx2), cy = sq_as_i32(by2);
    g.x0 = ax > 0 ? ax : 0;
    g.y0 = ay > 0 ? ay : 0;
    g.x1 = cx < W - 1 ? cx : W - 1;
    g.y1 = cy < H - 1 ? cy : H - 1;
    g.w = (int64_t)g.x1 - (int64_t)g.x0 + 1;
    g.h = (int64_t)g.y1 - (int64_t)g.y0 + 1;
    g.measured = g.w >= kSqGrid && g.h >= kSqGrid;
    return g;
}

// Edge k (0 .. 32) of a side of `len` pixels, relative to the region's origin: cell c holds the pixels [edge(c), edge(c + 1)).
SQ_HD inline int32_t sq_edge(int32_t k, int32_t len) { return (int32_t)(((int64_t)k * len) / kSqGrid); }

// The cell of pixel `rel` (0 .. len - 1, relative to the origin) of a side of len >= 32 pixels: the inverse of sq_edge.
// 32 * (rel + 1) - 1 < 2^20 * 32 fits 32 bits for len <= kSqMaxSide.
SQ_HD inline int32_t sq_cell(int32_t rel, int32_t len) { return (int32_t)((32u * (uint32_t)(rel + 1) - 1u) / (uint32_t)len); }

// The bounds of rfd_shot_quality_config; a refusal names its field in msg.
inline bool sq_config_ok(const rfd_shot_quality_config &c, char *msg, size_t cap)
{
    auto no = [&](const char *what) { snprintf(msg, cap, "%s", what); return false; };
    if (c.dark < 0 || c.dark > 255) return no("dark outside 0..255");
    if (c.bright < 0 || c.bright > 255) return no("bright outside 0..255");
    if (!(c.dark < c.bright)) return no("dark is not below bright");
    if (!std::isfinite(c.pitch0)) return no("pitch0 is not finite");
    if (!(std::isfinite(c.w_yaw) && c.w_yaw >= 0.0f)) return no("w_yaw is not finite and >= 0");
    if (!(std::isfinite(c.w_roll) && c.w_roll >= 0.0f)) return no("w_roll is not finite and >= 0");
    if (!(std::isfinite(c.w_pitch) && c.w_pitch >= 0.0f)) return no("w_pitch is not finite and >= 0");
    if (!(std::isfinite(c.sharp_ref) && c.sharp_ref > 0.0f)) return no("sharp_ref is not finite and > 0");
    if (!(std::isfinite(c.size_ref) && c.size_ref > 0.0f)) return no("size_ref is not finite and > 0");
    if (c.times_score != 0 && c.times_score != 1) return no("times_score is not 0 or 1");
    return true;
}

// The bounds of a frame; a refusal says what in msg.
inline bool sq_frame_ok(const rfd_image &im, int i, char *msg, size_t cap)
{
    auto no = [&](const char *what) { snprintf(msg, cap, "frame %d: %s", i, what); return false; };
    if (!im.data) return no("data is null");
    if (im.height <= 0 || im.width <= 0) return no("non-positive size");
    if (im.height > kSqMaxSide || im.width > kSqMaxSide) return no("a side exceeds 32768 pixels");
    if (im.stride < (ptrdiff_t)im.width * 3) return no("stride < width*3 (frames must be 3-channel 8-bit)");
    return true;
}

} // namespace rfd
