// redact_plan.h -- the geometry and the argument checks of the redaction (include/rfd.h, "redaction"): the region of a box with
// its margins in its frame, the ellipse rule, the tiles a workgroup owns and the grid of a call, which bounds a config and a
// frame must keep.  Plain code with nothing of HIP in it: tests/cpp/redact_plan_check.cpp builds it with the host compiler
// alone, and kernels_redact.hip compiles the very same functions for the device (RD_HD), so what the check program proves of
// the region, the ellipse sum and the tiles holds for the kernel.  redact_host.hip does the checks.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/rfd.h"

#if defined(__HIPCC__)
#define RD_HD __host__ __device__
#else
#define RD_HD
#endif

namespace rfd {

constexpr int kRdMaxSide = RFD_REDACT_MAX_SIDE; // sides <= 2^15: every term of the ellipse rule is <= 2^60
constexpr int kRdTileTarget = 64;               // a tile is the largest multiple of the cell that is <= 64 pixels a side
constexpr int kRdMinCell = 2, kRdMaxCell = 64;
constexpr int kRdMaxTileCells = (kRdTileTarget / kRdMinCell) * (kRdTileTarget / kRdMinCell); // 1024 cells of 2 x 2

// Rust's `as i32`: toward zero, saturating, NaN -> 0 (as sq_as_i32 of shot_quality_plan.h).
RD_HD inline int32_t rd_as_i32(float f)
{
    if (f != f) return 0;
    if (f >= 2147483648.0f) return 2147483647;
    if (f <= -2147483648.0f) return -2147483647 - 1;
    return (int32_t)f;
}

RD_HD inline bool rd_finite(float f) { return f >= -3.402823466e+38f && f <= 3.402823466e+38f; } // false for a NaN

// The region of a box, grown by its margins, in an H x W frame.  Every f32 step is one operation in the order rfd.h writes.
// Not skipped: 0 <= x0 <= x1 <= W - 1 and 0 <= y0 <= y1 <= H - 1.
struct RdRegion {
    int32_t x0, y0, x1, y1;
    bool skipped;
};

RD_HD inline RdRegion rd_region(float bx1, float by1, float bx2, float by2, float margin_x, float margin_top, float margin_bottom,
                                int32_t W, int32_t H)
{
    RdRegion g = {0, 0, -1, -1, true};
    if (!(rd_finite(bx1) && rd_finite(by1) && rd_finite(bx2) && rd_finite(by2))) return g;
    const float bw = bx2 - bx1, bh = by2 - by1;
    if (!(bw >= 0.0f) || !(bh >= 0.0f)) return g;
    const float gx = bw * margin_x, gt = bh * margin_top, gb = bh * margin_bottom;
    const float xa = bx1 - gx, xb = bx2 + gx, ya = by1 - gt, yb = by2 + gb;
    if (xa != xa || xb != xb || ya != ya || yb != yb) return g;
    const int32_t ax = rd_as_i32(xa), ay = rd_as_i32(ya), cx = rd_as_i32(xb), cy = rd_as_i32(yb);
    g.x0 = ax > 0 ? ax : 0;
    g.y0 = ay > 0 ? ay : 0;
    g.x1 = cx < W - 1 ? cx : W - 1;
    g.y1 = cy < H - 1 ? cy : H - 1;
    g.skipped = g.x1 < g.x0 || g.y1 < g.y0;
    return g;
}

// ELLIPSE: pixel (x, y) of a region of w x h pixels at (X0, Y0) is covered iff dx^2 h^2 + dy^2 w^2 <= w^2 h^2 with dx = 2 (x - X0)
// + 1 - w, dy = 2 (y - Y0) + 1 - h.  |dx| < w, |dy| < h <= 2^15, so a term is < 2^60 and the sum < 2^61.
RD_HD inline uint64_t rd_sq(int32_t v) { return (uint64_t)((int64_t)v * (int64_t)v); }
RD_HD inline uint64_t rd_ellipse_rhs(int32_t dy, int32_t w, int32_t h) { return rd_sq(w) * rd_sq(h) - rd_sq(dy) * rd_sq(w); } // what dx^2 h^2 may reach
RD_HD inline bool rd_ellipse_covers(int32_t dx, int32_t dy, int32_t w, int32_t h) { return rd_sq(dx) * rd_sq(h) <= rd_ellipse_rhs(dy, w, h); }

// Tiles: a workgroup owns a square of whole frame-anchored cells, `tile` pixels a side, cut by the frame's right and bottom edge.
RD_HD inline int32_t rd_tile_side(int32_t cell) { return cell * (kRdTileTarget / cell); } // 33 .. 64 for cell 2 .. 64
RD_HD inline int32_t rd_tiles(int32_t len, int32_t tile) { return (len + tile - 1) / tile; }
RD_HD inline int32_t rd_frame_tiles(int32_t W, int32_t H, int32_t tile) { return rd_tiles(W, tile) * rd_tiles(H, tile); } // <= 993^2

// The grid of a call: x = the tiles of its largest frame (workgroups past a smaller frame's tiles leave at once), y = the frame.
struct RdGrid {
    uint32_t x, y;
};
inline RdGrid rd_grid(const rfd_image *imgs, int n, int32_t cell)
{
    RdGrid g = {1, (uint32_t)n};
    const int32_t tile = rd_tile_side(cell);
    for (int i = 0; i < n; ++i) {
        const uint32_t t = (uint32_t)rd_frame_tiles(imgs[i].width, imgs[i].height, tile);
        if (t > g.x) g.x = t;
    }
    return g;
}

// The bounds of rfd_redact_config; a refusal names its field in msg.
inline bool rd_config_ok(const rfd_redact_config &c, char *msg, size_t cap)
{
    auto no = [&](const char *what) { snprintf(msg, cap, "%s", what); return false; };
    auto margin = [](float m) { return rd_finite(m) && m >= 0.0f && m <= 4.0f; };
    if (c.mode != RFD_REDACT_FILL && c.mode != RFD_REDACT_PIXELATE) return no("mode is not FILL or PIXELATE");
    if (c.shape != RFD_REDACT_RECT && c.shape != RFD_REDACT_ELLIPSE) return no("shape is not RECT or ELLIPSE");
    if (c.cell < kRdMinCell || c.cell > kRdMaxCell) return no("cell outside 2..64");
    if (c.fill[3] != 0) return no("fill[3] is not 0");
    if (!margin(c.margin_x)) return no("margin_x is not finite and in 0..4");
    if (!margin(c.margin_top)) return no("margin_top is not finite and in 0..4");
    if (!margin(c.margin_bottom)) return no("margin_bottom is not finite and in 0..4");
    for (int i = 0; i < 6; ++i)
        if (c.reserved[i] != 0) return no("reserved is not zero");
    return true;
}

// The bounds of a frame (what: "frame" or "dst"); a refusal says what in msg.
inline bool rd_frame_ok(const rfd_image &im, const char *what, int i, char *msg, size_t cap)
{
    auto no = [&](const char *why) { snprintf(msg, cap, "%s %d: %s", what, i, why); return false; };
    if (!im.data) return no("data is null");
    if (im.height <= 0 || im.width <= 0) return no("non-positive size");
    if (im.height > kRdMaxSide || im.width > kRdMaxSide) return no("a side exceeds 32768 pixels");
    if (im.stride < (ptrdiff_t)im.width * 3) return no("stride < width*3 (frames must be 3-channel 8-bit)");
    return true;
}

// dst[i] against imgs[i]: its own bounds, and the size of its source.
inline bool rd_dst_ok(const rfd_image &dst, const rfd_image &src, int i, char *msg, size_t cap)
{
    if (!rd_frame_ok(dst, "dst", i, msg, cap)) return false;
    if (dst.height != src.height || dst.width != src.width) {
        snprintf(msg, cap, "dst %d: size %d x %d differs from its frame's %d x %d", i, dst.width, dst.height, src.width, src.height);
        return false;
    }
    return true;
}

} // namespace rfd
