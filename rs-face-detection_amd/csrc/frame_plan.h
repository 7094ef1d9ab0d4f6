// frame_plan.h -- the host half of a frame conversion call (include/rfd.h, "frames in camera and decoder formats"): the planes
// of a format at a size, the checks that can refuse a call, the descriptor frame_convert_kernel reads for each frame, and
// the decomposition of a batch into work items and workgroups.  Plain code with nothing of HIP in it:
// tests/cpp/frame_plan_check.cpp builds it with the host compiler alone, frame_host.hip runs it before anything is enqueued,
// kernels_frame.hip reads the descriptors it fills.  rfd_frame_layout_of is frame_layout with a status.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/rfd.h"

namespace rfd {

constexpr int kFrameFormats = 10; // RFD_PIXEL_BGR .. RFD_PIXEL_UYVY
constexpr int kFrameColors = 4;   // RFD_COLOR_BT601_LIMITED .. RFD_COLOR_BT709_FULL
constexpr int kFrameGroup = 256;  // work items per workgroup: one thread each
constexpr int kFrameMaxSide = 1 << 28; // 4 * width stays inside rfd_frame_layout's int32 row_bytes

// lower case: the library holds no string that looks like one of its environment variables (tests/test_build_cpu.py)
inline const char *frame_format_name(int format)
{
    static const char *const names[kFrameFormats] = {"bgr", "rgb", "bgra", "rgba", "gray", "nv12", "nv21", "i420", "yuyv", "uyvy"};
    return format >= 0 && format < kFrameFormats ? names[format] : "unknown";
}

inline bool frame_is_420(int format) { return format == RFD_PIXEL_NV12 || format == RFD_PIXEL_NV21 || format == RFD_PIXEL_I420; }
inline bool frame_is_yuv(int format) { return format >= RFD_PIXEL_NV12 && format <= RFD_PIXEL_UYVY; }

// The planes of `format` at width x height: how many, the bytes of a row of each and its rows.  false: unknown format or a side
// outside 1 .. kFrameMaxSide; *out is then untouched.
inline bool frame_layout(int format, int width, int height, rfd_frame_layout *out)
{
    if (format < 0 || format >= kFrameFormats) return false;
    if (width < 1 || height < 1 || width > kFrameMaxSide || height > kFrameMaxSide) return false;
    const int32_t cw = (width + 1) / 2, ch = (height + 1) / 2;
    rfd_frame_layout l;
    memset(&l, 0, sizeof l);
    l.planes = 1;
    l.rows[0] = height;
    switch (format) {
    case RFD_PIXEL_BGR: case RFD_PIXEL_RGB: l.row_bytes[0] = 3 * width; break;
    case RFD_PIXEL_BGRA: case RFD_PIXEL_RGBA: l.row_bytes[0] = 4 * width; break;
    case RFD_PIXEL_GRAY: l.row_bytes[0] = width; break;
    case RFD_PIXEL_NV12: case RFD_PIXEL_NV21:
        l.planes = 2;
        l.row_bytes[0] = width;
        l.row_bytes[1] = 2 * cw; l.rows[1] = ch;
        break;
    case RFD_PIXEL_I420:
        l.planes = 3;
        l.row_bytes[0] = width;
        l.row_bytes[1] = l.row_bytes[2] = cw; l.rows[1] = l.rows[2] = ch;
        break;
    default: l.row_bytes[0] = 4 * cw; break; // YUYV, UYVY
    }
    *out = l;
    return true;
}

// The rows of rfd.h's table, x 2^20 rounded: CY, CVR, CUG, CVG, CUB, and what is taken off Y first (16 in the limited ranges).
struct FrameCoef {
    int32_t cy, cvr, cug, cvg, cub, y0;
};
inline FrameCoef frame_coef(int color)
{
    static const FrameCoef table[kFrameColors] = {
        {1220542, 1673527, -409993, -852492, 2116026, 16}, // BT.601 limited: OpenCV's ITUR_BT_601_* constants
        {1048576, 1470104, -360853, -748826, 1858077, 0},  // BT.601 full
        {1220542, 1880097, -223347, -558891, 2214593, 16}, // BT.709 limited
        {1048576, 1651297, -196423, -490864, 1945738, 0},  // BT.709 full
    };
    return table[color >= 0 && color < kFrameColors ? color : 0];
}

// What frame_convert_kernel reads for frame i.  A work item is 4 neighbouring pixels of one row, or of two rows (2r, 2r + 1)
// in the 4:2:0 formats, so that a chroma pair is read once; item q of a frame is quad q % quads of item row q / quads.  The
// frame's items fill whole workgroups of kFrameGroup, group0 is its first one: group0 ascends strictly over a batch.
struct FrameDesc {
    const uint8_t *plane[3];
    long long stride[3];
    uint8_t *out;
    long long out_stride;
    int32_t width, height, format;
    int32_t quads;     // ceil(width / 4)
    int32_t item_rows; // ceil(height / 2) in the 4:2:0 formats, else height
    int32_t group0;
    FrameCoef coef;
};

struct FramePlan {
    int32_t groups;     // workgroups of the one launch
    int64_t items;      // work items, before the rounding to whole workgroups
    size_t src_bytes;   // every needed plane with tight rows, each plane's start rounded up to 16 bytes: the upload staging
    size_t out_bytes;   // every output frame with tight rows, back to back: the packed output of the host form
};

inline size_t frame_round16(size_t v) { return (v + 15) & ~(size_t)15; }

// The checks of one call and its plan.  RFD_OK: desc[0 .. n) and *plan are filled, with the planes and outputs as the caller
// gave them (frame_host.hip redirects them to its staging where they are host memory).  Otherwise the status, the frame and the
// cause in msg, and nothing may be enqueued.  n >= 1; max_w / max_h: the context's max_src_w / max_src_h.
inline int frame_plan(const rfd_frame *src, int n, const rfd_image *out, int max_w, int max_h, FrameDesc *desc, FramePlan *plan, char *msg, size_t cap)
{
    auto no = [&](int status, int i, const char *what) { snprintf(msg, cap, "frame %d: %s", i, what); return status; };
    FramePlan p;
    memset(&p, 0, sizeof p);
    int64_t groups = 0;
    for (int i = 0; i < n; ++i) {
        const rfd_frame &f = src[i];
        char what[160];
        for (int k = 0; k < 4; ++k)
            if (f.reserved[k] != 0) return no(RFD_ERR_INVALID_ARG, i, "reserved is not zero");
        if (f.format < 0 || f.format >= kFrameFormats) {
            snprintf(what, sizeof what, "unknown pixel format %d", (int)f.format);
            return no(RFD_ERR_INVALID_ARG, i, what);
        }
        const char *name = frame_format_name(f.format);
        if (frame_is_yuv(f.format) && (f.color < 0 || f.color >= kFrameColors)) {
            snprintf(what, sizeof what, "unknown colour %d of a %s frame", (int)f.color, name);
            return no(RFD_ERR_INVALID_ARG, i, what);
        }
        if (f.width < 1 || f.height < 1) return no(RFD_ERR_INVALID_ARG, i, "non-positive size");
        if (f.width > max_w || f.height > max_h) {
            snprintf(what, sizeof what, "%s %d x %d exceeds max_src %d x %d", name, (int)f.width, (int)f.height, max_w, max_h);
            return no(RFD_ERR_CAPACITY, i, what);
        }
        rfd_frame_layout l;
        if (!frame_layout(f.format, f.width, f.height, &l)) return no(RFD_ERR_INVALID_ARG, i, "a side exceeds 2^28 pixels");
        for (int k = 0; k < l.planes; ++k) {
            if (!f.plane[k]) {
                snprintf(what, sizeof what, "plane %d of a %s frame is null", k, name);
                return no(RFD_ERR_INVALID_ARG, i, what);
            }
            if (f.stride[k] < (ptrdiff_t)l.row_bytes[k]) {
                snprintf(what, sizeof what, "stride %lld of plane %d is below the %d bytes of a %s row", (long long)f.stride[k], k, (int)l.row_bytes[k], name);
                return no(RFD_ERR_INVALID_ARG, i, what);
            }
        }
        if (!out[i].data) return no(RFD_ERR_INVALID_ARG, i, "the output frame's data is null");
        if (out[i].width != f.width || out[i].height != f.height) {
            snprintf(what, sizeof what, "the output frame is %d x %d, the %s frame %d x %d", out[i].width, out[i].height, name, (int)f.width, (int)f.height);
            return no(RFD_ERR_INVALID_ARG, i, what);
        }
        if (out[i].stride < (ptrdiff_t)f.width * 3) return no(RFD_ERR_INVALID_ARG, i, "the output frame's stride < 3 * width");
        FrameDesc &d = desc[i];
        memset(&d, 0, sizeof d);
        for (int k = 0; k < l.planes; ++k) {
            d.plane[k] = f.plane[k];
            d.stride[k] = (long long)f.stride[k];
            p.src_bytes = frame_round16(p.src_bytes) + (size_t)l.row_bytes[k] * (size_t)l.rows[k];
        }
        d.out = const_cast<uint8_t *>(out[i].data);
        d.out_stride = (long long)out[i].stride;
        d.width = f.width; d.height = f.height; d.format = f.format;
        d.quads = (f.width + 3) / 4;
        d.item_rows = frame_is_420(f.format) ? (f.height + 1) / 2 : f.height;
        d.coef = frame_coef(frame_is_yuv(f.format) ? f.color : 0);
        const int64_t items = (int64_t)d.quads * d.item_rows;
        if (items > (int64_t)INT32_MAX - kFrameGroup) { // the kernel numbers a frame's items, its last workgroup's tail included, in int
            snprintf(what, sizeof what, "%s %d x %d has more than 2^31 work items", name, (int)f.width, (int)f.height);
            return no(RFD_ERR_CAPACITY, i, what);
        }
        if (groups > INT32_MAX) return no(RFD_ERR_CAPACITY, i, "the batch exceeds 2^31 workgroups");
        d.group0 = (int32_t)groups;
        groups += (items + kFrameGroup - 1) / kFrameGroup;
        p.items += items;
        p.out_bytes += (size_t)f.width * 3 * (size_t)f.height;
    }
    if (groups > INT32_MAX) return no(RFD_ERR_CAPACITY, n - 1, "the batch exceeds 2^31 workgroups");
    p.groups = (int32_t)groups;
    *plan = p;
    return RFD_OK;
}

} // namespace rfd
