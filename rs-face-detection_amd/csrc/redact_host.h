// redact_host.h -- what the redaction (include/rfd.h, "redaction") keeps in a context, and what its kernel is told.
// redact_host.hip holds both rfd_redact_faces* entries; the kernel is kernels_redact.hip; the geometry and the argument checks
// are redact_plan.h.
#pragma once
#include "ctx_access.h" // what the entries need of their context: ctx_stream, ctx_device, ctx_redact
#include "host_resources.h"
#include "redact_plan.h"

namespace rfd {

// Where the kernel reads and writes frame i.  In place: dst = src, dstride = sstride.
struct RdImage {
    const uint8_t *src;
    long long sstride;
    uint8_t *dst;
    long long dstride;
    int h, w;
};

struct RdParams {
    // the call
    const RdImage *imgs; // device, [n]
    int n, max_det;
    const float *boxes;  // [n][max_det][5]
    const int *count;    // [n]
    const uint32_t *sel; // [n][max_det] or null
    int in_place;
    // the config
    int mode, shape, cell, tile; // tile = rd_tile_side(cell)
    uint32_t sel_mask, sel_value;
    uint32_t fill; // B | G << 8 | R << 16
    float margin_x, margin_top, margin_bottom;
    // the output
    int32_t *applied; // [n] or null
};

// grid.x x n workgroups of 256 threads (rd_grid); workgroup (t, b) owns tile t of frame b
int launch_redact(const RdParams &p, RdGrid grid, hipStream_t s);

// The part of a context that belongs to the redaction, all allocated by the first call that needs it.
struct Redact {
    static constexpr int kRing = 4;
    PinnedRing<kRing> ring; // RdImage [max_batch_size]
    DevBuf imgs;
    // host form: the packed frames and the device twins of the caller's arrays
    DevBuf h_frames, h_boxes, h_count, h_sel, h_applied;
};

} // namespace rfd
