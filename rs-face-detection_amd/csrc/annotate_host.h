// annotate_host.h -- what the annotation (include/rfd.h, "annotation") keeps in a context, and what its kernel is told.
// annotate_host.hip holds the rfd_annotate_faces* entries; the kernel is kernels_annotate.hip; the geometry, the text and the
// argument checks are annotate_plan.h.
#pragma once
#include "annotate_plan.h"
#include "redact_host.h" // RdImage: where the kernel reads and writes a frame; ctx_access.h, host_resources.h

namespace rfd {

struct AnParams {
    // the call
    const RdImage *imgs;    // device, [n]
    int n, max_det;
    const float *boxes;     // [n][max_det][5]
    const float *landmarks; // [n][max_det][10], or null when mark_radius == 0
    const int *count;       // [n]
    const uint32_t *sel;    // [n][max_det] or null
    const int32_t *label;   // [n][max_det], or null when label_source is NONE
    const float *value;     // [n][max_det], or null when value_source is not ARRAY
    int in_place;
    // the config
    int n_styles;
    uint32_t mask[RFD_ANNOTATE_MAX_STYLES], want[RFD_ANNOTATE_MAX_STYLES];
    uint32_t colour[RFD_ANNOTATE_MAX_STYLES]; // B | G << 8 | R << 16
    uint32_t text_colour;
    int thickness, mark_radius, label_source, value_source, text_scale, alpha;
    float margin_x, margin_top, margin_bottom;
    // the output
    int32_t *applied; // [n] or null
};

// grid.x x n workgroups of 256 threads (an_grid); workgroup (t, b) owns tile t of frame b
int launch_annotate(const AnParams &p, RdGrid grid, hipStream_t s);

// The part of a context that belongs to the annotation, all allocated by the first call that needs it.
struct Annotate {
    static constexpr int kRing = 4;
    PinnedRing<kRing> ring; // RdImage [max_batch_size]
    DevBuf imgs;
    // host form: the packed frames and the device twins of the caller's arrays
    DevBuf h_frames, h_boxes, h_landmarks, h_count, h_sel, h_label, h_value, h_applied;
};

} // namespace rfd
