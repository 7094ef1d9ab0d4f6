// frame_host.h -- what the frame conversion (include/rfd.h, "frames in camera and decoder formats") keeps in a context, and what
// its kernel is told.  frame_host.hip holds the three rfd_*_frames* entries; the kernel is kernels_frame.hip; layouts, checks,
// descriptors and the work decomposition are frame_plan.h.
#pragma once
#include "ctx_access.h" // what the entries need of their context: ctx_stream, ctx_device, ctx_frame_convert
#include "frame_plan.h"
#include "host_resources.h"

namespace rfd {

struct FrameParams {
    const FrameDesc *frames; // device, [n], group0 ascending
    int n;
    int groups;
};

// `groups` workgroups of kFrameGroup threads: one launch per batch, whatever the number, sizes and formats of its frames
int launch_frame_convert(const FrameParams &p, hipStream_t s);

// The part of a context that belongs to the frame conversion, all allocated by the first call that needs it.
struct FrameConvert {
    static constexpr int kRing = 4;
    PinnedRing<kRing> ring; // FrameDesc [max_batch_size]
    DevBuf desc;
    // Upload and host forms: the planes of a call with tight rows (FramePlan::src_bytes), and the host form's packed output.
    // Both grow on demand like the detector's frame staging and are reused by the next call in stream order: its copies into
    // them follow this call's kernel, so two asynchronous calls back to back are safe.
    DevBuf staging, packed;
};

} // namespace rfd
