// shot_quality_host.h -- what the shot quality (include/rfd.h, "shot quality") keeps in a context, and what its kernel is told.
// shot_quality_host.hip holds both rfd_shot_quality* entries; the kernel is kernels_shot_quality.hip; the geometry and the
// argument checks are shot_quality_plan.h.
#pragma once
#include "ctx_access.h" // what the entries need of their context: ctx_stream, ctx_device, ctx_shot_quality
#include "host_resources.h"
#include "shot_quality_plan.h"

namespace rfd {

// Where the kernel reads frame i.
struct SqImage {
    const uint8_t *src;
    long long stride;
    int h, w;
};

struct SqParams {
    // the call
    const SqImage *imgs; // device, [n]
    int n, max_det;
    const float *boxes; // [n][max_det][5]
    const float *lmk;   // [n][max_det][10]
    const int *count;   // [n]
    // the config
    int lo16, hi16; // 16 * dark, 16 * bright
    float pitch0, w_yaw, w_roll, w_pitch, sharp_ref, size_ref;
    int times_score;
    // the outputs
    float *quality;  // [n][max_det]
    float *parts;    // [n][max_det][8] or null
    int32_t *status; // [n][max_det] or null
};

constexpr int kSqGroupsPerFrame = 8; // workgroups that share the rows of one frame

// kSqGroupsPerFrame x n workgroups of 1024 threads; workgroup (j, b) walks rows j, j + 8, ... of frame b up to its count
int launch_shot_quality(const SqParams &p, hipStream_t s);

// The part of a context that belongs to the shot quality, all allocated by the first call that needs it.
struct ShotQuality {
    static constexpr int kRing = 4;
    PinnedRing<kRing> ring; // SqImage [max_batch_size]
    DevBuf imgs;
    // host form: the packed frames and the device twins of the caller's arrays
    DevBuf h_frames, h_boxes, h_lmk, h_count, h_quality, h_parts, h_status;
};

} // namespace rfd
