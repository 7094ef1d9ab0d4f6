// ctx_access.h -- what a layer next to detector.hip may ask of its context.  rfd_ctx stays private to detector.hip, which
// defines all of these; the layers (gallery, tracker, shot quality, frame conversion, face stage, JPEG encode, redaction, annotation) see it through them alone.
#pragma once
#include "host_resources.h"

namespace rfd {

struct PreImage;
struct ShotQuality;
struct FrameConvert;
struct FaceStage;
struct JpegEncoder;
struct Redact;
struct Annotate;

// The stream a layer's commands go on (the caller's after rfd_set_stream, so it is asked for at every call), and the device.
hipStream_t ctx_stream(const rfd_ctx *c);
int ctx_device(const rfd_ctx *c);
int ctx_max_batch_size(const rfd_ctx *c);
int ctx_max_det(const rfd_ctx *c);

// The part of the context that belongs to a layer.
ShotQuality &ctx_shot_quality(rfd_ctx *c);
FrameConvert &ctx_frame_convert(rfd_ctx *c);
FaceStage &ctx_face_stage(rfd_ctx *c);
JpegEncoder &ctx_jpeg_encoder(rfd_ctx *c);
Redact &ctx_redact(rfd_ctx *c);
Annotate &ctx_annotate(rfd_ctx *c);

// n images fit the context; the error names them as "<what> n<unit>".  ctx_check_images: n valid 3-channel frames that fit.
int ctx_check_batch(const rfd_ctx *c, int n, const char *what, const char *unit = "");
int ctx_check_images(const rfd_ctx *c, const rfd_image *imgs, int n);

// Where the kernels read frame i, into the two leading members { const uint8_t *src; long long stride; } of descriptor i
// (PreImage, LiveImage), the descriptors `pitch` bytes apart.  Device frames are read where they lie; host frames are packed
// into the context's frame staging on its stream, one 2-D copy each, and stay there until the next call that stages frames.
int ctx_place_frames(rfd_ctx *c, const rfd_image *imgs, int n, bool frames_on_device, void *desc, size_t pitch);
// The frames (host or device resident) and their letterbox geometry to the device: *staged is the device array of their n
// descriptors, good until the next call that stages frames.
int ctx_stage_frames(rfd_ctx *c, const rfd_image *imgs, int n, bool frames_on_device, const PreImage **staged);
// n descriptors that hold the sizes alone (no pixels, no geometry), staged likewise: for a launch that reads no pixel.
int ctx_stage_frame_sizes(rfd_ctx *c, const int32_t *img_w, const int32_t *img_h, int n, const PreImage **staged);

// The context's own detection slabs; detection slabs of n images between host and device, on the context's stream (`total`
// travels if dst has one); the detection of n frames into the own slabs, enqueued only, *staged as ctx_stage_frames gives it.
rfd_dets ctx_own_slabs(const rfd_ctx *c);
int ctx_copy_slabs(rfd_ctx *c, const rfd_dets &dst, const rfd_dets &src, int n, hipMemcpyKind kind);
int ctx_detect_own_slabs(rfd_ctx *c, const rfd_image *imgs, int n, bool frames_on_device, rfd_dets *dev, const PreImage **staged);

// Call after the host has synchronised with the stream: a device-side bounded wait that gave up since the last such call is
// the call's error.
int ctx_check_nms_flag(rfd_ctx *c);

} // namespace rfd
