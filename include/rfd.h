/*
 * rfd.h -- C ABI of librfd_hip.so: the MI355X-native (gfx950) replacement of the detection stage of
 * okieraised/rs-face-detection, i.e. of
 *     RetinaFaceDetection::call(&self, image:&Mat, is_debug) -> (Array2<f32>[K,5], Array3<f32>[K,5,2])
 *     (reference src/pipeline/module/face_detection.rs:496), invoked from
 *     FacePipeline::extract (src/pipeline/face_pipeline/pipeline.rs:198).
 *
 * The reference ships a 640x640 f32 tensor to a Triton server (face_detection.rs:279) and decodes
 * the 9 returned head tensors on the CPU.  Here preprocess, the RetinaFace network, decode, sort,
 * NMS and rescale all run on the GPU as HIP kernels; this header is what a Rust `extern "C"` block
 *  binds.  The only native ABI the reference itself declares is `_nms`
 * (src/rcnn/gpu_nms.hpp:7); a compatible symbol is exported too.
 *
 * Conventions (mirroring `_nms`): the caller allocates every input and output buffer; the context
 * owns device weights, workspaces, streams.  Every function returns 0 on success or a negative
 * rfd_status; rfd_last_error() returns a message for the last failure on the calling thread.
 * There is NO CPU fallback: without a usable HIP device rfd_create fails with RFD_ERR_NO_DEVICE.
 * A context is not re-entrant (one stream + workspace); use one context per thread.
 */
#ifndef RFD_H
#define RFD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RFD_VERSION 1

#if defined(__GNUC__)
#define RFD_API __attribute__((visibility("default")))
#else
#define RFD_API
#endif

typedef enum rfd_status {
    RFD_OK = 0,
    RFD_ERR_INVALID_ARG = -1, /* null pointer, bad shape, channels != 3 (reference: OpenCV error / at_2d failure, face_detection.rs:137,226) */
    RFD_ERR_NO_DEVICE = -2,   /* no HIP device / HIP runtime failure at creation */
    RFD_ERR_HIP = -3,         /* a HIP call or kernel failed, or a device-side bounded wait gave up (chunked NMS, ring convolution): the
                               * detections since the last synchronisation are invalid (reference: Triton RPC failure, face_detection.rs:282) */
    RFD_ERR_CAPACITY = -4,    /* batch / frame / detections exceed the configured capacity */
    RFD_ERR_STATE = -5,       /* weights not initialised (reference: empty model config, face_detection.rs:239) */
    RFD_ERR_IO = -6,          /* weight file could not be read / written */
    RFD_ERR_COMM = -7,        /* librccl missing, or an RCCL call failed (multi-GPU gather) */
    RFD_ERR_UNSUPPORTED = -8  /* a well-formed JPEG file of a kind the decoder does not do (progressive, 12-bit, ...): "JPEG decode" below */
} rfd_status;

typedef enum rfd_backbone {
    RFD_BACKBONE_R50 = 0,     /* RetinaFace ResNet-50 + FPN + SSH */
    RFD_BACKBONE_MNET025 = 1  /* RetinaFace MobileNet-0.25 (same head/anchor contract) */
} rfd_backbone;

/*
 * Mirrors FaceDetectionConfig (src/pipeline/face_pipeline/config.rs:13-33) and the arguments of
 * RetinaFaceDetection::new (face_detection.rs:41-49): image_size is (w,h); the Triton client /
 * model-config / model-name arguments are gone (the network runs in-process); device, batch
 * capacity and output capacity are new.
 */
typedef enum rfd_precision { RFD_PRECISION_BF16 = 0, RFD_PRECISION_F32 = 1 } rfd_precision;
typedef enum rfd_schedule { RFD_SCHEDULE_THROUGHPUT = 0, RFD_SCHEDULE_LATENCY = 1 } rfd_schedule;
/* Largest pass (images) a latency context runs with the split-K kernels. */
#define RFD_LATENCY_MAX_BATCH 2

typedef struct rfd_config {
    int image_w;                /* config.rs:26 image_size.0, default 640 */
    int image_h;                /* config.rs:26 image_size.1, default 640 */
    int max_batch_size;         /* config.rs:28 (reference: 1); frames per rfd_detect_batch call */
    float confidence_threshold; /* config.rs:29, default 0.7; keep rows with score >= threshold */
    float iou_threshold;        /* config.rs:30, default 0.45; suppress on IoU > threshold */
    int device_id;              /* HIP device ordinal */
    int max_det;                /* capacity (rows per image) of the output slabs; default 1024 */
    int max_src_w;              /* largest source frame the context must stage; default 3840 */
    int max_src_h;              /* default 2160 */
    int backbone;               /* rfd_backbone */
    int precision;              /* rfd_precision: 0 = bf16 activations / weights with f32 accumulation (the product path,
                                 * BASELINE.json configs[2]); 1 = the f32 parity mode (RetinaFace-R50 only): f32 weights
                                 * and activations, convolutions accumulated in f64 and rounded once per output -- the reference's
                                 * FP32 tensor contract (face_detection.rs:261), reproducible to the bit by any evaluation that
                                 * sums the same products exactly.  A correctness mode: plain FMA kernels, one stream, ~60x slower
                                 * than the bf16 path. */
    int schedule;               /* rfd_schedule: 0 = the throughput schedule (every context before this field existed); 1 = the
                                 * latency schedule (bf16 path only): a pass of n <= RFD_LATENCY_MAX_BATCH images runs the
                                 * long-K, few-tile convolutions as K segments over several workgroups (split-K); a larger pass
                                 * runs exactly the throughput kernels.  Contract: results are deterministic; a frame's nine head
                                 * tensors are bit-identical for every n <= RFD_LATENCY_MAX_BATCH and every position in the
                                 * batch; they are NOT promised to equal the throughput schedule's bits (a segmented f32 sum
                                 * rounds differently) -- both schedules meet the same per-op bound against the exact f64
                                 * result (tests/test_conv_exact_gpu.py, tests/test_latency_gpu.py). */
    int reserved[4];
} rfd_config;

/* A decoded source frame: HxWx3 u8, BGR, row stride in bytes (an OpenCV Mat CV_8UC3,
 * as produced by byte_data_to_opencv, src/utils/utils.rs:8-52). */
typedef struct rfd_image {
    const uint8_t *data;
    int height;
    int width;
    ptrdiff_t stride;
} rfd_image;

/*
 * Caller-allocated outputs for n frames.  Row layout equals the reference's return value
 * (face_detection.rs:432-464, 473-493): boxes row = x1,y1,x2,y2,score in SOURCE-image pixels,
 * rows in descending score (kept order); landmarks row = 5 x (x,y).
 *   boxes     [n][max_det][5]  f32
 *   landmarks [n][max_det][10] f32
 *   count     [n] i32 = min(K, max_det)
 *   total     [n] i32 = K, the untruncated number of detections (may be NULL)
 */
typedef struct rfd_dets {
    float *boxes;
    float *landmarks;
    int32_t *count;
    int32_t *total;
} rfd_dets;

/* Per-call stage timings measured with HIP events on the context's stream (milliseconds). */
typedef struct rfd_stats {
    float ms_h2d;
    float ms_preprocess;
    float ms_network;
    float ms_decode;
    float ms_sort;
    float ms_nms;
    float ms_d2h;
    float ms_total;
    int64_t candidates; /* rows with score >= threshold, summed over the batch */
    int64_t detections; /* kept rows, summed over the batch (host-output entry points only: the device-resident ones leave the counts in HBM and do not read them back) */
    int64_t reserved[4];
} rfd_stats;

typedef struct rfd_ctx rfd_ctx;

/* ---- lifecycle (replaces RetinaFaceDetection::new, face_detection.rs:41-129, and the Triton
 *      channel set-up of FacePipeline::new, pipeline.rs:64-128) ---- */
RFD_API void rfd_config_default(rfd_config *cfg);
RFD_API int rfd_create(const rfd_config *cfg, rfd_ctx **out);
RFD_API void rfd_destroy(rfd_ctx *ctx);
RFD_API const char *rfd_last_error(void);
RFD_API int rfd_version(void);

/* ---- network graph description (host only: works without a GPU).  The reference never sees the
 *      graph (it only knows the Triton model name, config.rs:25); these calls expose the
 *      build-defined graph so that tests can rebuild it layer by layer. ---- */
typedef struct rfd_graph rfd_graph;
typedef struct rfd_layer_desc {
    char name[64];
    int cin, cout, kh, kw, stride, pad;
    int has_affine; /* per-channel scale/shift + ReLU applied after the residual add (or the pool) */
    int kind;       /* 0 conv, 1 depthwise 3x3 (cin = 1, cout = channels; weights [C][3][3][1]), 2 first 3x3/2, 3 conv0 7x7/2 */
    int reserved[3];
} rfd_layer_desc;
typedef struct rfd_op_desc {
    int kind;  /* 0: conv0 7x7/2 + bias + ReLU, 1: maxpool 3x3/2 (+ affine + ReLU), 2: conv,
                  3: fused stem = kind 0 then kind 1 (conv0 result rounded to bf16 in between),
                  4: depthwise 3x3 + bias + ReLU, 5: first 3x3/2 conv (3 input channels) + bias + ReLU,
                  6: back-to-back pair: kind 2 (out = raw sum) followed by out_b = relu(conv(relu(affine(out)), layer_b)) */
    int layer; /* weights used (kind 1: the layer whose affine is applied) */
    int in, out, out2, outf, res; /* tensor ids, -1 = none: out = bf16 result, out2 = relu(affine(v)),
                                     outf = f32 result (heads), res = residual input */
    int relu, res_up2, res_post, head_softmax, y_coff;
    double macs; /* multiply-accumulates per image */
    int in2, layer2; /* fused 1x1 shortcut conv: + conv(tensor in2, layer2) (+ its bias); -1 = none */
    int in_affine;   /* >= 0: the input is first mapped through relu(x*scale+shift) of that layer's affine */
    int layer_n2;    /* >= 0: a sibling conv on the same input fused along N; its output channels follow */
    int x_coff;      /* the input is the channel slice [x_coff, x_coff + cin) of tensor `in` */
    int y_split, y_split_add; /* output channel n goes to y_coff + n (+ y_split_add if n >= y_split) */
    int n_valid;     /* only output channels < n_valid are stored */
    int branch;      /* 0 main chain; 1, 2: independent side chains that run on their own HIP streams */
    int layer_b, out_b; /* kind 6: the next unit's conv1 applied to relu(affine(out)), and its output tensor */
} rfd_op_desc;
typedef struct rfd_tensor_desc {
    int channels, height, width; /* channels = device channels: channels_logical zero-padded (to 64) */
    int is_f32, buffer, is_input, head_level; /* head_level: 1,2,3 = stride 32,16,8 head tensor */
    int channels_logical;
    int reserved[3];
} rfd_tensor_desc;
RFD_API int rfd_graph_create(int backbone, int image_w, int image_h, rfd_graph **out);
RFD_API void rfd_graph_destroy(rfd_graph *g);
RFD_API int rfd_graph_counts(const rfd_graph *g, int *layers, int *ops, int *tensors, int *buffers);
RFD_API int rfd_graph_layer(const rfd_graph *g, int idx, rfd_layer_desc *d);
RFD_API int rfd_graph_op(const rfd_graph *g, int idx, rfd_op_desc *d);
RFD_API int rfd_graph_tensor(const rfd_graph *g, int idx, rfd_tensor_desc *d);
RFD_API double rfd_graph_macs(const rfd_graph *g);            /* conv MACs per image */
RFD_API double rfd_graph_workspace_bytes(const rfd_graph *g); /* planned activation bytes per image */

/* ---- weights (replace Triton's model repository for "face_detection_retina", config.rs:25) ---- */
RFD_API int rfd_init_synthetic_weights(rfd_ctx *ctx, uint64_t seed);
RFD_API int rfd_num_layers(const rfd_ctx *ctx);
/* weights [cout][kh][kw][cin] f32 (values as stored on device, i.e. bf16-rounded), bias [cout];
 * BatchNorm is expected to be folded into weights/bias by the caller. */
RFD_API int rfd_get_layer_weights(rfd_ctx *ctx, int idx, float *weights, float *bias);
RFD_API int rfd_set_layer_weights(rfd_ctx *ctx, int idx, const float *weights, const float *bias);
/* Weight file (replaces Triton's model repository entry for the detector): little-endian; header "RFDW", u32
 * version = 1, u32 backbone, u32 n_layers; per layer: char name[64], i32 cin, cout, kh, kw, stride, pad, kind,
 * has_affine, then f32 weights [cout][kh][kw][cin], f32 bias [cout], and if has_affine f32 scale [cout], shift
 * [cout].  BatchNorm must be folded by the exporter.  rfd_load_weights checks every shape against the graph. */
RFD_API int rfd_save_weights(rfd_ctx *ctx, const char *path);
RFD_API int rfd_load_weights(rfd_ctx *ctx, const char *path);
/* the post-add affine (scale, shift per output channel) of layers with has_affine */
RFD_API int rfd_get_layer_affine(rfd_ctx *ctx, int idx, float *scale, float *shift);
RFD_API int rfd_set_layer_affine(rfd_ctx *ctx, int idx, const float *scale, const float *shift);

/* ---- the hot path: replaces RetinaFaceDetection::call (face_detection.rs:496-513) for a batch
 *      of frames.  Host buffers in, host buffers out; synchronous. ---- */
RFD_API int rfd_detect_batch(rfd_ctx *ctx, const rfd_image *imgs, int n, rfd_dets *out);

/* Same, with every `data` pointer of imgs[] and every pointer of `out` in DEVICE memory (frames
 * already resident in HBM, detections left in HBM for a following RCCL gather).  The imgs[] array
 * itself is host memory.  Enqueued on the context's stream; returns after the stream has drained
 * unless `async` is non-zero (then call rfd_sync before reading results / reusing buffers).
 * async = 1: the whole call is ordered on the context's stream (frames may be produced by earlier work on it).
 * async = 2: cross-call overlap -- the frames must be COMPLETE when the call is made (not still being written by
 *            enqueued work); the network chains then start without waiting for the previous call's decode / NMS, which
 *            stay on the context's stream together with this call's, so results, rfd_sync and a following collective
 *            on that stream behave as with async = 1.  Falls back to async = 1 for batches that are not split. */
RFD_API int rfd_detect_batch_device(rfd_ctx *ctx, const rfd_image *imgs, int n, rfd_dets *out, int async);
RFD_API int rfd_sync(rfd_ctx *ctx);
/* Enqueue on a caller-owned hipStream_t instead of the context's own stream (NULL restores it), so
 * that a following collective (RCCL gather of the detection slabs) is stream-ordered behind the
 * detector without a host synchronisation. */
RFD_API int rfd_set_stream(rfd_ctx *ctx, void *hip_stream);

/* ---- multi-GPU (the reference is single-device, one image per call: face_detection.rs:220).
 *      Frames shard image-parallel, one process (or thread) and one context per GPU, weights replicated; the only
 *      exchange step is the gather of the per-rank detection slabs, an RCCL all-gather over xGMI enqueued on the
 *      context's stream, i.e. stream-ordered behind the rank's NMS with no host synchronisation.
 *        rank 0:      rfd_comm_get_unique_id(id)          -> send the RFD_COMM_ID_BYTES bytes to every rank out of band
 *        every rank:  rfd_comm_init(ctx, id, rank, world) (collective: returns when all ranks have joined)
 *        per batch:   rfd_detect_batch_device(ctx, ..., &local, async) ; rfd_gather_detections(ctx, &local, n_local, &all)
 *      `local` and `all` are DEVICE slabs; every rank passes the same n_local (a short tail rank pads with count = 0) and
 *      `all` holds world * n_local frames, rank-major = the original frame order of a contiguous split:
 *      boxes [world*n_local][max_det][5], landmarks [..][max_det][10], count [..], total [..] (total may be NULL in both).
 *      librccl is loaded on first use (dlopen; RFD_RCCL_LIB overrides the name): single-GPU users never need it. ---- */
#define RFD_COMM_ID_BYTES 128 /* = NCCL_UNIQUE_ID_BYTES */
RFD_API int rfd_comm_get_unique_id(void *id /* RFD_COMM_ID_BYTES bytes, host */);
RFD_API int rfd_comm_init(rfd_ctx *ctx, const void *unique_id, int rank, int world);
RFD_API int rfd_comm_info(const rfd_ctx *ctx, int *rank, int *world); /* world = 0: no communicator */
RFD_API int rfd_gather_detections(rfd_ctx *ctx, const rfd_dets *local, int n_local, rfd_dets *all);
RFD_API int rfd_comm_destroy(rfd_ctx *ctx);

/* ---- stage-level entry points (parity tests; each mirrors one reference stage) ---- */

/* _preprocess + tensorise (face_detection.rs:131-198, 220-232) for n frames.
 * det_img [n][image_h][image_w][3] u8 (may be NULL), tensor [n][3][image_h][image_w] f32 R,G,B
 * planes raw 0..255 (may be NULL), det_scale [n] f32.  Host pointers. */
RFD_API int rfd_preprocess(rfd_ctx *ctx, const rfd_image *imgs, int n, uint8_t *det_img, float *tensor,
                   float *det_scale);

/* The network: tensor [n][3][image_h][image_w] f32 (the reference's Triton input contract,
 * face_detection.rs:220-277) -> 9 head tensors, f32, NCHW, in the reference's slot order
 * 32,16,8 x (cls [n,4,h,w], bbox [n,8,h,w], lmk [n,20,h,w]) (face_detection.rs:286-312, 319-407).
 * Host pointers. */
RFD_API int rfd_forward(rfd_ctx *ctx, const float *tensor, int n, float *const heads[9]);

/* Everything after the network (face_detection.rs:319-493) on caller-supplied head tensors
 * (same contract as rfd_forward's outputs), det_scale [n].  Host pointers.
 * gidx (may be NULL) [n][max_det] i32 receives the global anchor index of every kept row. */
RFD_API int rfd_decode_nms(rfd_ctx *ctx, const float *const heads[9], int n, const float *det_scale,
                   rfd_dets *out, int32_t *gidx);

/* Greedy NMS on boxes pre-sorted by score descending: the contract of the reference's (never
 * built) CUDA entry point `_nms` (src/rcnn/nms_kernel.cu:91-144, src/rcnn/gpu_nms.hpp:7) with the
 * live path's survivor rule (src/processing/nms.rs:58).  boxes: host [boxes_num][boxes_dim>=4]
 * f32; keep: capacity boxes_num.  Returns a status (the reference returns void and prints). */
RFD_API int rfd_nms_sorted(rfd_ctx *ctx, int32_t *keep, int *num_out, const float *boxes, int boxes_num,
                   int boxes_dim, float thresh);

/* Drop-in for the reference's declaration (gpu_nms.hpp:7): uses a process-wide context on
 * device_id, prints nothing, leaves *num_out = -1 on failure. */
RFD_API void _nms(int32_t *keep, int *num_out, float *boxes, int boxes_num, int boxes_dim, float thresh,
          int device_id);

/* ---- next stage: FaceSelection::call, face_selection.rs:72-189, as a device epilogue.
 *      Defaults = FaceSelectionConfig::new (config.rs:107-117).  found[i]: 0 = no face selected (reference:
 *      (None, None)), 1 = box only, 3 = box + key points.  Only the rows the detector returned (count <=
 *      max_det) take part. ---- */
typedef struct rfd_selection_config {
    float margin_center_left_ratio;  /* 0.3 */
    float margin_center_right_ratio; /* 0.3 */
    float margin_edge_ratio;         /* 0.1 */
    float minimum_face_ratio;        /* 0.0075 */
} rfd_selection_config;
RFD_API void rfd_selection_config_default(rfd_selection_config *cfg);
/* Stage-level: selection on host detections as returned by rfd_detect_batch (dets->boxes/landmarks/count),
 * img_h/img_w [n] = source frame sizes; out_box [n][5], out_kps [n][10], found [n].  Host pointers. */
RFD_API int rfd_select_faces(rfd_ctx *ctx, const rfd_dets *dets, const int *img_h, const int *img_w, int n,
                             const rfd_selection_config *cfg, int is_enroll, float *out_box, float *out_kps,
                             int32_t *found);
/* Fused: detect n frames (host buffers) and return only the selected face of each: detections stay in HBM,
 * 16 floats per frame cross PCIe.  = FacePipeline::extract lines 198-208 (pipeline.rs). */
RFD_API int rfd_detect_select_batch(rfd_ctx *ctx, const rfd_image *imgs, int n, const rfd_selection_config *cfg,
                                    int is_enroll, float *out_box, float *out_kps, int32_t *found);

/* ---- pipelined host entry (host decode + H2D staging, utils.rs:8-52 is the producer) ----
 *      rfd_detect_batch is synchronous, so the PCIe copy of a batch cannot overlap the compute of the previous one.
 *      rfd_submit_batch enqueues H2D (own copy stream) + the whole hot path + D2H of the detections and returns;
 *      rfd_collect_batch waits for the OLDEST submitted batch and fills `out` exactly as rfd_detect_batch would.
 *      Up to 2 batches may be in flight (a third submit returns RFD_ERR_STATE).  The frames must stay valid and
 *      unchanged until their batch has been collected.  For the copy to be a true asynchronous DMA the frames should
 *      live in page-locked memory: rfd_host_alloc / rfd_host_free hand it out (decode straight into it); pageable
 *      frames work but are copied synchronously by the runtime.  Not to be mixed with the other detect calls while a
 *      batch is in flight. ---- */
RFD_API int rfd_host_alloc(size_t bytes, void **ptr);
RFD_API int rfd_host_free(void *ptr);
RFD_API int rfd_submit_batch(rfd_ctx *ctx, const rfd_image *imgs, int n);
RFD_API int rfd_collect_batch(rfd_ctx *ctx, rfd_dets *out, int *n_out);

/* ---- FaceAlignment: FaceAlignment::call, src/pipeline/module/face_alignment.rs:27-141 --
 *      the step after selection in FacePipeline::extract (pipeline.rs:210-216).  For each frame the selected face is
 *      mapped onto the out_w x out_h template: 4-DOF similarity from its five key points to `standard_landmarks`
 *      as estimate_affine_partial_2d(LMEDS, 3.0, 2000, 0.99, 10) :48-60 computes it -- OpenCV's LMedS restated: 13
 *      two-point samples of the re-seeded cv::RNG, least median, inlier rule, least squares over the inliers (the
 *      fixed point of its Levenberg-Marquardt refinement; parity against a running OpenCV unpinned)
 *      + cv::warpAffine(INTER_LINEAR, BORDER_CONSTANT 0) :112-120 restated in integer
 *      arithmetic; degenerate key points take the reference's crop + resize branch :62-110.
 *      Defaults = FaceAlignmentConfig::new (config.rs:44-56): 112 x 112 and the ArcFace template.
 *      status[i]: 0 aligned, 1 crop + resize fallback, -1 no key points (the reference's call returns Err),
 *      -2 no face selected, -3 fallback ROI outside the frame (the reference's Mat::roi returns Err); crops with a
 *      negative status are zero-filled.  out_crops: [n][out_h][out_w][3] u8 BGR, host. ---- */
typedef struct rfd_alignment_config {
    int32_t out_w, out_h;            /* 112, 112 */
    float standard_landmarks[10];    /* x0,y0 ... x4,y4 */
    int32_t reserved[4];
} rfd_alignment_config;
RFD_API void rfd_alignment_config_default(rfd_alignment_config *cfg);
/* Stage-level: frames (host), selected boxes [n][5], key points [n][10] and flags found [n] as returned by
 * rfd_select_faces / rfd_detect_select_batch. */
RFD_API int rfd_align_faces(rfd_ctx *ctx, const rfd_image *imgs, int n, const float *boxes, const float *kps,
                            const int32_t *found, const rfd_alignment_config *cfg, uint8_t *out_crops,
                            int32_t *status);
/* Fused: detect + select + align n frames; the frames cross PCIe once, detections never leave HBM, 16 floats and one
 * crop per frame come back.  = FacePipeline::extract lines 198-216 (pipeline.rs). */
RFD_API int rfd_detect_select_align_batch(rfd_ctx *ctx, const rfd_image *imgs, int n,
                                          const rfd_selection_config *sel_cfg, int is_enroll,
                                          const rfd_alignment_config *align_cfg, float *out_box, float *out_kps,
                                          int32_t *found, uint8_t *out_crops, int32_t *status);

/* ---- the model inputs of the two stages after alignment, and what follows their models: FaceQuality::call
 *      (src/pipeline/module/face_quality.rs:40-186) and FaceExtraction::call (face_extraction.rs:30-150) -- the rest of
 *      FacePipeline::extract (pipeline.rs:218-249).  The two models themselves are remote and not part of this library.
 *      Before each model the reference runs, per face, cv::resize(INTER_LINEAR) to the model's image_size, COLOR_BGR2RGB,
 *      (p - mean) * scale per pixel and the NHWC -> NCHW permute (face_quality.rs:43-44,56-101, face_extraction.rs:38-77);
 *      here one launch does it for every face and every model.  The resize is the same restated cv::resize as the
 *      detector's letterbox (its exact-2x case is the 2x2 mean; equal sizes are a copy).  Byte-exact against the oracle's
 *      restatement; parity against a running OpenCV unpinned, like alignment. ---- */
#define RFD_MAX_FACE_TENSORS 4
typedef struct rfd_face_tensor_config {
    int32_t out_w, out_h;   /* the model's image_size (w, h) */
    float   mean[3];        /* per OUTPUT channel (R, G, B) */
    float   scale[3];       /* value = (float(p) - mean[c]) * scale[c]: two roundings, in this order */
    int32_t reserved[4];
} rfd_face_tensor_config;
RFD_API void rfd_face_tensor_config_quality(rfd_face_tensor_config *cfg);    /* 112x112; mean 123.675, 116.28, 103.53; scale 0.01712475, 0.017507, 0.01742919 (face_quality.rs:43-44) */
RFD_API void rfd_face_tensor_config_extraction(rfd_face_tensor_config *cfg); /* 112x112; mean 127.5 x3; scale 0.0078125 x3 (face_extraction.rs:38-39) */
/* Stage-level: crops [n][crop_h][crop_w][3] u8 BGR -> tensors[j] [n][3][cfgs[j].out_h][cfgs[j].out_w] f32, R,G,B planes,
 * 1 <= k <= RFD_MAX_FACE_TENSORS (more: RFD_ERR_CAPACITY), n <= max_batch_size.  Host pointers. */
RFD_API int rfd_face_tensors(rfd_ctx *ctx, const uint8_t *crops, int n, int crop_w, int crop_h,
                             const rfd_face_tensor_config *cfgs, int k, float *const *tensors);
/* rfd_detect_select_align_batch plus the k model inputs of every aligned face (k may be 0): tensors[j] as above, host.
 * out_crops may be NULL (the u8 crops are then not returned; with configs of the crop's own size they are never stored at
 * all).  A face with a negative alignment status gets all-zero tensors (0.0f in every plane, NOT (0 - mean) * scale), as its
 * crop is zero-filled. */
RFD_API int rfd_detect_select_align_tensors_batch(rfd_ctx *ctx, const rfd_image *imgs, int n,
                                                  const rfd_selection_config *sel_cfg, int is_enroll,
                                                  const rfd_alignment_config *align_cfg, float *out_box, float *out_kps,
                                                  int32_t *found, uint8_t *out_crops, int32_t *status,
                                                  const rfd_face_tensor_config *cfgs, int k, float *const *tensors);
/* Stage-level: rfd_align_faces plus the k model inputs of every face (the same kernels as the fused entry, on caller-supplied
 * selection results).  Host pointers; out_crops may be NULL. */
RFD_API int rfd_align_faces_tensors(rfd_ctx *ctx, const rfd_image *imgs, int n, const float *boxes, const float *kps,
                                    const int32_t *found, const rfd_alignment_config *cfg, uint8_t *out_crops,
                                    int32_t *status, const rfd_face_tensor_config *cfgs, int k, float *const *tensors);
/* The device-resident form (conventions of rfd_detect_batch_device): every imgs[i].data and every pointer of `out` is
 * DEVICE memory -- box [n][5], kps [n][10], found [n], crops [n][out_h][out_w][3] (may be NULL), status [n], tensors[j < k].
 * The whole call -- detection, selection, alignment, tensors -- is enqueued on the context's stream; async = 0 returns after
 * the stream has drained, any other value returns at once with no host synchronisation (call rfd_sync before reading the
 * results or reusing the buffers; the cross-call overlap of rfd_detect_batch_device's async = 2 is not offered here). */
typedef struct rfd_faces {
    float *box;
    float *kps;
    int32_t *found;
    uint8_t *crops; /* may be NULL */
    int32_t *status;
    float *tensors[RFD_MAX_FACE_TENSORS];
} rfd_faces;
RFD_API int rfd_detect_faces_device(rfd_ctx *ctx, const rfd_image *imgs, int n, const rfd_selection_config *sel_cfg,
                                    int is_enroll, const rfd_alignment_config *align_cfg,
                                    const rfd_face_tensor_config *cfgs, int k, rfd_faces *out, int async);
/* The quality decision rule (face_quality.rs:159-168) on the quality model's logits [n][classes]: klass[i] = the index of the
 * row's maximum -- on equal values the LAST such index, as Rust's max_by returns; klass 1 with logits[1] < threshold becomes
 * klass 0 (`<` is strict); score[i] = the logit of the final class.  Host pointers.
 * Divergence: a NaN logit makes the reference panic (partial_cmp(..).unwrap()); here the call returns RFD_ERR_INVALID_ARG for
 * the whole frame set and rfd_last_error() names the first such frame.  The device form cannot report without waiting for the
 * stream: it marks such a row with klass = -1 and score = NaN. */
RFD_API int rfd_quality_decide(rfd_ctx *ctx, const float *logits, int n, int classes, float threshold, float *score,
                               int32_t *klass);
/* normalize_outputs (src/utils/utils.rs:148-154) on the ID model's embeddings [n][dim]: out = emb / sqrt(sum emb^2) per row,
 * f32, deterministic (fixed summation order).  An all-zero row gives NaN, as the reference's division does.  Host pointers. */
RFD_API int rfd_normalize_embeddings(rfd_ctx *ctx, const float *emb, int n, int dim, float *out);
/* Both with DEVICE pointers, enqueued on the context's stream (no synchronisation; out may equal emb). */
RFD_API int rfd_quality_decide_device(rfd_ctx *ctx, const float *logits, int n, int classes, float threshold, float *score,
                                      int32_t *klass);
RFD_API int rfd_normalize_embeddings_device(rfd_ctx *ctx, const float *emb, int n, int dim, float *out);
/* The FaceQualityAssessment preset (src/pipeline/module/face_quality_assessment.rs:50-76): resize to the caller's w x h (the
 * reference reads it from its config), BGR -> RGB, (p - 127.5) * 0.00784313725 (the f32 value of that literal).  The existing
 * face-tensor entry points run it.  Its decision (:150-155) is `logit[0] > threshold ? 1 : 0` on the model's single logit: a
 * comparison the caller writes; it has no entry point here. */
RFD_API void rfd_face_tensor_config_quality_assessment(rfd_face_tensor_config *cfg, int w, int h);

/* ---- liveness: FaceAntiSpoofing::call (src/pipeline/module/face_antispoofing.rs), the other consumer of the selected box.
 *      The k miniFAS models are remote, like the quality and the ID model; this is what the reference runs on the CPU around
 *      them.  Before the models, per face (_get_scale_image :245-295): a crop box 0.94 x the box height wide around the box
 *      centre, then per model j (_get_new_box :342-385) that box scaled by min(scale[j], what the frame allows), shifted back
 *      into the frame, truncated to integer corners; Mat::roi + cv::resize(INTER_LINEAR) to out_w[j] x out_h[j] :323-337;
 *      planes of raw 0..255 floats in the frame's own channel order -- B, G, R for the library's BGR frames, where the
 *      detector's tensor is R, G, B (_preprocess :180-217: its cvt_color and its `2 - i` store cancel).  All f32 arithmetic
 *      is done in the reference's order with one rounding per operation; `as i32` truncates, saturates and maps NaN to 0;
 *      the i32 sums wrap (a release build).  Byte-exact against the oracle's restated cv::resize, parity against a running
 *      OpenCV unpinned, like alignment.  weights[i][j] = used scale / scale[j] (1 unless the frame capped the scale).
 *      After the models (_postprocess :219-243): the weighted mean of column 1 of the k outputs, live iff it exceeds a
 *      threshold.
 *      Divergences, both on purpose: (1) `call` :58-81 inserts one-image lists at index i for every image, so a
 *      call with more than one image does not pair images with weights; the stage is defined PER FACE here, each face equal
 *      to a single-image call, and the batch is not zero-padded to a multiple of batch_size.  (2) `_postprocess` zips the k
 *      outputs with a list of ONE weight, so as written only the first model counts (o0 * w0 / w0); rfd_liveness_decide
 *      computes the weighted mean over all k models that the function's structure and its computed weights are for.  The
 *      reference-as-written result is the k = 1 call on the first model's logits.  The reference compares with the literal
 *      0.55 (its `threshold` field is never read); here the threshold is an argument. ---- */
typedef struct rfd_liveness_config {
    int32_t k;                            /* models, 1 .. RFD_MAX_FACE_TENSORS */
    float   scale[RFD_MAX_FACE_TENSORS];  /* scales[j]: finite, > 0 */
    int32_t out_w[RFD_MAX_FACE_TENSORS];  /* image_sizes[j].0 */
    int32_t out_h[RFD_MAX_FACE_TENSORS];  /* image_sizes[j].1 */
    int32_t reserved[4];
} rfd_liveness_config;
/* The four models the reference names (:448-485): scale 4.0 -> 80x80, 2.7 -> 80x80, 2.0 -> 256x256, 1.0 -> 128x128. */
RFD_API void rfd_liveness_config_default(rfd_liveness_config *cfg);
/* Stage-level, host pointers: frames, boxes [n][5] and found [n] as rfd_select_faces / rfd_detect_select_batch return them
 * (only x1, y1, x2, y2 and bit 0 of found are read), cfg (NULL: the default) -> tensors[j] [n][3][out_h[j]][out_w[j]] f32,
 * weights [n][k], rois [n][k][4] = ltx, lty, rbx, rby of every model's ROI (may be NULL), status [n]: 0 ok, -2 no face (bit 0
 * of found[i] clear), -3 some model's ROI is not inside the frame or is empty (the reference's Mat::roi / cv::resize return
 * Err for the whole face).  A face with a negative status gets all-zero tensors and weights 0; its rois hold what was
 * computed (-3) or 0 (-2).  n <= max_batch_size; k > RFD_MAX_FACE_TENSORS: RFD_ERR_CAPACITY; a non-positive size or a scale
 * that is not finite and positive: RFD_ERR_INVALID_ARG.  The staging memory of this stage is allocated by its first call. */
RFD_API int rfd_liveness_tensors(rfd_ctx *ctx, const rfd_image *imgs, int n, const float *boxes, const int32_t *found,
                                 const rfd_liveness_config *cfg, float *const *tensors, float *weights, int32_t *rois,
                                 int32_t *status);
/* The device-resident form (conventions of rfd_detect_faces_device): every imgs[i].data and every other pointer is DEVICE
 * memory (imgs[], cfg and the tensors[] array itself are host memory).  Enqueued on the context's stream; async = 0 returns
 * after the stream has drained, any other value at once.  boxes / found may be the box / found arrays rfd_detect_faces_device
 * has just been asked to fill on the same stream: detection, selection, alignment, the ID / quality tensors and the liveness
 * tensors then run back to back with no host synchronisation in between. */
RFD_API int rfd_liveness_tensors_device(rfd_ctx *ctx, const rfd_image *imgs, int n, const float *boxes, const int32_t *found,
                                        const rfd_liveness_config *cfg, float *const *tensors, float *weights, int32_t *rois,
                                        int32_t *status, int async);
/* The decision rule on the outputs of k models (any k >= 1), logits[j] = [n][classes] f32 with classes >= 2, weights [n][k] as
 * the tensor call returned them: score[i] = (((0 + l0*w0) + l1*w1) + ...) / ((0 + w0) + w1 + ...) with l_j = logits[j][i][1],
 * every operation one f32 rounding in this order; live[i] = score[i] > threshold (strict; the reference's literal is 0.55).
 * Weights that sum to 0 -- every face with a negative status -- give score NaN and live 0, as the reference's division would.
 * Host pointers.  No output may overlap an input, except that score may be weights when k = 1. */
RFD_API int rfd_liveness_decide(rfd_ctx *ctx, const float *const *logits, int k, int n, int classes, const float *weights,
                                float threshold, float *score, int32_t *live);
/* The same with DEVICE pointers (the logits[] array itself is host memory), enqueued on the context's stream (no
 * synchronisation). */
RFD_API int rfd_liveness_decide_device(rfd_ctx *ctx, const float *const *logits, int k, int n, int classes,
                                       const float *weights, float threshold, float *score, int32_t *live);

/* ---- the face gallery: what FacePipeline::extract's `facial_feature` (pipeline.rs:188-249) is for.  With is_enroll the
 *      L2-normalised embedding is stored, otherwise it is compared with the stored ones; the reference leaves both to its caller.
 *      Here the stored set lives in HBM and one pass over it scores a batch of queries and returns the k best rows of each, so
 *      rfd_normalize_embeddings_device -> rfd_gallery_search_device runs back to back and only n * k pairs cross PCIe.
 *      A gallery belongs to ONE context (its device, its stream; same thread rule) and is destroyed BEFORE it.  It holds up to
 *      `capacity` rows of `dim` values, both fixed at creation, so no device pointer moves under enqueued work.  A row's index is
 *      its insertion order; the caller keeps the table from rows to identities and may hand it to the gallery ("identities" below), which then
 *      searches the k best identities instead of the k best rows.  rfd_gallery_clear empties the gallery; single
 *      rows leave and change through rfd_gallery_remove / _replace, and a gallery outlives its process through
 *      rfd_gallery_save / _load (both below).
 *      Storage: every added f32 value is stored as bf16, rounded to nearest-even.  Rows are expected to be unit vectors (the
 *      output of rfd_normalize_embeddings); they are not normalised again.  The layout is private (MFMA-fragment-major).
 *      Score: score[i][r] = the f32 MFMA-accumulated dot product of bf16(query i) and stored row r over dim, 32 elements per
 *      v_mfma_f32_16x16x32_bf16, K ascending, one accumulator.  The bits of a (query, row) score depend on nothing else: not on
 *      n, k, the gallery's size, the workgroup that scored the row or the query's place in the batch.
 *      Order: a query's results are the k best rows under the total order (score descending, row ascending), in that order:
 *      equal scores resolve to the lower row, and the result does not depend on how the rows are spread over workgroups.  A
 *      gallery of fewer than k rows leaves the tail at row = -1, score = -inf.
 *      Accuracy against the f32 inputs' exact dot product: RNE to bf16 moves a value by at most 2^-9 of itself, so
 *      bf16(q) bf16(g) = q g (1 + a)(1 + b) with |a|, |b| <= 2^-9, i.e. |bf16(q) bf16(g) - q g| <= (2 * 2^-9 + 2^-18) |q g|, and
 *          |score - sum_d q_d g_d| <= (2 * 2^-9 + 2^-18) * sum_d |q_d g_d| + the f32 accumulation error
 *      (a few 2^-24 sum_d |q_d g_d|: bf16 products are exact in f32).  By Cauchy-Schwarz sum_d |q_d g_d| <= |q| |g| = 1 for unit
 *      vectors: at most about 2^-8.
 *      Non-finite values: the host forms reject a NaN or an infinity in a row or a query with RFD_ERR_INVALID_ARG, nothing is
 *      added or searched, and rfd_last_error() names the first offender (row / query and element).  The device forms cannot
 *      look at the data: a NaN score compares false with everything and is never selected (nor is a score of -inf).
 *      Errors: an add beyond capacity returns RFD_ERR_CAPACITY and adds nothing; k < 1 RFD_ERR_INVALID_ARG; k >
 *      RFD_GALLERY_MAX_K RFD_ERR_CAPACITY; a dim that is not a multiple of 32 in 32..1024 RFD_ERR_INVALID_ARG; n = 0 is a no-op;
 *      searching an empty gallery returns all -1 / -inf.  Device pointers must be 16-byte aligned. ---- */
#define RFD_GALLERY_MAX_K 32
typedef struct rfd_gallery rfd_gallery;
RFD_API int rfd_gallery_create(rfd_ctx *ctx, int dim /* multiple of 32, 32..1024 */, int capacity, rfd_gallery **out);
RFD_API void rfd_gallery_destroy(rfd_gallery *g);
RFD_API int rfd_gallery_size(const rfd_gallery *g, int *rows, int *capacity, int *dim); /* any pointer may be NULL */
RFD_API int rfd_gallery_clear(rfd_gallery *g);
/* emb: host [n][dim]; *first_row (may be NULL) = the row the first one got.  Synchronous; staged through page-locked memory
 * that the first host call of a gallery allocates. */
RFD_API int rfd_gallery_add(rfd_gallery *g, const float *emb, int n, int *first_row);
/* emb: device; enqueued on the context's stream, no synchronisation.  The rows count at once (rfd_gallery_size, a following
 * search on the same stream). */
RFD_API int rfd_gallery_add_device(rfd_gallery *g, const float *emb, int n, int *first_row);
/* out: host [n][dim], the stored bf16 values of rows [row0, row0 + n) as f32 */
RFD_API int rfd_gallery_get_rows(rfd_gallery *g, int row0, int n, float *out);
/* queries: host [n][dim], any n: processed in groups of at most 32, one pass over the gallery per group.
 * scores [n][k] f32, rows [n][k] i32, host. */
RFD_API int rfd_gallery_search(rfd_gallery *g, const float *queries, int n, int k, float *scores, int32_t *rows);
/* The same with DEVICE pointers, by the conventions of rfd_detect_faces_device: enqueued on the context's stream; async = 0
 * returns after the stream has drained, any other value at once (rfd_sync before reading the results). */
RFD_API int rfd_gallery_search_device(rfd_gallery *g, const float *queries, int n, int k, float *scores, int32_t *rows, int async);
/* ---- remove and replace.  A row is LIVE from the add that made it until it is removed; a removed row keeps its number (add
 *      never reuses it: rfd_gallery_size's rows stay the number of slots handed out), is never returned by a search again, and
 *      its stored values are erased: rfd_gallery_get_rows reads +0.0 for it, nothing of the embedding stays in HBM.  Replace
 *      writes new values into a row's slot and makes it live, whether it was live or removed: the way to correct an enrolment
 *      and to reuse a hole.  rfd_gallery_clear also forgets every removal.
 *      Search with removed rows: the same scan with one more term in its predicate.  Liveness lives in HBM as one 16-bit word
 *      per block of 16 rows (bit i: row 16 b + i is live); the host keeps a copy, which answers _live and _removed.  Scores
 *      keep their bits (a score depends on its two vectors only) and the order stays total, so a gallery with removed rows
 *      returns what a gallery of its live rows alone would, under the map between the row numbers.  While no row is removed,
 *      a search launches exactly the kernels it launched before these calls existed.
 *      Stream order: remove and replace_device are enqueued on the context's stream in call order with no synchronisation
 *      (row lists travel through page-locked memory of the gallery), so add_device -> remove -> replace_device ->
 *      search_device(async) -> rfd_sync is one sequence without a host wait.  The host form of replace is synchronous.
 *      Errors: a row outside [0, rows) returns RFD_ERR_INVALID_ARG, rfd_last_error() names the first such row and nothing is
 *      changed; n = 0 is a no-op.  remove accepts duplicates and rows that are already removed (no-ops).  replace refuses a
 *      row listed twice (two writers of one slot have no defined order) and, in the host form, non-finite values (naming the
 *      row by its index in the call, as add does, and the element); the device form cannot look, as with add. ---- */
RFD_API int rfd_gallery_remove(rfd_gallery *g, const int32_t *rows /* host [n] */, int n);
/* rows: host [n], distinct; emb: host [n][dim].  Row rows[i] takes bf16(emb[i]) (RNE) and is live afterwards. */
RFD_API int rfd_gallery_replace(rfd_gallery *g, const int32_t *rows, const float *emb, int n);
/* The same with emb in DEVICE memory (16-byte aligned); the row list stays on the host. */
RFD_API int rfd_gallery_replace_device(rfd_gallery *g, const int32_t *rows, const float *emb, int n);
/* the number of live rows (rows - removed rows) */
RFD_API int rfd_gallery_live(const rfd_gallery *g, int *live_rows);
/* the removed rows in ascending order: at most cap of them into out (may be NULL when cap is 0); *count = how many there are,
 * also when that exceeds cap */
RFD_API int rfd_gallery_removed(const rfd_gallery *g, int32_t *out, int cap, int *count);
/* ---- identities.  A gallery holds several enrolments of a person (a passport photo, a selfie, a corrected enrolment), and the
 *      decision a gallery is for compares the best PERSON with the runner-up person; the k best rows of a well-enrolled person
 *      are k rows of that one person.  So every row carries an int32_t identity, and rfd_gallery_search_identities returns the
 *      k best identities.  RFD_GALLERY_NO_IDENTITY (-1) means unlabelled: the row is an identity of its own.  It is the value
 *      of every row after add, add_device, load and clear.  Valid identities are >= 0.
 *      Setting: rfd_gallery_set_identities gives rows[i] the identity ids[i] (>= 0, or RFD_GALLERY_NO_IDENTITY to unlabel it).
 *      It is enqueued on the context's stream in call order with no synchronisation (the lists travel through the gallery's
 *      page-locked memory, as remove's do), so add_device -> set_identities -> search_identities_device(async) -> rfd_sync is
 *      one sequence without a host wait.  A row outside [0, rows), a removed row, a row listed twice or an identity < -1
 *      returns RFD_ERR_INVALID_ARG, rfd_last_error() names the offender and nothing is changed; n = 0 is a no-op.
 *      Reading: _get_identities and _identities are answered from a host copy, as _live and _removed are, without a device wait.
 *      With the other calls: remove resets the row's identity to -1, in HBM too and in stream order (nothing of an erased
 *      enrolment stays); replace / replace_device leave it alone (they correct an enrolment; a reused hole is unlabelled, because
 *      its remove unlabelled it); clear resets all.  save / load and the "RFDG" file are unchanged: identities are NOT in the
 *      file.  The caller owns the table from rows to identities anyway and re-applies it with one set_identities after load.
 *      Memory: the identity array in HBM (capacity x 4 bytes) is allocated by the first set_identities.  Until then, and for
 *      rfd_gallery_search / _search_device always, every call launches exactly the kernels it launched before, with the same
 *      arguments.
 *      Search: for each query, every identity's key is its best live row under the total order (score descending, row
 *      ascending); unlabelled rows each form their own identity.  The result is the k best identity keys under that same
 *      order: the score, the row that achieved it and the identity (-1 for an unlabelled row).  Scores keep their bits, and the
 *      result does not depend on n, the query's place or how rows are spread over waves and workgroups.  Entries with
 *      !(score >= min_score) are replaced by the empty entry (-inf, -1, -1); they form a suffix.  min_score = -INFINITY disables
 *      the threshold; a NaN min_score is RFD_ERR_INVALID_ARG.  Fewer than k identities leave the tail empty.  Removed rows never
 *      count, NaN and -inf scores are never selected.  On a gallery that never had an identity set the call is the plain search
 *      plus ids = -1.  k, n, alignment and the host / device forms follow rfd_gallery_search / _search_device.
 *      Cost: the scan reads the identities of a block of 16 rows (64 bytes) only if a key of that block passes a list's
 *      filter, so its HBM traffic stays the gallery's bytes.  What grows is the selection: a key that beats the k-th best
 *      identity costs an insertion even where its identity is already listed with a better key, so few identities with many
 *      rows each, arriving together, are the expensive case (README, "Gallery search"). ---- */
#define RFD_GALLERY_NO_IDENTITY (-1)
RFD_API int rfd_gallery_set_identities(rfd_gallery *g, const int32_t *rows /* host [n], distinct */, const int32_t *ids /* host [n] */, int n);
/* out: host [n], the identities of rows [row0, row0 + n) (removed rows read -1) */
RFD_API int rfd_gallery_get_identities(const rfd_gallery *g, int row0, int n, int32_t *out);
/* the number of live rows with an identity >= 0 */
RFD_API int rfd_gallery_identities(const rfd_gallery *g, int *labelled_rows);
/* queries: host [n][dim], any n, in passes of 32; scores [n][k] f32, rows [n][k] i32, ids [n][k] i32, host */
RFD_API int rfd_gallery_search_identities(rfd_gallery *g, const float *queries, int n, int k, float min_score, float *scores, int32_t *rows,
                                          int32_t *ids);
/* The same with DEVICE pointers (queries 16-byte aligned); async as in rfd_gallery_search_device. */
RFD_API int rfd_gallery_search_identities_device(rfd_gallery *g, const float *queries, int n, int k, float min_score, float *scores, int32_t *rows,
                                                 int32_t *ids, int async);
/* ---- tags.  One gallery often holds several populations: a tenant per customer, an access list per door, a watch list beside
 *      the staff list, or "verify against the claimed person only".  So every row carries a uint32_t tag, and a filtered
 *      search gives every query q its own pair (mask[q], value[q]): row r is ELIGIBLE for q iff (tag[r] & mask[q]) == value[q].
 *      mask = 0xFFFFFFFF, value = t searches partition t (2^32 partitions); mask = value = 1u << b searches the rows on list
 *      b; a tenant number in the high bits and list bits in the low bits compose; mask = value = 0 matches every row.  A value
 *      with bits outside its mask matches nothing; it is not an error (the device form cannot look at it), the query's result
 *      is then all empty entries.  "Any of these bits" is not a rule: issue the query once per list in the same pass.
 *      The tag is 0 after add, add_device, load and clear; every 32-bit value is a valid tag.
 *      Setting: rfd_gallery_set_tags gives rows[i] the tag tags[i].  It follows rfd_gallery_set_identities in every rule:
 *      enqueued on the context's stream in call order with no synchronisation (the lists travel through the gallery's
 *      page-locked memory), so add_device -> set_tags -> search_filtered_device(async) -> rfd_sync is one sequence without a
 *      host wait.  A row outside [0, rows), a removed row or a row listed twice returns RFD_ERR_INVALID_ARG, rfd_last_error()
 *      names the offender and nothing is changed; n = 0 is a no-op.
 *      Reading: _get_tags is answered from a host copy, without a device wait.
 *      With the other calls: remove resets the row's tag to 0, in HBM too and in stream order (nothing of an erased enrolment
 *      stays); replace / replace_device leave it alone (a reused hole has tag 0, because its remove reset it); clear resets
 *      all.  save / load and the "RFDG" file are unchanged: tags are NOT in the file, the caller re-applies them after load.
 *      Memory: the tag array in HBM (capacity x 4 bytes, rounded up to whole blocks of 16 rows, zeroed) is allocated by the
 *      first set_tags or the first filtered search, in stream order ahead of every use.  Until then every other call launches
 *      exactly the kernels it launched before, with the same arguments; rfd_gallery_search* and
 *      rfd_gallery_search_identities* always do.
 *      Search: the result is that of rfd_gallery_search_identities computed on the rows that are live and eligible for the
 *      query.  Every identity's key is its best live, eligible row under (score descending, row ascending); unlabelled rows
 *      each form their own identity; the k best identity keys come back as (score, row, identity).  So an identity whose best
 *      row is not eligible for a query is represented by its best eligible row, and one without an eligible row is absent
 *      for that query alone.  Entries with !(score >= min_score) are the empty entry (-inf, -1, -1), a suffix; fewer than k
 *      eligible identities leave the tail empty; NaN and -inf scores are never selected.  Scores keep their bits, and the
 *      result does not depend on n, the query's place or how rows are spread over waves and workgroups.  On a gallery
 *      without identities ids is -1 throughout, so the filtered row search needs no entry of its own.  k, n (any, in passes
 *      of 32), min_score, alignment, async and the host / device forms follow rfd_gallery_search_identities / _device; the
 *      host form refuses non-finite queries; a null mask or value with n > 0 is RFD_ERR_INVALID_ARG.
 *      Cost: the scan reads the tags of a block of 16 rows (64 bytes beside its 16 KiB of operands at dim 512) only if a key
 *      of that block passes a list's filter.  A small partition's lists stay empty, so for it every block passes and pays that
 *      read and its wait; a block with nothing eligible then costs no offer (README, "Gallery search"). ---- */
RFD_API int rfd_gallery_set_tags(rfd_gallery *g, const int32_t *rows /* host [n], distinct */, const uint32_t *tags /* host [n] */, int n);
/* out: host [n], the tags of rows [row0, row0 + n) (removed rows read 0); host copy, no device wait */
RFD_API int rfd_gallery_get_tags(const rfd_gallery *g, int row0, int n, uint32_t *out);
/* queries: host [n][dim]; mask, value: host [n] each; scores [n][k] f32, rows [n][k] i32, ids [n][k] i32, host */
RFD_API int rfd_gallery_search_filtered(rfd_gallery *g, const float *queries, int n, int k, float min_score, const uint32_t *mask, const uint32_t *value,
                                        float *scores, int32_t *rows, int32_t *ids);
/* The same with DEVICE pointers (queries 16-byte aligned; mask, value: DEVICE [n] each); async as in rfd_gallery_search_device. */
RFD_API int rfd_gallery_search_filtered_device(rfd_gallery *g, const float *queries, int n, int k, float min_score, const uint32_t *mask,
                                               const uint32_t *value, float *scores, int32_t *rows, int32_t *ids, int async);
/* ---- nearest.  A deployment that enrols people also asks a question about the gallery itself: is this person already in it,
 *      under another name (de-duplication)?  It is asked of every enrolment batch, new rows against everything, and as a
 *      periodic sweep, every row against every row.  rfd_gallery_nearest answers it on the device: the rows are already stored
 *      as matrix-core operands, so nothing crosses PCIe but the answer, the gallery is read once per tile of rows instead of
 *      once per 32 queries, and the self-match never appears.
 *      Contract: for every row a in [row0, row0 + n), entry a - row0 is the best row b under the gallery's total order, which is
 *      score descending, then row ascending.  The candidates are the rows b that meet all of these conditions:
 *        - b is live;
 *        - b != a;
 *        - b is allowed by `mode`: RFD_GALLERY_NEAREST_OTHER_ROW allows every b, RFD_GALLERY_NEAREST_OTHER_IDENTITY additionally
 *          refuses id[a] >= 0 && id[b] == id[a] (an unlabelled row is an identity of its own, as in the identity search);
 *        - b is allowed by the tag rule: (tag[a] & tag_mask) == (tag[b] & tag_mask); tag_mask = 0 allows every row;
 *        - b's score is neither NaN nor -inf, and is >= min_score.
 *      `ids` receives the identity of b.  The empty entry is (-inf, -1, -1); it is written where a is removed, where no
 *      candidate qualifies, and where the gallery has one row.  min_score = -INFINITY disables the threshold.
 *      Score bits: score(a, b) has exactly the bits that rfd_gallery_search returns for row b when the query is
 *      rfd_gallery_get_rows(a): the same instruction, K ascending, one accumulator chain starting from +0 per (a, b).  So
 *      score(a, b) and score(b, a) have equal bits, and the result does not depend on row0, n, the number of CUs, or how the
 *      work is tiled and split.
 *      k is 1 on purpose: one best key per row lives in registers, the output has a fixed size, and a caller who wants
 *      clusters joins the links on the host.  Mind what that gives: nearest-neighbour links above a threshold CONNECT
 *      duplicates, they do NOT ENUMERATE all pairs -- of three enrolments of one person each may name only its best partner.
 *      Errors: row0 < 0, n < 0 or row0 + n beyond the rows handed out, an unknown mode, a non-zero reserved word, and a null or
 *      misaligned `scores` or `rows` (4-byte alignment suffices; `ids` may be NULL, else it follows the same rule) return
 *      RFD_ERR_INVALID_ARG; n = 0 is a no-op; a refused call writes nothing.
 *      Stream: the device form is enqueued on the context's stream in call order with no host wait, so add_device ->
 *      nearest_device runs back to back; async as in rfd_gallery_search_device.  The host form is synchronous and moves its
 *      outputs through the gallery's page-locked memory.  The call's workspace belongs to the gallery and is allocated on
 *      first use; the identity and the tag array are read where they exist and never allocated here.  Every other gallery
 *      call launches the kernels and arguments it launched before.
 *      Cost: rows are processed in tiles (rfd_debug_gallery_nearest_plan), and the gallery is read ceil(n / tile_rows) times;
 *      few rows against a large gallery are split over the gallery and merged, so they still occupy every CU. ---- */
#define RFD_GALLERY_NEAREST_OTHER_ROW      0   /* any live row b != a */
#define RFD_GALLERY_NEAREST_OTHER_IDENTITY 1   /* additionally not (id[a] >= 0 && id[b] == id[a]) */
typedef struct rfd_gallery_nearest_config {
    int32_t  mode;        /* one of the two above */
    float    min_score;   /* an entry whose best score is not >= min_score is empty; -inf: none is */
    uint32_t tag_mask;    /* b counts for a iff (tag[a] & tag_mask) == (tag[b] & tag_mask); 0: every row */
    int32_t  reserved[5]; /* must be 0 */
} rfd_gallery_nearest_config;                  /* 32 bytes */
RFD_API void rfd_gallery_nearest_config_default(rfd_gallery_nearest_config *cfg); /* OTHER_ROW, -inf, 0 */
RFD_API int rfd_gallery_nearest(rfd_gallery *g, int row0, int n, const rfd_gallery_nearest_config *cfg /* NULL: default */,
                                float *scores /* host [n] */, int32_t *rows /* host [n] */, int32_t *ids /* host [n] or NULL */);
/* The same with DEVICE outputs */
RFD_API int rfd_gallery_nearest_device(rfd_gallery *g, int row0, int n, const rfd_gallery_nearest_config *cfg,
                                       float *scores, int32_t *rows, int32_t *ids, int async);

/* ---- gallery file "RFDG", version 1, little-endian, in logical row order (not the private storage layout):
 *          bytes 0..19  "RFDG", u32 version = 1, u32 dim, u32 rows, u32 reserved = 0
 *          then         ceil(rows / 8) bytes of liveness, bit (r & 7) of byte r >> 3 set while row r is live, bits past rows 0
 *          then         rows x dim bf16 values, row-major; a removed row is present, as zeros
 *      Row numbers survive a round trip: after load, every rfd_gallery_get_rows and every search returns the bits it returned
 *      before save, and _live / _removed answer the same.
 *      save synchronises the context's stream, writes path + ".tmp" and renames it over path; a failure to open, write or
 *      rename returns RFD_ERR_IO and leaves path as it was.
 *      load validates the whole file before it allocates anything, then creates a gallery of `capacity` rows (0: the file's
 *      rows, at least 1; fewer than the file's rows: RFD_ERR_CAPACITY) on ctx, synchronously.
 *      Validation (all of it also in rfd_gallery_file_info, which needs no context and no device): a path that cannot be
 *      opened or read returns RFD_ERR_IO; a wrong magic or version, a dim that is not a multiple of 32 in 32..1024, a non-zero
 *      reserved field, a file length other than the header implies, liveness bits set beyond rows, or a non-finite bf16 value
 *      (row and element are named) returns RFD_ERR_INVALID_ARG, and rfd_last_error() names the cause.  Values of a removed
 *      row, which a file of this library holds as zeros, are loaded as zeros whatever the file holds. ---- */
RFD_API int rfd_gallery_save(rfd_gallery *g, const char *path);
RFD_API int rfd_gallery_load(rfd_ctx *ctx, const char *path, int capacity, rfd_gallery **out);
RFD_API int rfd_gallery_file_info(const char *path, int *dim, int *rows, int *live); /* any of the three may be NULL */
/* host only, no GPU: element offset of (row, d) in the private storage layout (-1: dim or an index out of range); the add
 * kernel scatters by this function and tests pin that it is a bijection and that an MFMA operand fetch is one 1 KiB span */
RFD_API int64_t rfd_debug_gallery_offset(int dim, int row, int d);
/* host only, no GPU, no context: how rfd_gallery_nearest of rows [row0, row0 + n) decomposes on a gallery of `rows` rows handed
 * out and `dim` values per row, on a device of `cus` compute units.  A workgroup owns one tile of tile_rows rows of the range
 * and one split: the row blocks (of 16 rows) b < blocks with (b / 4) % splits == s, at most blocks_per_split of them; grid =
 * tiles * splits <= ceil(n / tile_rows) + 4 * cus.  form: 0 = the rows of a tile in LDS (any dim), 1 = in registers (dim 512, calls
 * of more than 32 rows); tile_rows follows the form.
 * Arguments outside the gallery's rules return RFD_ERR_INVALID_ARG and a plan of zeros. */
typedef struct rfd_gallery_nearest_plan {
    int32_t form, tile_rows, tiles, splits, blocks, blocks_per_split;
    int64_t grid;     /* workgroups of the scan */
    int64_t ws_bytes; /* splits * n keys of 8 bytes */
} rfd_gallery_nearest_plan;
RFD_API int rfd_debug_gallery_nearest_plan(int rows, int row0, int n, int dim, int cus, rfd_gallery_nearest_plan *out);

/* ---- every detected face of a frame: the packed face list.  FaceSelection keeps one face per frame (eKYC); the gallery's
 *      search pass scores 32 queries at once, and a group photo or a door camera holds many faces.  Here up to max_faces
 *      detections of each of n frames become ONE dense list of T faces in HBM, and every listed face is aligned and tensorised
 *      by the arithmetic of the one-face path (the same kernels, reading frame[t] instead of frame t).  The whole path runs in the
 *      context's stream order with no host synchronisation; T itself is a number the host never needs.
 *      The list rule.  For frame b, walk rows i = 0 .. count[b]-1 of its detection slab in the detector's order (descending
 *      score; a count outside [0, max_det] is clamped).  A row PASSES when
 *          x2 - x1 >= min_face_px  &&  y2 - y1 >= min_face_px  &&  score >= min_score
 *      i.e. fminf(x2 - x1, y2 - y1) >= min_face_px on numbers; each difference is one f32 subtraction; a NaN in any of the five
 *      values makes its comparison false, so the row fails.  The first max_faces passing rows are TAKEN; c[b] is their number.
 *      first[b] = c[0] + .. + c[b-1] (first[0] = 0), first[n] = T = total[0].  Packed face t in [first[b], first[b+1]) is the
 *      (t - first[b])-th taken row of frame b: frame[t] = b, row[t] = its slab row, box[t] / kps[t] = that row's values.
 *      The caller gives the capacity `cap` of the per-face arrays, in faces (any cap >= 1: it is not bound by max_batch_size).
 *      total[0] = T is the untruncated count, as rfd_dets.total is; first[] is not truncated either.  Faces t >= cap are dropped,
 *      so later frames lose first.  EVERY PER-FACE OUTPUT ROW t >= min(T, cap) IS LEFT EXACTLY AS THE CALLER PASSED IT.
 *      Per packed face t < min(T, cap): status[t] is 0, 1 or -3 (-1 and -2 cannot occur: a listed face has a box and key
 *      points); crops[t] is written unless crops is NULL; tensors[j][t] for j < k.  All of them are byte-identical to what
 *      rfd_align_faces_tensors returns for the single frame frame[t] with box[t], kps[t] and found = 3.
 *      Errors: max_faces < 1, cap < 1, a negative or non-finite min_face_px, a non-finite min_score: RFD_ERR_INVALID_ARG, and
 *      rfd_last_error() names the field; k > RFD_MAX_FACE_TENSORS: RFD_ERR_CAPACITY; n > max_batch_size: RFD_ERR_CAPACITY.
 *      A NULL list config is the default one, a NULL alignment config the reference's. ---- */
typedef struct rfd_face_list_config {
    int32_t max_faces;     /* per frame, >= 1 */
    float   min_face_px;   /* >= 0, finite: the narrower side of the box, in source pixels */
    float   min_score;     /* finite */
    int32_t reserved[4];
} rfd_face_list_config;
RFD_API void rfd_face_list_config_default(rfd_face_list_config *cfg); /* 32, 0, 0: one gallery search pass per frame */
typedef struct rfd_face_list {
    int32_t *total;   /* [1]   */
    int32_t *first;   /* [n+1] */
    int32_t *frame;   /* [cap] */
    int32_t *row;     /* [cap] */
    float   *box;     /* [cap][5]  */
    float   *kps;     /* [cap][10] */
    int32_t *status;  /* [cap] */
    uint8_t *crops;   /* [cap][out_h][out_w][3], may be NULL */
    float   *tensors[RFD_MAX_FACE_TENSORS]; /* [j < k]: [cap][3][cfgs[j].out_h][cfgs[j].out_w] */
} rfd_face_list;
/* Stage-level, host pointers: frames, and detections as rfd_detect_batch returns them (dets->boxes / landmarks / count, as
 * rfd_select_faces takes them) -> the list, through the kernels of the two entries below.  k = 0 with crops = NULL gives the
 * list (and the status) alone.  The call waits for the stream once, to learn T, and then fetches only the min(T, cap) listed
 * rows: the tail of the caller's host arrays stays untouched too. */
RFD_API int rfd_align_detections(rfd_ctx *ctx, const rfd_image *imgs, int n, const rfd_dets *dets,
                                 const rfd_face_list_config *list_cfg, const rfd_alignment_config *align_cfg,
                                 const rfd_face_tensor_config *cfgs, int k, int cap, rfd_face_list *out);
/* Fused: host frames in, host list out; the frames cross PCIe once, detections never leave HBM. */
RFD_API int rfd_detect_align_all_batch(rfd_ctx *ctx, const rfd_image *imgs, int n, const rfd_face_list_config *list_cfg,
                                       const rfd_alignment_config *align_cfg, const rfd_face_tensor_config *cfgs, int k,
                                       int cap, rfd_face_list *out);
/* The device-resident form (conventions of rfd_detect_faces_device): every imgs[i].data and every pointer of `out` is DEVICE
 * memory.  Detection, the list, alignment and tensors are enqueued on the context's stream; async = 0 returns after the stream
 * has drained, any other value at once with nothing waited for.  tensors[j] with n = cap rows is what the models and then
 * rfd_normalize_embeddings_device -> rfd_gallery_search_device take; the rows past total are the caller's to ignore. */
RFD_API int rfd_detect_all_faces_device(rfd_ctx *ctx, const rfd_image *imgs, int n, const rfd_face_list_config *list_cfg,
                                        const rfd_alignment_config *align_cfg, const rfd_face_tensor_config *cfgs, int k,
                                        int cap, rfd_face_list *out, int async);

/* ---- JPEG decode: the first line of FacePipeline::extract (pipeline.rs:188-249), byte_data_to_opencv (src/utils/utils.rs:8-52),
 *      an imdecode of the file's bytes.  File bytes in, BGR frames in HBM out: the frames rfd_detect_batch_device and
 *      rfd_detect_faces_device read, with no JPEG library in the caller, no decoded frame on PCIe.
 *      Two halves.  The serial one -- marker parsing and Huffman decoding -- runs on host threads inside the call, one frame per
 *      task, on threads that never touch HIP (rfd_set_decode_threads: 1..16, default 4; never derived from the machine's CPU
 *      count).  It writes each block's QUANTISED coefficients, in zigzag order and only up to the last non-zero one, with one
 *      32-bit (offset, count) word per block, straight into page-locked memory of the context (allocated by the first decode
 *      call, sized by max_src_w, max_src_h and max_batch_size; the layout is private: DESIGN.md section 5).  The parallel half is
 *      two kernels per BATCH, whatever the number, sizes and samplings of its frames: dequantisation + libjpeg's accurate integer
 *      inverse DCT (jidctint.c: 13-bit constants, a column pass that keeps 2 extra bits, a row pass that descales by 18 and adds
 *      128, clamped to 0..255) into u8 component planes padded to whole MCUs; then libjpeg's fancy (triangle) chroma upsampling
 *      and its fixed-point YCbCr -> RGB tables, cropped to the image and stored as [H][W][3] u8 BGR at the caller's stride.
 *      Contract: the pixels equal libjpeg-turbo's defaults (JDCT_ISLOW, fancy upsampling) -- what cv::imdecode and Pillow return
 *      -- byte for byte (tests/test_jpeg_cpu.py pins the arithmetic against Pillow, tests/test_jpeg_gpu.py and
 *      tests/test_jpeg_sweep_gpu.py the kernels).  Edges
 *      are part of it: horizontally the filter runs over the component's own ceil(W h / hmax) samples, vertically the first and
 *      the last real sample row stand in for the rows beyond them, and a chroma plane of one or two samples per row is
 *      replicated, not filtered (libjpeg's own rule).  Outside the contract: coefficients that no 8-bit image produces (IDCT
 *      results far outside 0..255) decode without a fault to pixels that are not pinned -- libjpeg's own C and SIMD paths differ
 *      there; the arithmetic here wraps modulo 2^32 and clamps.
 *      Supported: baseline and extended sequential Huffman files (SOF0, SOF1) with 8-bit samples and ONE interleaved scan of one
 *      component (grey) or of three with luma sampling 1x1, 2x1 or 2x2 and chroma 1x1; 8- and 16-bit quantisation tables;
 *      restart intervals; APPn and COM segments are skipped (but for the orientation tag: "EXIF orientation" below), fill bytes
 *      and 0xFF00 stuffing understood.
 *      RFD_ERR_UNSUPPORTED: progressive (SOF2), lossless, hierarchical and arithmetic-coded files, 12-bit samples, four (or two)
 *      components, other sampling factors, files of more than one scan.  RFD_ERR_INVALID_ARG: a truncated or malformed file -- a
 *      length field that points past the end, a Huffman code that is not in its table, a coefficient index above 63, a table
 *      that was never defined, zero dimensions, a restart marker out of sequence, data that ends before the last MCU.  In both
 *      cases rfd_last_error() names the cause and the byte offset (and, in a batch, the frame), and NOTHING is enqueued for any
 *      frame of the call: every file is parsed and entropy-decoded before the first copy or kernel.  A file may end without EOI
 *      once its last MCU is complete (libjpeg warns and accepts).  (RFD_JPEG_ENTROPY_DEVICE, below, runs its entropy kernel
 *      before that point; it writes the context's own memory only, and no output frame of a refused call is written.)
 *      Divergence: a grey file gives B = G = R = Y in a 3-channel frame.  The reference decodes with IMREAD_UNCHANGED, which
 *      keeps such a file at one channel, and its detector then fails on it (at_2d::<Vec3b>, face_detection.rs:226). ---- */
typedef enum rfd_jpeg_sampling { RFD_JPEG_GRAY = 0, RFD_JPEG_444 = 1, RFD_JPEG_422 = 2, RFD_JPEG_420 = 3 } rfd_jpeg_sampling;
struct rfd_jpeg_info {
    int32_t width, height;
    int32_t components;       /* 1 or 3 */
    int32_t sampling;         /* rfd_jpeg_sampling */
    int32_t restart_interval; /* MCUs between restart markers, 0: none */
    int32_t reserved[3];      /* 0 */
};
/* Host only, no context, no device: everything from SOI to the end of the SOS header is parsed and validated, with the statuses
 * and messages the decode would give (the entropy-coded data itself is looked at by the decode only).  A refused file leaves
 * *out untouched.  (The struct shares its name with the function, so C and C++ both spell the type `struct rfd_jpeg_info`.) */
RFD_API int rfd_jpeg_info(const uint8_t *bytes, size_t len, struct rfd_jpeg_info *out);
/* Decodes n files into n caller-allocated DEVICE frames: out[i].data is device memory of out[i].height rows of out[i].stride
 * bytes; width and height must equal the file's (the ORIENTED size in RFD_JPEG_ORIENTATION_APPLY mode, "EXIF orientation" below,
 * the SCALED size after rfd_set_jpeg_scale, "JPEG decode, reduced size" below; else RFD_ERR_INVALID_ARG) and stride must be >= 3 * width; bytes of a row beyond 3 * width are not touched.  rfd_image declares data const because every other entry point reads frames; this one
 * WRITES through it (the library casts the const away).  The same array is then valid input to rfd_detect_batch_device,
 * rfd_detect_faces_device and rfd_liveness_tensors_device on the same stream, with no synchronisation in between.
 * bytes[] / len[] and the files are host memory and may be freed when the call returns.  Entropy decoding happens inside the
 * call; the copies and the two kernels go on the context's stream.  async as in rfd_gallery_search_device: 0 returns after the
 * stream has drained, any other value at once (rfd_sync before reading the frames from another stream).
 * n > max_batch_size, or a file wider than max_src_w or higher than max_src_h: RFD_ERR_CAPACITY.  n = 0 is a no-op.
 * Staging reuse: there is ONE page-locked staging area, guarded by an event -- a call waits, before its threads write into it,
 * until the copies the previous call enqueued from it have run (its kernels need not have: they read the device copy, which
 * the next call's copies follow in stream order).  So two asynchronous calls back to back are safe; the second one's entropy
 * decoding does not overlap the first one's PCIe copy. */
RFD_API int rfd_decode_jpeg_batch_device(rfd_ctx *ctx, const uint8_t *const *bytes, const size_t *len, int n, const rfd_image *out, int async);
/* The same into HOST frames (out[i].data is host memory, written through the same const cast); synchronous. */
RFD_API int rfd_decode_jpeg_batch(rfd_ctx *ctx, const uint8_t *const *bytes, const size_t *len, int n, const rfd_image *out);
/* Worker threads of the entropy decoder: 1 <= threads <= 16 (else RFD_ERR_INVALID_ARG); a batch uses min(threads, n) of them.
 * The pixels do not depend on it. */
RFD_API int rfd_set_decode_threads(rfd_ctx *ctx, int threads);
/* Test hook, host only, no context: the DEQUANTISED coefficients of every block, [blocks][64] i16 in natural (row-major) order,
 * blocks component-major, each component's plane padded to whole MCUs and walked row by row -- the input of the inverse DCT, so
 * the host half can be tested without a GPU (tests/jpeg_ref.py continues from here).  A product outside i16 (hostile files
 * only) saturates.  *blocks = the file's block count, also when it exceeds cap_blocks (then RFD_ERR_CAPACITY, nothing written);
 * out may be NULL when cap_blocks is 0. */
RFD_API int rfd_debug_jpeg_coefficients(const uint8_t *bytes, size_t len, int16_t *out, size_t cap_blocks, size_t *blocks);

/* ---- JPEG decode, entropy decoding on the device (opt-in).  A file with a restart interval (DRI) of R MCUs is cut into pieces
 *      that decode independently: after every R MCUs the bit stream is byte-aligned, a RSTn marker follows and every DC
 *      predictor is zero again.  In RFD_JPEG_ENTROPY_DEVICE mode the host only finds the markers of such a file (a pre-scan, no
 *      Huffman decoding); the file's entropy-coded bytes cross PCIe instead of its coefficients, and one device thread per
 *      restart interval decodes them straight into the pools the inverse-DCT kernel reads.
 *      Eligible is a frame of a DEVICE-mode call whose file has 1 <= R <= 128 MCUs, whose scan holds exactly ceil(MCUs / R)
 *      intervals with the markers in the sequence RST0, RST1, .. RST7, RST0, .., and whose scan bytes fit the staging (allocated
 *      by the first DEVICE-mode call, sized by max_src_w, max_src_h and max_batch_size: DESIGN.md section 5; a context that never
 *      selects the mode allocates nothing for it).  Every other frame -- no DRI, a longer interval, any structural oddity -- is
 *      decoded by the host threads exactly as in HOST mode, while the entropy kernel runs.
 *      Strict acceptance: the device decoder refuses a frame unless every interval decodes to EXACTLY its bytes (after the
 *      interval's last MCU fewer than 8 bits and no byte are unread), besides a code that is in no table, a coefficient index
 *      above 63, a zero run past 64 and the use of a bit beyond the interval.  That is a strict subset of what the lenient host
 *      decoder accepts (garbage in front of a restart marker, say), and on it the coefficients are identical.  A refused frame
 *      is decoded again by the host threads, which accept it or give the call its status and message.  So status, message,
 *      pixels and the promise that no output frame is written when any file is refused are the same in both modes for every
 *      input; only rfd_jpeg_last_paths tells the modes apart.
 *      async: the call enqueues the entropy kernel, copies one status word per frame back and waits for that copy.  In DEVICE
 *      mode a call with async != 0 therefore returns after the entropy kernel (and everything enqueued on the context's stream
 *      before it) has finished; it still returns before the inverse-DCT and colour kernels have run. ---- */
typedef enum rfd_jpeg_entropy { RFD_JPEG_ENTROPY_HOST = 0, RFD_JPEG_ENTROPY_DEVICE = 1 } rfd_jpeg_entropy;
/* HOST is the default; any other value than the two: RFD_ERR_INVALID_ARG.  May be changed between calls. */
RFD_API int rfd_set_jpeg_entropy(rfd_ctx *ctx, int mode);
/* How each frame of the last rfd_decode_jpeg_batch* call was entropy-decoded: 0 on the host because it was not eligible (always,
 * in HOST mode), 1 on the device, 2 on the host after the device refused it.  *n = the frames of that call (0 before the first),
 * also when n > cap (then RFD_ERR_CAPACITY, nothing written).  n may be NULL. */
RFD_API int rfd_jpeg_last_paths(rfd_ctx *ctx, int32_t *path, int cap, int *n);
/* Test hook, host only, no context: the marker pre-scan.  Interval k is bytes [begin[k], end[k]) of the file; end is the position
 * of the first 0xFF of the marker sequence that closes the interval (fill bytes and the marker are excluded).  *count = the
 * intervals the file must have, also when that exceeds cap (then RFD_ERR_CAPACITY).  RFD_ERR_UNSUPPORTED with a message when the
 * file is not eligible by its structure (no DRI, R above the limit, another number of intervals, markers out of sequence); the
 * header's own status where the header is refused. */
RFD_API int rfd_debug_jpeg_intervals(const uint8_t *bytes, size_t len, uint32_t *begin, uint32_t *end, size_t cap, size_t *count);
/* Test hook: rfd_debug_jpeg_coefficients with the quantised coefficients taken from the device entropy kernel, whatever the
 * context's mode.  Never falls back: RFD_ERR_UNSUPPORTED when the file is not eligible or the device refused it. */
RFD_API int rfd_debug_jpeg_coefficients_device(rfd_ctx *ctx, const uint8_t *bytes, size_t len, int16_t *out, size_t cap_blocks, size_t *blocks);

/* ---- JPEG decode, EXIF orientation (opt-in).  A phone stores a portrait photo as landscape pixels plus an orientation tag in
 *      an Exif APP1 segment.  cv::imdecode applies the tag under its default flags; the reference decodes with IMREAD_UNCHANGED
 *      (utils.rs:18), which does not.  So RFD_JPEG_ORIENTATION_IGNORE is the default, in which every call does what it did
 *      before the mode existed, bit for bit, and RFD_JPEG_ORIENTATION_APPLY is a mode the caller selects.
 *      The tag: of the segments between SOI and SOS, the FIRST APP1 whose payload begins with "Exif\0\0" is looked at, and only
 *      that one.  It holds a TIFF block -- byte order II or MM, the number 42, the 32-bit offset of IFD0 from the start of the
 *      block, and IFD0 (a 16-bit entry count, then 12-byte entries, anywhere in the payload).  The orientation is the first entry
 *      with tag 0x0112 that is one SHORT or one LONG, read in the file's byte order; values 1..8 are honoured.  In every other
 *      case -- no such segment or entry, a bad byte-order mark or 42, another type or count, another value, any read that would
 *      fall outside the payload -- the orientation is 1 and the decode goes on: EXIF damage never refuses a file.
 *      APPLY mode: with S[H][W] the stored image, rfd_decode_jpeg_batch* writes out[yo][xo] =
 *          orientation 1   S[yo][xo]              H x W  (rows x columns)
 *          orientation 2   S[yo][W-1-xo]          H x W
 *          orientation 3   S[H-1-yo][W-1-xo]      H x W
 *          orientation 4   S[H-1-yo][xo]          H x W
 *          orientation 5   S[xo][yo]              W x H
 *          orientation 6   S[H-1-xo][yo]          W x H
 *          orientation 7   S[H-1-xo][W-1-yo]      W x H
 *          orientation 8   S[xo][W-1-yo]          W x H
 *      which is what Pillow's ImageOps.exif_transpose gives.  out[i].width / height must equal the ORIENTED size
 *      (rfd_jpeg_orientation reports it), else RFD_ERR_INVALID_ARG naming the frame, with nothing enqueued and no frame written;
 *      stride, alignment and the promise that no byte beyond 3 * width of a row is touched hold for the oriented frame.  The
 *      capacity check against max_src_w / max_src_h stays on the STORED size, which is what the decoder's pools are sized by.
 *      The detect calls check the size of the frame they are given: a context fed portrait files of 1920 x 1080 stored pixels
 *      hands 1080 x 1920 frames to rfd_detect_batch_device and therefore needs max_src_h >= 1920.  Boxes and landmarks of a
 *      later detect call are in the ORIENTED frame's coordinates; the table above maps them back to stored ones.
 *      Frames of orientation 1 take the same colour kernel in both modes; frames of orientation 2..8 take a third launch, made
 *      only when a batch holds one, which computes the same pixels and stores them through the map.  The
 *      orientation does not depend on where a frame was entropy-decoded. ---- */
typedef enum rfd_jpeg_orientation_mode { RFD_JPEG_ORIENTATION_IGNORE = 0, RFD_JPEG_ORIENTATION_APPLY = 1 } rfd_jpeg_orientation_mode;
struct rfd_jpeg_orientation {
    int32_t orientation;                 /* 1..8 */
    int32_t width, height;               /* of the frame an APPLY-mode decode writes: the stored size, swapped for 5..8 */
    int32_t stored_width, stored_height; /* as rfd_jpeg_info reports them */
    int32_t reserved[3];                 /* 0 */
};
/* Host only, no context, no device: the header validation of rfd_jpeg_info with the same statuses and messages, then the tag.  A
 * refused file leaves *out untouched.  (Struct and function share the name, as rfd_jpeg_info does.) */
RFD_API int rfd_jpeg_orientation(const uint8_t *bytes, size_t len, struct rfd_jpeg_orientation *out);
/* IGNORE is the default; any other value than the two: RFD_ERR_INVALID_ARG.  May be changed between calls. */
RFD_API int rfd_set_jpeg_orientation(rfd_ctx *ctx, int mode);
/* The orientation that was applied to each frame of the last rfd_decode_jpeg_batch* call: all 1 in IGNORE mode.  *n = the frames
 * of that call (0 before the first), also when n > cap (then RFD_ERR_CAPACITY, nothing written).  n may be NULL. */
RFD_API int rfd_jpeg_last_orientations(rfd_ctx *ctx, int32_t *orientation, int cap, int *n);

/* ---- JPEG decode, reduced size (opt-in).  libjpeg's scale_num / scale_denom = 1 / s for s = 2, 4, 8 (cv::IMREAD_REDUCED_COLOR_2 /
 *      4 / 8, Pillow's draft): the frame is built at 1/s of the stored size directly from the low frequencies of every block by
 *      a reduced inverse DCT, instead of being decoded in full and shrunk by a filter of the caller's.  The reference decodes
 *      with IMREAD_UNCHANGED (utils.rs:18), which is full size.  So denominator 1 is the default, in which every call writes,
 *      copies and launches exactly what it did before the mode existed, and 2 / 4 / 8 is a mode the caller selects; it applies to
 *      every frame of a call.
 *      Contract: the pixels equal libjpeg-turbo's at that scale (what Pillow returns after draft()) byte for byte; the same
 *      things stay outside it as at full size.  With m = 8 / s:
 *        size        ceil(W / s) x ceil(H / s)
 *        IDCT size   per component n_c (jdmaster.c): n = m; while n < 8 and (hmax m) mod (h_c n 2) = 0 and (vmax m) mod (v_c n 2) = 0,
 *                    n doubles.  The component is then upsampled by (hmax m / (h_c n_c), vmax m / (v_c n_c)).
 *                      sampling   luma n at s = 2 / 4 / 8   chroma n at s = 2 / 4 / 8   remaining chroma upsampling
 *                      grey       4 / 2 / 1                 --                          --
 *                      4:4:4      4 / 2 / 1                 4 / 2 / 1                   none
 *                      4:2:2      4 / 2 / 1                 4 / 2 / 1                   h2v1
 *                      4:2:0      4 / 2 / 1                 8 / 4 / 2                   none: the chroma grows through its IDCT
 *        IDCTs       jidctred.c on dequantised coefficients, PASS1_BITS 2, descale(x, k) = (x + 2^(k-1)) >> k, x[r] the frequencies
 *                    of a column, then of a row of the work array; + 128, clamped to 0..255
 *                      4 x 4   reads frequencies 0 1 2 3 5 6 7 of each axis.  t0 = x0 << 14, t2 = 15137 x2 - 6270 x6, t10 = t0 + t2,
 *                              t12 = t0 - t2, a = -1730 x7 + 11893 x5 - 17799 x3 + 8697 x1, c = -4176 x7 - 4926 x5 + 7373 x3 +
 *                              20995 x1; outputs t10 + c, t12 + a, t12 - a, t10 - c; descale by 12, then by 19
 *                      2 x 2   reads 0 1 3 5 7.  t10 = x0 << 15, t0 = -5906 x7 + 6967 x5 - 10426 x3 + 29692 x1; outputs t10 + t0,
 *                              t10 - t0; descale by 13, then by 20
 *                      1 x 1   descale(dc, 3)
 *                      8 x 8   the full-size inverse DCT
 *        upsampling  the h2v1 left for 4:2:2 is h2v1_fancy_upsample over the component's own ceil(ceil(W / s) / 2) samples at s = 2
 *                    and 4 (a row of <= 2 samples is replicated); at s = 8 it is plain replication (jdsample.c turns the fancy
 *                    filter off when the smallest IDCT is 1 x 1).  The colour conversion is the full-size one.
 *      out[i].width / height must equal the SCALED size, and in RFD_JPEG_ORIENTATION_APPLY mode the scaled and then oriented size
 *      (rfd_jpeg_scaled_size reports it), else RFD_ERR_INVALID_ARG naming the frame, with nothing enqueued and no frame written;
 *      stride, alignment and the promise that no byte beyond 3 * width of a row is touched hold for the scaled frame.
 *      Orientation composes: the stored image is scaled, then the index map of "EXIF orientation" is applied to the scaled image.
 *      The capacity check against max_src_w / max_src_h stays on the STORED size, which is what the decoder's pools are sized by:
 *      a reduced decode needs a context as large as a full one.  A scaled frame is an ordinary frame to the detect, faces and
 *      liveness calls.  Boxes and landmarks are then in the scaled frame's coordinates; multiply by s to map them back, which is
 *      exact up to the rounding up of the size at the right and bottom edges (less than s stored pixels).
 *      What it saves is frame bytes, plane bytes, coefficient bytes on PCIe (a block's run ends at the last non-zero coefficient
 *      its IDCT reads) and kernel time.  It saves NO host time: the Huffman decoder still parses every code of every block. ---- */
struct rfd_jpeg_scaled_size {
    int32_t denom;                       /* as given */
    int32_t width, height;               /* of the frame a decode writes: ceil(stored / denom), swapped for orientations 5..8 in APPLY mode */
    int32_t stored_width, stored_height; /* as rfd_jpeg_info reports them */
    int32_t orientation;                 /* the one that will be applied: the tag in APPLY mode, 1 in IGNORE mode */
    int32_t reserved[2];                 /* 0 */
};
/* 1 is the default; any other value than 1, 2, 4, 8: RFD_ERR_INVALID_ARG.  May be changed between calls. */
RFD_API int rfd_set_jpeg_scale(rfd_ctx *ctx, int denom);
/* Host only, no context, no device: the header validation of rfd_jpeg_info with the same statuses and messages, then the size of
 * the frame a decode with this denominator and this rfd_jpeg_orientation_mode writes.  A denominator or a mode outside their
 * sets: RFD_ERR_INVALID_ARG.  A refused file leaves *out untouched. */
RFD_API int rfd_jpeg_scaled_size(const uint8_t *bytes, size_t len, int denom, int orientation_mode, struct rfd_jpeg_scaled_size *out);
/* Test hook, host only: the `count` the host entropy decoder puts into each block's record at this denominator (csrc/jpeg_parse.h),
 * one byte per block in the block order and with the capacity convention of rfd_debug_jpeg_coefficients. */
RFD_API int rfd_debug_jpeg_block_counts(const uint8_t *bytes, size_t len, int denom, uint8_t *count, size_t cap_blocks, size_t *blocks);

/* ---- views: detection over overlapping views of a frame, merged on the device.  No counterpart in the reference, whose
 *      RetinaFaceDetection::call letterboxes one image (face_detection.rs:131-198): a 1080p frame is then read at 1/3 scale, a
 *      4K frame at 1/6, and a face below about 50 px (100 px) meets no anchor.  Opt-in: no other entry changes.
 *
 *      A VIEW is a rectangle of a frame that goes through the network as an image of its own: letterboxed to the network size
 *      like a frame, one slot of the network batch.  The views of a frame may overlap and may include the whole frame.  The
 *      candidates of all views of a frame are decoded into ONE list in frame pixels; one sort and one greedy NMS run per
 *      FRAME, and the result is an ordinary rfd_dets slab [n_frames][max_det] that rfd_select_faces, rfd_align_detections, the
 *      face list and the liveness entries take as it is.
 *
 *      The rule, per candidate of a view, in NETWORK pixels on the clipped box (x1, y1, x2, y2), m = edge_margin, new_w x new_h
 *      the letterboxed extent of the view: for every set bit of the view's `inner` the matching inequality must hold,
 *          left x1 >= m,  top y1 >= m,  right x2 <= (float)(new_w - 1) - m,  bottom y2 <= (float)(new_h - 1) - m,
 *      else the candidate is dropped (a comparison with a NaN is false).  A face cut by an inner tile edge is thus left to the
 *      neighbouring tile, or to the full view, where it is whole.  Then X = x / det_scale + (float)x_offset in f32 (one
 *      division, one addition, each rounded) for the four box and ten landmark coordinates; the score is untouched.
 *      Order: score descending, then the view's position v among its frame's views, then the anchor -- total, deterministic.
 *      NMS runs in frame pixels with the context's iou_threshold, so duplicates from different scales meet in one unit.
 *
 *      Argument rules.  views: host, sorted by frame; every view non-empty and inside its frame; 1 <= n_views <=
 *      max_batch_size; edge_margin >= 0 and finite; `inner` uses bits 0..3 only: else RFD_ERR_INVALID_ARG, and a view that
 *      letterboxes to an empty image refuses the call like such a frame does.  A frame with no view yields count 0.
 *      Capacity, both RFD_ERR_CAPACITY: n_frames * Vmax <= max_batch_size, Vmax the most views any frame of the call has (the
 *      merge works in the context's per-image buffers, a frame taking Vmax of them); and Vmax * anchors must fit the NMS
 *      kernel's LDS bitmap -- 18 views at 640x640.  A refused call enqueues nothing.
 *      Cost: from 17 409 candidate slots per frame up (two views at 640x640) the NMS is the one-workgroup-per-frame streaming
 *      form; the register and chunked forms stop there ("views").
 *
 *      edge_margin: rfd_view_config_default gives 4 network pixels.  That is a CHOSEN value, not tuned on data: this
 *      repository has no trained weights to tune it on. ---- */
typedef struct rfd_view {
    int32_t frame;  /* index into frames[] */
    int32_t x, y;   /* top-left corner in the frame, pixels */
    int32_t w, h;   /* extent, pixels */
    uint32_t inner; /* bit 0 left, 1 top, 2 right, 3 bottom: that side of the view lies inside the frame, not on its border */
} rfd_view;
typedef struct rfd_view_config {
    int32_t tile_w, tile_h; /* tile extent in frame pixels */
    int32_t overlap;        /* least overlap of neighbouring tiles, 0 <= overlap < tile_w, tile_h */
    int32_t full_view;      /* non-zero: the whole frame is the first view when there is more than one tile */
    float edge_margin;      /* network pixels; not used by the plan, carried for the detect calls */
} rfd_view_config;
/* tile = the network size (scale 1), overlap = net_w / 5, full_view = 1, edge_margin = 4.0f */
RFD_API void rfd_view_config_default(rfd_view_config *cfg, int net_w, int net_h);
/* The views of one frame, host only (no context, no device).  Per axis of extent W, tile t, overlap o: W <= t gives one tile
 * [0, W); else n = ceil((W - o) / (t - o)) tiles of extent t, tile i at floor(i * (W - t) / (n - 1)) -- the last ends at W,
 * neighbours overlap by at least o, every pixel is covered.  Order: the whole frame (inner 0) if full_view and more than one
 * tile, then the tiles row-major, `inner` from the geometry.  *count is always written; count > cap: RFD_ERR_CAPACITY, nothing
 * else written.  overlap outside [0, tile), a non-positive extent, frame < 0: RFD_ERR_INVALID_ARG, *count = 0. */
RFD_API int rfd_view_plan(int frame, int frame_w, int frame_h, const rfd_view_config *cfg, rfd_view *out, int cap, int *count);
/* frames[]: host array, `data` in DEVICE memory; out: DEVICE slabs [n_frames][max_det], total required.  Enqueued on the
 * context's stream; async as rfd_detect_batch_device (non-zero: no host wait; the overlap mode does not exist here). */
RFD_API int rfd_detect_views_batch_device(rfd_ctx *ctx, const rfd_image *frames, int n_frames, const rfd_view *views, int n_views,
                                          float edge_margin, rfd_dets *out, int async);
/* Host frames, host slabs, synchronous.  Each FRAME is copied to the device once; its views read that copy. */
RFD_API int rfd_detect_views_batch(rfd_ctx *ctx, const rfd_image *frames, int n_frames, const rfd_view *views, int n_views,
                                   float edge_margin, rfd_dets *out);
/* Stage-level: everything after the network on caller-supplied heads of n_views images (the contract of rfd_forward's
 * outputs), image i being view i.  Host pointers.  gidx (may be NULL) [n_frames][max_det] receives v * anchors + g of every
 * kept row, v the view's position among its frame's views and g the anchor.  The views' frames are not seen: "inside its
 * frame" is not checked here. */
RFD_API int rfd_decode_nms_views(rfd_ctx *ctx, const float *const heads[9], const rfd_view *views, int n_views, int n_frames,
                                 float edge_margin, rfd_dets *out, int32_t *gidx);

/* ---- tracker: faces followed over the frames of a video stream, on the device.  No counterpart in the reference, whose
 *      FacePipeline::extract sees one image.  A person in front of a door for four seconds is 100 detections at 25 fps; the
 *      remote models are the stage this library cannot speed up, so the tracker's job is to send them fewer faces: one when a
 *      track is new, another only when the shot has improved.  The state lives in HBM and an update runs in the context's
 *      stream order between detection and the face list, with no host wait.
 *
 *      An rfd_tracker belongs to ONE context (its device, its stream; same thread rule) and is destroyed BEFORE it.  It follows
 *      `streams` cameras, each with max_tracks slots {serial (0 = free), box[4], missed, hits, shot_q} and a next_serial that
 *      starts at 1.  A track's public name is (stream, serial): an int32, unique within its stream, never reused by a reset;
 *      after INT32_MAX the counter restarts at 1 (2^31 - 1 births of one camera: a track born then may share its serial with a
 *      live one of that age).
 *
 *      The rule, for one frame of stream s: an IoU tracker (Bochinski et al. 2017: no motion model, association by overlap with
 *      the last box) with the two score thresholds of ByteTrack (Zhang et al. 2022).  Rows i = 0 .. min(max(count, 0), max_det)
 *      - 1 of the frame's slab, in slab order; every operation is f32 in the written order.
 *      1. Eligibility: row i is eligible when score >= min_score (false for a NaN).  Other rows get track 0, flags 0.
 *      2. Association, for eligible rows in row order: among the stream's live slots not yet matched in this frame, the IoU of the
 *         row's box with the slot's box -- the NMS's arithmetic (nms.rs:39-54: the +1 convention, inter / (area_i + area_j -
 *         inter), one IEEE division).  Candidates are the slots with iou >= iou_min (false for a NaN).  The row takes the
 *         candidate of greatest IoU, equal IoUs going to the lowest slot: box = the row's box, missed = 0, hits += 1, the slot is
 *         matched and the row gets its serial.  A row with no candidate stays unmatched.
 *      3. Ageing: every live slot not matched in this frame gets missed += 1.
 *      4. Ending: a slot with missed > max_missed ends: its serial goes to the frame's `ended` list, in ascending slot order, and
 *         the slot is free.
 *      5. Birth, in row order: an unmatched eligible row with score >= new_score takes the lowest free slot (those freed in step
 *         4 count): serial = next_serial++, the row's box, missed 0, hits 1, shot_q = -inf; the row gets RFD_TRACK_NEW.  With no
 *         free slot the row gets track 0 and counts as dropped.  An unmatched eligible row below new_score gets track 0.
 *      6. Confirmation: a matched or born row gets RFD_TRACK_CONFIRMED when its slot has hits >= min_hits.
 *      7. DUE: q = quality[b][i] if a quality array was given, else the row's score.  A matched or born row is RFD_TRACK_DUE when
 *         its slot is confirmed and q > shot_q * improve (one multiplication, one comparison; any finite q passes -inf, a NaN q
 *         never passes); then shot_q = q.  DUE means "hand this face to the models".
 *      Frames of one stream within a call are consecutive in time, in call order; frames of different streams are independent.
 *      A frame with no detections still ages its stream: pass it with count = 0.  Splitting a sequence of frames into calls in
 *      any way gives the same outputs and the same state.  Nothing here is atomic or order-dependent: the same bits on every run.
 *
 *      Outputs, all caller-allocated; EVERY ROW AT OR PAST A FRAME'S COUNT IS LEFT EXACTLY AS THE CALLER PASSED IT (track and
 *      flags past the frame's rows, the due slab and due_track past due.count[b], ended past stats[b][2]).  No output may
 *      overlap an input or another output.
 *      The defaults (rfd_tracker_config_default) are CHOSEN values, not tuned on data: this repository has no trained weights.
 *      Errors: RFD_ERR_INVALID_ARG with the field named in rfd_last_error() for every bound in the config comments, a NULL
 *      required pointer, a half-set `due` slab or a stream outside [0, streams); RFD_ERR_CAPACITY for n > max_batch_size, and at
 *      creation for a context whose max_det exceeds RFD_TRACKER_MAX_DET (the per-row results of a frame live in LDS); n = 0 is a
 *      no-op; nothing is enqueued when a check fails. ---- */
#define RFD_TRACK_NEW 1u
#define RFD_TRACK_CONFIRMED 2u
#define RFD_TRACK_DUE 4u
#define RFD_TRACKER_MAX_DET 8192
typedef struct rfd_tracker rfd_tracker;
typedef struct rfd_tracker_config {
    int32_t streams;     /* cameras, 1..4096 */
    int32_t max_tracks;  /* slots per stream: 64, 128 or 256 */
    float   iou_min;     /* a detection may take a track when iou >= iou_min; finite, > 0 */
    int32_t max_missed;  /* >= 0: a track ends at the frame that leaves it unmatched more than max_missed frames running */
    float   min_score;   /* rows below take no part */
    float   new_score;   /* an unmatched row starts a track when score >= new_score; new_score >= min_score */
    int32_t min_hits;    /* >= 1: a track is confirmed from its min_hits-th matched frame on (its birth counts) */
    float   improve;     /* >= 1, finite: see DUE */
    int32_t reserved[4];
} rfd_tracker_config;   /* default: 1, 64, 0.3, 5, ctx confidence threshold, the same, 2, 1.1 */
typedef struct rfd_track_out {
    int32_t  *track;     /* [n][max_det]  serial, 0 = none */
    uint32_t *flags;     /* [n][max_det]  RFD_TRACK_NEW 1, RFD_TRACK_CONFIRMED 2, RFD_TRACK_DUE 4 */
    int32_t  *stats;     /* [n][4] matched, born, ended, dropped; may be NULL */
    int32_t  *ended;     /* [n][max_tracks]; the first stats[b][2] entries are written; may be NULL */
    rfd_dets  due;       /* boxes/landmarks/count all NULL, or all set (total optional): the DUE rows of frame b, in row order */
    int32_t  *due_track; /* [n][max_det] serial of each due row; may be NULL */
} rfd_track_out;
typedef struct rfd_track {
    int32_t slot, serial;
    float   box[4];
    int32_t missed, hits;
    float   shot_q;
} rfd_track;
/* ctx NULL: the confidence threshold of rfd_config_default */
RFD_API int rfd_tracker_config_default(const rfd_ctx *ctx, rfd_tracker_config *cfg);
RFD_API int rfd_tracker_create(rfd_ctx *ctx, const rfd_tracker_config *cfg /* NULL: the default */, rfd_tracker **out);
RFD_API void rfd_tracker_destroy(rfd_tracker *t);
/* stream: host [n], the camera of each frame; dets: DEVICE slabs of n frames as rfd_detect_batch_device leaves them (boxes,
 * landmarks, count; total is not read); quality: DEVICE [n][max_det] or NULL; every pointer of `out`: DEVICE.  Enqueued on the
 * context's stream with no host wait (the stream list travels through a ring of page-locked slots); async = 0 returns after
 * the stream has drained, any other value at once.  n <= max_batch_size. */
RFD_API int rfd_tracker_update_device(rfd_tracker *t, const int32_t *stream, const rfd_dets *dets, const float *quality, int n,
                                      const rfd_track_out *out, int async);
/* Stage-level: the same with host pointers, through the same kernel; synchronous.  The output arrays travel to the device
 * and back whole, so what they held past the counts comes back as it was. */
RFD_API int rfd_tracker_update(rfd_tracker *t, const int32_t *stream, const rfd_dets *dets, const float *quality, int n,
                               const rfd_track_out *out);
/* The tracks of `stream` (-1: of all streams) vanish without an `ended` entry; next_serial is kept, so a serial is never
 * reused.  Enqueued in stream order, no host wait. */
RFD_API int rfd_tracker_reset(rfd_tracker *t, int stream);
/* The live slots of `stream` in ascending slot order: at most cap of them into out (may be NULL when cap is 0); *count = how
 * many there are, also when that exceeds cap.  Waits for the stream. */
RFD_API int rfd_tracker_get_tracks(rfd_tracker *t, int stream, rfd_track *out, int cap, int *count);
/* The device-resident form of rfd_align_detections (conventions of rfd_detect_all_faces_device, without its detection): every
 * imgs[i].data, every pointer of `dets` and of `out` is DEVICE memory.  The list, alignment and tensors are enqueued on the
 * context's stream; async = 0 returns after the stream has drained.  With the tracker's `due` slab as `dets`: detect -> track
 * -> align the due faces -> models -> gallery, in one stream order. */
RFD_API int rfd_align_detections_device(rfd_ctx *ctx, const rfd_image *imgs, int n, const rfd_dets *dets,
                                        const rfd_face_list_config *list_cfg, const rfd_alignment_config *align_cfg,
                                        const rfd_face_tensor_config *cfgs, int k, int cap, rfd_face_list *out, int async);

/* ---- track identities: the gallery's answer brought back to the track, on the device.  No counterpart in the reference, which
 *      sees one image.  The tracker hands out (stream, serial) and DUE; every due shot is embedded by the remote models and
 *      searched in the gallery.  Without this section each shot is searched on its own, and a detection row can only be selected
 *      "by person" after a host round trip that joins track, due_track and the search results by serial.  With it a track keeps
 *        - a TEMPLATE: the weighted sum of the normalised embeddings of its shots, so the gallery is asked once per shot with
 *          everything known about the track;
 *        - a NAME: the identity the gallery gave the fused template, under a two-threshold rule;
 *      and every detection row of every frame, the 24 of 25 per second that are not DUE included, gets an ANSWER in the shape
 *      rfd_redact_faces_device takes as `sel`:
 *        detect -> shot quality -> track -> align the due faces -> (models) -> fuse -> gallery search -> label -> who -> redact
 *      is one stream order with no host wait.
 *
 *      State.  rfd_tracker_identity_enable allocates, once per tracker, [streams][max_tracks] entries {serial, identity, row,
 *      score, named, shots, weight} and a template S[dim] f32 each, all zero.  Entry j of stream s belongs to the track in slot
 *      j ONLY WHILE entry.serial == slot.serial.  Serials are not reused (tracker section), so an entry whose serial differs is
 *      STALE: it belongs to a track that has ended, and it is cleared the first time the slot's new track is fused.  Hence the
 *      tracker's update kernel, its slots, rfd_tracker_config, rfd_track_out and rfd_track are untouched by this section, and
 *      rfd_tracker_reset needs no change either: the tracks it removes take their serials with them, and whatever is born in
 *      their slots finds a stale entry.  A tracker that never enables identities launches and allocates what it always did.
 *
 *      The observations of a call (rfd_track_obs) are described the way the pipeline already holds them: the face list's total,
 *      first and row, and the tracker's due_track as `serial`.  count = total ? min(max(total[0], 0), m) : m.  Frame b owns the
 *      observations t in [max(first[b], 0), min(first[b + 1], count)); observation t of frame b is the track (stream[b],
 *      serial[b][row[t]]).  The track is looked up by its serial among the stream's slots AT THE TIME THE KERNEL RUNS (the lowest
 *      slot that holds it): the models are remote, so embeddings may arrive several updates late.  A track that has ended since,
 *      a serial 0 or a row outside [0, max_det) is "no track": a status, not an error.  The observations of one stream are
 *      processed in the call order of its frames and in ascending t within a frame; the face list is in (frame, row) order, so
 *      that is ascending t and their order in time.  Streams are independent.  `stream` is a host array [n] that travels through
 *      the tracker's ring of page-locked slots, so no call waits for the context's stream.
 *
 *      1. Fuse (rfd_tracker_fuse_device).  emb [m][dim] f32, the ID model's raw output; weight [m] f32 or NULL for 1.0f (the
 *         natural source: the score array of rfd_quality_decide_device); query [m][dim] f32 and status [m] int32 are written.
 *         For observation t, every operation f32 in the written order:
 *         a. Normalise: e = emb[t] / |emb[t]| in the order of rfd_normalize_embeddings: lane l of 64 sums the squares of elements
 *            l, l + 64, ... in ascending order starting from 0 (a lane that owns no element holds 0), the 64 partial sums meet
 *            in the xor butterfly 32, 16, 8, 4, 2, 1 (s = s + partner's s), one sqrt, one division per element, every one an
 *            IEEE operation rounded to nearest: e has the bits of rfd_normalize_embeddings.
 *         b. Bad input: the norm is zero or not finite, or w is not (finite and > 0): status 2 (RFD_TRACK_FUSE_BAD_INPUT),
 *            query[t] = e as computed, no state changes.
 *         c. No track: status 1 (RFD_TRACK_FUSE_NO_TRACK), query[t] = e, no state changes.
 *         d. Fuse: a stale entry is cleared first (S = 0, shots = 0, weight = 0, unnamed: identity -1, row -1, score -inf,
 *            named 0; serial = the track's).  Then S[i] = S[i] + w * e[i]: one multiplication, one addition, no fma.  shots += 1,
 *            weight = weight + w.  query[t] = S normalised by the rule of (a).  Status 0 (RFD_TRACK_FUSE_OK); when the norm of S
 *            is not finite, status 3 (RFD_TRACK_FUSE_OVERFLOW): the state is kept as fused and query[t] is as computed.
 *         query and status at or past the count stay as passed.  Splitting the observations of a stream over calls in any way
 *         that keeps their order gives the same bits.
 *      2. Label (rfd_tracker_label_device).  scores, rows, ids [m][k], k in 1..32, as rfd_gallery_search_identities_device (or
 *         _filtered_device) wrote them for `query`; ids may be NULL (a plain search: every identity reads -1).  status_in is the
 *         fuse call's status: observations with a non-zero status are skipped, and so are those whose track is "no track" or
 *         whose entry is stale.  The same groups and order as the fuse call.  For observation t and its entry:
 *           top = entry 0 of t; it is EMPTY when rows[t][0] == -1 or scores[t][0] is NaN.  The runner-up is entry 1 when k >= 2,
 *           empty by the same rule.
 *           A named entry (identity X, row R) KEEPS its name iff top is non-empty, names the same person (ids[t][0] == X when
 *           X >= 0; rows[t][0] == R for an unlabelled gallery row, X = -1) and top.score >= release; then score = top.score and
 *           row = rows[t][0].
 *           Otherwise, and for an unnamed entry: the entry TAKES top as its name (named 1, identity, row, score of top) iff top
 *           is non-empty, top.score >= accept, and there is no non-empty runner-up or top.score - runner.score >= margin (one
 *           subtraction, one comparison).  If not, it is or becomes unnamed: named 0, identity -1, row -1, score -inf.
 *         A later observation of the same track in the same call supersedes the earlier one: its query held more evidence.
 *      3. Who (rfd_tracker_who_device), for every detection row of the n frames.  track [n][max_det] as rfd_track_out.track,
 *         count [n].  Row i < min(max(count[b], 0), max_det) gets who[b][i] = (flags_in ? flags_in[b][i] : 0) | (named ?
 *         RFD_TRACK_NAMED : 0), where "named" is: track[b][i] != 0, a slot of stream[b] holds that serial, its entry is not stale
 *         and is named.  identity[b][i] and id_score[b][i] (each may be NULL) get the entry's values then, -1 and -inf otherwise.
 *         who may be flags_in itself; no other overlap is allowed.  Rows at or past the count stay as passed.
 *         "Redact everyone the gallery did not name" is rfd_redact_faces_device with sel = who, sel_mask = RFD_TRACK_NAMED,
 *         sel_value = 0; "confirmed and unnamed" is sel_mask = RFD_TRACK_CONFIRMED | RFD_TRACK_NAMED, sel_value =
 *         RFD_TRACK_CONFIRMED.  A watch-list deployment searches with rfd_gallery_search_filtered_device restricted to the
 *         list's tag, so that "named" means "on the list".
 *
 *      The defaults (rfd_track_identity_config_default: dim 512, accept 0.5, release 0.4, margin 0.05) are CHOSEN values, not
 *      tuned on data: this repository has no trained weights.
 *      Errors: RFD_ERR_INVALID_ARG with the field named in rfd_last_error() for every bound in the config comments, for enabling
 *      twice, a NULL required pointer, m < 0, k outside 1..32, a stream outside [0, streams), and for every call of this section
 *      on a tracker without identities enabled; RFD_ERR_CAPACITY for a state above 1 GiB (streams * max_tracks * dim * 4) and
 *      for n > max_batch_size.  n = 0 or m = 0 is a no-op; nothing is enqueued when a check fails.  Nothing here is atomic or
 *      order-dependent: the same bits on every run.
 *      Out of scope: saving the state to a file, cross-camera linking, a decay of old shots, and any change to DUE.  (The
 *      identity of a track at the moment it ends is in its record: "track shots" below.) ---- */
#define RFD_TRACK_NAMED 8u
#define RFD_TRACK_FUSE_OK 0
#define RFD_TRACK_FUSE_NO_TRACK 1
#define RFD_TRACK_FUSE_BAD_INPUT 2
#define RFD_TRACK_FUSE_OVERFLOW 3
typedef struct rfd_track_identity_config {
    int32_t dim;      /* the gallery's: a multiple of 32, 32..1024 */
    float   accept;   /* an unnamed track takes a name when top score >= accept; finite */
    float   release;  /* a named track keeps it while the same identity scores >= release; finite, release <= accept */
    float   margin;   /* >= 0, finite: with k >= 2 and a non-empty runner-up, top - runner_up >= margin is also required to take a name */
    int32_t reserved[4];
} rfd_track_identity_config;   /* default: 512, 0.5, 0.4, 0.05 */
typedef struct rfd_track_obs {
    const int32_t *total;   /* [1] or NULL; observations t >= min(max(total[0],0), m) are skipped   (rfd_face_list.total) */
    const int32_t *first;   /* [n+1]: frame b owns t in [first[b], first[b+1])                     (rfd_face_list.first) */
    const int32_t *row;     /* [m]: row of t in its frame's slab                                   (rfd_face_list.row)   */
    const int32_t *serial;  /* [n][max_det]: the track of each slab row                            (rfd_track_out.due_track) */
} rfd_track_obs;
typedef struct rfd_track_identity {
    int32_t slot, serial;
    int32_t identity, row;  /* of the gallery; -1, -1 while unnamed */
    float   score;          /* -inf while unnamed */
    int32_t named, shots;
    float   weight;
} rfd_track_identity;
RFD_API int rfd_track_identity_config_default(rfd_track_identity_config *cfg);
/* cfg NULL: the default.  Once per tracker; the fill of the state is enqueued in stream order. */
RFD_API int rfd_tracker_identity_enable(rfd_tracker *t, const rfd_track_identity_config *cfg);
/* stream: host [n]; every pointer of obs, emb, weight, query, status: DEVICE.  Enqueued on the context's stream with no host
 * wait; async = 0 returns after the stream has drained, any other value at once. */
RFD_API int rfd_tracker_fuse_device(rfd_tracker *t, const int32_t *stream, int n, const rfd_track_obs *obs, int m, const float *emb,
                                    const float *weight, float *query, int32_t *status, int async);
RFD_API int rfd_tracker_label_device(rfd_tracker *t, const int32_t *stream, int n, const rfd_track_obs *obs, int m, int k,
                                     const float *scores, const int32_t *rows, const int32_t *ids, const int32_t *status_in, int async);
RFD_API int rfd_tracker_who_device(rfd_tracker *t, const int32_t *stream, int n, const int32_t *track, const int32_t *count,
                                   const uint32_t *flags_in, uint32_t *who, int32_t *identity, float *id_score, int async);
/* Stage-level: the same with host pointers, through the same kernels; synchronous.  The output arrays travel to the device
 * and back whole, so what they held past the counts comes back as it was. */
RFD_API int rfd_tracker_fuse(rfd_tracker *t, const int32_t *stream, int n, const rfd_track_obs *obs, int m, const float *emb,
                             const float *weight, float *query, int32_t *status);
RFD_API int rfd_tracker_label(rfd_tracker *t, const int32_t *stream, int n, const rfd_track_obs *obs, int m, int k, const float *scores,
                              const int32_t *rows, const int32_t *ids, const int32_t *status_in);
RFD_API int rfd_tracker_who(rfd_tracker *t, const int32_t *stream, int n, const int32_t *track, const int32_t *count,
                            const uint32_t *flags_in, uint32_t *who, int32_t *identity, float *id_score);
/* The entries of the live slots of `stream` that are not stale, in ascending slot order: at most cap of them into out (may be
 * NULL when cap is 0); *count = how many there are, also when that exceeds cap.  Waits for the stream. */
RFD_API int rfd_tracker_get_identities(rfd_tracker *t, int stream, rfd_track_identity *out, int cap, int *count);
/* The template S[dim] of the live track `serial` of `stream`; RFD_ERR_INVALID_ARG ("no such track") when no live slot holds
 * that serial or its entry is stale.  Waits for the stream. */
RFD_API int rfd_tracker_get_template(rfd_tracker *t, int stream, int32_t serial, float *out);

/* ---- track shots: the best aligned crop of every track kept on the device, and ended tracks listed as records.  No counterpart
 *      in the reference, which sees one image.  The product of a door camera is one record per visit: who it was, when, and the
 *      best picture as a JPEG file.  The aligned crop of a due face lives in rfd_face_list.crops for one call, and a track that
 *      ends leaves only its serial in `ended`; without this section a caller copies every due crop to the host on every call and
 *      joins crops, due_track and ended by (stream, serial) there.  With it
 *        detect -> shot quality -> track -> COLLECT -> align the due faces -> KEEP -> (models) -> fuse -> search -> label -> who
 *        -> redact -> rfd_encode_jpeg_batch_device of the records' crops
 *      is one stream order with a single wait at the end: rfd_track_records.crops is laid out as the encoder's crops are and
 *      rfd_track_records.total is a ready count_dev.
 *
 *      State.  rfd_tracker_shots_enable allocates, once per tracker, [streams][max_tracks] heads {serial, shots, kept, q,
 *      first_stamp, best_stamp} (32 bytes, all zero) and one crop of crop_w * crop_h * 3 bytes beside each.  Entry j of stream s
 *      belongs to the track in slot j ONLY WHILE head.serial == slot.serial; otherwise it is STALE, exactly as for the track
 *      identities, and it is cleared the first time a shot of the slot's new track is kept.  Hence the tracker's update kernel,
 *      its slots, rfd_tracker_config, rfd_track_out and rfd_track are untouched by this section, and rfd_tracker_reset needs no
 *      change either: the tracks it removes take their serials with them (and get no record: they have no `ended` entry).  A
 *      tracker that never enables shots launches and allocates what it always did.  `stream` and `stamp` are host arrays [n]
 *      that travel through a ring of page-locked slots owned by this state, so the tracker's own ring stays as it is and no call
 *      waits for the context's stream.  stamp[b] is the caller's time of frame b, any int64 (NULL: 0 for every frame); it is
 *      stored and handed back, never interpreted.
 *
 *      1. Keep (rfd_tracker_keep_shots_device).  The observations are rfd_track_obs, and the count, the ownership of
 *         observations by frames, the lookup of the track, the groups and the order are the fuse call's, word for word: count =
 *         total ? min(max(total[0], 0), m) : m; frame b owns t in [max(first[b], 0), min(first[b + 1], count)); observation t of
 *         frame b is the track (stream[b], serial[b][row[t]]), found by its serial among the stream's slots AT THE TIME THE
 *         KERNEL RUNS, at the lowest slot that holds it.  A track that has ended, serial 0 or a row outside [0, max_det) is "no
 *         track".  The observations of one stream are processed in the call order of its frames and in ascending t within a
 *         frame; streams are independent.  crops [m][crop_h][crop_w][3] u8 (rfd_face_list.crops, any byte address);
 *         face_status [m] int32 or NULL (rfd_face_list.status); q [m] f32 or NULL; status [m] int32 is written.  The natural
 *         sources of q: the score array of rfd_quality_decide_device (the remote quality model), as for `weight` in fuse; or
 *         NULL, since by the tracker's DUE rule every later due shot already beat the last one by `improve`.
 *         For observation t of frame b:
 *         a. face_status given and face_status[t] < 0 (the alignment zero-filled the crop), or q given and q[t] is NaN: status 2
 *            (RFD_TRACK_SHOT_BAD_INPUT), nothing changes.
 *         b. No track: status 1 (RFD_TRACK_SHOT_NO_TRACK), nothing changes.
 *         c. A stale entry is cleared first: serial = the track's, shots 0, kept 0, q -inf, first_stamp = stamp[b], best_stamp 0.
 *         d. shots += 1.  The shot is KEPT if and only if kept == 0, or q is NULL, or q[t] > head.q (one f32 comparison: an equal
 *            q keeps the earlier shot).  If kept: crop t becomes the entry's crop, head.q = q ? q[t] : 0.0f, best_stamp =
 *            stamp[b], kept += 1, status 0 (RFD_TRACK_SHOT_KEPT).  Otherwise status 3 (RFD_TRACK_SHOT_PASSED).
 *         A later kept observation of the same track in the same call supersedes the earlier one; both get status 0.  Splitting
 *         the observations of a stream over calls in any way that keeps their order gives the same state, byte for byte.  status
 *         at or past the count stays as passed.
 *      2. Collect (rfd_tracker_collect_ended_device).  stats [n][4] and ended [n][max_tracks] as rfd_track_out holds them.  For
 *         frame b in the call order of frames, then entries e = 0 .. min(max(stats[b][2], 0), max_tracks) - 1 of ended[b] in
 *         order: the serial ended[b][e] is looked up among the HEADS of stream[b] (the lowest j with head.serial == serial; serial
 *         0 never matches) -- the slot no longer holds the track, so the lookup cannot go through the slots.  If found it is a
 *         record; if not, the entry is skipped and no record is written (the track never had a kept shot, or its entry was
 *         already taken by a later track because the call came too late).  c[b] is the number of records of frame b; first[b] =
 *         c[0] + .. + c[b-1], first[n] = total[0], both untruncated, as in the face list.  Records r >= cap are dropped.  EVERY
 *         rec AND crops ROW AT OR PAST min(total, cap) IS LEFT EXACTLY AS PASSED.  Record r holds the head's fields (serial,
 *         shots, kept, q, first_stamp, best_stamp), stream = stream[b], frame = b, end_stamp = stamp[b], reserved = 0, and the
 *         stored crop in crops[r] (unless crops is NULL).  If identities are enabled and a head of the identity state of
 *         stream[b] holds the same serial (the lowest such j), the record has that head's identity, row, score, named, shots and
 *         weight as identity, row, id_score, named, id_shots, id_weight; otherwise -1, -1, -inf, 0, 0, 0.  Collect reads the
 *         state and changes nothing in it.
 *         WHERE THE CALL BELONGS: directly behind the rfd_tracker_update_device whose `ended` it reads, BEFORE that call's align
 *         -> keep -> fuse.  Two consequences: a slot reborn in the same frame still yields its old track's record (the new
 *         track's first keep, which clears the entry, comes later); and a track whose only due shot arrives after it ended has
 *         none (that keep is "no track").
 *      3. Readers, both waiting for the stream: rfd_tracker_get_shots lists the entries of the live slots that are not stale;
 *         rfd_tracker_get_shot_crop copies the stored crop of a live track.
 *
 *      Errors: RFD_ERR_INVALID_ARG with the field named in rfd_last_error() for every bound in the config comments, a non-zero
 *      reserved, enabling twice, a NULL required pointer, m < 0, cap < 1, a stream outside [0, streams), and for every call of
 *      this section on a tracker without shots enabled; RFD_ERR_CAPACITY for a bank above 1 GiB (streams * max_tracks * crop_w
 *      * crop_h * 3) and for n > max_batch_size.  n = 0 is a no-op, and so is m = 0 for keep; nothing is enqueued when a check
 *      fails.  Nothing here is atomic or order-dependent: the same bytes on every run.
 *      Out of scope: any change to the tracker's update or to DUE, saving the bank to a file, a device-side peek at the crops
 *      of live tracks (the two readers wait for the stream), source-frame context around the face (encode a rectangle of the
 *      frame for that), and cross-camera linking. ---- */
#define RFD_TRACK_SHOT_KEPT 0      /* the crop is now the track's stored shot */
#define RFD_TRACK_SHOT_NO_TRACK 1
#define RFD_TRACK_SHOT_BAD_INPUT 2
#define RFD_TRACK_SHOT_PASSED 3    /* a valid shot, not better than the stored one */
typedef struct rfd_track_shot_config {
    int32_t crop_w, crop_h;   /* 1..1024 each: rfd_alignment_config.out_w / out_h of the crops that will be kept */
    int32_t reserved[6];      /* 0 */
} rfd_track_shot_config;      /* 32 bytes; default 112, 112 */
typedef struct rfd_track_shot {      /* 40 bytes */
    int32_t slot, serial;
    int32_t shots, kept;             /* valid observations seen; times the stored crop was replaced */
    float   q;
    int32_t reserved;
    int64_t first_stamp, best_stamp;
} rfd_track_shot;
typedef struct rfd_track_record {    /* 80 bytes */
    int32_t stream, serial, frame;   /* frame: index b of the call's frame whose update ended the track */
    int32_t shots, kept;
    float   q;
    int64_t first_stamp, best_stamp, end_stamp;
    int32_t identity, row;
    float   id_score;
    int32_t named, id_shots;
    float   id_weight;
    int32_t reserved[2];             /* written as 0 */
} rfd_track_record;
typedef struct rfd_track_records {
    int32_t *total;          /* [1]   untruncated number of records */
    int32_t *first;          /* [n+1] records of frame b are [first[b], first[b+1]) */
    rfd_track_record *rec;   /* [cap] */
    uint8_t *crops;          /* [cap][crop_h][crop_w][3], may be NULL */
} rfd_track_records;
RFD_API int rfd_track_shot_config_default(rfd_track_shot_config *cfg);
/* cfg NULL: the default.  Once per tracker; the fill of the heads is enqueued in stream order. */
RFD_API int rfd_tracker_shots_enable(rfd_tracker *t, const rfd_track_shot_config *cfg);
/* stream: host [n]; stamp: host int64 [n] or NULL; every pointer of obs, crops, face_status, q, status: DEVICE.  Enqueued on the
 * context's stream with no host wait; async = 0 returns after the stream has drained, any other value at once. */
RFD_API int rfd_tracker_keep_shots_device(rfd_tracker *t, const int32_t *stream, const int64_t *stamp, int n, const rfd_track_obs *obs, int m,
                                          const uint8_t *crops, const int32_t *face_status, const float *q, int32_t *status, int async);
/* stats, ended and every pointer of out: DEVICE; total, first and rec are required. */
RFD_API int rfd_tracker_collect_ended_device(rfd_tracker *t, const int32_t *stream, const int64_t *stamp, int n, const int32_t *stats,
                                             const int32_t *ended, int cap, const rfd_track_records *out, int async);
/* Stage-level: the same with host pointers, through the same kernels; synchronous.  The output arrays travel to the device
 * and back whole, so what they held past the counts comes back as it was. */
RFD_API int rfd_tracker_keep_shots(rfd_tracker *t, const int32_t *stream, const int64_t *stamp, int n, const rfd_track_obs *obs, int m,
                                   const uint8_t *crops, const int32_t *face_status, const float *q, int32_t *status);
RFD_API int rfd_tracker_collect_ended(rfd_tracker *t, const int32_t *stream, const int64_t *stamp, int n, const int32_t *stats,
                                      const int32_t *ended, int cap, const rfd_track_records *out);
/* The entries of the live slots of `stream` that are not stale, in ascending slot order: at most cap of them into out (may be
 * NULL when cap is 0); *count = how many there are, also when that exceeds cap.  Waits for the stream. */
RFD_API int rfd_tracker_get_shots(rfd_tracker *t, int stream, rfd_track_shot *out, int cap, int *count);
/* The stored crop [crop_h][crop_w][3] of the live track `serial` of `stream`; RFD_ERR_INVALID_ARG ("no such track") when no live
 * slot holds that serial or its entry is stale.  Waits for the stream. */
RFD_API int rfd_tracker_get_shot_crop(rfd_tracker *t, int stream, int32_t serial, uint8_t *out);

/* ---- shot quality: a figure of merit in [0, 1] for every detection row, on the device, from the pixels under its box and its
 *      landmarks.  No counterpart in the reference.  It fills the quality[n][max_det] array that rfd_tracker_update_device reads,
 *      so that the tracker's DUE rule ("a better shot") compares sharpness, pose, exposure and size instead of the detector's
 *      score: detect -> quality -> track -> align the due faces -> models -> gallery is one stream order with no host wait.
 *
 *      The measure, for frame b (H x W, BGR u8, byte stride) and row i < min(max(count[b], 0), max_det); box row x1, y1, x2, y2,
 *      score; landmark row left eye (lx, ly), right eye (rx, ry), nose (nx, ny), left mouth (mlx, mly), right mouth (mrx, mry).
 *      Every step is integer, or one IEEE f32 / f64 operation in the written order with no contraction; as_i32(f) truncates
 *      toward zero, saturates at the int32 ends and maps a NaN to 0.
 *      Region.   X0 = max(as_i32(x1), 0), Y0 = max(as_i32(y1), 0), X1 = min(as_i32(x2), W - 1), Y1 = min(as_i32(y2), H - 1);
 *                w = X1 - X0 + 1, h = Y1 - Y0 + 1 as int64.  If w < 32 or h < 32 the row is UNMEASURED: status 1, sharp = mean =
 *                expo = 0 and q = +0 whatever the score; its landmark parts and its size are still computed.  Otherwise status 0.
 *      Cells.    A 32 x 32 grid over the region: column edges cx[k] = X0 + (k * w) / 32, row edges cy[k] = Y0 + (k * h) / 32,
 *                k = 0 .. 32, integer division; cell (r, c) holds the pixels cy[r] <= y < cy[r + 1], cx[c] <= x < cx[c + 1] (never
 *                empty).  Grey of a pixel: (B * 1868 + G * 9617 + R * 4899 + 8192) >> 14 (OpenCV's fixed-point BGR2GRAY).  Cell
 *                mean in 8.4 fixed point: m = (16 * S + cnt / 2) / cnt, S the cell's grey sum, cnt its pixel count; 0 .. 4080.
 *      Sharp.    Over the 30 x 30 interior cells L = 4 m[r][c] - m[r-1][c] - m[r+1][c] - m[r][c-1] - m[r][c+1]; A1 = sum L (int32),
 *                A2 = sum L * L (int64), V = 900 * A2 - A1 * A1 (int64, 0 <= V < 2^53); sharp = (f32)((f64)V / 207360000.0): the
 *                variance of the Laplacian of the face normalised to 32 x 32, in grey levels squared.
 *      Exposure. mean = (f32)((f64)(sum of the 1024 m) / 16384.0); n_lo = cells with m <= 16 * dark, n_hi = cells with m >= 16 *
 *                bright; expo = 1 - (f32)(n_lo + n_hi) / 1024.
 *      Pose.     d = rx - lx; ey = (ly + ry) * 0.5; my = (mly + mry) * 0.5; v = my - ey.  If !(d > 0) or !(v > 0) (a NaN fails
 *                either) pose = yaw = roll = pitch = 0.  Otherwise yaw = |(nx - lx) - (rx - nx)| / d, roll = |ry - ly| / d, pitch =
 *                |(ny - ey) / v - pitch0|, t = (yaw * w_yaw + roll * w_roll) + pitch * w_pitch, pose = t < 1 ? 1 - t : 0 (0 for a
 *                NaN t).
 *      Size.     size = (f32)min(w, h) (from int64; it may be zero or negative for a box outside the frame).
 *      Quality.  a = times_score ? score * pose : pose; q = ((a * min(sharp / sharp_ref, 1)) * min(size / size_ref, 1)) * expo,
 *                min(x, 1) = x < 1 ? x : 1.  A NaN score with times_score gives a NaN q, which the tracker never marks DUE.
 *      A NaN yaw, roll, pitch or q is stored as the quiet NaN 0x7FC00000, so every output bit is defined by the above.
 *      parts[8] of a row: sharp, mean, expo, yaw, roll, pitch, pose, size.
 *
 *      EVERY ROW AT OR PAST A FRAME'S COUNT IS LEFT EXACTLY AS THE CALLER PASSED IT, in quality, parts and status.
 *      The defaults (rfd_shot_quality_config_default) are CHOSEN values, not tuned on data: this repository has no trained weights
 *      and no labelled shots.  One workgroup reads a whole region, so a face that fills a 1080p frame is 6 MB through one CU.
 *      Errors: RFD_ERR_INVALID_ARG with the field named in rfd_last_error() for every bound in the config comments, for a NULL
 *      required pointer (ctx, imgs, dets and its boxes / landmarks / count, quality), for a frame with a NULL data pointer, a
 *      non-positive size, a side above RFD_SHOT_QUALITY_MAX_SIDE (the cell sums are int32) or a stride below 3 * width;
 *      RFD_ERR_CAPACITY for n > max_batch_size; n = 0 is a no-op; nothing is enqueued when a check fails. ---- */
#define RFD_SHOT_QUALITY_MAX_SIDE 32768
#define RFD_SHOT_QUALITY_PARTS 8
typedef struct rfd_shot_quality_config {
    int32_t dark;         /* 0..255, dark < bright: a cell with m <= 16 * dark is under-exposed */
    int32_t bright;       /* 0..255: a cell with m >= 16 * bright is over-exposed */
    float   pitch0;       /* finite: (ny - ey) / v of a frontal face */
    float   w_yaw;        /* finite, >= 0 */
    float   w_roll;       /* finite, >= 0 */
    float   w_pitch;      /* finite, >= 0 */
    float   sharp_ref;    /* finite, > 0: the sharpness from which a face counts as sharp */
    float   size_ref;     /* finite, > 0: the side in pixels from which a face counts as large */
    int32_t times_score;  /* 0 or 1 */
    int32_t reserved[4];
} rfd_shot_quality_config; /* default: 30, 225, 0.495 (the nose of the 112 x 112 alignment template), 1, 1, 2, 64, 112, 0 */
RFD_API int rfd_shot_quality_config_default(rfd_shot_quality_config *cfg);
/* imgs[] and cfg: host memory; every imgs[i].data, every pointer of `dets` (boxes, landmarks, count; total is not read) and
 * every output: DEVICE memory.  The counts are read on the device.  Enqueued on the context's stream, one launch, no host wait
 * (the frame descriptors travel through a ring of page-locked slots); async = 0 returns after the stream has drained, any other
 * value at once.  parts and status may be NULL. */
RFD_API int rfd_shot_quality_device(rfd_ctx *ctx, const rfd_image *imgs, int n, const rfd_dets *dets,
                                    const rfd_shot_quality_config *cfg /* NULL: the default */, float *quality /* [n][max_det] */,
                                    float *parts /* [n][max_det][8] or NULL */, int32_t *status /* [n][max_det] or NULL */, int async);
/* Stage-level: the same with host pointers (frames included), through the same kernel; synchronous.  The output arrays travel
 * to the device and back whole, so what they held past the counts comes back as it was. */
RFD_API int rfd_shot_quality(rfd_ctx *ctx, const rfd_image *imgs, int n, const rfd_dets *dets, const rfd_shot_quality_config *cfg,
                             float *quality, float *parts, int32_t *status);

/* ---- frames in camera and decoder formats: what a stream hands out -- NV12 or I420 from a video decoder, YUYV from a V4L2 or USB
 *      camera, BGRA from a screen or compositor surface -- converted on the device into the packed BGR frames every other entry
 *      point reads.  In the reference this is the channel handling of byte_data_to_opencv (src/utils/utils.rs:26-49): the fourth
 *      channel of a 4-channel Mat is dropped (utils.rs:29), a grey one is expanded.  It has no counterpart for the YUV formats.
 *      Uploading the planes (rfd_upload_frames_device) moves 1.5 bytes per pixel of NV12 over PCIe where a BGR frame is 3.
 *
 *      Layouts, for a frame of W x H pixels (rfd_frame_layout_of answers the same); every plane has its own byte stride >= the
 *      bytes of its rows; odd W and H are legal, cw = ceil(W / 2), ch = ceil(H / 2):
 *        BGR, RGB      1 plane  [H][W][3]
 *        BGRA, RGBA    1 plane  [H][W][4], the fourth byte is dropped whatever it holds
 *        GRAY          1 plane  [H][W], B = G = R = Y, bytes unchanged (no range expansion)
 *        NV12, NV21    2 planes Y [H][W]; chroma [ch][2 * cw], interleaved U V (NV12) or V U (NV21)
 *        I420          3 planes Y [H][W]; U [ch][cw]; V [ch][cw]
 *        YUYV, UYVY    1 plane  [H][4 * cw]: Y0 U Y1 V (YUYV) or U Y0 V Y1 (UYVY) per pair of pixels
 *      A chroma sample serves its 2 x 2 (NV12, NV21, I420) or 2 x 1 (YUYV, UYVY) luma samples UNFILTERED: pixel (x, y) takes the
 *      chroma of column x >> 1 (and row y >> 1).  In an odd-width YUYV / UYVY row the second luma byte of the last pair is not used.
 *
 *      The arithmetic of the YUV formats, with u = U - 128, v = V - 128, y = limited ? max(Y - 16, 0) : Y, everything int32,
 *      >> arithmetic (a floor), clamp255 to 0 .. 255:
 *        R = clamp255((CY * y + CVR * v           + 524288) >> 20)
 *        G = clamp255((CY * y + CUG * u + CVG * v + 524288) >> 20)
 *        B = clamp255((CY * y + CUB * u           + 524288) >> 20)
 *                              CY       CVR      CUG      CVG      CUB    the real coefficients x 2^20, rounded
 *        BT601_LIMITED    1220542  1673527  -409993  -852492  2116026    1.164, 1.596, -0.391, -0.813, 2.018
 *        BT601_FULL       1048576  1470104  -360853  -748826  1858077    1, 1.402, -0.344136, -0.714136, 1.772
 *        BT709_LIMITED    1220542  1880097  -223347  -558891  2214593    1.164, 1.793, -0.213, -0.533, 2.112
 *        BT709_FULL       1048576  1651297  -196423  -490864  1945738    1, 1.5748, -0.187324, -0.468124, 1.8556
 *      No sum leaves int32 (the largest magnitude is about 5.6e8).  The BT601_LIMITED row and the replication are what
 *      cv::cvtColor(COLOR_YUV2BGR_NV12 / _I420 / _YUY2) computes (the ITUR_BT_601_* constants and shift 20 of OpenCV's color_yuv);
 *      that is RESTATED here, unpinned against a running OpenCV, like the alignment.  tests/frame_ref.py is the same in numpy, and
 *      the kernel equals it bit for bit.  The other formats are byte moves.
 *
 *      Errors.  RFD_ERR_INVALID_ARG, with the frame and the cause named in rfd_last_error(): out[i].width / height differs from
 *      src[i]'s; out[i].stride < 3 * width; a stride below the layout's row_bytes; a needed plane (or out[i].data) is NULL; an
 *      unknown format, or an unknown colour of a YUV frame; a non-positive size; reserved not zero.  RFD_ERR_CAPACITY: n >
 *      max_batch_size, a frame wider than max_src_w or higher than max_src_h, a frame of 2^31 - 256 or more groups of four pixels.  n = 0 is a no-op.  A refused call enqueues nothing
 *      and writes no byte of any output frame.  Bytes of an output row at or past 3 * width are never written. ---- */
typedef enum rfd_pixel_format {
    RFD_PIXEL_BGR = 0,  RFD_PIXEL_RGB = 1,      /* [H][W][3]                                   1 plane  */
    RFD_PIXEL_BGRA = 2, RFD_PIXEL_RGBA = 3,     /* [H][W][4], 4th byte dropped (utils.rs:29)   1 plane  */
    RFD_PIXEL_GRAY = 4,                         /* [H][W], B = G = R = Y, bytes unchanged       1 plane  */
    RFD_PIXEL_NV12 = 5, RFD_PIXEL_NV21 = 6,     /* Y [H][W]; UV (VU) [ceil(H/2)][2*ceil(W/2)]   2 planes */
    RFD_PIXEL_I420 = 7,                         /* Y; U, V [ceil(H/2)][ceil(W/2)] each          3 planes */
    RFD_PIXEL_YUYV = 8, RFD_PIXEL_UYVY = 9      /* [H][4*ceil(W/2)]: Y0 U Y1 V / U Y0 V Y1      1 plane  */
} rfd_pixel_format;
typedef enum rfd_color { RFD_COLOR_BT601_LIMITED = 0, RFD_COLOR_BT601_FULL = 1,
                         RFD_COLOR_BT709_LIMITED = 2, RFD_COLOR_BT709_FULL = 3 } rfd_color;
typedef struct rfd_frame {
    const uint8_t *plane[3]; ptrdiff_t stride[3];   /* planes the format does not have are not read */
    int32_t width, height, format, color;           /* color is ignored by formats 0..4 */
    int32_t reserved[4];                            /* 0 */
} rfd_frame;                                        /* 80 bytes */
typedef struct rfd_frame_layout { int32_t planes; int32_t row_bytes[3]; int32_t rows[3]; int32_t reserved; } rfd_frame_layout;

/* Host only, no context: the planes of `format` at width x height.  RFD_ERR_INVALID_ARG for an unknown format, a NULL out or a
 * side outside 1 .. 2^28; *out is then untouched. */
RFD_API int rfd_frame_layout_of(int format, int width, int height, rfd_frame_layout *out);
/* Converts n frames into n caller-allocated DEVICE frames: every needed src[i].plane and out[i].data are device memory; src[] and
 * out[] themselves are host memory and may be freed when the call returns.  rfd_image declares data const because every other
 * entry point reads frames; this one WRITES through it (the library casts the const away), as rfd_decode_jpeg_batch_device
 * does.  The same array is then valid input to rfd_detect_batch_device, the views, the shot quality, the alignment and the
 * liveness calls on the same stream, with no synchronisation in between.  One launch per batch on the context's stream, whatever
 * the number, sizes and formats of its frames; the descriptors travel through a ring of page-locked slots, so a warm call
 * allocates nothing and does not wait for the previous one.  async as in rfd_decode_jpeg_batch_device: 0 returns after the
 * stream has drained, any other value at once (rfd_sync before reading the frames from another stream).  No output frame may
 * overlap a plane of the call: the conversion is not in place. */
RFD_API int rfd_convert_frames_device(rfd_ctx *ctx, const rfd_frame *src, int n, const rfd_image *out, int async);
/* The same with the planes in HOST memory, pageable or from rfd_host_alloc: each plane goes to device staging of the context with
 * one 2-D copy of tight rows, then the same launch writes the caller's DEVICE frames.  With async != 0 the planes must stay as
 * they are until the stream has run the copies (rfd_sync).  Staging reuse: the staging grows on demand and is reused by the next
 * call, whose copies follow this call's kernel in stream order, so two asynchronous calls back to back are safe. */
RFD_API int rfd_upload_frames_device(rfd_ctx *ctx, const rfd_frame *src, int n, const rfd_image *out, int async);
/* The same with everything in HOST memory (out[i].data is host memory, written through the same const cast); synchronous. */
RFD_API int rfd_convert_frames(rfd_ctx *ctx, const rfd_frame *src, int n, const rfd_image *out);

/* ---- JPEG encode: BGR frames and crops in device memory to baseline JPEG files, the inverse of "JPEG decode" above.  What a
 *      deployment stores as evidence (the best shot of a track, the enrolment thumbnail, the frame of an alarm) leaves the device
 *      as a file of some tens of KB, not as 6.2 MB of raw 1080p pixels for a JPEG library on the host.
 *
 *      Contract: the file equals, byte for byte from SOI to EOI, what libjpeg-turbo's default compressor writes for the same
 *      pixels and settings (JDCT_ISLOW, no smoothing, the standard Huffman tables, optimize off) -- Pillow's
 *      Image.save(f, "JPEG", quality=q, subsampling=s, restart_marker_rows=r).  tests/jpeg_encode_ref.py restates the rules in
 *      numpy, tests/test_jpeg_encode_cpu.py pins the restatement against Pillow, tests/test_jpeg_encode_gpu.py the kernels against
 *      the restatement.  Limits: baseline sequential only, 8 bits, the Annex-K tables (no optimised Huffman tables), one
 *      interleaved scan, no progressive files, no EXIF or other metadata (APP0 JFIF 1.01 alone), no arithmetic coding.
 *
 *      The arithmetic, all integer, FIX(x) = (int)(x * 65536 + 0.5):
 *        Y  = ( FIX(.299) R   + FIX(.587) G   + FIX(.114) B                 + 32768) >> 16
 *        Cb = (-FIX(.16874) R - FIX(.33126) G + FIX(.5) B     + (128 << 16) + 32767) >> 16
 *        Cr = ( FIX(.5) R     - FIX(.41869) G - FIX(.08131) B + (128 << 16) + 32767) >> 16      (a GRAY file holds Y only)
 *      A component of luma factors h x v under hmax x vmax (1x1, 2x1 for 4:2:2, 2x2 for 4:2:0; chroma is 1x1) has
 *      ceil(W h / hmax) x ceil(H v / vmax) samples in wb x hb real blocks.  Edges: the columns of the downsampler's INPUT are
 *      extended to wb * 8 * (hmax / h) by repeating the last pixel; its rows only to a whole row group (a multiple of vmax / v);
 *      the DOWNSAMPLED rows are then repeated down to hb * 8 (for 4:2:0 and H = 8 that differs from padding the input to 16
 *      rows).  Downsampling is a plain mean: (a + b + c + d + bias) >> 2 with bias 1, 2, 1, 2 .. along the output columns (2x2),
 *      (a + b + bias) >> 1 with bias 0, 1, 0, 1 .. (2x1).  Forward DCT: jfdctint.c on samples - 128 (rows first), the DCT scaled
 *      by 8.  Quantisation: libjpeg's quality scaling (5000 / q below 50, else 200 - 2 q; clamp((base * scale + 50) / 100, 1,
 *      255) on the two Annex-K tables, luma table 0, chroma table 1), v = (|c| + d / 2) / d with d = 8 * table and the sign put
 *      back; the kernel multiplies by a reciprocal that tests/cpp/jpeg_encode_plan_check.cpp proves equal for every |c| < 2^15 and
 *      every d.  The blocks of an MCU beyond wb or hb (dummy blocks) have zero AC and the DC of the block before them in the MCU's
 *      block order; in a dummy bottom row, every block takes the DC of the last block of the row above within the MCU.  Entropy
 *      coding: Annex-K tables, DC / AC 0 for Y and 1 for chroma, DC prediction per component and reset at each restart, every
 *      interval padded with 1-bits to a byte, FF -> FF 00 inside entropy data, FF D0+(i mod 8) between intervals.  Header: SOI,
 *      APP0, DQT 0 (and 1), SOF0 (component ids 1, 2, 3), DHT DC0 AC0 (DC1 AC1), DRI if there are restart rows, SOS.
 *
 *      Kernels (csrc/kernels_jpeg_encode.hip), all on the context's stream, four launches per call whatever the number and sizes
 *      of its images: pixels -> quantised coefficients (8 threads per block); the length of every restart interval (one workgroup
 *      per interval packs its blocks in parallel: a prefix sum of the blocks' bit lengths places them, LDS `or` packs them, a
 *      second prefix sum counts the stuffed FF bytes); one workgroup per image scans the interval lengths, checks the capacity
 *      and writes the header and size; the second run of the interval kernel writes its bytes where they belong in the slot.
 *      Running the entropy coder twice costs less memory than it saves: a workspace that held every interval at its worst case
 *      would be 20 MB per 1080p frame.  A file with restart_rows = 0 is ONE interval, hence one workgroup per image in the
 *      entropy kernels: right for crops, where a call has many images, slow for a lone large frame -- give frames restart rows.
 *      Workspace of a call: 128 bytes per block (3 bytes per pixel at 4:2:0), grown on demand and kept by the context. ---- */
typedef struct rfd_jpeg_encode_config {
    int32_t quality;      /* 1 .. 100, libjpeg's scale */
    int32_t sampling;     /* rfd_jpeg_sampling */
    int32_t restart_rows; /* 0: no restart markers; r >= 1: one interval per r MCU rows (Pillow's restart_marker_rows).  An
                             interval above 65535 MCUs (what DRI can say) is refused */
    int32_t reserved[5];  /* 0 */
} rfd_jpeg_encode_config; /* 32 bytes */
/* quality 90, RFD_JPEG_420, restart_rows 1 */
RFD_API int rfd_jpeg_encode_config_default(rfd_jpeg_encode_config *cfg);
/* Host only, no context.  *bytes = a size no file of this geometry can exceed.  It follows from the code-length limits of the
 * tables alone: a block is at most 22 + 63 * 26 bits (a DC symbol of at most 11 + 11 bits, 63 AC symbols of 16 + 10 bits), every interval
 * is padded to a byte, every byte may be FF and stuffed, then RSTn or EOI, plus the header.  Real files are some hundred times
 * smaller; a slot is better sized from experience and the -1 of size_dev handled. */
RFD_API int rfd_jpeg_encode_bound(int width, int height, const rfd_jpeg_encode_config *cfg, size_t *bytes);
/* Host only, no context.  The bytes of the file up to and including the SOS segment.  *len is set whenever the arguments are
 * valid; RFD_ERR_CAPACITY if cap < *len (out may then be NULL). */
RFD_API int rfd_jpeg_encode_header(int width, int height, const rfd_jpeg_encode_config *cfg, uint8_t *out, size_t cap, size_t *len);
/* Encodes n images: imgs[i].data, out, size_dev and the optional count_dev are DEVICE memory, imgs[] itself is host memory.  The
 * file of image i goes to out + i * slot_bytes and size_dev[i] is its length, or -1 if it does not fit slot_bytes (or exceeds
 * 2^31 - 1 bytes); then no byte of the slot is written.  Nothing is ever written outside a slot, nor behind a file's EOI.  With
 * count_dev given, the images i >= *count_dev are not read, their slots stay untouched and size_dev[i] = 0: rfd_face_list.total is
 * a ready count_dev and rfd_face_list.crops + t * crop bytes the image of crop t (stride 3 * out_w), so detect -> track -> align
 * the due faces -> encode their crops is one stream order.  A rectangle of a frame is a data pointer into it with the frame's
 * stride; any byte alignment and any stride >= 3 * width are legal.  The images of a call may differ in size; one config applies
 * to all.  Enqueued on the context's stream with no host wait inside; async as in rfd_convert_frames_device.
 * Errors, RFD_ERR_INVALID_ARG naming the field, with nothing enqueued: quality, sampling, restart_rows, reserved; a width or
 * height outside 1 .. 65535; stride < 3 * width; a NULL pointer.  RFD_ERR_CAPACITY: n > max_batch_size; a call of more than
 * 2^30 blocks.  n = 0 is a no-op. */
RFD_API int rfd_encode_jpeg_batch_device(rfd_ctx *ctx, const rfd_image *imgs, int n, const int32_t *count_dev, const rfd_jpeg_encode_config *cfg, uint8_t *out,
                                         size_t slot_bytes, int32_t *size_dev, int async);
/* The same with everything in HOST memory; synchronous.  The frames go to device staging with one 2-D copy each; only size[i]
 * bytes of file i come back over PCIe.  size[i] = -1: slot i is untouched. */
RFD_API int rfd_encode_jpeg_batch(rfd_ctx *ctx, const rfd_image *imgs, int n, const rfd_jpeg_encode_config *cfg, uint8_t *out, size_t slot_bytes, int32_t *size);
/* Test hook: the quantised coefficients the first kernel produced for one HOST image, dummy blocks included, in the layout of
 * rfd_debug_jpeg_coefficients ([blocks][64] i16, natural order, component-major over planes padded to whole MCUs).  *blocks is
 * always set; RFD_ERR_CAPACITY if cap_blocks < *blocks. */
RFD_API int rfd_debug_jpeg_encode_blocks(rfd_ctx *ctx, const rfd_image *img, const rfd_jpeg_encode_config *cfg, int16_t *out, size_t cap_blocks, size_t *blocks);
/* Test hook: the entropy and assembly kernels alone, on coefficients the caller supplies in that layout (HOST memory; DC within
 * -1024 .. 1023 and AC within -1023 .. 1023, else RFD_ERR_INVALID_ARG) for a file of width x height -> the file in out (HOST
 * memory, cap bytes) and its length, -1 if it does not fit. */
RFD_API int rfd_debug_jpeg_encode_coefficients(rfd_ctx *ctx, const int16_t *coef, size_t blocks, int width, int height, const rfd_jpeg_encode_config *cfg, uint8_t *out,
                                               size_t cap, int32_t *len);

/* ---- redaction: pixelate or fill the faces of detection rows in BGR frames on the device, between "we know where the faces are"
 *      and "write the file".  No counterpart in the reference.  The frame of an alarm also shows everyone else in front of the
 *      camera; detect -> track -> redact (out of place) -> rfd_encode_jpeg_batch_device is one stream order with no host wait, and
 *      the unredacted source stays available for the alignment and as evidence.
 *
 *      The rule, for frame b (H x W, BGR u8, byte stride).  Every step is integer, or one IEEE f32 operation in the written order
 *      with no contraction; as_i32 as in "shot quality" above (toward zero, saturating, NaN -> 0).
 *      Rows.     i < min(max(count[b], 0), max_det).  Row i is SELECTED when sel == NULL or (sel[b][i] & sel_mask) == sel_value:
 *                the tracker's flags array with sel_mask = sel_value = RFD_TRACK_CONFIRMED redacts confirmed tracks, a caller-written
 *                array can carry "not on the watch list", sel_mask = sel_value = 0 selects every row.
 *      Region.   bw = x2 - x1, bh = y2 - y1; xa = x1 - bw * margin_x, xb = x2 + bw * margin_x, ya = y1 - bh * margin_top, yb = y2 +
 *                bh * margin_bottom.  The row is SKIPPED if one of x1, y1, x2, y2 is not finite, if !(bw >= 0) or !(bh >= 0), or
 *                if one of xa, xb, ya, yb is a NaN.  X0 = max(as_i32(xa), 0), Y0 = max(as_i32(ya), 0), X1 = min(as_i32(xb), W - 1),
 *                Y1 = min(as_i32(yb), H - 1); the row is also skipped if X1 < X0 or Y1 < Y0.  w = X1 - X0 + 1, h = Y1 - Y0 + 1.
 *      Cover.    RECT: every pixel of the region.  ELLIPSE: with dx = 2 (x - X0) + 1 - w and dy = 2 (y - Y0) + 1 - h, pixel (x, y) of
 *                the region is covered iff dx^2 h^2 + dy^2 w^2 <= w^2 h^2 in int64 (sides <= 32768: a term is below 2^60).
 *      Colour.   FILL: (fill[0], fill[1], fill[2]).  PIXELATE: the pixel lies in the FRAME-ANCHORED cell (y / cell, x / cell); per
 *                channel m = (S + cnt / 2) / cnt, S the sum and cnt the count over ALL pixels of that cell inside the frame, read
 *                from the SOURCE frame.  The cells belong to the frame, not to a box: the result is a pure function of (source
 *                frame, set of covered pixels) and depends neither on the order of the rows nor on their overlaps.
 *      Output.   A pixel covered by at least one selected, non-skipped row gets its colour, every other pixel its source value.
 *                In place (dst == NULL): no byte of a non-covered pixel and no stride padding is ever written.  Out of place:
 *                dst[b] has the size of imgs[b] and a stride >= 3 * width, overlaps no source frame, receives all 3 * W bytes of
 *                every row (its padding is untouched), and the source is untouched.  applied[b] = the number of selected,
 *                non-skipped rows of frame b, written for every b < n.
 *
 *      Limits.  One cell size per call (no per-face cells), no Gaussian or box blur (a blur needs a halo and an out-of-place
 *      source), no outlines or landmarks drawn (that is "annotation" below), and sel is the caller's: the library does not derive it from gallery results.
 *      PIXELATION WITH A FIXED CELL IS WEAK ON VERY LARGE FACES (a 400-pixel face at cell 16 keeps 25 x 25 samples); FILL is the mode
 *      that guarantees removal.  The defaults (rfd_redact_config_default) are CHOSEN values, not tuned on data.
 *      Errors, all with nothing enqueued: RFD_ERR_INVALID_ARG with the field named in rfd_last_error() for every bound in the
 *      config comments, a non-zero reserved word, a NULL required pointer (ctx, imgs, dets and its boxes / count), a frame or dst
 *      with a NULL data pointer, a non-positive size, a side above RFD_REDACT_MAX_SIDE or a stride below 3 * width, a dst of
 *      another size than its frame; RFD_ERR_CAPACITY for n > max_batch_size; n = 0 is a no-op. ---- */
#define RFD_REDACT_FILL     0
#define RFD_REDACT_PIXELATE 1
#define RFD_REDACT_RECT     0
#define RFD_REDACT_ELLIPSE  1
#define RFD_REDACT_MAX_SIDE 32768
typedef struct rfd_redact_config {
    int32_t  mode;          /* RFD_REDACT_FILL or RFD_REDACT_PIXELATE */
    int32_t  shape;         /* RFD_REDACT_RECT or RFD_REDACT_ELLIPSE */
    int32_t  cell;          /* PIXELATE: side of the frame-anchored cells, 2 .. 64 (checked in both modes) */
    uint8_t  fill[4];       /* FILL: B, G, R; fill[3] = 0 */
    float    margin_x;      /* finite, 0 .. 4: the box grows by margin_x * its width on each side */
    float    margin_top;    /* finite, 0 .. 4: ... by margin_top * its height upwards (hair, forehead) */
    float    margin_bottom; /* finite, 0 .. 4: ... by margin_bottom * its height downwards */
    uint32_t sel_mask, sel_value;
    int32_t  reserved[6];   /* 0 */
} rfd_redact_config;        /* 60 bytes */
/* PIXELATE, ELLIPSE, cell 16, fill 0 0 0, margins 0.1 / 0.2 / 0.1, sel_mask 0, sel_value 0 (every row) */
RFD_API int rfd_redact_config_default(rfd_redact_config *cfg);
/* imgs[], dst[] and cfg: host memory; every imgs[i].data and dst[i].data, every pointer of `dets` (boxes, count; landmarks and
 * total are not read), sel and applied: DEVICE memory.  The counts are read on the device.  rfd_image declares data const; this
 * call WRITES through dst[i].data -- through imgs[i].data when dst is NULL -- as rfd_decode_jpeg_batch_device writes its `out`
 * frames.  Enqueued on the context's stream, ONE launch whatever the number, sizes and alignment of the frames, no host wait
 * (the frame descriptors travel through a ring of page-locked slots); async = 0 returns after the stream has drained, any other
 * value at once.  The frames of a call may differ in size; any byte alignment of data and any stride >= 3 * width are legal. */
RFD_API int rfd_redact_faces_device(rfd_ctx *ctx, const rfd_image *imgs, const rfd_image *dst /* NULL: in place */, int n,
                                    const rfd_dets *dets, const uint32_t *sel /* [n][max_det] or NULL */,
                                    const rfd_redact_config *cfg /* NULL: the default */, int32_t *applied /* [n] or NULL */, int async);
/* Stage-level: the same with host pointers (frames included), through the same kernel; synchronous.  The rows of dst[i] (of
 * imgs[i] when dst is NULL, written through the same const cast) come back with one 2-D copy of 3 * W bytes per row. */
RFD_API int rfd_redact_faces(rfd_ctx *ctx, const rfd_image *imgs, const rfd_image *dst, int n, const rfd_dets *dets, const uint32_t *sel,
                             const rfd_redact_config *cfg, int32_t *applied);

/* ---- annotation: box outlines, the five landmarks and a text label ("17 83%") drawn into BGR frames on the device, so a frame
 *      can SHOW what the pipeline decided without a round trip through the host.  No counterpart in the reference.  detect -> ...
 *      -> who -> redact (out of place) -> annotate (in place on that dst) -> rfd_encode_jpeg_batch_device is one stream order with
 *      no host wait.  sel is the tracker's flags or `who`, label is `identity` (or a serial's low bits), value is `id_score` or a
 *      quality figure; the library derives none of them.
 *
 *      The rule, for frame b (H x W, BGR u8, byte stride).  Every step is an integer, or one IEEE f32 operation in the written order
 *      with no contraction; as_i32 is the redaction's (toward zero, saturating, NaN -> 0).
 *      Rows and styles.  Row i < min(max(count[b], 0), max_det).  Word s = sel ? sel[b][i] : 0.  The row takes the FIRST style k <
 *                n_styles with (s & mask_k) == value_k; a row that matches none is not drawn.  Its colour C_row is that style's.
 *      Box.      bw, bh, xa, xb, ya, yb exactly as the redaction's Region line, and so are the skip conditions (a non-finite
 *                coordinate, !(bw >= 0), !(bh >= 0), a NaN among the four).  XA = as_i32(xa), XB = as_i32(xb), YA = as_i32(ya),
 *                YB = as_i32(yb), NOT clipped to the frame: a box leaving the frame draws no line along the frame's edge.  The row
 *                is also skipped if XB < XA or YB < YA.  All comparisons below are in int64.
 *      Layer 1, outline (t = thickness > 0).  Pixel (x, y) is on the outline iff XA <= x <= XB and YA <= y <= YB, and
 *                x < XA + t or x > XB - t or y < YA + t or y > YB - t.
 *      Layer 2, marks (r = mark_radius > 0).  For each of the five landmarks with both coordinates finite, cx = as_i32(lx) and
 *                cy = as_i32(ly); the pixel is marked iff (x - cx)^2 + (y - cy)^2 <= r^2.
 *      Text.     At most 15 glyphs from the set 0-9 - ? % space, with indices 0 .. 13.  label_source = ARRAY: "?" if label[b][i] < 0,
 *                else its decimal digits.  value_source != NONE: v is value[b][i] or the score boxes[b][i][4]; "--" if v is not
 *                finite or !(v >= 0), else the decimal digits of min(as_i32(v * 100.0f + 0.5f), 999); then "%".  If both parts are
 *                present, one space separates them.  len = 0 means no layers 3 and 4.
 *      Layer 3, plate.  With s = text_scale: PW = s * (6 * len + 1), PH = 9 * s, PX = XA, PY = YA - PH if YA - PH >= 0, else YA
 *                (above the box when there is room above, inside its top otherwise).  The plate is [PX, PX + PW) x [PY, PY + PH).
 *      Layer 4, text.  For a plate pixel, fx = (x - PX) div s and fy = (y - PY) div s.  It is a text pixel iff fx >= 1 and fy >= 1,
 *                k = (fx - 1) div 6 < len, u = (fx - 1) mod 6 < 5, v = fy - 1 < 7, and bit 4 - u of row v of glyph text[k] is set.
 *                The font is a 5 x 7 bitmap of 14 glyphs; the library holds the only copy (rfd_debug_annotate_glyph reads it).
 *      Winner.   Among the drawn, non-skipped rows that cover a pixel with any layer, the LOWEST row index wins (row 0 is the best
 *                score and ends on top); within that row the highest layer wins.  C = text_colour on layer 4, otherwise C_row.
 *      Output.   A covered pixel with source value P gets, per channel, C if alpha == 256, otherwise (alpha * C + (256 - alpha) * P
 *                + 128) >> 8; every other pixel its source value.  The result is a pure function of (source frame, rows).
 *                In place (dst == NULL): no byte of a non-covered pixel and no stride padding is ever written.  Out of place:
 *                dst[b] has the size of imgs[b] and a stride >= 3 * width, overlaps no source frame, receives all 3 * W bytes of
 *                every row (its padding is untouched), and the source is untouched.  applied[b] = the number of drawn,
 *                non-skipped rows of frame b (a row wholly outside the frame counts), written for every b < n.
 *
 *      Limits.  One thickness, radius and scale per call; no anti-aliased or vector text and no glyph beyond the 14; no corner
 *      brackets, trails or legends.  The defaults (rfd_annotate_config_default) are CHOSEN values, not tuned on data.
 *      Errors, all with nothing enqueued: RFD_ERR_INVALID_ARG with the field named in rfd_last_error() for every bound in the
 *      config comments, a non-zero reserved word, colour[3] or text_colour[3], a non-zero style at or past n_styles, label_source =
 *      ARRAY with `label` NULL, value_source = ARRAY with `value` NULL, mark_radius > 0 with dets->landmarks NULL, a NULL required
 *      pointer (ctx, imgs, dets and its boxes / count), and the redaction's frame and dst checks; RFD_ERR_CAPACITY for n >
 *      max_batch_size; n = 0 is a no-op.  The context is checked last. ---- */
#define RFD_ANNOTATE_NONE   0
#define RFD_ANNOTATE_ARRAY  1
#define RFD_ANNOTATE_SCORE  2            /* value_source only: the detection's own score, boxes[..][4] */
#define RFD_ANNOTATE_MAX_STYLES 4
typedef struct rfd_annotate_style {
    uint32_t sel_mask, sel_value;
    uint8_t  colour[4];                  /* B G R 0 */
} rfd_annotate_style;                    /* 12 bytes */
typedef struct rfd_annotate_config {
    int32_t n_styles;                    /* 1 .. 4 */
    rfd_annotate_style style[RFD_ANNOTATE_MAX_STYLES]; /* entries >= n_styles all zero */
    int32_t thickness;                   /* 0 .. 16, 0: no outline */
    int32_t mark_radius;                 /* 0 .. 8, 0: no landmarks; > 0 needs dets->landmarks */
    int32_t label_source;                /* RFD_ANNOTATE_NONE | RFD_ANNOTATE_ARRAY (needs `label`) */
    int32_t value_source;                /* RFD_ANNOTATE_NONE | RFD_ANNOTATE_ARRAY (needs `value`) | RFD_ANNOTATE_SCORE */
    int32_t text_scale;                  /* 1 .. 4 */
    uint8_t text_colour[4];              /* B G R 0 */
    int32_t alpha;                       /* 1 .. 256; 256 = opaque */
    float   margin_x, margin_top, margin_bottom; /* finite, 0 .. 4: the redaction's, so an outline can frame a redacted region */
    int32_t reserved[4];                 /* 0 */
} rfd_annotate_config;                   /* 108 bytes */
/* one style {0, 0, (0, 255, 0)} = every row green; thickness 2, mark_radius 2, label NONE, value SCORE, text_scale 2, text
 * (0, 0, 0), alpha 256, margins 0: "box, landmarks, score %" */
RFD_API int rfd_annotate_config_default(rfd_annotate_config *cfg);
/* Host and device memory as rfd_redact_faces_device: imgs[], dst[] and cfg are host memory; every imgs[i].data and dst[i].data,
 * the pointers of `dets` (boxes, count, and landmarks when mark_radius > 0), sel, label, value and applied are DEVICE memory.
 * The call WRITES through dst[i].data -- through imgs[i].data when dst is NULL -- by the same const cast.  Enqueued on the context's
 * stream, ONE launch whatever the number, sizes and alignment of the frames, no host wait, no global atomics, the same bits on
 * every run; async = 0 returns after the stream has drained, any other value at once.  The frames of a call may differ in size;
 * any byte alignment of data and any stride >= 3 * width are legal. */
RFD_API int rfd_annotate_faces_device(rfd_ctx *ctx, const rfd_image *imgs, const rfd_image *dst /* NULL: in place */, int n,
                                      const rfd_dets *dets, const uint32_t *sel /* [n][max_det] or NULL */,
                                      const int32_t *label /* [n][max_det] or NULL */, const float *value /* [n][max_det] or NULL */,
                                      const rfd_annotate_config *cfg /* NULL: the default */, int32_t *applied /* [n] or NULL */, int async);
/* Stage-level: the same with host pointers (frames included), through the same kernel; synchronous. */
RFD_API int rfd_annotate_faces(rfd_ctx *ctx, const rfd_image *imgs, const rfd_image *dst, int n, const rfd_dets *dets, const uint32_t *sel,
                               const int32_t *label, const float *value, const rfd_annotate_config *cfg, int32_t *applied);
/* Test hook: the seven rows (top first, bit 4 = the left column) of glyph 0 .. 13 of the font the library was built with. */
RFD_API int rfd_debug_annotate_glyph(int glyph, uint8_t rows[7]);

/* ---- introspection ---- */
RFD_API int rfd_get_stats(rfd_ctx *ctx, rfd_stats *stats);
RFD_API int rfd_get_config(const rfd_ctx *ctx, rfd_config *cfg);
/* confidence_threshold / iou_threshold are plain fields of the reference's struct
 * (face_detection.rs:26-27); they may be changed between calls. */
RFD_API int rfd_set_thresholds(rfd_ctx *ctx, float confidence_threshold, float iou_threshold);
/* Per-launch profiling of the network: when enabled, every network op is bracketed by HIP events on
 * the context's stream.  rfd_get_conv_profile returns, for the last synchronous detect/forward call,
 * the summed duration (ms) of the implicit-GEMM conv launches, the FLOPs they performed and their
 * number; rfd_get_op_profile copies the per-op durations (ms) and returns the op count. */
RFD_API int rfd_set_profiling(rfd_ctx *ctx, int enable);
RFD_API int rfd_get_conv_profile(rfd_ctx *ctx, float *ms_conv, double *flops_conv, int *launches);
RFD_API int rfd_get_op_profile(rfd_ctx *ctx, float *ms, int cap);

/* ---- test hooks (not part of the drop-in surface): raw access to a network tensor (device layout:
 *      NHWC, bf16 or f32 as rfd_tensor_desc says; n * C*H*W elements) and partial execution of the
 *      op list [first_op, last_op] (last_op < 0: to the end), so every op can be checked in isolation.
 *      In the f32 parity mode (RFD_PRECISION_F32) every tensor but the network input is f32: rfd_debug_tensor_io then moves
 *      n * C*H*W * 4 bytes of an intermediate tensor, the n images contiguous at the tensor's own size. */
RFD_API int rfd_debug_tensor_io(rfd_ctx *ctx, int tensor_id, int n, void *host, int write);
RFD_API int rfd_debug_run_ops(rfd_ctx *ctx, int n, int first_op, int last_op);
/* rfd_debug_run_ops as a chain of a split pass runs the range: on images [batch_off, batch_off + n) of the workspace
 * (batch_off + n <= max_batch_size), with the kernel choice of a chain that runs beside another one when co_running != 0. */
RFD_API int rfd_debug_run_chain(rfd_ctx *ctx, int n, int first_op, int last_op, int batch_off, int co_running);
/* the chains a pass of n images runs as: returns their number (1: the pass is not split) and fills sizes[0 .. that number);
 * chain p holds the images from the sum of the sizes before it.  The rule the pass itself uses; launches nothing. */
RFD_API int rfd_debug_pass_chains(rfd_ctx *ctx, int n, int *sizes, int cap);
/* raw access to the WHOLE workspace buffer that holds a tensor: max_batch_size * *image_pitch bytes.  The images of a chain at
 * batch_off start at byte batch_off * *image_pitch and follow each other at the tensor's own C*H*W size (tensors that share a
 * buffer differ in size, so the pitch belongs to the buffer).  host == NULL only reports the pitch. */
RFD_API int rfd_debug_buffer_io(rfd_ctx *ctx, int tensor_id, void *host, size_t bytes, int write, size_t *image_pitch);
/* force the conv tile configuration: 0 = heuristic, 1 = 128-row four-wave tiles, 2 = 256x128 tiles where legal, 16 = the
 * weight-resident pair kernel for stage 1's pairs, 17 = the wave-specialised ring form wherever the layer shape allows, 18 = the
 * eight-wave 128x128 generic tile, 19 = the four-wave merged-kx 3x3 kernel (all twenty, by name: enum ConvTile in csrc/kernels.h;
 * rfd_hip exports the same names) */
RFD_API int rfd_debug_set_conv_tile(rfd_ctx *ctx, int tile);
/* which kernel(s) op `op` of the network would be run by at `n` images per chain (co_running != 0: as one of the two chains of a
 * split pass) -- the names rocprofv3 reports without the rfd:: prefix, " + "-separated when an op takes two launches.  Nothing is
 * launched.  tools/traffic_model.py and tools/roof_gap.py attribute bytes and time to kernels through this call. */
RFD_API int rfd_debug_op_kernels(rfd_ctx *ctx, int n, int op, int co_running, char *names, int cap);
/* The same answer without a context or a GPU: the chooser (csrc/conv_select.hip) asked with the parameters a context of this
 * backbone and image size would build for op `op` of a chain of n images -- weight offsets from the layer table, split-K
 * capacities from the graph -- under forced tile `tile` (0 in production), schedule RFD_SCHEDULE_*, on a GPU of `cus` compute
 * units.  tests/test_kernel_choice_cpu.py replays the pinned choice table tests/golden/kernel_choice.json through it. */
RFD_API int rfd_debug_op_kernels_static(int backbone, int net_w, int net_h, int n, int op, int co_running, int tile, int schedule,
                                        int cus, char *names, int cap);
/* execution structure of the network pass: side streams for independent chains on/off; batch split into
 * clamp(n / split_min_part, 1, split_max_parts) contiguous parts that run as independent chains on their own streams
 * (split_max_parts <= 1 = never; at most 4); hipGraph replay of unsplit passes on/off.  Every structure gives
 * bit-identical results (tests/test_concurrency_gpu.py). */
RFD_API int rfd_debug_set_concurrency(rfd_ctx *ctx, int multi_stream, int split_min_part, int split_max_parts,
                                      int use_graph);

/* Sets the device word through which a chunk workgroup of the dense-crowd NMS -- or a wave of a ring convolution -- reports that
 * it gave up waiting (tests: the next call that synchronises must then fail with RFD_ERR_HIP and clear the word). */
RFD_API int rfd_debug_poke_nms_flag(rfd_ctx *ctx, int value);
/* Test hook: what the alignment's set-up kernel decides, which the crops show only rounded to 1/32 pixel.  boxes [n][5],
 * kps [n][10], found [n] and cfg as rfd_align_faces takes them, img_w / img_h [n] = the frame sizes (the set-up reads no
 * pixels); all host pointers, n <= max_batch_size.  Runs align_setup_kernel as rfd_align_faces launches it and copies back, per
 * face: mode (= the status), M [n][6] (the INVERTED map, crop -> frame, as cv::warpAffine computes it; zeros unless mode 0),
 * roi [n][4] = x0, y0, rw, rh and scale [n][2] = scale_x, scale_y of the fallback (zeros unless it was entered; the scales only
 * for mode 1), area_fast [n]. */
RFD_API int rfd_debug_align_setup(rfd_ctx *ctx, int n, const float *boxes, const float *kps, const int32_t *found,
                                  const int32_t *img_w, const int32_t *img_h, const rfd_alignment_config *cfg, int32_t *mode,
                                  double *M, int32_t *roi, double *scale, int32_t *area_fast);
/* The list of PERSISTENT kernels (one workgroup per CU, looping over work items) and the dynamic LDS every launch of one
 * requests -- always the CU's whole 160 KiB, so that no other kernel's workgroup can share the CU.
 * Needs no context and no GPU: tests/test_build_cpu.py walks it against the kernels of the code object.  Returns the number
 * of entries; fills name / lds_bytes for 0 <= i < that number. */
RFD_API int rfd_debug_persistent_kernel(int i, const char **name, size_t *lds_bytes);

#ifdef __cplusplus
}
#endif
#endif /* RFD_H */
