// kernels.h -- launch interfaces of the HIP kernels (all gfx950).
#pragma once
#include "gallery_nearest_plan.h"
#include "jpeg_desc.h"
#include "jpeg_entropy.h"
#include "rfd_common.h"

namespace rfd {

// ---------------------------------------------------------------- preprocess (kernels_pre.hip)
// One source frame and its letterbox geometry (reference face_detection.rs:131-198).
struct PreImage {
    const uint8_t *src; // device, HxWx3 u8 BGR
    long long stride;   // bytes per source row
    int h, w;
    int new_w, new_h;   // resized extent pasted at (0,0) of the canvas
    int area_fast;      // both scale factors exactly 2: OpenCV's INTER_LINEAR -> INTER_AREA switch
    int pad;
    double scale_x, scale_y; // 1 / (new_w / w), 1 / (new_h / h) in f64, as cv::resize computes them
};

struct PreParams {
    const PreImage *imgs; // device [n]
    int net_h, net_w;
    bf16_t *out_nhwc4;    // [n][net_h][net_w][4] bf16 R,G,B,0  (network input) or null
    uint8_t *out_det_img; // [n][net_h][net_w][3] u8 BGR canvas (reference det_img) or null
    float *out_tensor;    // [n][3][net_h][net_w] f32 R,G,B planes (reference Triton input) or null
};
int launch_preprocess(const PreParams &p, int n, hipStream_t s);
// [n][3][H][W] f32 planes -> [n][H][W][4] bf16 (used by rfd_forward, whose input is the tensor)
int launch_tensor_to_nhwc4(const float *tensor, bf16_t *out, int n, int H, int W, hipStream_t s);

// ---------------------------------------------------------------- decode / sort / NMS (kernels_post.hip)
struct DecodeParams {
    const float *cls[kNumLevels];
    const float *bbox[kNumLevels];
    const float *lmk[kNumLevels];
    int fh[kNumLevels], fw[kNumLevels], stride[kNumLevels], level_off[kNumLevels];
    float base_anchor[kNumLevels][kA][4];
    int total_anchors;
    int net_h, net_w;
    float conf_thr;
    float *rows;    // [n][total_anchors][16]
    uint64_t *keys; // [n][total_anchors]
    int *count;     // [n], zeroed before launch
};
int launch_decode(const DecodeParams &p, int n, bool nchw, hipStream_t s);

// Decode into per-FRAME lists (rfd.h, "views"): image b of the network batch is view b, the v-th view of frame f.  A candidate
// that passes the threshold and the inner-edge rule is written in frame pixels to rows[(f * vmax + v) * total_anchors + g] and
// its key (score bits << 32 | v * total_anchors + g) appended to keys[f * vmax * total_anchors + ...] through count[f]: frame f
// then looks to launch_sort / launch_nms like an image of vmax * total_anchors anchors.
struct ViewDesc {
    int frame, slot;  // f, v
    int x, y;         // the view's corner in the frame
    int new_w, new_h; // its letterboxed extent
    uint32_t inner;   // rfd_view::inner
    float det_scale;  // its letterbox scale
};
// views: device [n_views]; p.count [frames] zeroed before launch; p.rows / p.keys hold frames * vmax * total_anchors entries
int launch_decode_views(const DecodeParams &p, const ViewDesc *views, int n_views, int vmax, float edge_margin, bool nchw, hipStream_t s);

int launch_sort(uint64_t *keys, const int *count, const float *rows, uint64_t *sorted_keys,
                float4 *sorted_boxes, int total_anchors, int n, hipStream_t s);

struct NmsParams {
    const uint64_t *sorted_keys; // [n][total_anchors] (null with presorted boxes)
    const float4 *sorted_boxes;  // [n][total_anchors]
    const float *rows;           // [n][total_anchors][16] (null: emit indices only)
    const int *count;            // [n]
    const float *det_scale;      // [n]
    int presorted_n;             // >= 0: every image has exactly this many boxes (rfd_nms_sorted)
    int total_anchors;
    int max_det;
    int nwords_cap;              // filled by launch_nms
    float iou_thr;
    float *out_boxes;            // [n][max_det][5]
    float *out_lmk;              // [n][max_det][10]
    int *out_count;              // [n]
    int *out_total;              // [n]
    int *out_gidx;               // [n][max_det] or null
    // chunked kernel (dense crowds: kNmsChunks workgroups per image; all null / 0: one workgroup per image)
    float4 *kept_boxes;          // [n][total_anchors] scratch: the kept boxes of an image in score order, chunk after chunk
    int *chunk_state;            // [n][kNmsChunks][2]: {kept count, epoch of the launch that published it}; zero-initialised once
    int *spin_fail;              // set to 1 if a chunk gave up waiting for its predecessor (bounded spin; never expected)
    unsigned *ticket;            // two counters: workgroups draw their (image, chunk) from ticket[ticket_sel] in the order they start
    int ticket_sel;              // 0 / 1, alternating between the launches of a context (the idle counter is zeroed by ticket 0)
    int epoch;                   // > 0, different for every launch that uses chunk_state
};
constexpr int kNmsChunks = 4;
int launch_nms(NmsParams p, int n_images, hipStream_t s, bool *used_chunked = nullptr);
// launch_nms accepts this many anchors per image (its LDS check), so that a caller can refuse before it enqueues anything
bool nms_fits_lds(int total_anchors);

// FaceSelection::call on the device (face_selection.rs:72-189): per image, over its kept detections
struct SelectParams {
    const float *boxes; // [n][max_det][5]
    const float *lmk;   // [n][max_det][10]
    const int *count;   // [n]
    const int *img_h, *img_w; // [n] source frame sizes
    int n, max_det, is_enroll;
    float margin_center_left_ratio, margin_center_right_ratio, margin_edge_ratio, minimum_face_ratio;
    float *out_box;     // [n][5]
    float *out_kps;     // [n][10]
    int *out_found;     // [n]: 0 nothing selected, 1 box only, 3 box + key points
};
int launch_face_select(const SelectParams &p, hipStream_t s);

// The packed face list (rfd.h, "every detected face"): the first max_faces rows of every frame's slab that pass the
// predicate, in (frame, row) order, as one dense list.  One workgroup; the order is decided by ballots and prefix sums alone.
struct FaceListParams {
    const float *boxes; // [n][max_det][5]
    const float *lmk;   // [n][max_det][10]
    const int *count;   // [n]
    int n, max_det, max_faces, cap;
    float min_face_px, min_score;
    int *total;         // [1]: T, not clamped to cap
    int *first;         // [n + 1]: exclusive prefix of the per-frame counts; also the kernel's scratch for those counts
    int *frame;         // [cap]
    int *row;           // [cap]
    float *box;         // [cap][5]
    float *kps;         // [cap][10]
};
int launch_face_list(const FaceListParams &p, hipStream_t s);

// FaceAlignment::call on the device (face_alignment.rs:27-141): 5-point similarity to the template + cv::warpAffine
// (INTER_LINEAR, BORDER_CONSTANT 0) of the source frame, or the reference's crop + resize fallback
struct AlignFace {      // per face, filled by the set-up kernel
    double M[6];        // inverse map (dst -> src), as cv::warpAffine computes it
    double scale_x, scale_y; // fallback resize
    int mode;           // 0 warp, 1 crop + resize, < 0 nothing written (status)
    int x0, y0, rw, rh; // fallback ROI
    int area_fast;
};
struct AlignParams {
    const PreImage *imgs; // [n] frames of the batch (device descriptors)
    const float *box;     // [n][5] selected detection
    const float *kps;     // [n][10] its key points
    const int *found;     // [n] selection flags: bit 0 box, bit 1 key points; null: 3 for every face (a face list)
    float std_lmk[10];    // template (config.rs:46-52)
    int out_w, out_h, n;
    AlignFace *faces;     // [n] scratch
    int *status;          // [n]: 0 aligned, 1 fallback crop, -1 no key points (the reference's call errors), -2 no face,
                          //      -3 fallback ROI outside the frame (Mat::roi error)
    uint8_t *out;         // [n][out_h][out_w][3] u8 BGR
    // A packed face list: face t reads frame frame[t], and a face t >= min(*total, cap), both read on the device, is left
    // alone: nothing of it is written.  n is then the host-known bound of the launch.  Null / null: face b is frame b and all
    // n faces are done -- the one-face entries.  face0: the first face of this launch (the launchers split at the grid limit).
    const int *frame;
    const int *total;
    int cap, face0;
};
int launch_face_align(const AlignParams &p, hipStream_t s);
// the set-up launch of the two aligners alone: faces and status of p, no pixel read (rfd_debug_align_setup)
int launch_face_align_setup(const AlignParams &p, hipStream_t s);

// The model inputs of FaceQuality::call / FaceExtraction::call (face_quality.rs:43-44,56-101, face_extraction.rs:38-77):
// cv::resize(INTER_LINEAR) of the aligned crop to the model's image_size, COLOR_BGR2RGB, (p - mean) * scale, NHWC -> NCHW.
constexpr int kMaxFaceTensors = 4; // = RFD_MAX_FACE_TENSORS
struct FaceTensorCfg {
    float *out;              // [n][3][out_h][out_w] f32, R,G,B planes
    int out_w, out_h;
    float mean[3], scale[3]; // per OUTPUT channel: value = (float(p) - mean[c]) * scale[c], two roundings
    double scale_x, scale_y; // 1 / (out_w / crop_w), 1 / (out_h / crop_h) in f64, as cv::resize computes them
    int area_fast;           // both exactly 2: the 2x2 mean
    int same;                // out size == crop size: a copy
};
struct FaceTensorParams {
    const uint8_t *crops;    // [n][crop_h][crop_w][3] u8 BGR (face_tensor_kernel only)
    const int *status;       // [n] alignment status or null: a face with a negative status gets all-zero tensors
    int n, crop_w, crop_h, k;
    FaceTensorCfg cfg[kMaxFaceTensors];
    const int *total;        // as in AlignParams (null: all n faces)
    int cap, face0;
};
// every config of p from crops in HBM: one launch for all k configs and n faces
int launch_face_tensors(const FaceTensorParams &p, hipStream_t s);
// launch_face_align whose warp also writes the planes of every config of t (all of the crop's own size, t.k may be 0) from the
// registers that hold the pixel; a.out may be null (no u8 crop wanted)
int launch_face_align_tensors(const AlignParams &a, const FaceTensorParams &t, hipStream_t s);

// quality decision rule (face_quality.rs:159-168): klass = LAST index of the maximum, class 1 below the threshold -> class 0,
// score = the logit of the final class; a row that holds a NaN gets klass = -1, score = NaN.  One thread per row.
int launch_quality_decide(const float *logits, int n, int classes, float threshold, float *score, int *klass, hipStream_t s);
// out = emb / sqrt(sum emb^2) per row (utils.rs:148-154), one wave64 per row, deterministic
int launch_l2_normalize(const float *emb, int n, int dim, float *out, hipStream_t s);

// FaceAntiSpoofing (face_antispoofing.rs): the inputs of the miniFAS models from the source frame and the selected box --
// _get_scale_image :245-295, _get_new_box :342-385, Mat::roi + cv::resize(INTER_LINEAR) :323-337, _preprocess :180-217 --
// and the rule on their outputs, _postprocess :219-243.
struct LiveImage {
    const uint8_t *src; // device, HxWx3 u8 BGR
    long long stride;   // bytes per source row
    int h, w;
};
struct LiveRoi {             // per (face, model), filled by the geometry kernel
    double scale_x, scale_y; // 1 / (out_w / rw), 1 / (out_h / rh) in f64, as cv::resize computes them
    int x0, y0, rw, rh;      // the ROI inside the frame
    int area_fast;           // both exactly 2: the 2x2 mean
    int ok;                  // the FACE's status is 0 (every model's ROI is valid)
};
struct LiveCfg {
    float *out;       // [n][3][out_h][out_w] f32, planes in source channel order (B, G, R), raw 0..255
    float scale;      // scales[j]
    int out_w, out_h; // image_sizes[j]
    int tile0;        // first 256-pixel tile of this model in the flat tile table of the crop kernel
};
struct LiveParams {
    const LiveImage *imgs; // [n]
    const float *box;      // [n][5] selected detection (x1, y1, x2, y2, score)
    const int *found;      // [n] selection flags: bit 0 = a box
    int n, k, tiles;       // tiles = all 256-pixel tiles of one face's k outputs
    LiveCfg cfg[kMaxFaceTensors];
    LiveRoi *geo;          // [n][k] scratch
    float *weights;        // [n][k]: scale / scales[j]; 0 for a face with a negative status
    int *rois;             // [n][k][4] ltx, lty, rbx, rby, or null
    int *status;           // [n]: 0 ok, -2 no face, -3 some model's ROI is not inside the frame or is empty
};
// geometry (one thread per face and model) + crop, resize, tensorise (one launch for all n * k outputs)
int launch_liveness_tensors(const LiveParams &p, hipStream_t s);
// _postprocess: score = sum_j logits[j][b][1] * w[b][j] / sum_j w[b][j] in the reference's f32 order, live = score > threshold.
// Models [j0, j0 + kc) of k per launch (kc <= kLiveDecideChunk); the sums of a call of more models travel through acc [n][2].
constexpr int kLiveDecideChunk = 8;
struct LiveLogits { const float *p[kLiveDecideChunk]; };
int launch_liveness_decide(const LiveLogits &l, int kc, int k, int j0, int n, int classes, const float *weights, float threshold,
                           float *acc, float *score, int *live, hipStream_t s);

// ---------------------------------------------------------------- face gallery (kernels_gallery.hip)
// Element offset of (row, d) in a gallery's storage, the one statement of the layout (rfd_debug_gallery_offset returns it):
// rows in blocks of 16; a block holds dim / 32 K steps of 512 elements; inside a K step lane (row & 15) + 16 * ((d & 31) >> 3) of
// v_mfma_f32_16x16x32_bf16's B operand owns 8 consecutive elements.
__host__ __device__ static inline size_t gallery_offset(int dim, int row, int d)
{
    return ((size_t)(row >> 4) * (dim >> 5) + (d >> 5)) * 512 + (size_t)(((row & 15) + 16 * ((d & 31) >> 3)) * 8 + (d & 7));
}
constexpr int kGalleryMaxQueries = 32; // queries of one pass over the gallery (two 16-row M-tiles)
// emb [n][dim] f32 (device, 16-byte aligned) -> rows [row0, row0 + n) of store, bf16 RNE
int launch_gallery_add(const float *emb, int n, int dim, int row0, bf16_t *store, hipStream_t s);
// the stored values of rows [row0, row0 + n) -> out [n][dim] f32 (device)
int launch_gallery_get(const bf16_t *store, int row0, int n, int dim, float *out, hipStream_t s);
// workgroups a search over `rows` rows runs with, <= groups_max; ws must hold that many x n x k keys of 8 bytes
int gallery_search_groups(int rows, int groups_max);
// one pass: queries [n <= kGalleryMaxQueries][dim] f32 (device, 16-byte aligned) against rows [0, rows) -> scores / out_rows
// [n][k] under (score descending, row ascending); two launches (scan, merge of the workgroups' lists), no synchronisation.
// live: null (every row counts: the scan without the mask), or one 16-bit word per block of 16 rows, bit i = row 16 b + i counts
int launch_gallery_search(const bf16_t *store, const uint16_t *live, int rows, int dim, const float *queries, int n, int k, uint2 *ws, int groups_max,
                          float *scores, int32_t *out_rows, hipStream_t s);
// The identity form (rfd.h, "identities"): the k best identities of each query, each under its best row's key -> scores /
// out_rows / out_ids [n][k]; entries with !(score >= min_score) become the empty entry (-inf, -1, -1).  ids: one int32 per row
// (-1: the row is an identity of its own), allocated in whole blocks of 16 rows (the scan reads a block's 16 words), or null: no row is labelled, the plain scan runs and out_ids is all -1.
int launch_gallery_search_identities(const bf16_t *store, const uint16_t *live, const int32_t *ids, int rows, int dim, const float *queries, int n, int k,
                                     float min_score, uint2 *ws, int groups_max, float *scores, int32_t *out_rows, int32_t *out_ids, hipStream_t s);
// ids[rows[i]] = vals[i] for i < n, or -1 where vals is null (rows: device list of distinct rows)
int launch_gallery_set_identities(int32_t *ids, const int32_t *rows, const int32_t *vals, int n, hipStream_t s);
// The filtered form (rfd.h, "tags"): launch_gallery_search_identities on the rows r that are eligible for query q, (tags[r] &
// fmask[q]) == fvalue[q].  tags: one uint32 per row, allocated in whole blocks of 16 rows and zero beyond the rows (the scan
// reads a block's 16 words); fmask / fvalue: device [n].  ids as above (null: out_ids is all -1).
int launch_gallery_search_filtered(const bf16_t *store, const uint16_t *live, const int32_t *ids, const uint32_t *tags, const uint32_t *fmask,
                                   const uint32_t *fvalue, int rows, int dim, const float *queries, int n, int k, float min_score, uint2 *ws, int groups_max,
                                   float *scores, int32_t *out_rows, int32_t *out_ids, hipStream_t s);
// tags[rows[i]] = vals[i] for i < n, or 0 where vals is null (rows: device list, distinct where vals is given)
int launch_gallery_set_tags(uint32_t *tags, const int32_t *rows, const uint32_t *vals, int n, hipStream_t s);
// rows[i] (device list, distinct unless emb is null) of store takes bf16(emb[i]), or zeros where emb is null; then live[blk[j]] =
// word[j] for j < nwords <= n (device lists, blk distinct)
int launch_gallery_put(const float *emb, const int32_t *rows, int n, int dim, bf16_t *store, const int32_t *blk, const int32_t *word, int nwords,
                       uint16_t *live, hipStream_t s);
// sets the live bits of rows [row0, row1), row0 < row1
int launch_gallery_live_range(uint16_t *live, int row0, int row1, hipStream_t s);
// bf16 values [n][dim] in row-major order (device, 16-byte aligned) <-> rows [row0, row0 + n) of store, bit for bit
int launch_gallery_import(const bf16_t *src, int n, int dim, int row0, bf16_t *store, hipStream_t s);
int launch_gallery_export(const bf16_t *store, int row0, int n, int dim, bf16_t *out, hipStream_t s);
// The self-join (rfd.h, "nearest"; kernels_gallery_nearest.hip): for every row a of [row0, row0 + n), the best live row b != a
// that `mode` and the tag rule allow -> scores / out_rows / out_ids [n] (device; out_ids may be null); entries with
// !(score >= min_score) or without a candidate become (-inf, -1, -1).  plan: gallery_nearest_plan(rows, row0, n, dim, cus); ws
// holds plan.ws_bytes.  live / ids / tags as in the searches, each may be null (all live / all unlabelled / all 0).  Two
// launches (scan, merge of the splits), no synchronisation.
int launch_gallery_nearest(const bf16_t *store, const uint16_t *live, const int32_t *ids, const uint32_t *tags, int rows, int dim, int row0, int n, int mode,
                           float min_score, uint32_t tag_mask, const GalleryNearestPlan &plan, uint2 *ws, float *scores, int32_t *out_rows, int32_t *out_ids,
                           hipStream_t s);

// ---------------------------------------------------------------- JPEG decode (kernels_jpeg.hip)
// The parallel half of the baseline JPEG decoder (rfd.h, "JPEG decode"); the serial half is csrc/jpeg_parse.h on the host.  The
// descriptors are in jpeg_desc.h.
// kernel 1: zigzag run -> dequantise -> libjpeg's accurate integer IDCT -> u8 planes; kernel 2: fancy upsampling + YCbCr -> BGR
int launch_jpeg_decode(const JpegParams &p, hipStream_t s);
// a batch with at least one oriented frame: the inverse DCT over p, the colour kernel over `upright` (its own frame table and
// tile count, the pools of p; skipped where upright.n is 0), the oriented kernel over o
int launch_jpeg_decode_oriented(const JpegParams &p, const JpegParams &upright, const JpegOrientedParams &o, hipStream_t s);
// one reduced inverse DCT over the batch, one colour launch over the upright frames, one over the oriented ones, each where it
// has a frame
int launch_jpeg_decode_scaled(const JpegScaledParams &p, hipStream_t s);

// ---------------------------------------------------------------- JPEG entropy decode (kernels_jpeg_entropy.hip)
int launch_jpeg_entropy(const JpegEntropyParams &p, hipStream_t s);

// ---------------------------------------------------------------- convolution engine (kernels_conv.hip)
// Activations: NHWC bf16.  Weights: [Cout][KH][KW][Cin] bf16 (K contiguous).  f32 accumulate on MFMA.
struct ConvParams {
    const bf16_t *x;      // [B][H][W][Cin]
    const bf16_t *w;      // [Cout][KH*KW*Cin (+ Cin2)]: row pitch = total K
    const bf16_t *x2;     // optional second K segment: a 1x1 conv (stride2, no pad) over [B][H2][W2][Cin2]
    const float *bias2;   // its bias (added to `bias`), or null
    const float *bias;    // [Cout] (BN folded)
    const bf16_t *zero;   // >= 16 bytes of zeros (source of padding taps for the LDS-DMA)
    const bf16_t *res;    // residual [B][RH][RW][Cout] or null; added before relu / raw store
    const float *in_scale; // optional per-INPUT-channel affine + ReLU applied to the im2col operand (1x1 convs
    const float *in_shift; // only): x' = relu(x * in_scale[c] + in_shift[c]) -- the BN+ReLU of the producer unit
    const float *scale2;  // second output: act = relu(v * scale2 + shift2), or null
    const float *shift2;
    bf16_t *y;            // primary output [B][Ho][Wo][ldy] at channel offset y_coff (null: skip)
    bf16_t *y2;           // activated second output [B][Ho][Wo][Cout] or null
    float *yf;            // f32 output [B][Ho][Wo][Cout] (heads) or null
    int B, H, W, Cin, Cout, KH, KW, stride, pad, Ho, Wo;
    int H2, W2, Cin2, stride2;
    int ldy, y_coff;      // primary output row pitch (channels) and channel offset (SSH concat)
    int ldx, x_coff;      // input row pitch (channels per pixel, >= Cin) and channel offset: reads a channel slice
    int y_split, y_split_add; // output channels >= y_split land y_split_add further (two destinations, one GEMM)
    int n_valid;          // primary-output channels >= n_valid (zero-padded weight rows) are not stored
    int relu;             // relu on the primary output
    int res_up2;          // residual is half resolution: read at (ho/2, wo/2) (FPN nearest 2x)
    int res_post;         // add the residual AFTER the ReLU (FPN: relu(lateral) + upsampled)
    int force_tile;       // ConvTile: TILE_HEURISTIC in production, a forced choice in tuning / tests
    int co_running;       // another chain of the same pass runs concurrently (batch split): affects the tile heuristic
    int head_softmax;     // heads: channels [0,4) are cls logits -> 2-class softmax pairs (a, A+a)
    int k_chunk_major;    // set by choose_conv: K order (chunk, ky, kx) instead of (ky, kx, chunk) (see conv_igemm_kernel)
    // back-to-back pair (OP_B2B beyond stage 1): after this 1x1 conv3 (+ residual -> y = the raw sum), the NEXT unit's conv1 on
    // relu(y * scale2 + shift2) -- or, for the last unit of a stage (y null), on its activated output y2 --:
    // t1 = relu(W1 . act + bias1), [B][H][W][N1], N1 = the next unit's bottleneck width (this Cin; 128 for the stage 1 -> 2 boundary).
    // choose_conv runs the pair in one kernel (pw_b2b_kernel, pw_pair_kernel) where that pays and as two launches otherwise: same bits.
    const bf16_t *w1;     // [n1][Cout] (row pitch Cout), or null: no pair
    const float *bias1;
    bf16_t *t1;
    int n1;               // conv1's output channels (128 or 256)
    int *fail;            // device word a kernel with bounded spin waits (kernels_ring.hip) sets when a wave gives up, or null
    // latency schedule (kernels_splitk.hip): set by Network::run for a pass of <= RFD_LATENCY_MAX_BATCH images of a latency context
    int latency;          // the layers conv_splitk_wants() accepts run as K segments over several workgroups
    float *sk_ws;         // f32 partial tiles [tile][segment][BM * BN] of this op's stream
    unsigned *sk_cnt;     // this op's arrival counters [tile]: zero between launches
    size_t sk_ws_bytes;   // capacities, checked on the host before every launch
    int sk_cnt_n;
};
// ---- kernel choice (conv_select.hip): pure host functions; the launchers below execute what they return ----
// ConvParams::force_tile / rfd_debug_set_conv_tile.  "Persistent kernels": pw_stream, pw_wide, pw_gemm, conv3x3_c64, conv3x3_halo,
// the pair kernels and stage 1's persistent back-to-back forms; each runs a layer only from a size threshold in production.
enum ConvTile : int {
    TILE_HEURISTIC = 0,        // production: every rule by its measured size threshold
    TILE_128 = 1,              // generic 128 x 128 tile, four waves, 2 slots (128 x 192: four waves); no persistent, merged-kx or pair kernel,
                               // stage 1's pairs in the one-tile kernel
    TILE_256x128 = 2,          // generic 256 x 128 tile; otherwise as TILE_128
    TILE_256x64 = 3,           // 256 x 64 instead of 128 x 64 on the layers the generic rules give a 64-wide tile
    TILE_NO_128 = 4,           // never a 128-wide generic tile: 128 x 64 / 128 x 32
    TILE_NO_PW_STREAM = 5,     // none of the persistent convolution or pair kernels (stage 1's back-to-back forms keep their size rule, as
                               // under every tile that does not name them); the merged-kx 3x3 kernel stays
    TILE_PERSISTENT = 6,       // every persistent kernel wherever its shape rule holds, whatever the size
    TILE_GENERIC = 7,          // as TILE_NO_PW_STREAM, and stage 1's pairs in the one-tile kernel
    TILE_PW_STREAM = 8,        // of the persistent kernels only pw_stream, by its size rule
    TILE_C64 = 9,              // of the persistent kernels only conv3x3_c64, by its size rule
    TILE_PW_STREAM_K128 = 10,  // as TILE_PW_STREAM for the K = 128 layers alone
    TILE_PW_STREAM_K256 = 11,  // as TILE_PW_STREAM for the K = 256 layers alone
    TILE_PW_WIDE = 12,         // pw_wide wherever its shape rule holds, whatever the size
    TILE_HALO_SMALL = 13,      // conv3x3_halo with its smallest work item, whatever the size
    TILE_HALO_LARGE = 14,      // conv3x3_halo with its largest work item, whatever the size
    TILE_PW_GEMM = 15,         // pw_gemm with 256 x 128 items (never the wide item), whatever the size
    TILE_PAIR = 16,            // the fused pair kernels whatever the size (stage 1: pw_pair); a pair run as two convolutions: heuristic
    TILE_RING = 17,            // the loader / consumer ring wherever its shape rule holds
    TILE_128_EIGHT_WAVES = 18, // generic 128 x 128 tile with eight waves on every Cout % 128 == 0 layer without input affine
    TILE_KX_FOUR_WAVES = 19,   // the merged-kx 3x3 kernel (and the 128 x 192 tile) in the four-wave form
    TILE_COUNT = 20
};

// every shipped conv-path instantiation: id, display name (the string rocprofv3 reports, without the rfd:: prefix)
#define RFD_CONV_KERNELS(X)                                                                           \
    X(K_STEM, "stem_kernel")                                                                          \
    X(K_STEM_PERSISTENT, "stem_persistent_kernel<false>")                                             \
    X(K_STEM_PERSISTENT_CONV1, "stem_persistent_kernel<true>")                                        \
    X(K_FIRST3X3, "first3x3_kernel")                                                                  \
    X(K_DWCONV3X3, "dwconv3x3_kernel")                                                                \
    X(K_B2B_S1, "conv_b2b_s1_kernel")                                                                 \
    X(K_B2B_S1_PERSISTENT, "conv_b2b_s1_persistent_kernel")                                           \
    X(K_B2B_S1_PERSISTENT_K128, "conv_b2b_s1_persistent_k128_kernel")                                 \
    X(K_IGEMM_256_128_4_2_3, "conv_igemm_kernel<256, 128, 4, 2, 3, false>")                           \
    X(K_IGEMM_256_128_4_2_3_CM, "conv_igemm_kernel<256, 128, 4, 2, 3, true>")                         \
    X(K_IGEMM_128_128_2_2_2, "conv_igemm_kernel<128, 128, 2, 2, 2, false>")                           \
    X(K_IGEMM_128_128_2_2_2_CM, "conv_igemm_kernel<128, 128, 2, 2, 2, true>")                         \
    X(K_IGEMM_128_128_4_2_3, "conv_igemm_kernel<128, 128, 4, 2, 3, false>")                           \
    X(K_IGEMM_128_128_4_2_3_CM, "conv_igemm_kernel<128, 128, 4, 2, 3, true>")                         \
    X(K_IGEMM_128_128_2_2_3, "conv_igemm_kernel<128, 128, 2, 2, 3, false>")                           \
    X(K_IGEMM_128_192_2_2_2, "conv_igemm_kernel<128, 192, 2, 2, 2, false>")                           \
    X(K_IGEMM_128_192_2_2_2_CM, "conv_igemm_kernel<128, 192, 2, 2, 2, true>")                         \
    X(K_IGEMM_128_192_4_2_2, "conv_igemm_kernel<128, 192, 4, 2, 2, false>")                           \
    X(K_IGEMM_128_192_4_2_2_CM, "conv_igemm_kernel<128, 192, 4, 2, 2, true>")                         \
    X(K_IGEMM_256_64_4_1_2, "conv_igemm_kernel<256, 64, 4, 1, 2, false>")                             \
    X(K_IGEMM_128_64_4_1_2, "conv_igemm_kernel<128, 64, 4, 1, 2, false>")                             \
    X(K_IGEMM_128_32_4_1_2, "conv_igemm_kernel<128, 32, 4, 1, 2, false>")                             \
    X(K_CONV3X3_KX_128_2_2, "conv3x3_kx_kernel<128, 2, 2>")                                           \
    X(K_CONV3X3_KX_128_4_2, "conv3x3_kx_kernel<128, 4, 2>")                                           \
    X(K_CONV3X3_C64, "conv3x3_c64_kernel")                                                            \
    X(K_HALO_40_6_6, "conv3x3_halo_kernel<40, 6, 6>")                                                 \
    X(K_HALO_16_16_6, "conv3x3_halo_kernel<16, 16, 6>")                                               \
    X(K_HALO_16_16_8, "conv3x3_halo_kernel<16, 16, 8>")                                               \
    X(K_HALO_40_6_4, "conv3x3_halo_kernel<40, 6, 4>")                                                 \
    X(K_HALO_16_16_4, "conv3x3_halo_kernel<16, 16, 4>")                                               \
    X(K_PW_STREAM_1_Y2, "pw_stream_kernel<1, false, true>")                                           \
    X(K_PW_STREAM_2_Y, "pw_stream_kernel<2, true, false>")                                            \
    X(K_PW_STREAM_2_Y2, "pw_stream_kernel<2, false, true>")                                           \
    X(K_PW_STREAM_4_Y, "pw_stream_kernel<4, true, false>")                                            \
    X(K_PW_STREAM_4_Y2, "pw_stream_kernel<4, false, true>")                                           \
    X(K_PW_B2B_2, "pw_b2b_kernel<2, false>")                                                          \
    X(K_PW_PAIR_2_1_RAW_4, "pw_pair_kernel<2, 1, false, 4, 0, false>")                                \
    X(K_PW_PAIR_4_2_RAW, "pw_pair_kernel<4, 2, false, 0, 0, false>")                                  \
    X(K_PW_PAIR_2_2_ACT, "pw_pair_kernel<2, 2, true, 0, 0, false>")                                   \
    X(K_PW_PAIR_1_1_ACT_0_2, "pw_pair_kernel<1, 1, true, 0, 2, false>")                               \
    X(K_PW_PAIR_1_1_RAW_1_2_HALF, "pw_pair_kernel<1, 1, false, 1, 2, true>")                          \
    X(K_PW_PAIR_1_1_RAW_0_2_HALF, "pw_pair_kernel<1, 1, false, 0, 2, true>")                          \
    X(K_PW_GEMM, "pw_gemm_kernel<false, false>")                                                      \
    X(K_PW_GEMM_WIDE, "pw_gemm_kernel<false, true>")                                                  \
    X(K_PW_GEMM_AFF, "pw_gemm_kernel<true, false>")                                                   \
    X(K_PW_GEMM_AFF_WIDE, "pw_gemm_kernel<true, true>")                                               \
    X(K_PW_WIDE, "pw_wide_kernel")                                                                    \
    X(K_RING, "conv_ring_kernel<false>")                                                              \
    X(K_RING_KX3, "conv_ring_kernel<true>")                                                           \
    X(K_SPLITK_64_64_2_2, "conv_splitk_kernel<64, 64, 2, 2>")
enum ConvKernel : int {
    K_NONE = 0,
#define RFD_ID(id, name) id,
    RFD_CONV_KERNELS(RFD_ID)
#undef RFD_ID
};
const char *conv_kernel_name(ConvKernel k);

struct ConvStep {
    ConvKernel kernel;
    ConvParams p; // what the kernel runs with: k_chunk_major set, the two convolutions of an unfused pair derived
};
struct ConvPlan {
    int steps; // 1, or 2: a pair run as its two convolutions
    ConvStep step[2];
};
// The pair kernels address both filter banks through ONE 32-bit buffer descriptor based at the first: the second must lie behind
// it, within 1 GiB.  A relation of the banks' offsets into the weight buffer, wherever that buffer is.
static inline bool bank_behind(const bf16_t *w, const bf16_t *w1) { return (uintptr_t)w1 > (uintptr_t)w && (uintptr_t)w1 - (uintptr_t)w < (1u << 30); }
// validates p (launch_conv's errors, in its order) and fills the plan
int choose_conv(const ConvParams &p, bool w1_behind_w, ConvPlan *plan);
int launch_conv(const ConvParams &p, hipStream_t s); // validate, choose, execute

// split-K form of the generic implicit-GEMM tile (kernels_splitk.hip; the latency schedule).  The plan is a pure function of the
// layer (K, Cout), the pixels of one image and -- for the grid and the workspace only -- the batch.
constexpr int kSplitKMaxSegments = 8;
struct SplitKPlan {
    int S, bm, bn;    // K segments, tile
    int tiles;        // output tiles = arrival counters
    size_t ws_bytes;  // tiles * S * bm * bn f32
};
int conv_splitk_segments(int nk);
bool conv_splitk_plan(int K, int Cout, int HoWo, int B, SplitKPlan *pl);
bool conv_splitk_wants(const ConvParams &p, SplitKPlan *pl); // false: the throughput kernels run the layer
int launch_conv_splitk(const ConvParams &p, hipStream_t s);
// wave-specialised loader / consumer ring form of the 128 x 128 implicit-GEMM tile (kernels_ring.hip)
bool conv_ring_supports(const ConvParams &p, bool *kx3);
int launch_conv_ring(const ConvParams &p, hipStream_t s);
int device_cus(); // CU count of the current device (cached per device)
// entry i of the list of persistent kernels (name prefix, dynamic LDS every launch of it requests); returns the list length
int persistent_kernel_table(int i, const char **name, size_t *lds_bytes);
// ---- f32 parity mode (kernels_f32.hip): ConvParams with f32 tensors and weights; same field meanings ----
struct ConvF32Params {
    const float *x, *w, *x2;   // [B][H][W][ldx] (channel slice at x_coff), [Cout][ldw], optional [B][H2][W2][Cin2]
    const float *bias, *bias2; // [Cout]; the fused shortcut's bias or null
    const float *res;          // residual [B][RH][RW][Cout] or null
    const float *in_scale, *in_shift, *scale2, *shift2;
    float *y, *y2, *yf;
    int B, H, W, Cin, Cout, KH, KW, stride, pad, Ho, Wo;
    int H2, W2, Cin2, stride2;
    int ldw;                   // weight row pitch in elements (KH*KW*Cin + Cin2)
    int ldy, y_coff, ldx, x_coff, y_split, y_split_add, n_valid;
    int relu, res_up2, res_post, head_softmax;
};
int launch_conv_f32(const ConvF32Params &p, hipStream_t s);
int launch_conv0_f32(const bf16_t *x4, const float *w, const float *bias, float *y, int B, int H, int W, hipStream_t s);
int launch_maxpool_f32(const float *x, float *y, const float *scale, const float *shift, int B, int H, int W, int C, hipStream_t s);

// back-to-back fusion (stage 1): raw = conv3(x) [+ 1x1 shortcut(x2)] + bias (+ res); t1 = relu(conv1(relu(raw*scale+shift)) + bias1)
struct B2BParams {
    const bf16_t *x, *x2;      // [M][Cin], optional [M][Cin2] (stride-1 shortcut source)
    const bf16_t *w3;          // [256][Cin + Cin2]
    const float *bias3, *bias3b; // conv3 bias, shortcut bias (or null)
    const bf16_t *res;         // [M][256] or null
    const float *scale, *shift; // the unit's post-add affine
    bf16_t *raw;               // [M][256]
    const bf16_t *w1;          // [64][256]
    const float *bias1;
    bf16_t *t1;                // [M][64]
    int B, H, W, Cin, Cin2;
    int force_tile;            // as ConvParams::force_tile
};
// st->kernel: one of stage 1's three kernels (they run with p itself), or a pw_pair form with its parameters in st->p
void choose_b2b_s1(const B2BParams &p, bool w1_behind_w3, ConvStep *st);
int launch_conv_b2b_s1(const B2BParams &p, hipStream_t s);
// fused stem: conv0 (7x7/2 + bias + ReLU) -> 3x3/2 max pool -> affine + ReLU, NHWC4 in, [B][H/4][W/4][64] out
// w1 / bias1 / t1 / fused (all or none): the first unit's conv1 (1x1, 64 -> 64, bias + ReLU) computed on the pooled tile and stored to
// t1 when the persistent form runs; *fused tells the caller whether it was (then the conv's own op must not run)
constexpr int kStemPH = 4, kStemPW = 16; // pooled tile of a stem workgroup
ConvKernel choose_stem(int B, int H, int W, bool conv1_offered, int force_tile, int cus); // K_STEM, K_STEM_PERSISTENT or K_STEM_PERSISTENT_CONV1
int launch_stem(const bf16_t *x4, const bf16_t *w, const float *bias, const float *scale, const float *shift,
                bf16_t *y, int B, int H, int W, hipStream_t s, int force_tile = 0, const bf16_t *w1 = nullptr,
                const float *bias1 = nullptr, bf16_t *t1 = nullptr, bool *fused = nullptr);
// MobileNet-0.25 helpers: first 3x3/2 conv (3 -> 8 real channels, output padded to Cd) and depthwise 3x3
int launch_first3x3(const bf16_t *x4, const bf16_t *w, const float *bias, bf16_t *y, int B, int H, int W, int Cd,
                    hipStream_t s);
int launch_dwconv3x3(const bf16_t *x, const bf16_t *w, const float *bias, bf16_t *y, int B, int H, int W, int C,
                     int stride, hipStream_t s);
// head tensors [B][h][w][32] f32 (cls4 bbox8 lmk20) -> reference NCHW contract (rfd_forward)
int launch_heads_to_nchw(const float *h32, float *cls, float *bbox, float *lmk, int B, int fh,
                         int fw, hipStream_t s);

} // namespace rfd
