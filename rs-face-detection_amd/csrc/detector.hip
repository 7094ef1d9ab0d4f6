// detector.hip -- host side of the detection stage: the C++ mirror of the reference's
// `RetinaFaceDetection` (src/pipeline/module/face_detection.rs:19-513) driving the HIP kernels, and
// the C ABI of include/rfd.h on top of it.  (The reference's host language, Rust, has no toolchain
// in this image; INTEGRATION.md shows the `extern "C"` facade that keeps its `call` signature.)
// This file is the context (rfd_ctx, private to it) and the detection alone: frames in, network, decode / sort / NMS, the
// views, the pipelined and multi-GPU entries, weights, and the test hooks of those.  Every other stateful layer of the ABI has a
// file of its own and sees the context through ctx_access.h: the face stage behind the detection (face_host.hip), the JPEG decode
// (jpeg_host.hip), the JPEG encode (jpeg_encode_host.hip), the frame conversion (frame_host.hip), the shot quality (shot_quality_host.hip), the redaction (redact_host.hip), the annotation (annotate_host.hip), the face gallery
// (gallery_host.hip) and the tracker (tracker_host.hip).
#include <dlfcn.h>
#include <stdarg.h>
#include <stdlib.h>

#include <algorithm>
#include <cmath>
#include <memory>
#include <mutex>
#include <vector>

#include "annotate_host.h"
#include "ctx_access.h"
#include "face_host.h"
#include "frame_host.h"
#include "host_resources.h"
#include "jpeg_encode_host.h"
#include "jpeg_host.h"
#include "network.h"
#include "redact_host.h"
#include "shot_quality_host.h"
#include "view_plan.h"

namespace rfd {

static thread_local char g_err[512] = "";

void set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
}
const char *get_error() { return g_err; }

// ---- anchors: generate_anchors_fpn2 with the production config (face_detection.rs:55-98,
//      generate_anchors.rs:20-39, 61-93, 116-157); f32 arithmetic in the reference's order ----
static void make_base_anchors(float out[kNumLevels][kA][4])
{
    static const float scales[kNumLevels][kA] = {{32.f, 16.f}, {8.f, 4.f}, {2.f, 1.f}};
    const int base_size = 16;
    const float ratio = 1.0f;
    for (int l = 0; l < kNumLevels; ++l) {
        // base anchor [0,0,15,15] -> (w,h,ctr)
        const float b0 = 1.0f - 1.0f, b2 = (float)base_size - 1.0f;
        float w = b2 - b0 + 1.0f, h = b2 - b0 + 1.0f;
        float xc = b0 + 0.5f * (w - 1.0f), yc = b0 + 0.5f * (h - 1.0f);
        // _ratio_enum
        const float ws = roundf(sqrtf(w * h / ratio)), hs = ws * ratio;
        const float r0 = xc - 0.5f * (ws - 1.0f), r1 = yc - 0.5f * (hs - 1.0f);
        const float r2 = xc + 0.5f * (ws - 1.0f), r3 = yc + 0.5f * (hs - 1.0f);
        // _scale_enum
        w = r2 - r0 + 1.0f; h = r3 - r1 + 1.0f;
        xc = r0 + 0.5f * (w - 1.0f); yc = r1 + 0.5f * (h - 1.0f);
        for (int a = 0; a < kA; ++a) {
            const float sw = w * scales[l][a], sh = h * scales[l][a];
            out[l][a][0] = xc - 0.5f * (sw - 1.0f);
            out[l][a][1] = yc - 0.5f * (sh - 1.0f);
            out[l][a][2] = xc + 0.5f * (sw - 1.0f);
            out[l][a][3] = yc + 0.5f * (sh - 1.0f);
        }
    }
}

// ---- _preprocess geometry (face_detection.rs:140-153) + cv::resize's scale bookkeeping ----
static void letterbox(int img_h, int img_w, int size_w, int size_h, PreImage *pi, float *det_scale)
{
    const float im_ratio = (float)img_h / (float)img_w;
    const float model_ratio = (float)size_h / (float)size_w;
    int new_w, new_h;
    if (im_ratio > model_ratio) {
        new_h = size_h;
        new_w = (int)((float)new_h / im_ratio);
    } else {
        new_w = size_w;
        new_h = (int)((float)new_w * im_ratio);
    }
    *det_scale = (float)new_h / (float)img_h;
    pi->h = img_h; pi->w = img_w; pi->new_w = new_w; pi->new_h = new_h; pi->pad = 0;
    pi->scale_x = pi->scale_y = 1.0;
    pi->area_fast = 0;
    if (new_w > 0 && new_h > 0) {
        const ResizeScale r = resize_scale(img_w, img_h, new_w, new_h);
        pi->scale_x = r.scale_x; pi->scale_y = r.scale_y; pi->area_fast = r.area_fast;
    }
}

// ---- RCCL, bound at run time: single-GPU users (and the CPU-side ABI tests) never load the 500 MB library.  Only the
//      handful of entry points the gather needs; types restated from rccl.h (ABI-stable since NCCL 2.0). ----
struct Rccl {
    typedef struct { char internal[RFD_COMM_ID_BYTES]; } UniqueId;
    typedef void *Comm;
    enum { kInt32 = 2 }; // ncclInt32
    int (*GetUniqueId)(UniqueId *) = nullptr;
    int (*CommInitRank)(Comm *, int, UniqueId, int) = nullptr;
    int (*CommDestroy)(Comm) = nullptr;
    int (*AllGather)(const void *, void *, size_t, int, Comm, hipStream_t) = nullptr;
    int (*GroupStart)() = nullptr;
    int (*GroupEnd)() = nullptr;
    const char *(*GetErrorString)(int) = nullptr;
    void *handle = nullptr;
    bool ok = false;
};
static Rccl g_rccl;
static std::mutex g_rccl_mu;

static int rccl_load()
{
    std::lock_guard<std::mutex> lk(g_rccl_mu);
    if (g_rccl.ok) return RFD_OK;
    const char *env = getenv("RFD_RCCL_LIB");
    void *h = nullptr;
    if (env && *env) h = dlopen(env, RTLD_NOW | RTLD_GLOBAL);
    // a copy some other component of the process already loaded (e.g. the one PyTorch bundles) comes first: one RCCL per process
    static const char *names[] = {"librccl.so", "librccl.so.1"};
    for (int pass = 0; pass < 2 && !h; ++pass)
        for (const char *nm : names) {
            h = dlopen(nm, RTLD_NOW | RTLD_GLOBAL | (pass == 0 ? RTLD_NOLOAD : 0));
            if (h) break;
        }
    if (!h) h = dlopen("/opt/rocm/lib/librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!h) {
        const char *why = dlerror(); // NULL when the last attempt was a NOLOAD probe that found nothing
        set_error("librccl could not be loaded (%s); set RFD_RCCL_LIB", why ? why : "not found on the loader path");
        return RFD_ERR_COMM;
    }
    Rccl r;
    r.handle = h;
    r.GetUniqueId = (decltype(r.GetUniqueId))dlsym(h, "ncclGetUniqueId");
    r.CommInitRank = (decltype(r.CommInitRank))dlsym(h, "ncclCommInitRank");
    r.CommDestroy = (decltype(r.CommDestroy))dlsym(h, "ncclCommDestroy");
    r.AllGather = (decltype(r.AllGather))dlsym(h, "ncclAllGather");
    r.GroupStart = (decltype(r.GroupStart))dlsym(h, "ncclGroupStart");
    r.GroupEnd = (decltype(r.GroupEnd))dlsym(h, "ncclGroupEnd");
    r.GetErrorString = (decltype(r.GetErrorString))dlsym(h, "ncclGetErrorString");
    if (!r.GetUniqueId || !r.CommInitRank || !r.CommDestroy || !r.AllGather || !r.GroupStart || !r.GroupEnd || !r.GetErrorString) {
        set_error("the loaded librccl lacks a required entry point");
        (void)dlclose(h); // do not keep a handle per failed attempt
        return RFD_ERR_COMM;
    }
    r.ok = true;
    g_rccl = r;
    return RFD_OK;
}

#define RFD_RCCL(expr)                                                                                      \
    do {                                                                                                    \
        const int _r = (expr);                                                                              \
        if (_r != 0) {                                                                                      \
            ::rfd::set_error("%s failed: %s (%s:%d)", #expr, g_rccl.GetErrorString(_r), __FILE__, __LINE__); \
            return RFD_ERR_COMM;                                                                            \
        }                                                                                                   \
    } while (0)

} // namespace rfd

using namespace rfd;

// The context = the reference's `RetinaFaceDetection` struct (face_detection.rs:19-38) minus the
// Triton client/model config, plus device state.
struct rfd_ctx {
    rfd_config cfg;
    // The streams come first, so that they are destroyed last: after every event recorded on them and every buffer their
    // commands use.  `stream` is the caller's (rfd_set_stream) or own_stream.
    Stream own_stream, copy_stream, d2h_stream;
    hipStream_t stream = nullptr;
    Event ev[10];
    float base_anchor[kNumLevels][kA][4];
    int fh[kNumLevels], fw[kNumLevels], level_off[kNumLevels], total_anchors = 0;
    Network net;
    bool net_created = false;
    // device state sized for max_batch_size
    DevBuf staging, imgs, in4, rows, keys, sorted_keys, sorted_boxes, count, det_scale;
    // chunked NMS (dense crowds): kept-box lists, and nms_state, in ints:
    //   {count, epoch} of every chunk [max_batch_size][kNmsChunks] | the fault word | pad | the two chunk-ticket counters (8-byte aligned)
    // The fault word is the one sticky word every bounded device-side wait reports into (check_nms_flag).
    DevBuf nms_kept, nms_state;
    size_t fault_word_index() const { return (size_t)cfg.max_batch_size * kNmsChunks * 2; }
    size_t nms_state_ints() const { return fault_word_index() + 4; }
    int *fault_word() const { return (int *)nms_state.p + fault_word_index(); }
    int nms_epoch = 0;
    int nms_ticket_sel = 0;  // which of the two chunk-ticket counters the next chunked NMS launch draws from
    bool nms_chunked = true; // RFD_NMS_CHUNKED=0: one workgroup per image always (A/B and fallback)
    // host mirror (page-locked) of the fault word: copied stream-ordered behind every NMS launch, looked at wherever the host
    // synchronises with the stream (check_nms_flag)
    Pinned<int> h_nms_flag;
    DevBuf out_boxes, out_lmk, out_count, out_total, out_gidx;
    DevBuf scratch[12];
    FaceStage face; // selection, alignment, model inputs, face list, liveness (rfd.h): face_host.h
    // Per-call descriptors travel through rings of page-locked slots, so enqueueing never blocks on the previous call.
    static constexpr int kRing = 4;
    PinnedRing<kRing> frame_ring; // PreImage [B] | det_scale f32 [B]; its events can be timed
    // views (rfd.h, "views"), both allocated by the first views call: the per-view descriptors of decode_views_kernel
    DevBuf view_desc;
    PinnedRing<kRing> views_ring; // ViewDesc [B]
    JpegDecoder jpeg; // JPEG decode (rfd.h, "JPEG decode"): jpeg_host.h
    ShotQuality shot; // shot quality (rfd.h, "shot quality"): shot_quality_host.h
    FrameConvert frames; // frames in camera and decoder formats (rfd.h): frame_host.h
    JpegEncoder encoder; // JPEG encode (rfd.h, "JPEG encode"): jpeg_encode_host.h
    Redact redact; // redaction (rfd.h, "redaction"): redact_host.h
    Annotate annotate; // annotation (rfd.h, "annotation"): annotate_host.h
    // pipelined host entry (rfd_submit_batch / rfd_collect_batch): two slots, H2D on its own stream
    struct PipeSlot {
        DevBuf frames, imgs, scale, ob, ol, oc, ot;
        Pinned<PreImage> pin_imgs;
        Pinned<float> pin_scale, h_ob, h_ol;
        Pinned<int> h_oc, h_ot;
        Event h2d, done, post;
        int n = 0;
    };
    static constexpr int kPipe = 2;
    static constexpr int kPipeRows = 128; // rows per image the pipelined entry copies back unconditionally
    PipeSlot pipe[kPipe];
    int pipe_head = 0, pipe_tail = 0, pipe_inflight = 0;
    // cross-call overlap (rfd_detect_batch_device, async = 2): per-parity descriptors and events
    DevBuf ov_imgs[2], ov_scale[2];
    Event ov_chain_done[2][2], ov_post_done[2], ov_desc;
    bool ov_post_valid[2] = {false, false};
    int ov_parity = 0;
    // batch size of the previous call if it ran in the overlap mode, else -1: the part boundary (n+1)/2 and with it the
    // workspace / input slices of the two chains depend on n, and every other entry point runs the network on the
    // caller's stream, so a chain may start under the previous call only when that call had the same shape
    int ov_last_n = -1;
    Event ov_resync;
    // multi-GPU: RCCL communicator of this rank (rfd_comm_init)
    Rccl::Comm comm = nullptr;
    int comm_rank = 0, comm_world = 0;
    rfd_stats stats;
    float conv_ms = 0.f;
    double conv_flops = 0.0;
    int conv_launches = 0;

    int ensure_network()
    {
        if (net_created) return RFD_OK;
        RFD_TRY(net.create(cfg.backbone, cfg.image_w, cfg.image_h, cfg.max_batch_size, cfg.precision, cfg.schedule));
        net.d_fail = fault_word(); // the ring convolutions' bounded spins report into the same device word as the chunked NMS
        net_created = true;
        return RFD_OK;
    }
};

namespace {

int ctx_alloc(rfd_ctx *c)
{
    const size_t B = (size_t)c->cfg.max_batch_size, NA = (size_t)c->total_anchors, MD = (size_t)c->cfg.max_det;
    RFD_TRY(c->imgs.reserve(B * sizeof(PreImage)));
    RFD_TRY(c->rows.reserve(B * NA * kDetRow * sizeof(float)));
    RFD_TRY(c->keys.reserve(B * NA * sizeof(uint64_t)));
    RFD_TRY(c->sorted_keys.reserve(B * NA * sizeof(uint64_t)));
    RFD_TRY(c->sorted_boxes.reserve(B * NA * sizeof(float4)));
    RFD_TRY(c->nms_kept.reserve(B * NA * sizeof(float4)));
    RFD_TRY(c->nms_state.reserve(c->nms_state_ints() * sizeof(int)));
    RFD_HIP(hipMemset(c->nms_state.p, 0, c->nms_state_ints() * sizeof(int)));
    RFD_HIP(hipDeviceSynchronize()); // the fill runs on the NULL stream, which the context's non-blocking stream is not ordered with
    RFD_TRY(c->count.reserve(B * sizeof(int)));
    RFD_TRY(c->det_scale.reserve(B * sizeof(float)));
    RFD_TRY(c->out_boxes.reserve(B * MD * 5 * sizeof(float)));
    RFD_TRY(c->out_lmk.reserve(B * MD * 10 * sizeof(float)));
    RFD_TRY(c->out_count.reserve(B * sizeof(int)));
    RFD_TRY(c->out_total.reserve(B * sizeof(int)));
    RFD_TRY(c->out_gidx.reserve(B * MD * sizeof(int)));
    return RFD_OK;
}

// n images fit the context; the error names them as "<what> n<unit>"
int check_batch(const rfd_ctx *c, int n, const char *what, const char *unit = "")
{
    if (n < 1 || n > c->cfg.max_batch_size) {
        set_error("%s %d%s exceeds max_batch_size %d", what, n, unit, c->cfg.max_batch_size);
        return RFD_ERR_CAPACITY;
    }
    return RFD_OK;
}

int check_images(const rfd_ctx *c, const rfd_image *imgs, int n)
{
    RFD_CHECK_ARG(imgs != nullptr, "imgs is null");
    RFD_TRY(check_batch(c, n, "batch of", " frames"));
    for (int i = 0; i < n; ++i) {
        RFD_CHECK_ARG(imgs[i].data != nullptr, "frame data is null");
        RFD_CHECK_ARG(imgs[i].height > 0 && imgs[i].width > 0, "frame has a non-positive size");
        RFD_CHECK_ARG(imgs[i].stride >= (ptrdiff_t)imgs[i].width * 3, "frame stride < width*3 (frames must be 3-channel 8-bit)");
    }
    return RFD_OK;
}

size_t frames_bytes(const rfd_image *imgs, int n) // packed back to back with tight rows
{
    size_t total = 0;
    for (int i = 0; i < n; ++i) total += (size_t)imgs[i].height * imgs[i].width * 3;
    return total;
}

// Where the kernels read frame i: the two leading members of descriptor i (PreImage, LiveImage), the descriptors `pitch` bytes
// apart.  Device frames are read where they lie; host frames are packed into c->staging on the context's stream, one 2-D copy
// each.
struct FrameWhere {
    const uint8_t *src;
    long long stride;
};
static_assert(offsetof(PreImage, src) == 0 && offsetof(PreImage, stride) == offsetof(FrameWhere, stride) &&
              offsetof(LiveImage, src) == 0 && offsetof(LiveImage, stride) == offsetof(FrameWhere, stride),
              "place_frames writes src and stride there");

int place_frames(rfd_ctx *c, const rfd_image *imgs, int n, bool frames_on_device, void *desc, size_t pitch)
{
    if (!frames_on_device) RFD_TRY(c->staging.reserve(frames_bytes(imgs, n)));
    size_t off = 0;
    for (int i = 0; i < n; ++i) {
        FrameWhere w = {imgs[i].data, (long long)imgs[i].stride};
        if (!frames_on_device) {
            uint8_t *dst = (uint8_t *)c->staging.p + off;
            const size_t row = (size_t)imgs[i].width * 3;
            RFD_HIP(hipMemcpy2DAsync(dst, row, imgs[i].data, (size_t)imgs[i].stride, row, imgs[i].height,
                                     hipMemcpyHostToDevice, c->stream));
            w = FrameWhere{dst, (long long)row};
            off += row * imgs[i].height;
        }
        memcpy((char *)desc + (size_t)i * pitch, &w, sizeof w);
    }
    return RFD_OK;
}

// The letterbox geometry of frame i (all of *pi but src / stride) and its det_scale.
int fill_pre_image(const rfd_ctx *c, const rfd_image &im, int i, PreImage *pi, float *det_scale)
{
    letterbox(im.height, im.width, c->cfg.image_w, c->cfg.image_h, pi, det_scale);
    if (pi->new_w <= 0 || pi->new_h <= 0) { // the reference's cv::resize errors out on an empty dsize (face_detection.rs:156-159)
        set_error("invalid argument: frame %d (%dx%d) letterboxes to an empty %dx%d image", i, im.width, im.height, pi->new_w, pi->new_h);
        return RFD_ERR_INVALID_ARG;
    }
    return RFD_OK;
}

// The next slot of the frame ring: descriptors and det_scales of up to max_batch_size frames, one event for both.
int acquire_frame_slot(rfd_ctx *c, PreImage **pis, float **scales)
{
    RFD_TRY(c->frame_ring.acquire(pis));
    *scales = (float *)(*pis + c->cfg.max_batch_size);
    return RFD_OK;
}

// Stage the frames (host or device resident) and their letterbox geometry on the device.  A frame that cannot be letterboxed
// refuses the call before anything is enqueued.
int stage_frames(rfd_ctx *c, const rfd_image *imgs, int n, bool frames_on_device, const float **det_scales = nullptr)
{
    PreImage *pis;
    float *pin_scales;
    RFD_TRY(acquire_frame_slot(c, &pis, &pin_scales));
    for (int i = 0; i < n; ++i) RFD_TRY(fill_pre_image(c, imgs[i], i, &pis[i], &pin_scales[i]));
    if (det_scales) *det_scales = pin_scales; // the slot: good until kRing - 1 more calls have taken theirs
    RFD_TRY(place_frames(c, imgs, n, frames_on_device, pis, sizeof *pis));
    RFD_HIP(hipMemcpyAsync(c->imgs.p, pis, n * sizeof(PreImage), hipMemcpyHostToDevice, c->stream));
    RFD_HIP(hipMemcpyAsync(c->det_scale.p, pin_scales, n * sizeof(float), hipMemcpyHostToDevice, c->stream));
    return c->frame_ring.record(c->stream);
}

// preprocess parameters for the frames whose descriptors start at `imgs` (device); into the network's input from image `net_off`
// on, or (net_off < 0) with no output chosen yet
PreParams pre_params(const rfd_ctx *c, const void *imgs, int net_off)
{
    PreParams pp;
    memset(&pp, 0, sizeof pp);
    pp.imgs = (const PreImage *)imgs;
    pp.net_h = c->cfg.image_h; pp.net_w = c->cfg.image_w;
    if (net_off >= 0) pp.out_nhwc4 = (bf16_t *)c->net.tensor_ptr(c->net.g.input) + (size_t)net_off * c->cfg.image_h * c->cfg.image_w * 4;
    return pp;
}

// decode parameters; net_heads: with the heads of the network's own pass (of the current head parity) filled in
DecodeParams decode_params(const rfd_ctx *c, bool net_heads)
{
    DecodeParams p;
    memset(&p, 0, sizeof p);
    for (int l = 0; l < kNumLevels; ++l) {
        p.fh[l] = c->fh[l]; p.fw[l] = c->fw[l]; p.stride[l] = kStrides[l]; p.level_off[l] = c->level_off[l];
    }
    memcpy(p.base_anchor, c->base_anchor, sizeof p.base_anchor);
    p.total_anchors = c->total_anchors;
    p.net_h = c->cfg.image_h; p.net_w = c->cfg.image_w;
    p.conf_thr = c->cfg.confidence_threshold;
    p.rows = (float *)c->rows.p;
    p.keys = (uint64_t *)c->keys.p;
    p.count = (int *)c->count.p;
    for (int l = 0; net_heads && l < kNumLevels; ++l) p.cls[l] = (const float *)c->net.tensor_ptr(c->net.g.heads[l]);
    return p;
}

// the context's own detection slabs
rfd_dets own_slabs(const rfd_ctx *c)
{
    return rfd_dets{(float *)c->out_boxes.p, (float *)c->out_lmk.p, (int32_t *)c->out_count.p, (int32_t *)c->out_total.p};
}

// detection slabs of n images between host and device, on the context's stream; `total` travels if dst has one
int copy_slabs(rfd_ctx *c, const rfd_dets &dst, const rfd_dets &src, int n, hipMemcpyKind kind)
{
    const size_t MD = (size_t)c->cfg.max_det;
    RFD_HIP(hipMemcpyAsync(dst.boxes, src.boxes, n * MD * 5 * sizeof(float), kind, c->stream));
    RFD_HIP(hipMemcpyAsync(dst.landmarks, src.landmarks, n * MD * 10 * sizeof(float), kind, c->stream));
    RFD_HIP(hipMemcpyAsync(dst.count, src.count, n * sizeof(int), kind, c->stream));
    if (dst.total) RFD_HIP(hipMemcpyAsync(dst.total, src.total, n * sizeof(int), kind, c->stream));
    return RFD_OK;
}

// The views of a call as post_network sees them: n_views images of heads decoded into the lists of n frames, vmax slots each.
struct ViewsPost { const ViewDesc *desc; int n_views, vmax; float edge_margin; };

// decode -> sort -> NMS on device-resident heads; outputs to device slabs `o*`.  views: the n images of the sort and the NMS are
// frames of views->vmax * total_anchors anchors each, filled by decode_views_kernel from views->n_views images of heads.
int post_network(rfd_ctx *c, DecodeParams &dp, bool nchw, int n, float *oboxes, float *olmk, int *ocount,
                 int *ototal, int *ogidx, const float *det_scale = nullptr, const ViewsPost *views = nullptr)
{
    const int anchors = views ? views->vmax * c->total_anchors : c->total_anchors;
    RFD_HIP(hipMemsetAsync(c->count.p, 0, n * sizeof(int), c->stream));
    if (views) RFD_TRY(launch_decode_views(dp, views->desc, views->n_views, views->vmax, views->edge_margin, nchw, c->stream));
    else RFD_TRY(launch_decode(dp, n, nchw, c->stream));
    RFD_HIP(hipEventRecord(c->ev[4], c->stream));
    RFD_TRY(launch_sort((uint64_t *)c->keys.p, (const int *)c->count.p, (const float *)c->rows.p,
                        (uint64_t *)c->sorted_keys.p, (float4 *)c->sorted_boxes.p, anchors, n, c->stream));
    RFD_HIP(hipEventRecord(c->ev[5], c->stream));
    NmsParams np;
    memset(&np, 0, sizeof np);
    np.sorted_keys = (const uint64_t *)c->sorted_keys.p;
    np.sorted_boxes = (const float4 *)c->sorted_boxes.p;
    np.rows = (const float *)c->rows.p;
    np.count = (const int *)c->count.p;
    np.det_scale = det_scale ? det_scale : (const float *)c->det_scale.p;
    np.presorted_n = -1;
    np.total_anchors = anchors;
    np.max_det = c->cfg.max_det;
    np.iou_thr = c->cfg.iou_threshold;
    np.out_boxes = oboxes; np.out_lmk = olmk; np.out_count = ocount; np.out_total = ototal; np.out_gidx = ogidx;
    if (c->nms_chunked) { // kNmsChunks workgroups per image; images with few candidates are done by the first alone
        np.kept_boxes = (float4 *)c->nms_kept.p;
        np.chunk_state = (int *)c->nms_state.p;
        np.spin_fail = c->fault_word();
        np.ticket = (unsigned *)(np.spin_fail + 2);
        np.ticket_sel = c->nms_ticket_sel;
        c->nms_epoch = c->nms_epoch == 0x7fffffff ? 1 : c->nms_epoch + 1;
        np.epoch = c->nms_epoch;
    }
    bool used_chunked = false;
    RFD_TRY(launch_nms(np, n, c->stream, &used_chunked));
    if (used_chunked) c->nms_ticket_sel ^= 1; // that launch leaves its counter at the grid size and zeroes the other one
    RFD_HIP(hipEventRecord(c->ev[6], c->stream));
    // the device word is sticky (the kernel only ever sets it), so a later call's copy cannot hide an earlier give-up
    // (copied whether or not the chunked kernel ran: the ring convolutions of the network pass report into the same word)
    RFD_HIP(hipMemcpyAsync(c->h_nms_flag, c->fault_word(), sizeof(int), hipMemcpyDeviceToHost, c->stream));
    return RFD_OK;
}

// Call after the host has synchronised with c->stream.  A chunk workgroup of nms_chunked_kernel that gave up waiting for its
// predecessor (bounded spin; forward progress rests on in-order workgroup dispatch, which the hardware does not promise)
// produced a wrong kept set: that is an error, as every failure of the reference's call is an Err (face_detection.rs:498-509),
// never RFD_OK with wrong detections.
int check_nms_flag(rfd_ctx *c)
{
    if (!c->h_nms_flag || *c->h_nms_flag == 0) return RFD_OK;
    *c->h_nms_flag = 0;
    RFD_HIP(hipMemsetAsync(c->fault_word(), 0, sizeof(int), c->stream));
    RFD_HIP(hipStreamSynchronize(c->stream));
    set_error("a device-side bounded wait gave up (chunked NMS: a workgroup waiting for its predecessor chunk; ring convolution: a "
              "wave waiting for a ring slot; split-K convolution: an arrival counter left dirty by an earlier fault); the detections of the batches since the last synchronisation are invalid "
              "(re-submit them; RFD_NMS_CHUNKED=0 selects the one-workgroup-per-image NMS kernel, RFD_CONV_RING=0 the barrier-per-step convolutions)");
    return RFD_ERR_HIP;
}

int finish_stats(rfd_ctx *c, int n, bool have_pre, bool have_net)
{
    float ms;
    memset(&c->stats, 0, sizeof c->stats);
    auto el = [&](int a, int b) { return hipEventElapsedTime(&ms, c->ev[a], c->ev[b]) == hipSuccess ? ms : 0.f; };
    if (have_pre) { c->stats.ms_h2d = el(0, 1); c->stats.ms_preprocess = el(1, 2); }
    if (have_net) c->stats.ms_network = el(2, 3);
    c->stats.ms_decode = el(3, 4);
    c->stats.ms_sort = el(4, 5);
    c->stats.ms_nms = el(5, 6);
    c->stats.ms_d2h = el(6, 7);
    c->stats.ms_total = el(have_pre ? 0 : (have_net ? 2 : 3), 7);
    std::vector<int> cnt(n), tot(n);
    RFD_HIP(hipMemcpy(cnt.data(), c->count.p, n * sizeof(int), hipMemcpyDeviceToHost));
    for (int i = 0; i < n; ++i) c->stats.candidates += cnt[i];
    if (c->net_created && c->net.profiling) {
        RFD_TRY(c->net.collect_profile());
        c->conv_ms = 0.f; c->conv_flops = 0.0; c->conv_launches = 0;
        for (size_t i = 0; i < c->net.g.ops.size(); ++i)
            if (c->net.g.ops[i].kind == OP_CONV || c->net.g.ops[i].kind == OP_B2B) {
                c->conv_ms += c->net.op_ms[i];
                c->conv_flops += 2.0 * c->net.g.layer_macs((int)i) * n;
                ++c->conv_launches;
            }
    }
    return RFD_OK;
}

// Cross-call overlap (rfd_detect_batch_device with async = 2; frames and outputs in HBM, frames complete at call time).
// The two parts of the batch run as chains on their OWN streams (not the caller's): preprocess of the part -> network ->
// (side streams joined).  Nothing of call i+1 waits for call i except through the chain's own stream order, so the head
// of chain A of call i+1 overlaps the tail of chain B of call i and the decode / sort / NMS of call i, which stay on the
// caller's stream behind both chains.  Hazards and how they are closed:
//   heads, frame descriptors, det_scale : double-buffered by call parity; a chain of call i+2 first waits for the
//                                          post-processing of call i (ov_post_done) before it touches that parity again
//   workspace slices, network input       : private to a part, protected by the part stream's order
//   output slabs (caller's)               : written by NMS on the caller's stream, i.e. in the caller's own order
int detect_overlapped(rfd_ctx *c, const rfd_image *imgs, int n, rfd_dets *out, hipEvent_t frames_ready = nullptr)
{
    Network &net = c->net;
    RFD_TRY(net.ensure_alt_heads());
    const size_t B = (size_t)c->cfg.max_batch_size;
    if (!c->ov_desc) {
        RFD_TRY(c->ov_desc.create());
        RFD_TRY(c->ov_resync.create());
        for (int a = 0; a < 2; ++a) {
            RFD_TRY(c->ov_post_done[a].create());
            for (int b = 0; b < 2; ++b) RFD_TRY(c->ov_chain_done[a][b].create());
            RFD_TRY(c->ov_imgs[a].reserve(B * sizeof(PreImage)));
            RFD_TRY(c->ov_scale[a].reserve(B * sizeof(float)));
        }
    }
    const int par = (c->ov_parity ^= 1);
    PreImage *pis;
    float *pin_scales;
    RFD_TRY(acquire_frame_slot(c, &pis, &pin_scales));
    for (int i = 0; i < n; ++i) RFD_TRY(fill_pre_image(c, imgs[i], i, &pis[i], &pin_scales[i]));
    RFD_TRY(place_frames(c, imgs, n, true, pis, sizeof *pis));
    hipStream_t st[2] = {net.part_stream[0], net.part_stream[1]};
    if (c->ov_last_n != n) {
        // Different slices than the previous call's chains (another batch size), or the previous call ran on the caller's
        // stream (any other entry point): both chains start behind everything enqueued so far.  The caller's stream has
        // already waited for every earlier chain (post_network of each overlapped call sits behind ov_chain_done).
        RFD_HIP(hipEventRecord(c->ov_resync, c->stream));
        for (int p = 0; p < 2; ++p) RFD_HIP(hipStreamWaitEvent(st[p], c->ov_resync, 0));
    }
    c->ov_last_n = n;
    // (Round 3 also ran each call as ONE whole-batch chain on the stream of its parity, the next call beside it in a second copy of
    //  the workspace: bit-exact, and no faster than the half-batch chains -- 7 721 / 7 432 / 7 474 / 7 534 against 7 439 / 7 642 /
    //  7 486 / 7 421 img/s, profiles/r03_ab_whole_call_chains.jsonl: at 32 images nearly every kernel fills the chip, so the two
    //  chains simply alternate.  Removed.)
    if (frames_ready) // pipelined host entry: the frames of this call are still crossing PCIe on the copy stream
        for (int p = 0; p < 2; ++p) RFD_HIP(hipStreamWaitEvent(st[p], frames_ready, 0));
    if (c->ov_post_valid[par])
        for (int p = 0; p < 2; ++p) RFD_HIP(hipStreamWaitEvent(st[p], c->ov_post_done[par], 0));
    RFD_HIP(hipMemcpyAsync(c->ov_imgs[par].p, pis, n * sizeof(PreImage), hipMemcpyHostToDevice, st[0]));
    RFD_HIP(hipMemcpyAsync(c->ov_scale[par].p, pin_scales, n * sizeof(float), hipMemcpyHostToDevice, st[0]));
    RFD_TRY(c->frame_ring.record(st[0]));
    RFD_HIP(hipEventRecord(c->ov_desc, st[0]));
    RFD_HIP(hipStreamWaitEvent(st[1], c->ov_desc, 0));
    net.head_parity = par;
    net.co_running = 1;
    int chain[Network::kMaxParts];
    if (net.pass_chains(n, chain) != 2) { set_error("overlapped calls run as two chains"); return RFD_ERR_STATE; }
    const int B0 = chain[0];
    int status = RFD_OK;
    for (int p = 0; p < 2 && status == RFD_OK; ++p) {
        const int off = p ? B0 : 0, Bp = chain[p];
        status = launch_preprocess(pre_params(c, (const PreImage *)c->ov_imgs[par].p + off, off), Bp, st[p]);
        if (status == RFD_OK) status = net.run(Bp, st[p], 0, -1, off, p);
        if (status == RFD_OK && hipEventRecord(c->ov_chain_done[par][p], st[p]) != hipSuccess) status = RFD_ERR_HIP;
    }
    net.co_running = 0;
    if (status != RFD_OK) { net.head_parity = 0; c->ov_last_n = -1; return status; }
    for (int p = 0; p < 2; ++p) RFD_HIP(hipStreamWaitEvent(c->stream, c->ov_chain_done[par][p], 0));
    DecodeParams dp = decode_params(c, true);
    net.head_parity = 0;
    RFD_TRY(post_network(c, dp, false, n, out->boxes, out->landmarks, out->count, out->total, nullptr,
                         (const float *)c->ov_scale[par].p));
    RFD_HIP(hipEventRecord(c->ov_post_done[par], c->stream));
    c->ov_post_valid[par] = true;
    return RFD_OK;
}

int detect_impl(rfd_ctx *c, const rfd_image *imgs, int n, rfd_dets *out, bool on_device, int async, bool frames_on_device)
{
    RFD_CHECK_ARG(c != nullptr, "ctx is null");
    RFD_CHECK_ARG(out && out->boxes && out->landmarks && out->count, "output buffers are null");
    RFD_TRY(check_images(c, imgs, n));
    RFD_TRY(c->ensure_network());
    if (!c->net.weights_ready) { set_error("network weights are not initialised"); return RFD_ERR_STATE; }
    if (async == 2 && on_device && frames_on_device && !c->net.profiling && c->net.multi_stream && c->net.num_parts(n) == 2) {
        RFD_HIP(hipSetDevice(c->cfg.device_id));
        return detect_overlapped(c, imgs, n, out);
    }
    RFD_HIP(hipSetDevice(c->cfg.device_id));
    c->ov_last_n = -1;
    RFD_HIP(hipEventRecord(c->ev[0], c->stream));
    RFD_TRY(stage_frames(c, imgs, n, frames_on_device));
    RFD_HIP(hipEventRecord(c->ev[1], c->stream));
    RFD_TRY(launch_preprocess(pre_params(c, c->imgs.p, 0), n, c->stream));
    RFD_HIP(hipEventRecord(c->ev[2], c->stream));
    RFD_TRY(c->net.run_graphed(n, c->stream));
    RFD_HIP(hipEventRecord(c->ev[3], c->stream));
    DecodeParams dp = decode_params(c, true);
    const rfd_dets dev = on_device ? *out : own_slabs(c);
    RFD_TRY(post_network(c, dp, false, n, dev.boxes, dev.landmarks, dev.count, dev.total, nullptr));
    if (!on_device) RFD_TRY(copy_slabs(c, *out, dev, n, hipMemcpyDeviceToHost));
    RFD_HIP(hipEventRecord(c->ev[7], c->stream));
    if (async && on_device) return RFD_OK;
    RFD_HIP(hipStreamSynchronize(c->stream));
    RFD_TRY(check_nms_flag(c));
    RFD_TRY(finish_stats(c, n, true, true));
    if (!on_device)
        for (int i = 0; i < n; ++i) c->stats.detections += out->total ? out->total[i] : out->count[i];
    return RFD_OK;
}

// host head tensors of n images (rfd_forward's contract) -> scratch[3..11], named in dp
int upload_heads(rfd_ctx *c, const float *const heads[9], int n, DecodeParams &dp)
{
    static const int chans[3] = {2 * kA, 4 * kA, 10 * kA};
    for (int l = 0; l < kNumLevels; ++l)
        for (int k = 0; k < 3; ++k) {
            const size_t bytes = (size_t)n * chans[k] * c->fh[l] * c->fw[l] * sizeof(float);
            DevBuf &b = c->scratch[3 + 3 * l + k];
            RFD_TRY(b.reserve(bytes));
            RFD_HIP(hipMemcpyAsync(b.p, heads[3 * l + k], bytes, hipMemcpyHostToDevice, c->stream));
            (k == 0 ? dp.cls[l] : k == 1 ? dp.bbox[l] : dp.lmk[l]) = (const float *)b.p;
        }
    return RFD_OK;
}

// ---- views (rfd.h, "views") ----
// Everything a views call decides before it enqueues: the argument rules, each view's slot among its frame's views
// (view_plan.h), its letterbox, and the two capacity limits.  frames may be null (rfd_decode_nms_views: the frames are not
// seen).  Fills vd [n_views] and, where given, the geometry of pis [n_views] (src / stride are the caller's).
int plan_views(const rfd_ctx *c, const rfd_image *frames, int n_frames, const rfd_view *views, int n_views, float edge_margin,
               ViewDesc *vd, PreImage *pis, int *vmax)
{
    RFD_CHECK_ARG(views != nullptr, "views is null");
    RFD_CHECK_ARG(n_frames >= 1, "n_frames < 1");
    RFD_TRY(check_batch(c, n_views, "batch of", " views"));
    RFD_CHECK_ARG(edge_margin >= 0.0f && std::isfinite(edge_margin), "edge_margin must be finite and >= 0");
    std::vector<int32_t> slot(n_views);
    int bad = -1;
    switch (view_slots(views, n_views, n_frames, slot.data(), vmax, &bad)) {
    case kViewOk: break;
    case kViewFrameRange: set_error("invalid argument: view %d names frame %d of %d", bad, views[bad].frame, n_frames); return RFD_ERR_INVALID_ARG;
    case kViewFrameOrder: set_error("invalid argument: views must be sorted by frame (view %d names frame %d after frame %d)", bad, views[bad].frame, views[bad - 1].frame); return RFD_ERR_INVALID_ARG;
    case kViewEmpty: set_error("invalid argument: view %d is empty (%dx%d)", bad, views[bad].w, views[bad].h); return RFD_ERR_INVALID_ARG;
    case kViewOrigin: set_error("invalid argument: view %d starts at (%d, %d), outside its frame", bad, views[bad].x, views[bad].y); return RFD_ERR_INVALID_ARG;
    case kViewInnerBits: set_error("invalid argument: view %d sets bits of inner (0x%x) beyond the four sides", bad, views[bad].inner); return RFD_ERR_INVALID_ARG;
    }
    for (int i = 0; i < n_views; ++i) {
        const rfd_view &v = views[i];
        if (frames && !view_inside(v, frames[v.frame].width, frames[v.frame].height)) {
            set_error("invalid argument: view %d (%dx%d at %d, %d) does not lie inside frame %d (%dx%d)", i, v.w, v.h, v.x, v.y, v.frame,
                      frames[v.frame].width, frames[v.frame].height);
            return RFD_ERR_INVALID_ARG;
        }
        PreImage pi;
        float det_scale;
        letterbox(v.h, v.w, c->cfg.image_w, c->cfg.image_h, &pi, &det_scale);
        if (pi.new_w <= 0 || pi.new_h <= 0) { // as fill_pre_image refuses such a frame
            set_error("invalid argument: view %d (%dx%d) letterboxes to an empty %dx%d image", i, v.w, v.h, pi.new_w, pi.new_h);
            return RFD_ERR_INVALID_ARG;
        }
        vd[i] = ViewDesc{v.frame, slot[i], v.x, v.y, pi.new_w, pi.new_h, v.inner, det_scale};
        if (pis) pis[i] = pi;
    }
    if ((long long)n_frames * *vmax > c->cfg.max_batch_size) {
        set_error("%d frames of up to %d views each take %lld image slots, max_batch_size is %d", n_frames, *vmax, (long long)n_frames * *vmax,
                  c->cfg.max_batch_size);
        return RFD_ERR_CAPACITY;
    }
    if (!nms_fits_lds(*vmax * c->total_anchors)) {
        set_error("%d views of a frame make %d candidate slots (%d anchors each): the NMS bitmap does not fit LDS", *vmax, *vmax * c->total_anchors,
                  c->total_anchors);
        return RFD_ERR_CAPACITY;
    }
    return RFD_OK;
}

// the descriptors of a planned call to the device, and ones as the det_scale of its frames (the rows are in frame pixels already)
int stage_views(rfd_ctx *c, const ViewDesc *vd, int n_views, float *pin_ones, int n_frames)
{
    for (int i = 0; i < n_frames; ++i) pin_ones[i] = 1.0f;
    RFD_HIP(hipMemcpyAsync(c->view_desc.p, vd, n_views * sizeof(ViewDesc), hipMemcpyHostToDevice, c->stream));
    RFD_HIP(hipMemcpyAsync(c->det_scale.p, pin_ones, n_frames * sizeof(float), hipMemcpyHostToDevice, c->stream));
    RFD_TRY(c->views_ring.record(c->stream));
    return c->frame_ring.record(c->stream);
}

int acquire_views_slot(rfd_ctx *c, ViewDesc **vd)
{
    RFD_TRY(c->view_desc.reserve((size_t)c->cfg.max_batch_size * sizeof(ViewDesc)));
    RFD_TRY(c->views_ring.ensure((size_t)c->cfg.max_batch_size * sizeof(ViewDesc)));
    return c->views_ring.acquire(vd);
}

int detect_views_impl(rfd_ctx *c, const rfd_image *frames, int n_frames, const rfd_view *views, int n_views, float edge_margin,
                      rfd_dets *out, bool on_device, int async)
{
    RFD_CHECK_ARG(c != nullptr, "ctx is null");
    RFD_CHECK_ARG(out && out->boxes && out->landmarks && out->count, "output buffers are null");
    RFD_CHECK_ARG(!on_device || out->total, "the device form needs out->total");
    RFD_TRY(check_images(c, frames, n_frames));
    RFD_HIP(hipSetDevice(c->cfg.device_id));
    PreImage *pis;
    float *pin_ones;
    ViewDesc *vd;
    int vmax = 0;
    RFD_TRY(acquire_frame_slot(c, &pis, &pin_ones));
    RFD_TRY(acquire_views_slot(c, &vd));
    RFD_TRY(plan_views(c, frames, n_frames, views, n_views, edge_margin, vd, pis, &vmax));
    RFD_TRY(c->ensure_network());
    if (!c->net.weights_ready) { set_error("network weights are not initialised"); return RFD_ERR_STATE; }
    c->ov_last_n = -1;
    RFD_HIP(hipEventRecord(c->ev[0], c->stream));
    std::vector<FrameWhere> where(n_frames); // each FRAME is placed once; its views point into it
    RFD_TRY(place_frames(c, frames, n_frames, on_device, where.data(), sizeof(FrameWhere)));
    for (int i = 0; i < n_views; ++i) {
        const FrameWhere &f = where[views[i].frame];
        pis[i].src = f.src + (long long)views[i].y * f.stride + 3ll * views[i].x;
        pis[i].stride = f.stride;
    }
    RFD_HIP(hipMemcpyAsync(c->imgs.p, pis, n_views * sizeof(PreImage), hipMemcpyHostToDevice, c->stream));
    RFD_TRY(stage_views(c, vd, n_views, pin_ones, n_frames));
    RFD_HIP(hipEventRecord(c->ev[1], c->stream));
    RFD_TRY(launch_preprocess(pre_params(c, c->imgs.p, 0), n_views, c->stream));
    RFD_HIP(hipEventRecord(c->ev[2], c->stream));
    RFD_TRY(c->net.run_graphed(n_views, c->stream));
    RFD_HIP(hipEventRecord(c->ev[3], c->stream));
    DecodeParams dp = decode_params(c, true);
    const ViewsPost vp = {(const ViewDesc *)c->view_desc.p, n_views, vmax, edge_margin};
    const rfd_dets dev = on_device ? *out : own_slabs(c);
    RFD_TRY(post_network(c, dp, false, n_frames, dev.boxes, dev.landmarks, dev.count, dev.total, nullptr, nullptr, &vp));
    if (!on_device) RFD_TRY(copy_slabs(c, *out, dev, n_frames, hipMemcpyDeviceToHost));
    RFD_HIP(hipEventRecord(c->ev[7], c->stream));
    if (async && on_device) return RFD_OK;
    RFD_HIP(hipStreamSynchronize(c->stream));
    RFD_TRY(check_nms_flag(c));
    RFD_TRY(finish_stats(c, n_frames, true, true));
    if (!on_device)
        for (int i = 0; i < n_frames; ++i) c->stats.detections += out->total ? out->total[i] : out->count[i];
    return RFD_OK;
}

std::mutex g_nms_mu;
rfd_ctx *g_nms_ctx[16] = {};

} // namespace

// ---- what the layers next to this file ask of their context (ctx_access.h) ----
hipStream_t rfd::ctx_stream(const rfd_ctx *c) { return c->stream; }
int rfd::ctx_device(const rfd_ctx *c) { return c->cfg.device_id; }
int rfd::ctx_max_batch_size(const rfd_ctx *c) { return c->cfg.max_batch_size; }
int rfd::ctx_max_det(const rfd_ctx *c) { return c->cfg.max_det; }
ShotQuality &rfd::ctx_shot_quality(rfd_ctx *c) { return c->shot; }
FrameConvert &rfd::ctx_frame_convert(rfd_ctx *c) { return c->frames; }
JpegEncoder &rfd::ctx_jpeg_encoder(rfd_ctx *c) { return c->encoder; }
Redact &rfd::ctx_redact(rfd_ctx *c) { return c->redact; }
Annotate &rfd::ctx_annotate(rfd_ctx *c) { return c->annotate; }
FaceStage &rfd::ctx_face_stage(rfd_ctx *c) { return c->face; }
int rfd::ctx_check_batch(const rfd_ctx *c, int n, const char *what, const char *unit) { return check_batch(c, n, what, unit); }
int rfd::ctx_check_images(const rfd_ctx *c, const rfd_image *imgs, int n) { return check_images(c, imgs, n); }
int rfd::ctx_place_frames(rfd_ctx *c, const rfd_image *imgs, int n, bool frames_on_device, void *desc, size_t pitch)
{
    return place_frames(c, imgs, n, frames_on_device, desc, pitch);
}
int rfd::ctx_stage_frames(rfd_ctx *c, const rfd_image *imgs, int n, bool frames_on_device, const PreImage **staged)
{
    *staged = (const PreImage *)c->imgs.p;
    return stage_frames(c, imgs, n, frames_on_device);
}
int rfd::ctx_stage_frame_sizes(rfd_ctx *c, const int32_t *img_w, const int32_t *img_h, int n, const PreImage **staged)
{
    PreImage *pis;
    float *pin_scales;
    RFD_TRY(acquire_frame_slot(c, &pis, &pin_scales));
    memset(pis, 0, (size_t)n * sizeof(PreImage));
    for (int i = 0; i < n; ++i) { pis[i].w = img_w[i]; pis[i].h = img_h[i]; }
    RFD_HIP(hipMemcpyAsync(c->imgs.p, pis, n * sizeof(PreImage), hipMemcpyHostToDevice, c->stream));
    *staged = (const PreImage *)c->imgs.p;
    return c->frame_ring.record(c->stream);
}
rfd_dets rfd::ctx_own_slabs(const rfd_ctx *c) { return own_slabs(c); }
int rfd::ctx_copy_slabs(rfd_ctx *c, const rfd_dets &dst, const rfd_dets &src, int n, hipMemcpyKind kind) { return copy_slabs(c, dst, src, n, kind); }
int rfd::ctx_detect_own_slabs(rfd_ctx *c, const rfd_image *imgs, int n, bool frames_on_device, rfd_dets *dev, const PreImage **staged)
{
    RFD_CHECK_ARG(c != nullptr, "ctx is null");
    *dev = own_slabs(c);
    *staged = (const PreImage *)c->imgs.p;
    return detect_impl(c, imgs, n, dev, /*outputs stay on the device*/ true, /*async*/ 1, frames_on_device);
}
int rfd::ctx_check_nms_flag(rfd_ctx *c) { return check_nms_flag(c); }

// ================================================================================================
// C ABI
// ================================================================================================
extern "C" {

void rfd_config_default(rfd_config *cfg)
{
    if (!cfg) return;
    memset(cfg, 0, sizeof *cfg);
    cfg->image_w = 640;                 // config.rs:26
    cfg->image_h = 640;
    cfg->max_batch_size = 1;            // config.rs:28
    cfg->confidence_threshold = 0.7f;   // config.rs:29
    cfg->iou_threshold = 0.45f;         // config.rs:30
    cfg->device_id = 0;
    cfg->max_det = 1024;
    cfg->max_src_w = 3840;
    cfg->max_src_h = 2160;
    cfg->backbone = RFD_BACKBONE_R50;
}

int rfd_version(void) { return RFD_VERSION; }
const char *rfd_last_error(void) { return get_error(); }

int rfd_create(const rfd_config *cfg, rfd_ctx **out)
{
    RFD_CHECK_ARG(cfg && out, "cfg/out is null");
    *out = nullptr;
    RFD_CHECK_ARG(cfg->image_w > 0 && cfg->image_h > 0 && cfg->image_w % 32 == 0 && cfg->image_h % 32 == 0,
                  "image_size must be positive multiples of 32");
    RFD_CHECK_ARG(cfg->max_batch_size >= 1, "max_batch_size < 1");
    RFD_CHECK_ARG(cfg->max_det >= 1, "max_det < 1");
    RFD_CHECK_ARG(cfg->precision == RFD_PRECISION_BF16 || cfg->precision == RFD_PRECISION_F32, "precision must be RFD_PRECISION_BF16 or RFD_PRECISION_F32");
    RFD_CHECK_ARG(cfg->precision == RFD_PRECISION_BF16 || cfg->backbone == RFD_BACKBONE_R50, "the f32 parity mode exists for RetinaFace-R50 only");
    RFD_CHECK_ARG(cfg->schedule == RFD_SCHEDULE_THROUGHPUT || cfg->schedule == RFD_SCHEDULE_LATENCY, "schedule must be RFD_SCHEDULE_THROUGHPUT or RFD_SCHEDULE_LATENCY");
    RFD_CHECK_ARG(cfg->schedule == RFD_SCHEDULE_THROUGHPUT || cfg->precision == RFD_PRECISION_BF16, "the latency schedule exists for the bf16 path only (not the f32 parity mode)");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        set_error("no HIP device is available: librfd_hip has no CPU fallback");
        return RFD_ERR_NO_DEVICE;
    }
    if (cfg->device_id < 0 || cfg->device_id >= ndev) {
        set_error("device_id %d out of range (%d devices)", cfg->device_id, ndev);
        return RFD_ERR_NO_DEVICE;
    }
    if (hipSetDevice(cfg->device_id) != hipSuccess) {
        set_error("hipSetDevice(%d) failed", cfg->device_id);
        return RFD_ERR_NO_DEVICE;
    }
    std::unique_ptr<rfd_ctx> c(new rfd_ctx()); // an early return frees whatever was built so far
    c->cfg = *cfg;
    if (const char *e = getenv("RFD_NMS_CHUNKED")) c->nms_chunked = atoi(e) != 0;
    make_base_anchors(c->base_anchor);
    int off = 0;
    for (int l = 0; l < kNumLevels; ++l) {
        c->fh[l] = cfg->image_h / kStrides[l];
        c->fw[l] = cfg->image_w / kStrides[l];
        c->level_off[l] = off;
        off += c->fh[l] * c->fw[l] * kA;
    }
    c->total_anchors = off;
    memset(&c->stats, 0, sizeof c->stats);
    const size_t B = (size_t)cfg->max_batch_size;
    RFD_TRY(c->own_stream.create());
    c->stream = c->own_stream;
    for (Event &e : c->ev) RFD_TRY(e.create(hipEventDefault));
    RFD_TRY(c->frame_ring.ensure(B * (sizeof(PreImage) + sizeof(float)), hipEventDefault));
    RFD_TRY(c->face.dims_ring.ensure(B * 2 * sizeof(int)));
    RFD_TRY(c->h_nms_flag.alloc(1));
    *c->h_nms_flag = 0;
    RFD_TRY(ctx_alloc(c.get()));
    *out = c.release();
    return RFD_OK;
}

void rfd_destroy(rfd_ctx *c)
{
    if (!c) return;
    (void)hipSetDevice(c->cfg.device_id);
    (void)hipDeviceSynchronize(); // part / side / copy streams included
    if (c->comm) { (void)g_rccl.CommDestroy(c->comm); c->comm = nullptr; }
    if (c->net_created) c->net.destroy();
    delete c;
}

int rfd_get_config(const rfd_ctx *c, rfd_config *cfg)
{
    RFD_CHECK_ARG(c && cfg, "null argument");
    *cfg = c->cfg;
    return RFD_OK;
}

int rfd_get_stats(rfd_ctx *c, rfd_stats *stats)
{
    RFD_CHECK_ARG(c && stats, "null argument");
    *stats = c->stats;
    return RFD_OK;
}

int rfd_set_stream(rfd_ctx *c, void *hip_stream)
{
    RFD_CHECK_ARG(c, "ctx is null");
    RFD_HIP(hipStreamSynchronize(c->stream));
    c->stream = hip_stream ? (hipStream_t)hip_stream : c->own_stream.s;
    return RFD_OK;
}

int rfd_set_thresholds(rfd_ctx *c, float confidence_threshold, float iou_threshold)
{
    RFD_CHECK_ARG(c, "ctx is null");
    c->cfg.confidence_threshold = confidence_threshold;
    c->cfg.iou_threshold = iou_threshold;
    return RFD_OK;
}

int rfd_set_profiling(rfd_ctx *c, int enable)
{
    RFD_CHECK_ARG(c, "ctx is null");
    RFD_TRY(c->ensure_network());
    if (enable && c->net.precision != 0) { set_error("per-op profiling is not available in the f32 parity mode"); return RFD_ERR_STATE; }
    c->net.profiling = enable != 0;
    return RFD_OK;
}

int rfd_get_conv_profile(rfd_ctx *c, float *ms_conv, double *flops_conv, int *launches)
{
    RFD_CHECK_ARG(c, "ctx is null");
    if (ms_conv) *ms_conv = c->conv_ms;
    if (flops_conv) *flops_conv = c->conv_flops;
    if (launches) *launches = c->conv_launches;
    return RFD_OK;
}

int rfd_get_op_profile(rfd_ctx *c, float *ms, int cap)
{
    RFD_CHECK_ARG(c && ms, "null argument");
    if (!c->net_created) { set_error("no network"); return RFD_ERR_STATE; }
    const int n = (int)c->net.op_ms.size();
    for (int i = 0; i < n && i < cap; ++i) ms[i] = c->net.op_ms[i];
    return n;
}

// ---- graph description (host only; usable without a GPU) ----
int rfd_graph_create(int backbone, int image_w, int image_h, rfd_graph **out)
{
    RFD_CHECK_ARG(out, "out is null");
    Graph *g = new Graph();
    const int st = g->build(backbone, image_w, image_h);
    if (st != RFD_OK) { delete g; *out = nullptr; return st; }
    *out = reinterpret_cast<rfd_graph *>(g);
    return RFD_OK;
}
void rfd_graph_destroy(rfd_graph *g) { delete reinterpret_cast<Graph *>(g); }
int rfd_graph_counts(const rfd_graph *gg, int *layers, int *ops, int *tensors, int *buffers)
{
    RFD_CHECK_ARG(gg, "graph is null");
    const Graph *g = reinterpret_cast<const Graph *>(gg);
    if (layers) *layers = (int)g->layers.size();
    if (ops) *ops = (int)g->ops.size();
    if (tensors) *tensors = (int)g->tensors.size();
    if (buffers) *buffers = (int)g->buffer_bytes_per_image.size();
    return RFD_OK;
}
int rfd_graph_layer(const rfd_graph *gg, int idx, rfd_layer_desc *d)
{
    RFD_CHECK_ARG(gg && d, "null argument");
    const Graph *g = reinterpret_cast<const Graph *>(gg);
    RFD_CHECK_ARG(idx >= 0 && idx < (int)g->layers.size(), "layer index out of range");
    const Layer &L = g->layers[idx];
    memset(d, 0, sizeof *d);
    snprintf(d->name, sizeof d->name, "%s", L.name.c_str());
    d->cin = L.cin; d->cout = L.cout; d->kh = L.kh; d->kw = L.kw; d->stride = L.stride; d->pad = L.pad;
    d->has_affine = L.has_affine;
    d->kind = L.kind;
    return RFD_OK;
}
int rfd_graph_op(const rfd_graph *gg, int idx, rfd_op_desc *d)
{
    RFD_CHECK_ARG(gg && d, "null argument");
    const Graph *g = reinterpret_cast<const Graph *>(gg);
    RFD_CHECK_ARG(idx >= 0 && idx < (int)g->ops.size(), "op index out of range");
    const Op &o = g->ops[idx];
    memset(d, 0, sizeof *d);
    d->kind = o.kind; d->layer = o.layer; d->in = o.in; d->out = o.out; d->out2 = o.out2; d->outf = o.outf;
    d->res = o.res; d->relu = o.relu; d->res_up2 = o.res_up2; d->res_post = o.res_post;
    d->head_softmax = o.head_softmax; d->y_coff = o.y_coff;
    d->in2 = o.in2; d->layer2 = o.layer2; d->in_affine = o.in_affine;
    d->layer_n2 = o.layer_n2; d->x_coff = o.x_coff; d->y_split = o.y_split; d->y_split_add = o.y_split_add;
    d->n_valid = o.n_valid; d->layer_b = o.layer_b; d->out_b = o.out_b; d->branch = o.branch;
    d->macs = g->layer_macs(idx);
    return RFD_OK;
}
int rfd_graph_tensor(const rfd_graph *gg, int idx, rfd_tensor_desc *d)
{
    RFD_CHECK_ARG(gg && d, "null argument");
    const Graph *g = reinterpret_cast<const Graph *>(gg);
    RFD_CHECK_ARG(idx >= 0 && idx < (int)g->tensors.size(), "tensor index out of range");
    const TensorDesc &t = g->tensors[idx];
    memset(d, 0, sizeof *d);
    d->channels = t.C; d->channels_logical = t.C_logical; d->height = t.H; d->width = t.W; d->is_f32 = t.is_f32;
    d->buffer = t.buffer;
    d->is_input = idx == g->input;
    for (int l = 0; l < 3; ++l)
        if (g->heads[l] == idx) d->head_level = l + 1;
    return RFD_OK;
}
double rfd_graph_macs(const rfd_graph *gg)
{
    return gg ? reinterpret_cast<const Graph *>(gg)->macs_per_image() : 0.0;
}
double rfd_graph_workspace_bytes(const rfd_graph *gg)
{
    if (!gg) return 0.0;
    double s = 0;
    for (size_t b : reinterpret_cast<const Graph *>(gg)->buffer_bytes_per_image) s += (double)b;
    return s;
}

// ---- test hooks: raw tensor access and partial execution of the network ----
int rfd_debug_tensor_io(rfd_ctx *c, int tensor_id, int n, void *host, int write)
{
    RFD_CHECK_ARG(c && host, "null argument");
    RFD_HIP(hipSetDevice(c->cfg.device_id));
    RFD_TRY(c->ensure_network());
    RFD_CHECK_ARG(tensor_id >= 0 && tensor_id < (int)c->net.g.tensors.size(), "tensor id out of range");
    RFD_CHECK_ARG(n >= 1 && n <= c->cfg.max_batch_size, "batch out of range");
    const TensorDesc &td = c->net.g.tensors[tensor_id];
    size_t bytes = td.bytes_per_image() * (size_t)n;
    void *dev = c->net.tensor_ptr(tensor_id);
    c->ov_last_n = -1;
    if (c->net.precision != 0 && !td.is_f32 && tensor_id != c->net.g.input) {
        // f32 parity mode: an intermediate tensor lives in the f32 workspace, n images of C*H*W floats, contiguous at the tensor's
        // own size as the f32 kernels index them (Network::tensor_ptr32)
        bytes = (size_t)n * td.C * td.H * td.W * sizeof(float);
        dev = c->net.tensor_ptr32(tensor_id);
    }
    if (write) RFD_HIP(hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, c->stream));
    else RFD_HIP(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, c->stream));
    RFD_HIP(hipStreamSynchronize(c->stream));
    return RFD_OK;
}
int rfd_debug_set_conv_tile(rfd_ctx *c, int tile)
{
    RFD_CHECK_ARG(c && tile >= 0 && tile <= 31, "bad argument");
    RFD_TRY(c->ensure_network());
    c->net.force_tile = tile;
    return RFD_OK;
}
int rfd_debug_set_concurrency(rfd_ctx *c, int multi_stream, int split_min_part, int split_max_parts, int use_graph)
{
    RFD_CHECK_ARG(c, "ctx is null");
    RFD_TRY(c->ensure_network());
    RFD_HIP(hipStreamSynchronize(c->stream));
    c->net.multi_stream = multi_stream != 0;
    c->net.split_min_part = split_min_part;
    c->net.split_max_parts = split_max_parts;
    c->net.tuned = false; // the stream choice depends on the number of parts
    c->net.use_graph = use_graph != 0;
    for (hipGraphExec_t &ge : c->net.graph_exec)
        if (ge) { (void)hipGraphExecDestroy(ge); ge = nullptr; }
    return RFD_OK;
}
int rfd_debug_poke_nms_flag(rfd_ctx *c, int value)
{
    RFD_CHECK_ARG(c, "ctx is null");
    RFD_HIP(hipSetDevice(c->cfg.device_id));
    RFD_HIP(hipMemcpyAsync(c->fault_word(), &value, sizeof(int), hipMemcpyHostToDevice, c->stream));
    RFD_HIP(hipStreamSynchronize(c->stream));
    return RFD_OK;
}
int rfd_debug_persistent_kernel(int i, const char **name, size_t *lds_bytes) { return rfd::persistent_kernel_table(i, name, lds_bytes); }
int rfd_debug_run_ops(rfd_ctx *c, int n, int first_op, int last_op)
{
    RFD_CHECK_ARG(c, "ctx is null");
    RFD_HIP(hipSetDevice(c->cfg.device_id));
    RFD_TRY(c->ensure_network());
    c->ov_last_n = -1;
    RFD_TRY(c->net.run(n, c->stream, first_op, last_op));
    RFD_HIP(hipMemcpyAsync(c->h_nms_flag, c->net.d_fail, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    RFD_HIP(hipStreamSynchronize(c->stream));
    if (c->net.profiling) RFD_TRY(c->net.collect_profile());
    return check_nms_flag(c);
}

int rfd_debug_run_chain(rfd_ctx *c, int n, int first_op, int last_op, int batch_off, int co_running)
{
    RFD_CHECK_ARG(c, "ctx is null");
    RFD_HIP(hipSetDevice(c->cfg.device_id));
    RFD_TRY(c->ensure_network());
    RFD_CHECK_ARG(n >= 1 && batch_off >= 0 && batch_off + n <= c->cfg.max_batch_size, "chain [batch_off, batch_off + n) out of range");
    c->ov_last_n = -1;
    const int saved = c->net.co_running;
    c->net.co_running = co_running != 0;
    const int st = c->net.run(n, c->stream, first_op, last_op, batch_off, 0);
    c->net.co_running = saved;
    RFD_TRY(st);
    RFD_HIP(hipMemcpyAsync(c->h_nms_flag, c->net.d_fail, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    RFD_HIP(hipStreamSynchronize(c->stream));
    if (c->net.profiling) RFD_TRY(c->net.collect_profile());
    return check_nms_flag(c);
}
int rfd_debug_pass_chains(rfd_ctx *c, int n, int *sizes, int cap)
{
    RFD_CHECK_ARG(c && sizes, "null argument");
    RFD_TRY(c->ensure_network());
    RFD_CHECK_ARG(n >= 1 && n <= c->cfg.max_batch_size, "batch out of range");
    int chain[Network::kMaxParts];
    const int P = c->net.pass_chains(n, chain);
    RFD_CHECK_ARG(cap >= P, "sizes holds fewer entries than the pass has chains");
    for (int p = 0; p < P; ++p) sizes[p] = chain[p];
    return P;
}
int rfd_debug_buffer_io(rfd_ctx *c, int tensor_id, void *host, size_t bytes, int write, size_t *image_pitch)
{
    RFD_CHECK_ARG(c, "ctx is null");
    RFD_HIP(hipSetDevice(c->cfg.device_id));
    RFD_TRY(c->ensure_network());
    RFD_CHECK_ARG(tensor_id >= 0 && tensor_id < (int)c->net.g.tensors.size(), "tensor id out of range");
    if (c->net.precision != 0) { set_error("f32 parity mode keeps its own workspace"); return RFD_ERR_STATE; }
    const size_t pitch = c->net.g.buffer_bytes_per_image[c->net.g.tensors[tensor_id].buffer];
    if (image_pitch) *image_pitch = pitch;
    if (!host) return RFD_OK;
    RFD_CHECK_ARG(bytes == pitch * (size_t)c->cfg.max_batch_size, "bytes is not the size of the buffer (max_batch_size * image pitch)");
    c->ov_last_n = -1;
    if (write) RFD_HIP(hipMemcpyAsync(c->net.tensor_ptr(tensor_id), host, bytes, hipMemcpyHostToDevice, c->stream));
    else RFD_HIP(hipMemcpyAsync(host, c->net.tensor_ptr(tensor_id), bytes, hipMemcpyDeviceToHost, c->stream));
    RFD_HIP(hipStreamSynchronize(c->stream));
    return RFD_OK;
}

int rfd_debug_op_kernels(rfd_ctx *c, int n, int op, int co_running, char *names, int cap)
{
    RFD_CHECK_ARG(c && names && cap > 0, "null argument");
    RFD_HIP(hipSetDevice(c->cfg.device_id));
    RFD_TRY(c->ensure_network());
    RFD_CHECK_ARG(n >= 1 && n <= c->cfg.max_batch_size && op >= 0 && op < (int)c->net.g.ops.size(), "batch or op out of range");
    if (c->net.precision != 0) { set_error("kernel-choice introspection covers the bf16 path"); return RFD_ERR_STATE; }
    if (!c->net.weights_ready) { set_error("network weights are not initialised (rfd_init_synthetic_weights / rfd_set_layer_weights)"); return RFD_ERR_STATE; }
    const int saved = c->net.co_running;
    c->net.co_running = co_running != 0;   // as for a chain of a split pass (batches >= 16 run as two chains of n / 2 images)
    std::string out;
    const int st = c->net.op_kernel_names(n, op, device_cus(), &out);
    c->net.co_running = saved;
    RFD_TRY(st);
    snprintf(names, (size_t)cap, "%s", out.c_str());
    return RFD_OK;
}

int rfd_debug_op_kernels_static(int backbone, int net_w, int net_h, int n, int op, int co_running, int tile, int schedule, int cus, char *names, int cap)
{
    RFD_CHECK_ARG(names && cap > 0 && n >= 1 && cus >= 1 && tile >= 0 && tile <= 31, "bad argument");
    Network net; // never created: no device, no allocation
    RFD_TRY(net.g.build(backbone, net_w, net_h));
    RFD_CHECK_ARG(op >= 0 && op < (int)net.g.ops.size(), "op out of range");
    net.max_batch = n;
    net.schedule = schedule;
    net.force_tile = tile;
    net.co_running = co_running != 0;
    if (schedule == RFD_SCHEDULE_LATENCY) (void)net.plan_splitk();
    // Operands "present" for the chooser: addresses at the offsets of the layer table and the workspace plan from a made-up base.
    // Nothing reads through them; the relation of two filter banks is one of their offsets, as on a device.
    char *const base = reinterpret_cast<char *>((uintptr_t)1 << 32);
    net.d_w = reinterpret_cast<bf16_t *>(base);
    net.d_b = reinterpret_cast<float *>(base);
    net.d_zero = reinterpret_cast<bf16_t *>(base);
    net.d_buffers.assign(net.g.buffer_bytes_per_image.size(), base);
    for (int b = 0; b < 3; ++b) net.d_sk_ws[b] = reinterpret_cast<float *>(base);
    net.d_sk_cnt = reinterpret_cast<unsigned *>(base);
    std::string out;
    RFD_TRY(net.op_kernel_names(n, op, cus, &out));
    snprintf(names, (size_t)cap, "%s", out.c_str());
    return RFD_OK;
}

// ---- weights ----
int rfd_init_synthetic_weights(rfd_ctx *c, uint64_t seed)
{
    RFD_CHECK_ARG(c, "ctx is null");
    RFD_HIP(hipSetDevice(c->cfg.device_id));
    RFD_TRY(c->ensure_network());
    return c->net.init_synthetic(seed, c->stream);
}
int rfd_num_layers(const rfd_ctx *c)
{
    if (!c || !c->net_created) return 0;
    return (int)c->net.g.layers.size();
}
int rfd_get_layer_weights(rfd_ctx *c, int idx, float *weights, float *bias)
{
    RFD_CHECK_ARG(c, "ctx is null");
    RFD_TRY(c->ensure_network());
    return c->net.get_layer(idx, weights, bias, c->stream);
}
int rfd_set_layer_weights(rfd_ctx *c, int idx, const float *weights, const float *bias)
{
    RFD_CHECK_ARG(c && weights, "null argument");
    RFD_TRY(c->ensure_network());
    RFD_TRY(c->net.set_layer(idx, weights, bias, c->stream));
    c->net.weights_ready = true;
    return RFD_OK;
}
int rfd_get_layer_affine(rfd_ctx *c, int idx, float *scale, float *shift)
{
    RFD_CHECK_ARG(c && scale && shift, "null argument");
    RFD_TRY(c->ensure_network());
    return c->net.get_affine(idx, scale, shift, c->stream);
}
int rfd_set_layer_affine(rfd_ctx *c, int idx, const float *scale, const float *shift)
{
    RFD_CHECK_ARG(c && scale && shift, "null argument");
    RFD_TRY(c->ensure_network());
    return c->net.set_affine(idx, scale, shift, c->stream);
}

namespace {
struct LayerRecord { char name[64]; int32_t cin, cout, kh, kw, stride, pad, kind, has_affine; };
}

int rfd_save_weights(rfd_ctx *c, const char *path)
{
    RFD_CHECK_ARG(c && path, "null argument");
    RFD_HIP(hipSetDevice(c->cfg.device_id));
    RFD_TRY(c->ensure_network());
    if (!c->net.weights_ready) { set_error("network weights are not initialised"); return RFD_ERR_STATE; }
    FILE *f = fopen(path, "wb");
    if (!f) { set_error("cannot open %s for writing", path); return RFD_ERR_IO; }
    const uint32_t hdr[3] = {1u, (uint32_t)c->cfg.backbone, (uint32_t)c->net.g.layers.size()};
    bool ok = fwrite("RFDW", 1, 4, f) == 4 && fwrite(hdr, 4, 3, f) == 3;
    for (size_t i = 0; ok && i < c->net.g.layers.size(); ++i) {
        const Layer &L = c->net.g.layers[i];
        LayerRecord rec;
        memset(&rec, 0, sizeof rec);
        snprintf(rec.name, sizeof rec.name, "%s", L.name.c_str());
        rec.cin = L.cin; rec.cout = L.cout; rec.kh = L.kh; rec.kw = L.kw; rec.stride = L.stride; rec.pad = L.pad;
        rec.kind = L.kind; rec.has_affine = L.has_affine;
        const size_t nw = (size_t)L.cout * L.kh * L.kw * L.cin;
        std::vector<float> w(nw), b(L.cout), sc(L.cout), sh(L.cout);
        const int st = c->net.get_layer((int)i, w.data(), b.data(), c->stream);
        if (st != RFD_OK) { fclose(f); return st; }
        ok = fwrite(&rec, sizeof rec, 1, f) == 1 && fwrite(w.data(), 4, nw, f) == nw && fwrite(b.data(), 4, L.cout, f) == (size_t)L.cout;
        if (ok && L.has_affine) {
            const int sa = c->net.get_affine((int)i, sc.data(), sh.data(), c->stream);
            if (sa != RFD_OK) { fclose(f); return sa; }
            ok = fwrite(sc.data(), 4, L.cout, f) == (size_t)L.cout && fwrite(sh.data(), 4, L.cout, f) == (size_t)L.cout;
        }
    }
    ok = (fclose(f) == 0) && ok;
    if (!ok) { set_error("short write to %s", path); return RFD_ERR_IO; }
    return RFD_OK;
}

int rfd_load_weights(rfd_ctx *c, const char *path)
{
    RFD_CHECK_ARG(c && path, "null argument");
    RFD_HIP(hipSetDevice(c->cfg.device_id));
    RFD_TRY(c->ensure_network());
    FILE *f = fopen(path, "rb");
    if (!f) { set_error("cannot open %s", path); return RFD_ERR_IO; }
    char magic[4];
    uint32_t hdr[3];
    if (fread(magic, 1, 4, f) != 4 || memcmp(magic, "RFDW", 4) != 0 || fread(hdr, 4, 3, f) != 3 || hdr[0] != 1u) {
        fclose(f);
        set_error("%s is not an RFDW version-1 weight file", path);
        return RFD_ERR_IO;
    }
    if (hdr[1] != (uint32_t)c->cfg.backbone || hdr[2] != (uint32_t)c->net.g.layers.size()) {
        fclose(f);
        set_error("%s holds backbone %u with %u layers; the context expects backbone %d with %zu layers", path, hdr[1], hdr[2],
                  c->cfg.backbone, c->net.g.layers.size());
        return RFD_ERR_INVALID_ARG;
    }
    for (size_t i = 0; i < c->net.g.layers.size(); ++i) {
        const Layer &L = c->net.g.layers[i];
        LayerRecord rec;
        if (fread(&rec, sizeof rec, 1, f) != 1) { fclose(f); set_error("%s is truncated (layer %zu)", path, i); return RFD_ERR_IO; }
        rec.name[63] = 0;
        if (rec.cin != L.cin || rec.cout != L.cout || rec.kh != L.kh || rec.kw != L.kw || rec.stride != L.stride ||
            rec.kind != L.kind || rec.has_affine != L.has_affine) {
            fclose(f);
            set_error("%s: layer %zu (%s) does not match the graph's %s", path, i, rec.name, L.name.c_str());
            return RFD_ERR_INVALID_ARG;
        }
        const size_t nw = (size_t)L.cout * L.kh * L.kw * L.cin;
        std::vector<float> w(nw), b(L.cout), sc(L.cout), sh(L.cout);
        bool ok = fread(w.data(), 4, nw, f) == nw && fread(b.data(), 4, L.cout, f) == (size_t)L.cout;
        if (ok && L.has_affine) ok = fread(sc.data(), 4, L.cout, f) == (size_t)L.cout && fread(sh.data(), 4, L.cout, f) == (size_t)L.cout;
        if (!ok) { fclose(f); set_error("%s is truncated (layer %zu)", path, i); return RFD_ERR_IO; }
        int st = c->net.set_layer((int)i, w.data(), b.data(), c->stream);
        if (st == RFD_OK && L.has_affine) st = c->net.set_affine((int)i, sc.data(), sh.data(), c->stream);
        if (st != RFD_OK) { fclose(f); return st; }
    }
    fclose(f);
    c->net.weights_ready = true;
    return RFD_OK;
}

// ---- hot path ----
int rfd_detect_batch(rfd_ctx *c, const rfd_image *imgs, int n, rfd_dets *out)
{
    return detect_impl(c, imgs, n, out, false, 0, false);
}
int rfd_detect_batch_device(rfd_ctx *c, const rfd_image *imgs, int n, rfd_dets *out, int async)
{
    RFD_CHECK_ARG(out && out->total, "out->total must be a device buffer for the device entry point");
    return detect_impl(c, imgs, n, out, true, async, true);
}
int rfd_sync(rfd_ctx *c)
{
    RFD_CHECK_ARG(c, "ctx is null");
    RFD_HIP(hipStreamSynchronize(c->stream));
    return check_nms_flag(c);
}

// ---- multi-GPU gather ----
int rfd_comm_get_unique_id(void *id)
{
    RFD_CHECK_ARG(id != nullptr, "id is null");
    RFD_TRY(rccl_load());
    Rccl::UniqueId u;
    RFD_RCCL(g_rccl.GetUniqueId(&u));
    memcpy(id, &u, sizeof u);
    return RFD_OK;
}

int rfd_comm_init(rfd_ctx *c, const void *unique_id, int rank, int world)
{
    RFD_CHECK_ARG(c && unique_id, "null argument");
    RFD_CHECK_ARG(world >= 1 && rank >= 0 && rank < world, "rank / world out of range");
    if (c->comm) { set_error("the context already has a communicator: call rfd_comm_destroy first"); return RFD_ERR_STATE; }
    RFD_TRY(rccl_load());
    RFD_HIP(hipSetDevice(c->cfg.device_id)); // the communicator binds to the calling thread's current device
    Rccl::UniqueId u;
    memcpy(&u, unique_id, sizeof u);
    Rccl::Comm comm = nullptr;
    RFD_RCCL(g_rccl.CommInitRank(&comm, world, u, rank));
    c->comm = comm; c->comm_rank = rank; c->comm_world = world;
    return RFD_OK;
}

int rfd_comm_info(const rfd_ctx *c, int *rank, int *world)
{
    RFD_CHECK_ARG(c, "ctx is null");
    if (rank) *rank = c->comm ? c->comm_rank : 0;
    if (world) *world = c->comm ? c->comm_world : 0;
    return RFD_OK;
}

int rfd_gather_detections(rfd_ctx *c, const rfd_dets *local, int n_local, rfd_dets *all)
{
    RFD_CHECK_ARG(c && local && all, "null argument");
    RFD_CHECK_ARG(local->boxes && local->landmarks && local->count && all->boxes && all->landmarks && all->count,
                  "slab pointers are null");
    RFD_CHECK_ARG((local->total != nullptr) == (all->total != nullptr), "total must be given in both slabs or in neither");
    if (!c->comm) { set_error("no communicator: call rfd_comm_init first"); return RFD_ERR_STATE; }
    RFD_TRY(check_batch(c, n_local, "n_local"));
    RFD_HIP(hipSetDevice(c->cfg.device_id));
    const size_t MD = (size_t)c->cfg.max_det, n = (size_t)n_local;
    // four arrays, one fused collective; everything moves as 32-bit words (floats are not interpreted)
    RFD_RCCL(g_rccl.GroupStart());
    int r = g_rccl.AllGather(local->boxes, all->boxes, n * MD * 5, Rccl::kInt32, c->comm, c->stream);
    if (r == 0) r = g_rccl.AllGather(local->landmarks, all->landmarks, n * MD * 10, Rccl::kInt32, c->comm, c->stream);
    if (r == 0) r = g_rccl.AllGather(local->count, all->count, n, Rccl::kInt32, c->comm, c->stream);
    if (r == 0 && local->total) r = g_rccl.AllGather(local->total, all->total, n, Rccl::kInt32, c->comm, c->stream);
    const int e = g_rccl.GroupEnd();
    if (r != 0 || e != 0) {
        set_error("ncclAllGather of the detection slabs failed: %s", g_rccl.GetErrorString(r != 0 ? r : e));
        return RFD_ERR_COMM;
    }
    return RFD_OK;
}

int rfd_comm_destroy(rfd_ctx *c)
{
    RFD_CHECK_ARG(c, "ctx is null");
    if (!c->comm) return RFD_OK;
    RFD_HIP(hipSetDevice(c->cfg.device_id));
    RFD_HIP(hipStreamSynchronize(c->stream));
    RFD_RCCL(g_rccl.CommDestroy(c->comm));
    c->comm = nullptr; c->comm_world = 0; c->comm_rank = 0;
    return RFD_OK;
}

// ---- pipelined host entry ----
int rfd_host_alloc(size_t bytes, void **ptr)
{
    RFD_CHECK_ARG(ptr && bytes > 0, "bad argument");
    RFD_HIP(hipHostMalloc(ptr, bytes, hipHostMallocDefault));
    return RFD_OK;
}
int rfd_host_free(void *ptr)
{
    if (ptr) RFD_HIP(hipHostFree(ptr));
    return RFD_OK;
}

int rfd_submit_batch(rfd_ctx *c, const rfd_image *imgs, int n)
{
    RFD_CHECK_ARG(c != nullptr, "ctx is null");
    RFD_TRY(check_images(c, imgs, n));
    if (c->pipe_inflight >= rfd_ctx::kPipe) {
        set_error("%d batches are already in flight: call rfd_collect_batch first", c->pipe_inflight);
        return RFD_ERR_STATE;
    }
    RFD_HIP(hipSetDevice(c->cfg.device_id));
    RFD_TRY(c->ensure_network());
    const size_t B = (size_t)c->cfg.max_batch_size, MD = (size_t)c->cfg.max_det;
    rfd_ctx::PipeSlot &ps = c->pipe[c->pipe_head];
    RFD_TRY(c->copy_stream.create());
    if (!ps.done) { // first use of this slot
        RFD_TRY(ps.h2d.create());
        RFD_TRY(ps.done.create());
        RFD_TRY(ps.pin_imgs.alloc(B));
        RFD_TRY(ps.pin_scale.alloc(B));
        RFD_TRY(ps.h_ob.alloc(B * MD * 5));
        RFD_TRY(ps.h_ol.alloc(B * MD * 10));
        RFD_TRY(ps.h_oc.alloc(B));
        RFD_TRY(ps.h_ot.alloc(B));
        RFD_TRY(ps.imgs.reserve(B * sizeof(PreImage)));
        RFD_TRY(ps.scale.reserve(B * sizeof(float)));
        RFD_TRY(ps.ob.reserve(B * MD * 5 * sizeof(float)));
        RFD_TRY(ps.ol.reserve(B * MD * 10 * sizeof(float)));
        RFD_TRY(ps.oc.reserve(B * sizeof(int)));
        RFD_TRY(ps.ot.reserve(B * sizeof(int)));
    }
    const size_t total = frames_bytes(imgs, n);
    if (total > ps.frames.cap) { // growing the frame buffer frees the old one: nothing of this slot is in flight (it was collected)
        RFD_TRY(ps.frames.reserve(total + total / 4));
    }
    // copy stream: frames + descriptors of THIS batch while the main stream still computes the previous one
    size_t off = 0;
    for (int i = 0; i < n; ++i) {
        RFD_TRY(fill_pre_image(c, imgs[i], i, &ps.pin_imgs[i], &ps.pin_scale[i]));
        ps.pin_imgs[i].src = (uint8_t *)ps.frames.p + off;
        ps.pin_imgs[i].stride = (long long)imgs[i].width * 3;
        off += (size_t)imgs[i].width * 3 * imgs[i].height;
    }
    // Frames that lie back to back in host memory with tight rows (a decoder writing into one rfd_host_alloc block) travel as
    // ONE copy per run: every copy command on the copy stream costs the compute streams a little (the same 39 MB as 32 commands
    // measured 0.1 ms per batch slower than as one, round 3).
    for (int i = 0; i < n;) {
        size_t bytes = (size_t)imgs[i].width * 3 * imgs[i].height;
        int j = i + 1;
        if (imgs[i].stride == (ptrdiff_t)imgs[i].width * 3) {
            while (j < n && imgs[j].stride == (ptrdiff_t)imgs[j].width * 3 && imgs[j].data == imgs[i].data + bytes) {
                bytes += (size_t)imgs[j].width * 3 * imgs[j].height;
                ++j;
            }
            RFD_HIP(hipMemcpyAsync((void *)ps.pin_imgs[i].src, imgs[i].data, bytes, hipMemcpyHostToDevice, c->copy_stream));
        } else {
            const size_t row = (size_t)imgs[i].width * 3;
            RFD_HIP(hipMemcpy2DAsync((void *)ps.pin_imgs[i].src, row, imgs[i].data, (size_t)imgs[i].stride, row, imgs[i].height,
                                     hipMemcpyHostToDevice, c->copy_stream));
        }
        i = j;
    }
    RFD_HIP(hipMemcpyAsync(ps.imgs.p, ps.pin_imgs, n * sizeof(PreImage), hipMemcpyHostToDevice, c->copy_stream));
    RFD_HIP(hipMemcpyAsync(ps.scale.p, ps.pin_scale, n * sizeof(float), hipMemcpyHostToDevice, c->copy_stream));
    RFD_HIP(hipEventRecord(ps.h2d, c->copy_stream));
    if (!c->net.profiling && c->net.multi_stream && c->net.num_parts(n) == 2 && c->net.weights_ready) {
        // Round 3: the same two-chain, cross-call-overlapped pass rfd_detect_batch_device(async = 2) runs -- the chains of this
        // batch wait for its frames (h2d) and otherwise only for their own stream order, so they start under the tail and the
        // decode / sort / NMS of the previous batch.  (Until round 2 the whole pass sat on the caller's stream behind the previous
        // batch, D2H included: 7.0 k against 7.5 k img/s device-resident.)
        std::vector<rfd_image> dev(n);
        for (int i = 0; i < n; ++i) {
            dev[i].data = (const uint8_t *)ps.pin_imgs[i].src; dev[i].height = imgs[i].height; dev[i].width = imgs[i].width;
            dev[i].stride = (ptrdiff_t)imgs[i].width * 3;
        }
        rfd_dets dd;
        dd.boxes = (float *)ps.ob.p; dd.landmarks = (float *)ps.ol.p; dd.count = (int *)ps.oc.p; dd.total = (int *)ps.ot.p;
        RFD_TRY(detect_overlapped(c, dev.data(), n, &dd, ps.h2d));
    } else {
        // main stream: the whole hot path of this batch, behind the previous batch
        c->ov_last_n = -1;
        RFD_HIP(hipStreamWaitEvent(c->stream, ps.h2d, 0));
        RFD_TRY(launch_preprocess(pre_params(c, ps.imgs.p, 0), n, c->stream));
        RFD_TRY(c->net.run_graphed(n, c->stream));
        DecodeParams dp = decode_params(c, true);
        RFD_TRY(post_network(c, dp, false, n, (float *)ps.ob.p, (float *)ps.ol.p, (int *)ps.oc.p, (int *)ps.ot.p, nullptr,
                             (const float *)ps.scale.p));
    }
    // detections go back on their own stream: neither the next batch's compute (caller's stream) nor its frames (copy stream,
    // enqueued earlier than this batch's NMS finishes) queue behind them
    RFD_TRY(c->d2h_stream.create());
    RFD_TRY(ps.post.create());
    RFD_HIP(hipEventRecord(ps.post, c->stream));
    RFD_HIP(hipStreamWaitEvent(c->d2h_stream, ps.post, 0));
    // the first kPipeRows rows of every image now (two strided copies); an image that kept more has the rest fetched by
    // rfd_collect_batch -- dense crowds only: the slabs hold max_det rows per image, a typical frame uses a few dozen
    const size_t R = std::min<size_t>(MD, rfd_ctx::kPipeRows);
    RFD_HIP(hipMemcpy2DAsync(ps.h_ob, MD * 5 * sizeof(float), ps.ob.p, MD * 5 * sizeof(float), R * 5 * sizeof(float), n, hipMemcpyDeviceToHost, c->d2h_stream));
    RFD_HIP(hipMemcpy2DAsync(ps.h_ol, MD * 10 * sizeof(float), ps.ol.p, MD * 10 * sizeof(float), R * 10 * sizeof(float), n, hipMemcpyDeviceToHost, c->d2h_stream));
    RFD_HIP(hipMemcpyAsync(ps.h_oc, ps.oc.p, n * sizeof(int), hipMemcpyDeviceToHost, c->d2h_stream));
    RFD_HIP(hipMemcpyAsync(ps.h_ot, ps.ot.p, n * sizeof(int), hipMemcpyDeviceToHost, c->d2h_stream));
    RFD_HIP(hipEventRecord(ps.done, c->d2h_stream));
    ps.n = n;
    c->pipe_head = (c->pipe_head + 1) % rfd_ctx::kPipe;
    ++c->pipe_inflight;
    return RFD_OK;
}

int rfd_collect_batch(rfd_ctx *c, rfd_dets *out, int *n_out)
{
    RFD_CHECK_ARG(c && out && out->boxes && out->landmarks && out->count, "null argument");
    if (c->pipe_inflight <= 0) { set_error("no batch in flight"); return RFD_ERR_STATE; }
    rfd_ctx::PipeSlot &ps = c->pipe[c->pipe_tail];
    RFD_HIP(hipEventSynchronize(ps.done));
    if (*c->h_nms_flag) { // drop the batch: its detections cannot be trusted
        c->pipe_tail = (c->pipe_tail + 1) % rfd_ctx::kPipe;
        --c->pipe_inflight;
        return check_nms_flag(c);
    }
    const size_t MD = (size_t)c->cfg.max_det;
    bool more = false;
    for (int i = 0; i < ps.n; ++i)
        if ((size_t)ps.h_oc[i] > (size_t)rfd_ctx::kPipeRows) { // rows beyond the prefix copied by rfd_submit_batch
            const size_t R = rfd_ctx::kPipeRows, k = (size_t)ps.h_oc[i];
            RFD_HIP(hipMemcpyAsync(ps.h_ob + ((size_t)i * MD + R) * 5, (const float *)ps.ob.p + ((size_t)i * MD + R) * 5, (k - R) * 5 * sizeof(float), hipMemcpyDeviceToHost, c->d2h_stream));
            RFD_HIP(hipMemcpyAsync(ps.h_ol + ((size_t)i * MD + R) * 10, (const float *)ps.ol.p + ((size_t)i * MD + R) * 10, (k - R) * 10 * sizeof(float), hipMemcpyDeviceToHost, c->d2h_stream));
            more = true;
        }
    if (more) RFD_HIP(hipStreamSynchronize(c->d2h_stream));
    for (int i = 0; i < ps.n; ++i) {
        const int k = ps.h_oc[i];
        memcpy(out->boxes + (size_t)i * MD * 5, ps.h_ob + (size_t)i * MD * 5, (size_t)k * 5 * sizeof(float));
        memcpy(out->landmarks + (size_t)i * MD * 10, ps.h_ol + (size_t)i * MD * 10, (size_t)k * 10 * sizeof(float));
        out->count[i] = k;
        if (out->total) out->total[i] = ps.h_ot[i];
    }
    if (n_out) *n_out = ps.n;
    c->pipe_tail = (c->pipe_tail + 1) % rfd_ctx::kPipe;
    --c->pipe_inflight;
    return RFD_OK;
}

// ---- stage-level entry points ----
int rfd_preprocess(rfd_ctx *c, const rfd_image *imgs, int n, uint8_t *det_img, float *tensor, float *det_scale)
{
    RFD_CHECK_ARG(c != nullptr, "ctx is null");
    RFD_TRY(check_images(c, imgs, n));
    RFD_HIP(hipSetDevice(c->cfg.device_id));
    const float *scales;
    RFD_TRY(stage_frames(c, imgs, n, false, &scales));
    const size_t npix = (size_t)n * c->cfg.image_h * c->cfg.image_w;
    PreParams pp = pre_params(c, c->imgs.p, -1);
    if (det_img) { RFD_TRY(c->scratch[0].reserve(npix * 3)); pp.out_det_img = (uint8_t *)c->scratch[0].p; }
    if (tensor) { RFD_TRY(c->scratch[1].reserve(npix * 3 * sizeof(float))); pp.out_tensor = (float *)c->scratch[1].p; }
    RFD_TRY(launch_preprocess(pp, n, c->stream));
    if (det_img) RFD_HIP(hipMemcpyAsync(det_img, pp.out_det_img, npix * 3, hipMemcpyDeviceToHost, c->stream));
    if (tensor) RFD_HIP(hipMemcpyAsync(tensor, pp.out_tensor, npix * 3 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    RFD_HIP(hipStreamSynchronize(c->stream));
    if (det_scale) memcpy(det_scale, scales, n * sizeof(float));
    return RFD_OK;
}

int rfd_forward(rfd_ctx *c, const float *tensor, int n, float *const heads[9])
{
    RFD_CHECK_ARG(c && tensor && heads, "null argument");
    for (int i = 0; i < 9; ++i) RFD_CHECK_ARG(heads[i] != nullptr, "head pointer is null");
    RFD_TRY(check_batch(c, n, "batch"));
    RFD_HIP(hipSetDevice(c->cfg.device_id));
    RFD_TRY(c->ensure_network());
    c->ov_last_n = -1;
    const size_t plane = (size_t)c->cfg.image_h * c->cfg.image_w;
    RFD_TRY(c->scratch[1].reserve(n * plane * 3 * sizeof(float)));
    RFD_HIP(hipMemcpyAsync(c->scratch[1].p, tensor, n * plane * 3 * sizeof(float), hipMemcpyHostToDevice, c->stream));
    RFD_TRY(launch_tensor_to_nhwc4((const float *)c->scratch[1].p, (bf16_t *)c->net.tensor_ptr(c->net.g.input), n,
                                   c->cfg.image_h, c->cfg.image_w, c->stream));
    RFD_TRY(c->net.run(n, c->stream));
    RFD_HIP(hipMemcpyAsync(c->h_nms_flag, c->net.d_fail, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    for (int l = 0; l < kNumLevels; ++l) {
        const size_t hw = (size_t)c->fh[l] * c->fw[l];
        RFD_TRY(c->scratch[2].reserve(n * hw * 32 * sizeof(float)));
        float *base = (float *)c->scratch[2].p;
        float *cls = base, *bbox = base + n * hw * 4, *lmk = base + n * hw * 12;
        RFD_TRY(launch_heads_to_nchw((const float *)c->net.tensor_ptr(c->net.g.heads[l]), cls, bbox, lmk, n,
                                     c->fh[l], c->fw[l], c->stream));
        RFD_HIP(hipMemcpyAsync(heads[3 * l + 0], cls, n * hw * 4 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
        RFD_HIP(hipMemcpyAsync(heads[3 * l + 1], bbox, n * hw * 8 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
        RFD_HIP(hipMemcpyAsync(heads[3 * l + 2], lmk, n * hw * 20 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
        RFD_HIP(hipStreamSynchronize(c->stream)); // scratch[2] is reused by the next level
    }
    if (c->net.profiling) RFD_TRY(c->net.collect_profile());
    return check_nms_flag(c);
}

int rfd_decode_nms(rfd_ctx *c, const float *const heads[9], int n, const float *det_scale, rfd_dets *out,
                   int32_t *gidx)
{
    RFD_CHECK_ARG(c && heads && det_scale, "null argument");
    RFD_CHECK_ARG(out && out->boxes && out->landmarks && out->count, "output buffers are null");
    for (int i = 0; i < 9; ++i) RFD_CHECK_ARG(heads[i] != nullptr, "head pointer is null");
    RFD_TRY(check_batch(c, n, "batch"));
    RFD_HIP(hipSetDevice(c->cfg.device_id));
    DecodeParams dp = decode_params(c, false);
    RFD_TRY(upload_heads(c, heads, n, dp));
    RFD_HIP(hipMemcpyAsync(c->det_scale.p, det_scale, n * sizeof(float), hipMemcpyHostToDevice, c->stream));
    RFD_HIP(hipEventRecord(c->ev[3], c->stream));
    const rfd_dets dev = own_slabs(c);
    RFD_TRY(post_network(c, dp, true, n, dev.boxes, dev.landmarks, dev.count, dev.total, gidx ? (int *)c->out_gidx.p : nullptr));
    RFD_TRY(copy_slabs(c, *out, dev, n, hipMemcpyDeviceToHost));
    if (gidx) RFD_HIP(hipMemcpyAsync(gidx, c->out_gidx.p, (size_t)n * c->cfg.max_det * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    RFD_HIP(hipEventRecord(c->ev[7], c->stream));
    RFD_HIP(hipStreamSynchronize(c->stream));
    RFD_TRY(check_nms_flag(c));
    RFD_TRY(finish_stats(c, n, false, false));
    for (int i = 0; i < n; ++i) c->stats.detections += out->total ? out->total[i] : out->count[i];
    return RFD_OK;
}

// ---- views (rfd.h, "views") ----
void rfd_view_config_default(rfd_view_config *cfg, int net_w, int net_h)
{
    if (cfg) view_config_default(cfg, net_w, net_h);
}

int rfd_view_plan(int frame, int frame_w, int frame_h, const rfd_view_config *cfg, rfd_view *out, int cap, int *count)
{
    const int status = view_plan(frame, frame_w, frame_h, cfg, out, cap, count);
    if (status == RFD_ERR_CAPACITY) set_error("the plan of a %dx%d frame has %d views, cap is %d", frame_w, frame_h, *count, cap);
    else if (status != RFD_OK)
        set_error("invalid argument: a view plan needs cfg and count, frame >= 0, a frame and tiles of at least 1x1 and 0 <= overlap < tile_w, tile_h");
    return status;
}

int rfd_detect_views_batch_device(rfd_ctx *c, const rfd_image *frames, int n_frames, const rfd_view *views, int n_views, float edge_margin,
                                  rfd_dets *out, int async)
{
    return detect_views_impl(c, frames, n_frames, views, n_views, edge_margin, out, true, async);
}

int rfd_detect_views_batch(rfd_ctx *c, const rfd_image *frames, int n_frames, const rfd_view *views, int n_views, float edge_margin, rfd_dets *out)
{
    return detect_views_impl(c, frames, n_frames, views, n_views, edge_margin, out, false, 0);
}

int rfd_decode_nms_views(rfd_ctx *c, const float *const heads[9], const rfd_view *views, int n_views, int n_frames, float edge_margin,
                         rfd_dets *out, int32_t *gidx)
{
    RFD_CHECK_ARG(c && heads, "null argument");
    RFD_CHECK_ARG(out && out->boxes && out->landmarks && out->count, "output buffers are null");
    for (int i = 0; i < 9; ++i) RFD_CHECK_ARG(heads[i] != nullptr, "head pointer is null");
    RFD_HIP(hipSetDevice(c->cfg.device_id));
    PreImage *pis;
    float *pin_ones;
    ViewDesc *vd;
    int vmax = 0;
    RFD_TRY(acquire_frame_slot(c, &pis, &pin_ones));
    RFD_TRY(acquire_views_slot(c, &vd));
    RFD_TRY(plan_views(c, nullptr, n_frames, views, n_views, edge_margin, vd, nullptr, &vmax));
    DecodeParams dp = decode_params(c, false);
    RFD_TRY(upload_heads(c, heads, n_views, dp));
    RFD_TRY(stage_views(c, vd, n_views, pin_ones, n_frames));
    RFD_HIP(hipEventRecord(c->ev[3], c->stream));
    const ViewsPost vp = {(const ViewDesc *)c->view_desc.p, n_views, vmax, edge_margin};
    const rfd_dets dev = own_slabs(c);
    RFD_TRY(post_network(c, dp, true, n_frames, dev.boxes, dev.landmarks, dev.count, dev.total, gidx ? (int *)c->out_gidx.p : nullptr, nullptr, &vp));
    RFD_TRY(copy_slabs(c, *out, dev, n_frames, hipMemcpyDeviceToHost));
    if (gidx) RFD_HIP(hipMemcpyAsync(gidx, c->out_gidx.p, (size_t)n_frames * c->cfg.max_det * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    RFD_HIP(hipEventRecord(c->ev[7], c->stream));
    RFD_HIP(hipStreamSynchronize(c->stream));
    RFD_TRY(check_nms_flag(c));
    RFD_TRY(finish_stats(c, n_frames, false, false));
    for (int i = 0; i < n_frames; ++i) c->stats.detections += out->total ? out->total[i] : out->count[i];
    return RFD_OK;
}

int rfd_nms_sorted(rfd_ctx *c, int32_t *keep, int *num_out, const float *boxes, int boxes_num, int boxes_dim,
                   float thresh)
{
    RFD_CHECK_ARG(c && keep && num_out && (boxes || boxes_num == 0), "null argument");
    RFD_CHECK_ARG(boxes_num >= 0 && boxes_dim >= 4, "boxes_num < 0 or boxes_dim < 4");
    *num_out = 0;
    if (boxes_num == 0) return RFD_OK;
    RFD_HIP(hipSetDevice(c->cfg.device_id));
    std::vector<float4> packed(boxes_num);
    for (int i = 0; i < boxes_num; ++i) {
        const float *b = boxes + (size_t)i * boxes_dim;
        packed[i] = make_float4(b[0], b[1], b[2], b[3]);
    }
    RFD_TRY(c->scratch[0].reserve((size_t)boxes_num * sizeof(float4)));
    RFD_TRY(c->scratch[1].reserve((size_t)boxes_num * sizeof(int) + 2 * sizeof(int)));
    RFD_HIP(hipMemcpyAsync(c->scratch[0].p, packed.data(), boxes_num * sizeof(float4), hipMemcpyHostToDevice, c->stream));
    NmsParams np;
    memset(&np, 0, sizeof np);
    np.sorted_boxes = (const float4 *)c->scratch[0].p;
    np.presorted_n = boxes_num;
    np.total_anchors = boxes_num;
    np.max_det = boxes_num;
    np.iou_thr = thresh;
    int *d_total = (int *)c->scratch[1].p;
    np.out_total = d_total;
    np.out_gidx = d_total + 2;
    RFD_TRY(launch_nms(np, 1, c->stream));
    int total = 0;
    RFD_HIP(hipMemcpyAsync(&total, d_total, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    RFD_HIP(hipStreamSynchronize(c->stream));
    RFD_HIP(hipMemcpy(keep, d_total + 2, (size_t)total * sizeof(int), hipMemcpyDeviceToHost));
    *num_out = total;
    return RFD_OK;
}

void _nms(int32_t *keep, int *num_out, float *boxes, int boxes_num, int boxes_dim, float thresh, int device_id)
{
    if (num_out) *num_out = -1;
    if (device_id < 0 || device_id >= 16 || !keep || !num_out) return;
    std::lock_guard<std::mutex> lk(g_nms_mu);
    if (!g_nms_ctx[device_id]) {
        rfd_config cfg;
        rfd_config_default(&cfg);
        cfg.device_id = device_id;
        cfg.max_det = 1;
        if (rfd_create(&cfg, &g_nms_ctx[device_id]) != RFD_OK) { g_nms_ctx[device_id] = nullptr; return; }
    }
    if (rfd_nms_sorted(g_nms_ctx[device_id], keep, num_out, boxes, boxes_num, boxes_dim, thresh) != RFD_OK) *num_out = -1;
}

// ---- JPEG decode (rfd.h, "JPEG decode"): the entries; the host side of a decode call is csrc/jpeg_host.hip ----
int rfd_jpeg_info(const uint8_t *bytes, size_t len, struct rfd_jpeg_info *out)
{
    char msg[256] = "";
    const int st = jpeg_info(bytes, len, out, msg, sizeof msg);
    if (st != RFD_OK) set_error("%s", msg);
    return st;
}

int rfd_jpeg_orientation(const uint8_t *bytes, size_t len, struct rfd_jpeg_orientation *out)
{
    char msg[256] = "";
    const int st = jpeg_orientation(bytes, len, out, msg, sizeof msg);
    if (st != RFD_OK) set_error("%s", msg);
    return st;
}

int rfd_debug_jpeg_coefficients(const uint8_t *bytes, size_t len, int16_t *out, size_t cap_blocks, size_t *blocks)
{
    RFD_CHECK_ARG(out || cap_blocks == 0, "out is null");
    char msg[256] = "";
    const int st = jpeg_debug_coefficients(bytes, len, out, cap_blocks, blocks, msg, sizeof msg);
    if (st != RFD_OK) set_error("%s", msg);
    return st;
}

int rfd_jpeg_scaled_size(const uint8_t *bytes, size_t len, int denom, int orientation_mode, struct rfd_jpeg_scaled_size *out)
{
    if (!jpeg_scale_valid(denom)) { set_error("invalid argument: JPEG scale denominator %d (1, 2, 4 or 8)", denom); return RFD_ERR_INVALID_ARG; }
    if (orientation_mode != RFD_JPEG_ORIENTATION_IGNORE && orientation_mode != RFD_JPEG_ORIENTATION_APPLY) {
        set_error("invalid argument: JPEG orientation mode %d (0: ignore, 1: apply)", orientation_mode);
        return RFD_ERR_INVALID_ARG;
    }
    char msg[256] = "";
    const int st = jpeg_scaled_size(bytes, len, denom, orientation_mode, out, msg, sizeof msg);
    if (st != RFD_OK) set_error("%s", msg);
    return st;
}

int rfd_debug_jpeg_block_counts(const uint8_t *bytes, size_t len, int denom, uint8_t *count, size_t cap_blocks, size_t *blocks)
{
    RFD_CHECK_ARG(count || cap_blocks == 0, "count is null");
    if (!jpeg_scale_valid(denom)) { set_error("invalid argument: JPEG scale denominator %d (1, 2, 4 or 8)", denom); return RFD_ERR_INVALID_ARG; }
    char msg[256] = "";
    const int st = jpeg_debug_coefficients(bytes, len, nullptr, cap_blocks, blocks, msg, sizeof msg, denom, count);
    if (st != RFD_OK) set_error("%s", msg);
    return st;
}

int rfd_set_decode_threads(rfd_ctx *c, int threads)
{
    RFD_CHECK_ARG(c, "ctx is null");
    if (threads < 1 || threads > 16) { set_error("invalid argument: %d decode threads (1..16)", threads); return RFD_ERR_INVALID_ARG; }
    c->jpeg.decode_threads = threads;
    return RFD_OK;
}

int rfd_set_jpeg_entropy(rfd_ctx *c, int mode)
{
    RFD_CHECK_ARG(c, "ctx is null");
    if (mode != RFD_JPEG_ENTROPY_HOST && mode != RFD_JPEG_ENTROPY_DEVICE) { set_error("invalid argument: JPEG entropy mode %d (0: host, 1: device)", mode); return RFD_ERR_INVALID_ARG; }
    c->jpeg.entropy = mode;
    return RFD_OK;
}

int rfd_set_jpeg_scale(rfd_ctx *c, int denom)
{
    RFD_CHECK_ARG(c, "ctx is null");
    if (!jpeg_scale_valid(denom)) { set_error("invalid argument: JPEG scale denominator %d (1, 2, 4 or 8)", denom); return RFD_ERR_INVALID_ARG; }
    c->jpeg.scale = denom;
    return RFD_OK;
}

int rfd_set_jpeg_orientation(rfd_ctx *c, int mode)
{
    RFD_CHECK_ARG(c, "ctx is null");
    if (mode != RFD_JPEG_ORIENTATION_IGNORE && mode != RFD_JPEG_ORIENTATION_APPLY) { set_error("invalid argument: JPEG orientation mode %d (0: ignore, 1: apply)", mode); return RFD_ERR_INVALID_ARG; }
    c->jpeg.orientation = mode;
    return RFD_OK;
}

int rfd_jpeg_last_orientations(rfd_ctx *c, int32_t *orientation, int cap, int *n)
{
    RFD_CHECK_ARG(c, "ctx is null");
    RFD_CHECK_ARG(cap >= 0 && (orientation || cap == 0), "orientation is null");
    const int have = (int)c->jpeg.orientations.size();
    if (n) *n = have;
    if (have > cap) { set_error("the last decode call had %d frames, the output holds %d", have, cap); return RFD_ERR_CAPACITY; }
    for (int i = 0; i < have; ++i) orientation[i] = c->jpeg.orientations[(size_t)i];
    return RFD_OK;
}

int rfd_jpeg_last_paths(rfd_ctx *c, int32_t *path, int cap, int *n)
{
    RFD_CHECK_ARG(c, "ctx is null");
    RFD_CHECK_ARG(cap >= 0 && (path || cap == 0), "path is null");
    const int have = (int)c->jpeg.paths.size();
    if (n) *n = have;
    if (have > cap) { set_error("the last decode call had %d frames, the output holds %d", have, cap); return RFD_ERR_CAPACITY; }
    for (int i = 0; i < have; ++i) path[i] = c->jpeg.paths[(size_t)i];
    return RFD_OK;
}

int rfd_debug_jpeg_intervals(const uint8_t *bytes, size_t len, uint32_t *begin, uint32_t *end, size_t cap, size_t *count)
{
    RFD_CHECK_ARG((begin && end) || cap == 0, "begin or end is null");
    std::unique_ptr<JpegHeader> h(new JpegHeader);
    const int st = jpeg_parse_header(bytes, len, *h);
    if (st != RFD_OK) { set_error("%s", h->msg); return st; }
    char msg[200] = "";
    size_t want = 0;
    bool ok = jpeg_device_eligible(bytes, len, *h, begin, end, 0, &want, msg, sizeof msg); // the header's part of the rule, and the count
    if (count) *count = want;
    if (ok && want > cap) { set_error("the file has %zu restart intervals, the output holds %zu", want, cap); return RFD_ERR_CAPACITY; }
    ok = ok && jpeg_device_eligible(bytes, len, *h, begin, end, cap, &want, msg, sizeof msg);
    if (!ok) { set_error("%s", msg); return RFD_ERR_UNSUPPORTED; }
    return RFD_OK;
}

int rfd_debug_jpeg_coefficients_device(rfd_ctx *c, const uint8_t *bytes, size_t len, int16_t *out, size_t cap_blocks, size_t *blocks)
{
    RFD_CHECK_ARG(c, "ctx is null");
    RFD_CHECK_ARG(out || cap_blocks == 0, "out is null");
    return c->jpeg.debug_coefficients(c->stream, c->cfg, bytes, len, out, cap_blocks, blocks);
}

// both forms of the decode: the argument checks that need the context, JpegDecoder::decode, and the fault word where it synchronised
static int jpeg_decode_entry(rfd_ctx *c, const uint8_t *const *bytes, const size_t *len, int n, const rfd_image *out, bool out_on_device, int async)
{
    RFD_CHECK_ARG(c, "ctx is null");
    RFD_CHECK_ARG(n >= 0, "n < 0");
    if (n == 0) return RFD_OK;
    RFD_CHECK_ARG(bytes && len && out, "null argument");
    RFD_TRY(check_batch(c, n, "batch of", " files"));
    RFD_TRY(c->jpeg.decode(c->stream, c->cfg, bytes, len, n, out, out_on_device, async != 0));
    if (async && out_on_device) return RFD_OK;
    return check_nms_flag(c);
}

int rfd_decode_jpeg_batch_device(rfd_ctx *c, const uint8_t *const *bytes, const size_t *len, int n, const rfd_image *out, int async)
{
    return jpeg_decode_entry(c, bytes, len, n, out, true, async);
}

int rfd_decode_jpeg_batch(rfd_ctx *c, const uint8_t *const *bytes, const size_t *len, int n, const rfd_image *out)
{
    return jpeg_decode_entry(c, bytes, len, n, out, false, 0);
}

} // extern "C"
