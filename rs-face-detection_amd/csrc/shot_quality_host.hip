// shot_quality_host.hip -- the rfd_shot_quality* entries of include/rfd.h ("shot quality").  What a context keeps for them is
// shot_quality_host.h, their checks and geometry are shot_quality_plan.h, their kernel is kernels_shot_quality.hip.
#include "shot_quality_host.h"

#include <memory>

using namespace rfd;

int rfd_shot_quality_config_default(rfd_shot_quality_config *cfg)
{
    RFD_CHECK_ARG(cfg != nullptr, "cfg is null");
    memset(cfg, 0, sizeof *cfg);
    // chosen values, not tuned on data (rfd.h)
    cfg->dark = 30;
    cfg->bright = 225;
    cfg->pitch0 = 0.495f; // the nose between the eye line and the mouth line of the 112 x 112 alignment template
    cfg->w_yaw = 1.0f;
    cfg->w_roll = 1.0f;
    cfg->w_pitch = 2.0f;
    cfg->sharp_ref = 64.0f;
    cfg->size_ref = 112.0f;
    cfg->times_score = 0;
    return RFD_OK;
}

// The checks both forms share, in an order that needs the context last: nothing is enqueued before they pass.  *cfg is
// replaced by the default when NULL.  n = 0 passes with whatever pointers.
static int shot_quality_check(rfd_ctx *c, const rfd_image *imgs, int n, const rfd_dets *dets, const rfd_shot_quality_config **cfg,
                              rfd_shot_quality_config *def, const float *quality, int *max_batch, int *max_det)
{
    char msg[128];
    if (!*cfg) { RFD_TRY(rfd_shot_quality_config_default(def)); *cfg = def; }
    if (!sq_config_ok(**cfg, msg, sizeof msg)) { set_error("invalid argument: shot quality config: %s", msg); return RFD_ERR_INVALID_ARG; }
    RFD_CHECK_ARG(n >= 0, "n < 0");
    if (n > 0) {
        RFD_CHECK_ARG(imgs != nullptr, "imgs is null");
        RFD_CHECK_ARG(dets && dets->boxes && dets->landmarks && dets->count, "dets: boxes, landmarks or count is null");
        RFD_CHECK_ARG(quality != nullptr, "quality is null");
    }
    RFD_CHECK_ARG(c != nullptr, "ctx is null");
    rfd_config cc;
    RFD_TRY(rfd_get_config(c, &cc));
    if (n > cc.max_batch_size) {
        set_error("shot quality of %d frames exceeds max_batch_size %d", n, cc.max_batch_size);
        return RFD_ERR_CAPACITY;
    }
    for (int i = 0; i < n; ++i)
        if (!sq_frame_ok(imgs[i], i, msg, sizeof msg)) { set_error("invalid argument: %s", msg); return RFD_ERR_INVALID_ARG; }
    *max_batch = cc.max_batch_size;
    *max_det = cc.max_det;
    return RFD_OK;
}

// descriptors, copy, launch: all device pointers, enqueued only.  desc: where the kernel reads each frame.
static int shot_quality_enqueue(rfd_ctx *c, const SqImage *desc, int n, int max_batch, int max_det, const rfd_dets &dets,
                                const rfd_shot_quality_config &cfg, float *quality, float *parts, int32_t *status)
{
    ShotQuality &sq = ctx_shot_quality(c);
    const hipStream_t s = ctx_stream(c);
    RFD_TRY(sq.ring.ensure((size_t)max_batch * sizeof(SqImage))); // first call on this context
    RFD_TRY(sq.imgs.reserve((size_t)max_batch * sizeof(SqImage)));
    SqImage *slot;
    RFD_TRY(sq.ring.acquire(&slot));
    memcpy(slot, desc, (size_t)n * sizeof(SqImage));
    RFD_HIP(hipMemcpyAsync(sq.imgs.p, slot, (size_t)n * sizeof(SqImage), hipMemcpyHostToDevice, s));
    RFD_TRY(sq.ring.record(s));
    SqParams p;
    memset(&p, 0, sizeof p);
    p.imgs = (const SqImage *)sq.imgs.p;
    p.n = n; p.max_det = max_det;
    p.boxes = dets.boxes; p.lmk = dets.landmarks; p.count = dets.count;
    p.lo16 = 16 * cfg.dark; p.hi16 = 16 * cfg.bright;
    p.pitch0 = cfg.pitch0; p.w_yaw = cfg.w_yaw; p.w_roll = cfg.w_roll; p.w_pitch = cfg.w_pitch;
    p.sharp_ref = cfg.sharp_ref; p.size_ref = cfg.size_ref; p.times_score = cfg.times_score;
    p.quality = quality; p.parts = parts; p.status = status;
    return launch_shot_quality(p, s);
}

int rfd_shot_quality_device(rfd_ctx *c, const rfd_image *imgs, int n, const rfd_dets *dets, const rfd_shot_quality_config *cfg,
                            float *quality, float *parts, int32_t *status, int async)
{
    rfd_shot_quality_config def;
    int max_batch = 0, max_det = 0;
    RFD_TRY(shot_quality_check(c, imgs, n, dets, &cfg, &def, quality, &max_batch, &max_det));
    if (n == 0) return RFD_OK;
    RFD_HIP(hipSetDevice(ctx_device(c)));
    SqImage desc[64];
    std::unique_ptr<SqImage[]> big;
    SqImage *d = desc;
    if (n > 64) { big.reset(new SqImage[(size_t)n]); d = big.get(); }
    for (int i = 0; i < n; ++i) d[i] = SqImage{imgs[i].data, (long long)imgs[i].stride, imgs[i].height, imgs[i].width};
    RFD_TRY(shot_quality_enqueue(c, d, n, max_batch, max_det, *dets, *cfg, quality, parts, status));
    if (async) return RFD_OK;
    RFD_HIP(hipStreamSynchronize(ctx_stream(c)));
    return RFD_OK;
}

int rfd_shot_quality(rfd_ctx *c, const rfd_image *imgs, int n, const rfd_dets *dets, const rfd_shot_quality_config *cfg,
                     float *quality, float *parts, int32_t *status)
{
    rfd_shot_quality_config def;
    int max_batch = 0, max_det = 0;
    RFD_TRY(shot_quality_check(c, imgs, n, dets, &cfg, &def, quality, &max_batch, &max_det));
    if (n == 0) return RFD_OK;
    RFD_HIP(hipSetDevice(ctx_device(c)));
    ShotQuality &sq = ctx_shot_quality(c);
    const hipStream_t s = ctx_stream(c);
    const size_t N = (size_t)n, MD = (size_t)max_det;
    // the frames, packed back to back with tight rows, one 2-D copy each
    size_t total = 0;
    for (int i = 0; i < n; ++i) total += (size_t)imgs[i].height * imgs[i].width * 3;
    RFD_TRY(sq.h_frames.reserve(total));
    // every array with its device twin; the outputs go up too, so that what they hold past the counts comes back as it was
    struct Twin { DevBuf *dev; const void *in; void *back; size_t bytes; };
    const Twin twins[] = {
        {&sq.h_boxes, dets->boxes, nullptr, N * MD * 5 * sizeof(float)},
        {&sq.h_lmk, dets->landmarks, nullptr, N * MD * 10 * sizeof(float)},
        {&sq.h_count, dets->count, nullptr, N * sizeof(int32_t)},
        {&sq.h_quality, quality, quality, N * MD * sizeof(float)},
        {&sq.h_parts, parts, parts, N * MD * RFD_SHOT_QUALITY_PARTS * sizeof(float)},
        {&sq.h_status, status, status, N * MD * sizeof(int32_t)},
    };
    for (const Twin &w : twins)
        if (w.in) RFD_TRY(w.dev->reserve(w.bytes));
    std::unique_ptr<SqImage[]> desc(new SqImage[N]);
    size_t off = 0;
    for (int i = 0; i < n; ++i) {
        uint8_t *dst = (uint8_t *)sq.h_frames.p + off;
        const size_t rowb = (size_t)imgs[i].width * 3;
        RFD_HIP(hipMemcpy2DAsync(dst, rowb, imgs[i].data, (size_t)imgs[i].stride, rowb, (size_t)imgs[i].height, hipMemcpyHostToDevice, s));
        desc[i] = SqImage{dst, (long long)rowb, imgs[i].height, imgs[i].width};
        off += rowb * (size_t)imgs[i].height;
    }
    for (const Twin &w : twins)
        if (w.in) RFD_HIP(hipMemcpyAsync(w.dev->p, w.in, w.bytes, hipMemcpyHostToDevice, s));
    auto dev = [&](int i) -> void * { return twins[i].in ? twins[i].dev->p : nullptr; };
    const rfd_dets d = {(float *)dev(0), (float *)dev(1), (int32_t *)dev(2), nullptr};
    RFD_TRY(shot_quality_enqueue(c, desc.get(), n, max_batch, max_det, d, *cfg, (float *)dev(3), (float *)dev(4), (int32_t *)dev(5)));
    for (const Twin &w : twins)
        if (w.back) RFD_HIP(hipMemcpyAsync(w.back, w.dev->p, w.bytes, hipMemcpyDeviceToHost, s));
    RFD_HIP(hipStreamSynchronize(s));
    return RFD_OK;
}
