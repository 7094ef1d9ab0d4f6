// annotate_host.hip -- the rfd_annotate_faces* entries of include/rfd.h ("annotation").  What a context keeps for them is
// annotate_host.h, their checks, geometry and text are annotate_plan.h, their kernel is kernels_annotate.hip.
#include "annotate_host.h"

#include <memory>

using namespace rfd;

int rfd_annotate_config_default(rfd_annotate_config *cfg)
{
    RFD_CHECK_ARG(cfg != nullptr, "cfg is null");
    memset(cfg, 0, sizeof *cfg);
    // chosen values, not tuned on data (rfd.h): box, landmarks, score %
    cfg->n_styles = 1;
    cfg->style[0].colour[1] = 255; // every row green
    cfg->thickness = 2;
    cfg->mark_radius = 2;
    cfg->label_source = RFD_ANNOTATE_NONE;
    cfg->value_source = RFD_ANNOTATE_SCORE;
    cfg->text_scale = 2;
    cfg->alpha = 256;
    return RFD_OK;
}

int rfd_debug_annotate_glyph(int glyph, uint8_t rows[7])
{
    RFD_CHECK_ARG(glyph >= 0 && glyph < kAnGlyphs, "glyph outside 0..13");
    RFD_CHECK_ARG(rows != nullptr, "rows is null");
    memcpy(rows, kAnFont[glyph], 7);
    return RFD_OK;
}

// The checks both forms share, in an order that needs the context last: nothing is enqueued before they pass.  *cfg is
// replaced by the default when NULL.  n = 0 passes with whatever pointers.
static int annotate_check(rfd_ctx *c, const rfd_image *imgs, const rfd_image *dst, int n, const rfd_dets *dets, const int32_t *label,
                          const float *value, const rfd_annotate_config **cfg, rfd_annotate_config *def, int *max_batch, int *max_det)
{
    char msg[160];
    if (!*cfg) { RFD_TRY(rfd_annotate_config_default(def)); *cfg = def; }
    if (!an_config_ok(**cfg, msg, sizeof msg)) { set_error("invalid argument: annotate config: %s", msg); return RFD_ERR_INVALID_ARG; }
    RFD_CHECK_ARG(n >= 0, "n < 0");
    if (n > 0) {
        RFD_CHECK_ARG(imgs != nullptr, "imgs is null");
        RFD_CHECK_ARG(dets && dets->boxes && dets->count, "dets: boxes or count is null");
        RFD_CHECK_ARG((*cfg)->mark_radius == 0 || dets->landmarks, "dets: landmarks is null with mark_radius > 0");
        RFD_CHECK_ARG((*cfg)->label_source != RFD_ANNOTATE_ARRAY || label, "label is null with label_source = ARRAY");
        RFD_CHECK_ARG((*cfg)->value_source != RFD_ANNOTATE_ARRAY || value, "value is null with value_source = ARRAY");
    }
    RFD_CHECK_ARG(c != nullptr, "ctx is null");
    rfd_config cc;
    RFD_TRY(rfd_get_config(c, &cc));
    if (n > cc.max_batch_size) {
        set_error("annotation of %d frames exceeds max_batch_size %d", n, cc.max_batch_size);
        return RFD_ERR_CAPACITY;
    }
    for (int i = 0; i < n; ++i) {
        const bool ok = rd_frame_ok(imgs[i], "frame", i, msg, sizeof msg) && (!dst || rd_dst_ok(dst[i], imgs[i], i, msg, sizeof msg));
        if (!ok) { set_error("invalid argument: %s", msg); return RFD_ERR_INVALID_ARG; }
    }
    *max_batch = cc.max_batch_size;
    *max_det = cc.max_det;
    return RFD_OK;
}

// descriptors, copy, launch: all device pointers, enqueued only.  desc: where the kernel reads and writes each frame; sizes: the
// frames' sizes for the grid.  An array its source does not name is not handed to the kernel.
static int annotate_enqueue(rfd_ctx *c, const RdImage *desc, const rfd_image *sizes, int n, bool in_place, int max_batch, int max_det,
                            const rfd_dets &dets, const uint32_t *sel, const int32_t *label, const float *value, const rfd_annotate_config &cfg,
                            int32_t *applied)
{
    Annotate &an = ctx_annotate(c);
    const hipStream_t s = ctx_stream(c);
    RFD_TRY(an.ring.ensure((size_t)max_batch * sizeof(RdImage))); // first call on this context
    RFD_TRY(an.imgs.reserve((size_t)max_batch * sizeof(RdImage)));
    RdImage *slot;
    RFD_TRY(an.ring.acquire(&slot));
    memcpy(slot, desc, (size_t)n * sizeof(RdImage));
    RFD_HIP(hipMemcpyAsync(an.imgs.p, slot, (size_t)n * sizeof(RdImage), hipMemcpyHostToDevice, s));
    RFD_TRY(an.ring.record(s));
    auto bgr = [](const uint8_t col[4]) { return (uint32_t)col[0] | ((uint32_t)col[1] << 8) | ((uint32_t)col[2] << 16); };
    AnParams p;
    memset(&p, 0, sizeof p);
    p.imgs = (const RdImage *)an.imgs.p;
    p.n = n; p.max_det = max_det;
    p.boxes = dets.boxes; p.count = dets.count; p.sel = sel;
    p.landmarks = cfg.mark_radius > 0 ? dets.landmarks : nullptr;
    p.label = cfg.label_source == RFD_ANNOTATE_ARRAY ? label : nullptr;
    p.value = cfg.value_source == RFD_ANNOTATE_ARRAY ? value : nullptr;
    p.in_place = in_place ? 1 : 0;
    p.n_styles = cfg.n_styles;
    for (int k = 0; k < RFD_ANNOTATE_MAX_STYLES; ++k) {
        p.mask[k] = cfg.style[k].sel_mask; p.want[k] = cfg.style[k].sel_value; p.colour[k] = bgr(cfg.style[k].colour);
    }
    p.text_colour = bgr(cfg.text_colour);
    p.thickness = cfg.thickness; p.mark_radius = cfg.mark_radius; p.label_source = cfg.label_source; p.value_source = cfg.value_source;
    p.text_scale = cfg.text_scale; p.alpha = cfg.alpha;
    p.margin_x = cfg.margin_x; p.margin_top = cfg.margin_top; p.margin_bottom = cfg.margin_bottom;
    p.applied = applied;
    return launch_annotate(p, an_grid(sizes, n), s);
}

int rfd_annotate_faces_device(rfd_ctx *c, const rfd_image *imgs, const rfd_image *dst, int n, const rfd_dets *dets, const uint32_t *sel,
                              const int32_t *label, const float *value, const rfd_annotate_config *cfg, int32_t *applied, int async)
{
    rfd_annotate_config def;
    int max_batch = 0, max_det = 0;
    RFD_TRY(annotate_check(c, imgs, dst, n, dets, label, value, &cfg, &def, &max_batch, &max_det));
    if (n == 0) return RFD_OK;
    RFD_HIP(hipSetDevice(ctx_device(c)));
    RdImage desc[64];
    std::unique_ptr<RdImage[]> big;
    RdImage *d = desc;
    if (n > 64) { big.reset(new RdImage[(size_t)n]); d = big.get(); }
    for (int i = 0; i < n; ++i) {
        const rfd_image &o = dst ? dst[i] : imgs[i]; // rfd_image declares data const; this call writes through it (rfd.h)
        d[i] = RdImage{imgs[i].data, (long long)imgs[i].stride, const_cast<uint8_t *>(o.data), (long long)o.stride, imgs[i].height, imgs[i].width};
    }
    RFD_TRY(annotate_enqueue(c, d, imgs, n, dst == nullptr, max_batch, max_det, *dets, sel, label, value, *cfg, applied));
    if (async) return RFD_OK;
    RFD_HIP(hipStreamSynchronize(ctx_stream(c)));
    return RFD_OK;
}

int rfd_annotate_faces(rfd_ctx *c, const rfd_image *imgs, const rfd_image *dst, int n, const rfd_dets *dets, const uint32_t *sel,
                       const int32_t *label, const float *value, const rfd_annotate_config *cfg, int32_t *applied)
{
    rfd_annotate_config def;
    int max_batch = 0, max_det = 0;
    RFD_TRY(annotate_check(c, imgs, dst, n, dets, label, value, &cfg, &def, &max_batch, &max_det));
    if (n == 0) return RFD_OK;
    RFD_HIP(hipSetDevice(ctx_device(c)));
    Annotate &an = ctx_annotate(c);
    const hipStream_t s = ctx_stream(c);
    const size_t N = (size_t)n, MD = (size_t)max_det;
    // the frames, packed back to back with tight rows, one 2-D copy each; the kernel paints them in place there -- the result
    // is a function of the source and the rows alone -- and their rows go back to dst, or to the frames themselves
    size_t total = 0;
    for (int i = 0; i < n; ++i) total += (size_t)imgs[i].height * imgs[i].width * 3;
    RFD_TRY(an.h_frames.reserve(total));
    struct Twin { DevBuf *dev; const void *in; void *back; size_t bytes; };
    const Twin twins[] = {
        {&an.h_boxes, dets->boxes, nullptr, N * MD * 5 * sizeof(float)},
        {&an.h_count, dets->count, nullptr, N * sizeof(int32_t)},
        {&an.h_landmarks, cfg->mark_radius > 0 ? dets->landmarks : nullptr, nullptr, N * MD * 10 * sizeof(float)},
        {&an.h_sel, sel, nullptr, N * MD * sizeof(uint32_t)},
        {&an.h_label, cfg->label_source == RFD_ANNOTATE_ARRAY ? label : nullptr, nullptr, N * MD * sizeof(int32_t)},
        {&an.h_value, cfg->value_source == RFD_ANNOTATE_ARRAY ? value : nullptr, nullptr, N * MD * sizeof(float)},
        {&an.h_applied, applied, applied, N * sizeof(int32_t)},
    };
    for (const Twin &w : twins)
        if (w.in) RFD_TRY(w.dev->reserve(w.bytes));
    std::unique_ptr<RdImage[]> desc(new RdImage[N]);
    size_t off = 0;
    for (int i = 0; i < n; ++i) {
        uint8_t *at = (uint8_t *)an.h_frames.p + off;
        const size_t rowb = (size_t)imgs[i].width * 3;
        RFD_HIP(hipMemcpy2DAsync(at, rowb, imgs[i].data, (size_t)imgs[i].stride, rowb, (size_t)imgs[i].height, hipMemcpyHostToDevice, s));
        desc[i] = RdImage{at, (long long)rowb, at, (long long)rowb, imgs[i].height, imgs[i].width};
        off += rowb * (size_t)imgs[i].height;
    }
    for (int i = 0; i < 6; ++i)
        if (twins[i].in) RFD_HIP(hipMemcpyAsync(twins[i].dev->p, twins[i].in, twins[i].bytes, hipMemcpyHostToDevice, s));
    auto dev = [&](int i) -> void * { return twins[i].in ? twins[i].dev->p : nullptr; };
    const rfd_dets d = {(float *)dev(0), (float *)dev(2), (int32_t *)dev(1), nullptr};
    RFD_TRY(annotate_enqueue(c, desc.get(), imgs, n, true, max_batch, max_det, d, (const uint32_t *)dev(3), (const int32_t *)dev(4),
                             (const float *)dev(5), *cfg, (int32_t *)dev(6)));
    for (int i = 0; i < n; ++i) {
        const rfd_image &o = dst ? dst[i] : imgs[i];
        const size_t rowb = (size_t)imgs[i].width * 3;
        RFD_HIP(hipMemcpy2DAsync(const_cast<uint8_t *>(o.data), (size_t)o.stride, desc[i].src, rowb, rowb, (size_t)imgs[i].height, hipMemcpyDeviceToHost, s));
    }
    for (const Twin &w : twins)
        if (w.back) RFD_HIP(hipMemcpyAsync(w.back, w.dev->p, w.bytes, hipMemcpyDeviceToHost, s));
    RFD_HIP(hipStreamSynchronize(s));
    return RFD_OK;
}
