// redact_host.hip -- the rfd_redact_faces* entries of include/rfd.h ("redaction").  What a context keeps for them is
// redact_host.h, their checks and geometry are redact_plan.h, their kernel is kernels_redact.hip.
#include "redact_host.h"

#include <memory>

using namespace rfd;

int rfd_redact_config_default(rfd_redact_config *cfg)
{
    RFD_CHECK_ARG(cfg != nullptr, "cfg is null");
    memset(cfg, 0, sizeof *cfg);
    // chosen values, not tuned on data (rfd.h)
    cfg->mode = RFD_REDACT_PIXELATE;
    cfg->shape = RFD_REDACT_ELLIPSE;
    cfg->cell = 16;
    cfg->margin_x = 0.1f;
    cfg->margin_top = 0.2f; // hair, forehead
    cfg->margin_bottom = 0.1f;
    return RFD_OK;
}

// The checks both forms share, in an order that needs the context last: nothing is enqueued before they pass.  *cfg is
// replaced by the default when NULL.  n = 0 passes with whatever pointers.
static int redact_check(rfd_ctx *c, const rfd_image *imgs, const rfd_image *dst, int n, const rfd_dets *dets, const rfd_redact_config **cfg,
                        rfd_redact_config *def, int *max_batch, int *max_det)
{
    char msg[160];
    if (!*cfg) { RFD_TRY(rfd_redact_config_default(def)); *cfg = def; }
    if (!rd_config_ok(**cfg, msg, sizeof msg)) { set_error("invalid argument: redact config: %s", msg); return RFD_ERR_INVALID_ARG; }
    RFD_CHECK_ARG(n >= 0, "n < 0");
    if (n > 0) {
        RFD_CHECK_ARG(imgs != nullptr, "imgs is null");
        RFD_CHECK_ARG(dets && dets->boxes && dets->count, "dets: boxes or count is null");
    }
    RFD_CHECK_ARG(c != nullptr, "ctx is null");
    rfd_config cc;
    RFD_TRY(rfd_get_config(c, &cc));
    if (n > cc.max_batch_size) {
        set_error("redaction of %d frames exceeds max_batch_size %d", n, cc.max_batch_size);
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
// frames' sizes for the grid.
static int redact_enqueue(rfd_ctx *c, const RdImage *desc, const rfd_image *sizes, int n, bool in_place, int max_batch, int max_det,
                          const rfd_dets &dets, const uint32_t *sel, const rfd_redact_config &cfg, int32_t *applied)
{
    Redact &rd = ctx_redact(c);
    const hipStream_t s = ctx_stream(c);
    RFD_TRY(rd.ring.ensure((size_t)max_batch * sizeof(RdImage))); // first call on this context
    RFD_TRY(rd.imgs.reserve((size_t)max_batch * sizeof(RdImage)));
    RdImage *slot;
    RFD_TRY(rd.ring.acquire(&slot));
    memcpy(slot, desc, (size_t)n * sizeof(RdImage));
    RFD_HIP(hipMemcpyAsync(rd.imgs.p, slot, (size_t)n * sizeof(RdImage), hipMemcpyHostToDevice, s));
    RFD_TRY(rd.ring.record(s));
    RdParams p;
    memset(&p, 0, sizeof p);
    p.imgs = (const RdImage *)rd.imgs.p;
    p.n = n; p.max_det = max_det;
    p.boxes = dets.boxes; p.count = dets.count; p.sel = sel;
    p.in_place = in_place ? 1 : 0;
    p.mode = cfg.mode; p.shape = cfg.shape; p.cell = cfg.cell; p.tile = rd_tile_side(cfg.cell);
    p.sel_mask = cfg.sel_mask; p.sel_value = cfg.sel_value;
    p.fill = (uint32_t)cfg.fill[0] | ((uint32_t)cfg.fill[1] << 8) | ((uint32_t)cfg.fill[2] << 16);
    p.margin_x = cfg.margin_x; p.margin_top = cfg.margin_top; p.margin_bottom = cfg.margin_bottom;
    p.applied = applied;
    return launch_redact(p, rd_grid(sizes, n, cfg.cell), s);
}

int rfd_redact_faces_device(rfd_ctx *c, const rfd_image *imgs, const rfd_image *dst, int n, const rfd_dets *dets, const uint32_t *sel,
                            const rfd_redact_config *cfg, int32_t *applied, int async)
{
    rfd_redact_config def;
    int max_batch = 0, max_det = 0;
    RFD_TRY(redact_check(c, imgs, dst, n, dets, &cfg, &def, &max_batch, &max_det));
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
    RFD_TRY(redact_enqueue(c, d, imgs, n, dst == nullptr, max_batch, max_det, *dets, sel, *cfg, applied));
    if (async) return RFD_OK;
    RFD_HIP(hipStreamSynchronize(ctx_stream(c)));
    return RFD_OK;
}

int rfd_redact_faces(rfd_ctx *c, const rfd_image *imgs, const rfd_image *dst, int n, const rfd_dets *dets, const uint32_t *sel,
                     const rfd_redact_config *cfg, int32_t *applied)
{
    rfd_redact_config def;
    int max_batch = 0, max_det = 0;
    RFD_TRY(redact_check(c, imgs, dst, n, dets, &cfg, &def, &max_batch, &max_det));
    if (n == 0) return RFD_OK;
    RFD_HIP(hipSetDevice(ctx_device(c)));
    Redact &rd = ctx_redact(c);
    const hipStream_t s = ctx_stream(c);
    const size_t N = (size_t)n, MD = (size_t)max_det;
    // the frames, packed back to back with tight rows, one 2-D copy each; the kernel paints them in place there -- the result
    // is a function of the source and the covered pixels alone -- and their rows go back to dst, or to the frames themselves
    size_t total = 0;
    for (int i = 0; i < n; ++i) total += (size_t)imgs[i].height * imgs[i].width * 3;
    RFD_TRY(rd.h_frames.reserve(total));
    struct Twin { DevBuf *dev; const void *in; void *back; size_t bytes; };
    const Twin twins[] = {
        {&rd.h_boxes, dets->boxes, nullptr, N * MD * 5 * sizeof(float)},
        {&rd.h_count, dets->count, nullptr, N * sizeof(int32_t)},
        {&rd.h_sel, sel, nullptr, N * MD * sizeof(uint32_t)},
        {&rd.h_applied, applied, applied, N * sizeof(int32_t)},
    };
    for (const Twin &w : twins)
        if (w.in) RFD_TRY(w.dev->reserve(w.bytes));
    std::unique_ptr<RdImage[]> desc(new RdImage[N]);
    size_t off = 0;
    for (int i = 0; i < n; ++i) {
        uint8_t *at = (uint8_t *)rd.h_frames.p + off;
        const size_t rowb = (size_t)imgs[i].width * 3;
        RFD_HIP(hipMemcpy2DAsync(at, rowb, imgs[i].data, (size_t)imgs[i].stride, rowb, (size_t)imgs[i].height, hipMemcpyHostToDevice, s));
        desc[i] = RdImage{at, (long long)rowb, at, (long long)rowb, imgs[i].height, imgs[i].width};
        off += rowb * (size_t)imgs[i].height;
    }
    for (int i = 0; i < 3; ++i)
        if (twins[i].in) RFD_HIP(hipMemcpyAsync(twins[i].dev->p, twins[i].in, twins[i].bytes, hipMemcpyHostToDevice, s));
    auto dev = [&](int i) -> void * { return twins[i].in ? twins[i].dev->p : nullptr; };
    const rfd_dets d = {(float *)dev(0), nullptr, (int32_t *)dev(1), nullptr};
    RFD_TRY(redact_enqueue(c, desc.get(), imgs, n, true, max_batch, max_det, d, (const uint32_t *)dev(2), *cfg, (int32_t *)dev(3)));
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
