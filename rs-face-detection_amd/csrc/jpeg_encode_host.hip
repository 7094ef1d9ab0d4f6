// jpeg_encode_host.hip -- the rfd_*jpeg_encode* entries of include/rfd.h ("JPEG encode").  What a context keeps for them is
// jpeg_encode_host.h, their checks, geometry, tables, header and bound are jpeg_encode_plan.h, their kernels are
// kernels_jpeg_encode.hip.
#include "jpeg_encode_host.h"

#include <memory>
#include <vector>

using namespace rfd;

int rfd_jpeg_encode_config_default(rfd_jpeg_encode_config *cfg)
{
    RFD_CHECK_ARG(cfg != nullptr, "cfg is null");
    jpeg_encode_config_default(cfg);
    return RFD_OK;
}

namespace {

// the config alone, before anything else of a call is looked at: a bad field is named even where there is no context
int check_config(const rfd_jpeg_encode_config *cfg)
{
    RFD_CHECK_ARG(cfg != nullptr, "cfg is null");
    char msg[200];
    if (!jpeg_encode_check_config(*cfg, msg, sizeof msg)) {
        set_error("invalid argument: %s", msg);
        return RFD_ERR_INVALID_ARG;
    }
    return RFD_OK;
}

// the checks of the two host-only calls: the config, then the geometry of one image
int check_one(int width, int height, const rfd_jpeg_encode_config *cfg, EncImage *d)
{
    RFD_TRY(check_config(cfg));
    char msg[200];
    if (!jpeg_encode_geometry(width, height, *cfg, d, msg, sizeof msg)) {
        set_error("invalid argument: %s", msg);
        return RFD_ERR_INVALID_ARG;
    }
    return RFD_OK;
}

} // namespace

int rfd_jpeg_encode_bound(int width, int height, const rfd_jpeg_encode_config *cfg, size_t *bytes)
{
    RFD_CHECK_ARG(bytes != nullptr, "bytes is null");
    EncImage d;
    memset(&d, 0, sizeof d);
    RFD_TRY(check_one(width, height, cfg, &d));
    uint8_t header[kEncHeaderMax];
    *bytes = jpeg_encode_bound_of(d, jpeg_encode_header(width, height, cfg->quality, cfg->sampling, d.dri, header, nullptr, nullptr));
    return RFD_OK;
}

int rfd_jpeg_encode_header(int width, int height, const rfd_jpeg_encode_config *cfg, uint8_t *out, size_t cap, size_t *len)
{
    RFD_CHECK_ARG(len != nullptr, "len is null");
    EncImage d;
    memset(&d, 0, sizeof d);
    RFD_TRY(check_one(width, height, cfg, &d));
    uint8_t header[kEncHeaderMax];
    const int n = jpeg_encode_header(width, height, cfg->quality, cfg->sampling, d.dri, header, nullptr, nullptr);
    *len = (size_t)n;
    if (cap < (size_t)n || !out) {
        set_error("the header is %d bytes, the buffer %zu", n, out ? cap : (size_t)0);
        return RFD_ERR_CAPACITY;
    }
    memcpy(out, header, (size_t)n);
    return RFD_OK;
}

int JpegEncoder::stage_frames(hipStream_t s, const rfd_image *imgs, EncImage *desc_host, int n, const EncPlan &plan)
{
    RFD_TRY(staging.reserve(plan.src_bytes));
    size_t at = 0;
    for (int i = 0; i < n; ++i) {
        at = jpeg_encode_round16(at);
        const size_t row = (size_t)imgs[i].width * 3;
        uint8_t *dst = (uint8_t *)staging.p + at;
        RFD_HIP(hipMemcpy2DAsync(dst, row, imgs[i].data, (size_t)imgs[i].stride, row, (size_t)imgs[i].height, hipMemcpyHostToDevice, s));
        desc_host[i].src = dst;
        desc_host[i].stride = (long long)row;
        at += row * (size_t)imgs[i].height;
    }
    return RFD_OK;
}

int JpegEncoder::enqueue(hipStream_t s, int max_batch, const rfd_jpeg_encode_config &cfg, const EncTables &tables, const EncImage *desc_host, int n, const EncPlan &plan,
                         const int32_t *count_dev, size_t slot_bytes, int32_t *size_dev, int stages)
{
    const size_t blob = sizeof(EncTables) + (size_t)max_batch * sizeof(EncImage);
    RFD_TRY(ring.ensure(blob)); // first call on this context
    RFD_TRY(desc.reserve(blob));
    RFD_TRY(coef.reserve(plan.coef_bytes));
    RFD_TRY(intervals.reserve(plan.interval_bytes));
    char *slot;
    RFD_TRY(ring.acquire(&slot));
    memcpy(slot, &tables, sizeof tables);
    memcpy(slot + sizeof tables, desc_host, (size_t)n * sizeof(EncImage));
    RFD_HIP(hipMemcpyAsync(desc.p, slot, sizeof tables + (size_t)n * sizeof(EncImage), hipMemcpyHostToDevice, s));
    RFD_TRY(ring.record(s));
    const EncSampling sm = jpeg_encode_sampling(cfg.sampling);
    EncParams p;
    memset(&p, 0, sizeof p);
    p.tables = (const EncTables *)desc.p;
    p.imgs = (const EncImage *)((const char *)desc.p + sizeof(EncTables));
    p.n = n;
    p.ncomp = sm.ncomp; p.h = sm.h; p.v = sm.v;
    p.count = count_dev;
    p.coef = (int16_t *)coef.p;
    p.interval_len = (uint32_t *)intervals.p;
    p.interval_off = p.interval_len + plan.intervals;
    p.slot_bytes = (unsigned long long)slot_bytes;
    p.size = size_dev;
    if (stages & 1) RFD_TRY(launch_jpeg_encode_blocks(p, plan.groups, s));
    if (stages & 2) {
        RFD_TRY(launch_jpeg_encode_entropy(p, (int)plan.intervals, false, s));
        RFD_TRY(launch_jpeg_encode_assemble(p, s));
        RFD_TRY(launch_jpeg_encode_entropy(p, (int)plan.intervals, true, s));
    }
    return RFD_OK;
}

namespace {

// What every entry settles before the first copy or kernel, behind check_config: the batch limit and every image's geometry.  desc: n descriptors.
int plan_call(rfd_ctx *c, const rfd_image *imgs, int n, const rfd_jpeg_encode_config *cfg, uint8_t *slots, size_t slot_bytes, EncTables *tables,
              std::unique_ptr<EncImage[]> *desc, EncPlan *plan)
{
    RFD_TRY(ctx_check_batch(c, n, "batch of", " images"));
    char msg[256];
    jpeg_encode_tables(*cfg, tables);
    desc->reset(new EncImage[(size_t)n]);
    const int planned = jpeg_encode_plan(imgs, n, *cfg, slots, slot_bytes, tables->header_len, desc->get(), plan, msg, sizeof msg);
    if (planned != RFD_OK) {
        set_error(planned == RFD_ERR_INVALID_ARG ? "invalid argument: %s" : "%s", msg);
        return planned;
    }
    return RFD_OK;
}

} // namespace

int rfd_encode_jpeg_batch_device(rfd_ctx *c, const rfd_image *imgs, int n, const int32_t *count_dev, const rfd_jpeg_encode_config *cfg, uint8_t *out, size_t slot_bytes,
                                 int32_t *size_dev, int async)
{
    RFD_TRY(check_config(cfg));
    RFD_CHECK_ARG(c != nullptr, "ctx is null");
    RFD_CHECK_ARG(n >= 0, "n < 0");
    if (n == 0) return RFD_OK;
    RFD_CHECK_ARG(imgs != nullptr && out != nullptr && size_dev != nullptr, "imgs, out or size_dev is null");
    EncTables tables;
    std::unique_ptr<EncImage[]> desc;
    EncPlan plan;
    RFD_TRY(plan_call(c, imgs, n, cfg, out, slot_bytes, &tables, &desc, &plan));
    RFD_HIP(hipSetDevice(ctx_device(c)));
    const hipStream_t s = ctx_stream(c);
    RFD_TRY(ctx_jpeg_encoder(c).enqueue(s, ctx_max_batch_size(c), *cfg, tables, desc.get(), n, plan, count_dev, slot_bytes, size_dev, 3));
    if (async) return RFD_OK;
    RFD_HIP(hipStreamSynchronize(s));
    return RFD_OK;
}

int rfd_encode_jpeg_batch(rfd_ctx *c, const rfd_image *imgs, int n, const rfd_jpeg_encode_config *cfg, uint8_t *out, size_t slot_bytes, int32_t *size)
{
    RFD_TRY(check_config(cfg));
    RFD_CHECK_ARG(c != nullptr, "ctx is null");
    RFD_CHECK_ARG(n >= 0, "n < 0");
    if (n == 0) return RFD_OK;
    RFD_CHECK_ARG(imgs != nullptr && out != nullptr && size != nullptr, "imgs, out or size is null");
    EncTables tables;
    std::unique_ptr<EncImage[]> desc;
    EncPlan plan;
    RFD_TRY(plan_call(c, imgs, n, cfg, nullptr, 0, &tables, &desc, &plan));
    RFD_HIP(hipSetDevice(ctx_device(c)));
    const hipStream_t s = ctx_stream(c);
    JpegEncoder &e = ctx_jpeg_encoder(c);
    // a device slot never needs more than the largest bound of the call; below it, the caller's capacity decides what fits
    const size_t dev_slot = slot_bytes < plan.max_bound ? slot_bytes : plan.max_bound;
    RFD_TRY(e.slots.reserve((size_t)n * dev_slot + 1));
    RFD_TRY(e.sizes.reserve((size_t)ctx_max_batch_size(c) * sizeof(int32_t)));
    RFD_TRY(e.stage_frames(s, imgs, desc.get(), n, plan));
    for (int i = 0; i < n; ++i) desc[i].out = (uint8_t *)e.slots.p + (size_t)i * dev_slot;
    RFD_TRY(e.enqueue(s, ctx_max_batch_size(c), *cfg, tables, desc.get(), n, plan, nullptr, dev_slot, (int32_t *)e.sizes.p, 3));
    RFD_HIP(hipMemcpyAsync(size, e.sizes.p, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    RFD_HIP(hipStreamSynchronize(s));
    for (int i = 0; i < n; ++i)
        if (size[i] > 0) RFD_HIP(hipMemcpyAsync(out + (size_t)i * slot_bytes, (const uint8_t *)e.slots.p + (size_t)i * dev_slot, (size_t)size[i], hipMemcpyDeviceToHost, s));
    RFD_HIP(hipStreamSynchronize(s));
    return RFD_OK;
}

int rfd_debug_jpeg_encode_blocks(rfd_ctx *c, const rfd_image *img, const rfd_jpeg_encode_config *cfg, int16_t *out, size_t cap_blocks, size_t *blocks)
{
    RFD_TRY(check_config(cfg));
    RFD_CHECK_ARG(c != nullptr, "ctx is null");
    RFD_CHECK_ARG(img != nullptr && blocks != nullptr, "img, cfg or blocks is null");
    EncTables tables;
    std::unique_ptr<EncImage[]> desc;
    EncPlan plan;
    RFD_TRY(plan_call(c, img, 1, cfg, nullptr, 0, &tables, &desc, &plan));
    *blocks = (size_t)plan.blocks;
    if (cap_blocks < (size_t)plan.blocks || !out) {
        set_error("the image has %lld blocks, the buffer %zu", (long long)plan.blocks, out ? cap_blocks : (size_t)0);
        return RFD_ERR_CAPACITY;
    }
    RFD_HIP(hipSetDevice(ctx_device(c)));
    const hipStream_t s = ctx_stream(c);
    JpegEncoder &e = ctx_jpeg_encoder(c);
    RFD_TRY(e.stage_frames(s, img, desc.get(), 1, plan));
    RFD_TRY(e.enqueue(s, ctx_max_batch_size(c), *cfg, tables, desc.get(), 1, plan, nullptr, 0, nullptr, 1));
    std::vector<int16_t> zz((size_t)plan.blocks * 64);
    RFD_HIP(hipMemcpyAsync(zz.data(), e.coef.p, plan.coef_bytes, hipMemcpyDeviceToHost, s));
    RFD_HIP(hipStreamSynchronize(s));
    for (size_t b = 0; b < (size_t)plan.blocks; ++b)
        for (int k = 0; k < 64; ++k) out[b * 64 + kEncNatural[k]] = zz[b * 64 + k];
    return RFD_OK;
}

int rfd_debug_jpeg_encode_coefficients(rfd_ctx *c, const int16_t *coef, size_t blocks, int width, int height, const rfd_jpeg_encode_config *cfg, uint8_t *out, size_t cap,
                                       int32_t *len)
{
    RFD_TRY(check_config(cfg));
    RFD_CHECK_ARG(c != nullptr, "ctx is null");
    RFD_CHECK_ARG(coef != nullptr && out != nullptr && len != nullptr, "coef, cfg, out or len is null");
    rfd_image img;
    memset(&img, 0, sizeof img);
    img.data = reinterpret_cast<const uint8_t *>(coef); // no pixel is read: the block kernel does not run
    img.width = width; img.height = height; img.stride = (ptrdiff_t)width * 3;
    EncTables tables;
    std::unique_ptr<EncImage[]> desc;
    EncPlan plan;
    RFD_TRY(plan_call(c, &img, 1, cfg, nullptr, 0, &tables, &desc, &plan));
    if (blocks != (size_t)plan.blocks) {
        set_error("invalid argument: blocks is %zu, a %d x %d file of this sampling has %lld", blocks, width, height, (long long)plan.blocks);
        return RFD_ERR_INVALID_ARG;
    }
    std::vector<int16_t> zz(blocks * 64);
    for (size_t b = 0; b < blocks; ++b)
        for (int k = 0; k < 64; ++k) {
            const int v = coef[b * 64 + kEncNatural[k]];
            if (v < (k == 0 ? -1024 : -1023) || v > 1023) {
                set_error("invalid argument: coef %d at block %zu, zigzag position %d, is outside what the tables code", v, b, k);
                return RFD_ERR_INVALID_ARG;
            }
            zz[b * 64 + k] = (int16_t)v;
        }
    RFD_HIP(hipSetDevice(ctx_device(c)));
    const hipStream_t s = ctx_stream(c);
    JpegEncoder &e = ctx_jpeg_encoder(c);
    const size_t dev_slot = cap < plan.max_bound ? cap : plan.max_bound;
    RFD_TRY(e.slots.reserve(dev_slot + 1));
    RFD_TRY(e.sizes.reserve((size_t)ctx_max_batch_size(c) * sizeof(int32_t)));
    RFD_TRY(e.coef.reserve(plan.coef_bytes));
    desc[0].src = nullptr;
    desc[0].out = (uint8_t *)e.slots.p;
    RFD_HIP(hipMemcpyAsync(e.coef.p, zz.data(), plan.coef_bytes, hipMemcpyHostToDevice, s));
    RFD_TRY(e.enqueue(s, ctx_max_batch_size(c), *cfg, tables, desc.get(), 1, plan, nullptr, dev_slot, (int32_t *)e.sizes.p, 2));
    RFD_HIP(hipMemcpyAsync(len, e.sizes.p, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    RFD_HIP(hipStreamSynchronize(s));
    if (*len > 0) RFD_HIP(hipMemcpy(out, e.slots.p, (size_t)*len, hipMemcpyDeviceToHost));
    return RFD_OK;
}
