// frame_host.hip -- the rfd_*_frames* entries of include/rfd.h ("frames in camera and decoder formats").  What a context keeps for
// them is frame_host.h, their layouts, checks and work decomposition are frame_plan.h, their kernel is kernels_frame.hip.
#include "frame_host.h"

#include <memory>

using namespace rfd;

int rfd_frame_layout_of(int format, int width, int height, rfd_frame_layout *out)
{
    RFD_CHECK_ARG(out != nullptr, "out is null");
    if (format < 0 || format >= kFrameFormats) { set_error("invalid argument: unknown pixel format %d", format); return RFD_ERR_INVALID_ARG; }
    if (!frame_layout(format, width, height, out)) {
        set_error("invalid argument: a %s frame of %d x %d: a side outside 1 .. 2^28", frame_format_name(format), width, height);
        return RFD_ERR_INVALID_ARG;
    }
    return RFD_OK;
}

namespace {

enum class Where { Device, Upload, Host }; // planes and outputs on the device; planes on the host; both on the host

// All three forms.  Everything that can refuse the call is settled by frame_plan before the first copy or kernel is enqueued.
int convert_frames(rfd_ctx *c, const rfd_frame *src, int n, const rfd_image *out, Where where, int async)
{
    RFD_CHECK_ARG(c != nullptr, "ctx is null");
    RFD_CHECK_ARG(n >= 0, "n < 0");
    if (n == 0) return RFD_OK;
    RFD_CHECK_ARG(src != nullptr && out != nullptr, "src or out is null");
    rfd_config cfg;
    RFD_TRY(rfd_get_config(c, &cfg));
    if (n > cfg.max_batch_size) {
        set_error("batch of %d frames exceeds max_batch_size %d", n, cfg.max_batch_size);
        return RFD_ERR_CAPACITY;
    }
    FrameDesc local[64];
    std::unique_ptr<FrameDesc[]> big;
    FrameDesc *desc = local;
    if (n > 64) { big.reset(new FrameDesc[(size_t)n]); desc = big.get(); }
    FramePlan plan;
    char msg[256];
    const int checked = frame_plan(src, n, out, cfg.max_src_w, cfg.max_src_h, desc, &plan, msg, sizeof msg);
    if (checked != RFD_OK) {
        set_error(checked == RFD_ERR_INVALID_ARG ? "invalid argument: %s" : "%s", msg);
        return checked;
    }
    RFD_HIP(hipSetDevice(ctx_device(c)));
    FrameConvert &fc = ctx_frame_convert(c);
    const hipStream_t s = ctx_stream(c);
    RFD_TRY(fc.ring.ensure((size_t)cfg.max_batch_size * sizeof(FrameDesc))); // first call on this context
    RFD_TRY(fc.desc.reserve((size_t)cfg.max_batch_size * sizeof(FrameDesc)));
    if (where != Where::Device) RFD_TRY(fc.staging.reserve(plan.src_bytes));
    if (where == Where::Host) RFD_TRY(fc.packed.reserve(plan.out_bytes));
    // host planes: each one to the staging with one 2-D copy of tight rows, and the descriptor follows it there
    if (where != Where::Device) {
        size_t at = 0;
        for (int i = 0; i < n; ++i) {
            rfd_frame_layout l;
            frame_layout(desc[i].format, desc[i].width, desc[i].height, &l);
            for (int k = 0; k < l.planes; ++k) {
                at = frame_round16(at);
                uint8_t *dst = (uint8_t *)fc.staging.p + at;
                RFD_HIP(hipMemcpy2DAsync(dst, (size_t)l.row_bytes[k], desc[i].plane[k], (size_t)desc[i].stride[k], (size_t)l.row_bytes[k], (size_t)l.rows[k],
                                         hipMemcpyHostToDevice, s));
                desc[i].plane[k] = dst;
                desc[i].stride[k] = l.row_bytes[k];
                at += (size_t)l.row_bytes[k] * (size_t)l.rows[k];
            }
        }
    }
    if (where == Where::Host) { // the kernel writes the packed twin of the caller's frames
        size_t at = 0;
        for (int i = 0; i < n; ++i) {
            desc[i].out = (uint8_t *)fc.packed.p + at;
            desc[i].out_stride = (long long)desc[i].width * 3;
            at += (size_t)desc[i].width * 3 * (size_t)desc[i].height;
        }
    }
    FrameDesc *slot;
    RFD_TRY(fc.ring.acquire(&slot));
    memcpy(slot, desc, (size_t)n * sizeof(FrameDesc));
    RFD_HIP(hipMemcpyAsync(fc.desc.p, slot, (size_t)n * sizeof(FrameDesc), hipMemcpyHostToDevice, s));
    RFD_TRY(fc.ring.record(s));
    FrameParams p;
    memset(&p, 0, sizeof p);
    p.frames = (const FrameDesc *)fc.desc.p;
    p.n = n;
    p.groups = plan.groups;
    RFD_TRY(launch_frame_convert(p, s));
    if (where == Where::Host) {
        size_t at = 0;
        for (int i = 0; i < n; ++i) {
            const size_t row = (size_t)desc[i].width * 3;
            RFD_HIP(hipMemcpy2DAsync(const_cast<uint8_t *>(out[i].data), (size_t)out[i].stride, (const uint8_t *)fc.packed.p + at, row, row, (size_t)desc[i].height,
                                     hipMemcpyDeviceToHost, s));
            at += row * (size_t)desc[i].height;
        }
    }
    if (async && where != Where::Host) return RFD_OK;
    RFD_HIP(hipStreamSynchronize(s));
    return RFD_OK;
}

} // namespace

int rfd_convert_frames_device(rfd_ctx *c, const rfd_frame *src, int n, const rfd_image *out, int async)
{
    return convert_frames(c, src, n, out, Where::Device, async);
}

int rfd_upload_frames_device(rfd_ctx *c, const rfd_frame *src, int n, const rfd_image *out, int async)
{
    return convert_frames(c, src, n, out, Where::Upload, async);
}

int rfd_convert_frames(rfd_ctx *c, const rfd_frame *src, int n, const rfd_image *out)
{
    return convert_frames(c, src, n, out, Where::Host, 0);
}
