// jpeg_host.hip -- the host side of a JPEG decode call (jpeg_host.h): csrc/jpeg_parse.h on host threads, the tables of
// csrc/jpeg_plan.h, then csrc/kernels_jpeg.hip; in DEVICE entropy mode csrc/kernels_jpeg_entropy.hip in front of them.
#include "jpeg_host.h"

#include <atomic>
#include <functional>
#include <memory>
#include <thread>

#include "kernels.h"

namespace rfd {

// One decode call: the caller's files and what the call knows of each.
struct JpegCall {
    const uint8_t *const *bytes;
    const size_t *len;
    int n;
    std::unique_ptr<JpegCallFrame[]> f;
    int n_oriented = 0;
    JpegEntropyFill fill;
    bool launched = false; // the entropy kernel ran for this call: the records of its frames are on the device already
    JpegCall(const uint8_t *const *bytes_, const size_t *len_, int n_) : bytes(bytes_), len(len_), n(n_), f(new JpegCallFrame[(size_t)n_]) {}
};

// fn(i) for every i of items on min(threads, items) threads that never touch HIP; false: no thread could be started
static bool jpeg_on_threads(int threads, const std::vector<int> &items, const std::function<void(int)> &fn)
{
    if (items.empty()) return true;
    std::atomic<size_t> next{0};
    auto work = [&]() {
        for (size_t k; (k = next.fetch_add(1)) < items.size();) fn(items[k]);
    };
    std::vector<std::thread> pool;
    const int T = std::min(threads, (int)items.size());
    try {
        for (int t = 0; t < T; ++t) pool.emplace_back(work);
    } catch (...) {
    }
    for (std::thread &t : pool) t.join();
    return !pool.empty();
}

// first decode call of a context: the page-locked staging, its device twin, the plane pool; in DEVICE mode the page-locked scan /
// interval staging and its device twin
int JpegDecoder::ensure_staging(const rfd_config &cfg, bool device_entropy)
{
    if (!pin) {
        RFD_CHECK_ARG(cfg.max_src_w >= 1 && cfg.max_src_h >= 1, "max_src_w / max_src_h < 1");
        const JpegStageLayout l(cfg.max_batch_size, cfg.max_src_w, cfg.max_src_h);
        if (l.blocks_max * 64 > kJpegMaxCoefs) {
            set_error("max_src %d x %d exceeds the JPEG decoder's %u coefficient slots per frame", cfg.max_src_w, cfg.max_src_h, kJpegMaxCoefs);
            return RFD_ERR_CAPACITY;
        }
        stage = l;
        RFD_TRY(pin_done.create());
        RFD_TRY(dev.reserve(l.total));
        RFD_TRY(planes.reserve(l.plane_bytes()));
        RFD_TRY(pin.alloc(l.total));
    }
    if (device_entropy && !ent_pin) {
        ent = JpegEntLayout(cfg.max_batch_size, cfg.max_src_w, cfg.max_src_h, stage.blocks_max);
        RFD_TRY(ent_done.create());
        RFD_TRY(ent_dev.reserve(ent.total));
        RFD_TRY(ent_pin.alloc(ent.total));
    }
    return RFD_OK;
}

// ---- entropy decoding on the device (rfd_set_jpeg_entropy): csrc/jpeg_entropy.h, csrc/kernels_jpeg_entropy.hip ----
// Places the frames that may take the interval path, stages them on threads, and runs the kernel over those that stayed.
int JpegDecoder::entropy_stage(hipStream_t s, JpegCall &k)
{
    std::vector<int> placed;
    for (int i = 0; i < k.n; ++i)
        if ((uint64_t)k.f[i].hdr.nblocks * 64 <= kJpegMaxCoefs && jpeg_entropy_place(ent, k.fill, k.f[i], k.len[i])) placed.push_back(i);
    if (!jpeg_on_threads(decode_threads, placed, [&](int i) { jpeg_entropy_stage_frame(ent, ent_pin.p, k.f[i], k.bytes[i], k.len[i]); })) {
        set_error("cannot start a JPEG decode thread");
        return RFD_ERR_STATE;
    }
    for (int i : placed) k.launched |= k.f[i].staged;
    if (k.launched) RFD_TRY(entropy_enqueue(s, k));
    return RFD_OK;
}

// Descriptors, the copies out of the staging, the kernel, the status words back (ent_done behind them).
int JpegDecoder::entropy_enqueue(hipStream_t s, const JpegCall &k)
{
    JpegEntropyParams p = jpeg_plan_entropy(k.f.get(), k.n, ent, ent_pin.p);
    void *d = ent_dev.p;
    auto copies = [&]() -> int {
        RFD_HIP(hipMemcpyAsync(d, ent_pin.p, (size_t)p.n * sizeof(JpegEntropyFrame), hipMemcpyHostToDevice, s));
        RFD_HIP(hipMemcpyAsync(ent.intervals(d), ent.intervals(ent_pin.p), k.fill.ivl_used * sizeof(uint32_t), hipMemcpyHostToDevice, s));
        if (k.fill.scan_used) RFD_HIP(hipMemcpyAsync(ent.scan(d), ent.scan(ent_pin.p), k.fill.scan_used, hipMemcpyHostToDevice, s));
        RFD_HIP(hipMemsetAsync(ent.status(d), 0, (size_t)k.n * sizeof(uint32_t), s));
        return RFD_OK;
    };
    const int copied = copies();
    const hipError_t recorded = hipEventRecord(pin_done, s); // the next call waits for these before it writes the staging
    RFD_TRY(copied);
    RFD_HIP(recorded);
    p.frames = ent.frames(d);
    p.scan = ent.scan(d);
    p.intervals = ent.intervals(d);
    p.rec = stage.rec(dev.p);
    p.coef = stage.coef(dev.p);
    p.status = ent.status(d);
    RFD_TRY(launch_jpeg_entropy(p, s));
    RFD_HIP(hipMemcpyAsync(ent.status(ent_pin.p), ent.status(d), (size_t)k.n * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    RFD_HIP(hipEventRecord(ent_done, s));
    return RFD_OK;
}

// Waits for the status words; the frames the device refused leave the staged set and are listed.
int JpegDecoder::entropy_collect(JpegCall &k, std::vector<int> &refused)
{
    RFD_HIP(hipEventSynchronize(ent_done));
    const uint32_t *status = ent.status(ent_pin.p);
    for (int i = 0; i < k.n; ++i)
        if (k.f[i].staged && status[i]) { k.f[i].staged = false; refused.push_back(i); }
    return RFD_OK;
}

// one frame per task; the workers touch nothing but their frame's bytes, header and slices of the staging
bool JpegDecoder::decode_on_host(JpegCall &k, const std::vector<int> &which)
{
    uint32_t *rec = stage.rec(pin.p);
    int16_t *coef = stage.coef(pin.p);
    return jpeg_on_threads(decode_threads, which, [&](int i) {
        JpegCallFrame &f = k.f[i];
        f.status = jpeg_decode_scan(k.bytes[i], k.len[i], f.hdr, rec + f.rec0, coef + f.rec0 * 64, &f.used, scale != 1 ? f.idct_n : nullptr);
    });
}

// The descriptors, the records and coefficients the host decoded, the lists of the colour launches; pin_done behind them.
int JpegDecoder::upload(hipStream_t s, const JpegCall &k, const JpegTables &t)
{
    char *d = (char *)dev.p;
    auto copies = [&]() -> int {
        if (!k.launched) RFD_HIP(hipMemcpyAsync(d, pin.p, stage.frames_rec_bytes(t.blocks), hipMemcpyHostToDevice, s));
        else { // the records the entropy kernel wrote stay: the descriptors, then the records of the host-decoded frames one by one
            RFD_HIP(hipMemcpyAsync(d, pin.p, stage.frames_bytes(k.n), hipMemcpyHostToDevice, s));
            for (int i = 0; i < k.n; ++i)
                if (!k.f[i].staged)
                    RFD_HIP(hipMemcpyAsync(stage.rec(d) + k.f[i].rec0, stage.rec(pin.p) + k.f[i].rec0, (size_t)k.f[i].hdr.nblocks * sizeof(uint32_t), hipMemcpyHostToDevice, s));
        }
        for (int i = 0; i < k.n; ++i)
            if (k.f[i].used)
                RFD_HIP(hipMemcpyAsync(stage.coef(d) + k.f[i].rec0 * 64, stage.coef(pin.p) + k.f[i].rec0 * 64, (size_t)k.f[i].used * sizeof(int16_t), hipMemcpyHostToDevice, s));
        if (t.lists_bytes) RFD_HIP(hipMemcpyAsync(d + t.lists_off, pin.p + t.lists_off, t.lists_bytes, hipMemcpyHostToDevice, s));
        return RFD_OK;
    };
    const int copied = copies();
    // also where a copy failed after others were enqueued: the next call must wait for those before it writes the staging
    const hipError_t recorded = hipEventRecord(pin_done, s);
    RFD_TRY(copied);
    RFD_HIP(recorded);
    return RFD_OK;
}

// One of three paths: a scaled batch; an unscaled batch without an oriented frame; an unscaled batch with one.
int JpegDecoder::launch(hipStream_t s, const JpegCall &k, const JpegTables &t)
{
    void *d = dev.p;
    JpegParams p, upright;
    memset(&p, 0, sizeof p);
    p.frames = stage.frames(d);
    p.n = k.n;
    p.groups = t.groups; p.tiles = t.tiles;
    p.rec = stage.rec(d);
    p.coef = stage.coef(d);
    p.planes = (uint8_t *)planes.p;
    if (scale != 1) {
        JpegScaledParams sp;
        memset(&sp, 0, sizeof sp);
        sp.frames = p.frames;
        sp.scaled = stage.scaled(d);
        sp.upright = stage.scaled_upright(d);
        sp.oriented = stage.scaled_oriented(d);
        sp.n = k.n; sp.groups = t.cgroups;
        sp.n_upright = t.upright.n; sp.tiles_upright = t.upright.tiles;
        sp.n_oriented = t.oriented.n; sp.tiles_oriented = t.oriented.tiles;
        sp.rec = p.rec; sp.coef = p.coef; sp.planes = p.planes;
        return launch_jpeg_decode_scaled(sp, s);
    }
    if (!k.n_oriented) return launch_jpeg_decode(p, s);
    JpegOrientedParams oriented;
    memset(&upright, 0, sizeof upright);
    memset(&oriented, 0, sizeof oriented);
    upright.frames = stage.upright(d);
    upright.n = t.upright.n; upright.tiles = t.upright.tiles;
    upright.rec = p.rec; upright.coef = p.coef; upright.planes = p.planes;
    oriented.frames = p.frames;
    oriented.oriented = stage.oriented(d);
    oriented.n = t.oriented.n; oriented.tiles = t.oriented.tiles;
    oriented.planes = p.planes;
    return launch_jpeg_decode_oriented(p, upright, oriented, s);
}

// Both forms.  Everything that can refuse the call -- arguments, headers, entropy data -- is settled before the first copy or
// kernel that writes an output frame is enqueued.  In DEVICE mode the entropy kernel, which writes the decoder's own pools only,
// runs before that point, and the call waits for its status words.
int JpegDecoder::decode(hipStream_t s, const rfd_config &cfg, const uint8_t *const *bytes, const size_t *len, int n, const rfd_image *out, bool out_on_device, bool async)
{
    JpegCall k(bytes, len, n);
    char msg[512];
    const int checked = jpeg_plan_frames(bytes, len, n, out, scale, orientation == RFD_JPEG_ORIENTATION_APPLY, cfg.max_src_w, cfg.max_src_h, k.f.get(), &k.n_oriented, msg, sizeof msg);
    if (checked != RFD_OK) { set_error("%s", msg); return checked; }
    RFD_HIP(hipSetDevice(cfg.device_id));
    RFD_TRY(ensure_staging(cfg, entropy == RFD_JPEG_ENTROPY_DEVICE));
    RFD_HIP(hipEventSynchronize(pin_done)); // the previous call's copies out of the staging have run
    paths.assign((size_t)n, 0);
    orientations.resize((size_t)n);
    for (int i = 0; i < n; ++i) orientations[(size_t)i] = k.f[i].orientation;
    if (entropy == RFD_JPEG_ENTROPY_DEVICE) RFD_TRY(entropy_stage(s, k));
    std::vector<int> host_frames, refused;
    for (int i = 0; i < n; ++i)
        if (!k.f[i].staged) host_frames.push_back(i);
    bool threads_ok = decode_on_host(k, host_frames); // while the entropy kernel runs
    if (k.launched) {
        for (int i = 0; i < n; ++i) paths[(size_t)i] = k.f[i].staged;
        RFD_TRY(entropy_collect(k, refused));
        for (int i : refused) paths[(size_t)i] = 2;
        threads_ok = decode_on_host(k, refused) && threads_ok; // the host decoder judges what the device refused
    }
    if (!threads_ok) { set_error("cannot start a JPEG decode thread"); return RFD_ERR_STATE; }
    size_t out_bytes = 0;
    for (int i = 0; i < n; ++i) {
        if (k.f[i].status != RFD_OK) { set_error("file %d: %s", i, k.f[i].hdr.msg); return k.f[i].status; }
        out_bytes += (size_t)k.f[i].out_w * 3 * k.f[i].out_h;
    }
    if (!out_on_device) RFD_TRY(packed.reserve(out_bytes));
    const JpegOutput where = {out_on_device ? out : nullptr, (uint8_t *)packed.p};
    const JpegTables t = jpeg_plan_tables(k.f.get(), n, scale, k.n_oriented != 0, where, stage, pin.p);
    RFD_TRY(upload(s, k, t));
    RFD_TRY(launch(s, k, t));
    if (!out_on_device) {
        size_t out_at = 0;
        for (int i = 0; i < n; ++i) {
            const size_t row = (size_t)k.f[i].out_w * 3;
            RFD_HIP(hipMemcpy2DAsync(const_cast<uint8_t *>(out[i].data), (size_t)out[i].stride, (const uint8_t *)packed.p + out_at, row, row, (size_t)k.f[i].out_h,
                                     hipMemcpyDeviceToHost, s));
            out_at += row * k.f[i].out_h;
        }
    }
    if (async && out_on_device) return RFD_OK;
    RFD_HIP(hipStreamSynchronize(s));
    return RFD_OK;
}

int JpegDecoder::debug_coefficients(hipStream_t s, const rfd_config &cfg, const uint8_t *bytes, size_t len, int16_t *out, size_t cap_blocks, size_t *blocks)
{
    JpegCall k(&bytes, &len, 1);
    JpegHeader &h = k.f[0].hdr;
    const int st = jpeg_parse_header(bytes, len, h);
    if (st != RFD_OK) { set_error("%s", h.msg); return st; }
    if (blocks) *blocks = (size_t)h.nblocks;
    if ((uint64_t)h.nblocks * 64 > kJpegMaxCoefs) { set_error("a JPEG frame of %d blocks exceeds the decoder's %u coefficient slots", h.nblocks, kJpegMaxCoefs); return RFD_ERR_CAPACITY; }
    if ((size_t)h.nblocks > cap_blocks) { set_error("the file has %d blocks, the output holds %zu", h.nblocks, cap_blocks); return RFD_ERR_CAPACITY; }
    if (h.width > cfg.max_src_w || h.height > cfg.max_src_h) {
        set_error("%d x %d exceeds max_src %d x %d", h.width, h.height, cfg.max_src_w, cfg.max_src_h);
        return RFD_ERR_CAPACITY;
    }
    RFD_HIP(hipSetDevice(cfg.device_id));
    RFD_TRY(ensure_staging(cfg, true));
    RFD_HIP(hipEventSynchronize(pin_done));
    RFD_TRY(entropy_stage(s, k));
    if (!k.f[0].staged) { set_error("%s", h.msg); return RFD_ERR_UNSUPPORTED; }
    std::vector<int> refused;
    RFD_TRY(entropy_collect(k, refused));
    if (!refused.empty()) {
        set_error("the device entropy decoder refused the file: an interval of the scan at byte %zu does not decode to exactly its bytes", h.scan);
        return RFD_ERR_UNSUPPORTED;
    }
    const size_t nb = (size_t)h.nblocks;
    std::vector<uint32_t> rec(nb);
    std::vector<int16_t> coef(nb * 64);
    RFD_HIP(hipMemcpyAsync(rec.data(), stage.rec(dev.p), nb * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    RFD_HIP(hipMemcpyAsync(coef.data(), stage.coef(dev.p), nb * 64 * sizeof(int16_t), hipMemcpyDeviceToHost, s));
    RFD_HIP(hipStreamSynchronize(s));
    jpeg_dequantise_natural(h, rec.data(), coef.data(), out);
    return RFD_OK;
}

} // namespace rfd
