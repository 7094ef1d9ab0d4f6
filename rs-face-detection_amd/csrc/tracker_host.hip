// tracker_host.hip -- every rfd_tracker_* entry of include/rfd.h ("tracker").  What a tracker owns is tracker_host.h, its host
// decisions are track_plan.h, its kernel is kernels_track.hip.
#include "tracker_host.h"

#include <memory>
#include <vector>

using namespace rfd;

int rfd_tracker_config_default(const rfd_ctx *c, rfd_tracker_config *cfg)
{
    RFD_CHECK_ARG(cfg != nullptr, "cfg is null");
    rfd_config cc;
    if (c) RFD_TRY(rfd_get_config(c, &cc));
    else rfd_config_default(&cc); // no context: the threshold a default context would have
    memset(cfg, 0, sizeof *cfg);
    // chosen values, not tuned on data (rfd.h)
    cfg->streams = 1;
    cfg->max_tracks = 64;
    cfg->iou_min = 0.3f;
    cfg->max_missed = 5;
    cfg->min_score = cc.confidence_threshold;
    cfg->new_score = cc.confidence_threshold;
    cfg->min_hits = 2;
    cfg->improve = 1.1f;
    return RFD_OK;
}

int rfd_tracker_create(rfd_ctx *c, const rfd_tracker_config *cfg, rfd_tracker **out)
{
    RFD_CHECK_ARG(out != nullptr, "out is null");
    *out = nullptr;
    char msg[128];
    // a caller's config is judged first: its refusals need no context
    if (cfg && !track_config_ok(*cfg, msg, sizeof msg)) { set_error("invalid argument: tracker config: %s", msg); return RFD_ERR_INVALID_ARG; }
    RFD_CHECK_ARG(c != nullptr, "ctx is null");
    rfd_tracker_config def;
    if (!cfg) { RFD_TRY(rfd_tracker_config_default(c, &def)); cfg = &def; }
    if (!track_config_ok(*cfg, msg, sizeof msg)) { set_error("invalid argument: tracker config: %s", msg); return RFD_ERR_INVALID_ARG; }
    rfd_config cc;
    RFD_TRY(rfd_get_config(c, &cc));
    if (cc.max_det > RFD_TRACKER_MAX_DET) {
        set_error("tracker: the context's max_det %d exceeds %d rows per frame", cc.max_det, RFD_TRACKER_MAX_DET);
        return RFD_ERR_CAPACITY;
    }
    RFD_HIP(hipSetDevice(ctx_device(c)));
    const hipStream_t s = ctx_stream(c);
    std::unique_ptr<rfd_tracker> t(new rfd_tracker()); // an early return frees whatever was built so far
    t->ctx = c;
    t->cfg = *cfg;
    t->max_batch = cc.max_batch_size;
    t->max_det = cc.max_det;
    const size_t slot_bytes = (size_t)cfg->streams * cfg->max_tracks * sizeof(TrackSlot);
    RFD_TRY(t->slots.reserve(slot_bytes));
    RFD_TRY(t->next_serial.reserve((size_t)cfg->streams * sizeof(int32_t)));
    RFD_TRY(t->plan.reserve(track_plan_ints(t->max_batch) * sizeof(int32_t)));
    RFD_TRY(t->plan_ring.ensure(track_plan_ints(t->max_batch) * sizeof(int32_t)));
    if (hipMemsetAsync(t->slots.p, 0, slot_bytes, s) != hipSuccess ||
        hipMemsetD32Async((hipDeviceptr_t)t->next_serial.p, 1, (size_t)cfg->streams, s) != hipSuccess) {
        set_error("the fill of the tracker's state failed");
        (void)hipStreamSynchronize(s); // a fill that was enqueued has run before its buffer is freed
        return RFD_ERR_HIP;
    }
    *out = t.release();
    return RFD_OK;
}

void rfd_tracker_destroy(rfd_tracker *t)
{
    if (!t) return;
    (void)hipSetDevice(ctx_device(t->ctx));
    (void)hipStreamSynchronize(ctx_stream(t->ctx));
    delete t;
}

// the checks both update forms share; nothing is enqueued before they pass
static int tracker_check_update(const rfd_tracker *t, const int32_t *stream, const rfd_dets *dets, int n, const rfd_track_out *out)
{
    RFD_CHECK_ARG(t != nullptr, "tracker is null");
    RFD_CHECK_ARG(n >= 0, "n < 0");
    if (n > t->max_batch) {
        set_error("tracker update of %d frames exceeds max_batch_size %d", n, t->max_batch);
        return RFD_ERR_CAPACITY;
    }
    if (n == 0) return RFD_OK;
    RFD_CHECK_ARG(stream != nullptr, "stream is null");
    RFD_CHECK_ARG(dets && dets->boxes && dets->landmarks && dets->count, "dets: boxes, landmarks or count is null");
    RFD_CHECK_ARG(out && out->track && out->flags, "out: track or flags is null");
    const int set = (out->due.boxes != nullptr) + (out->due.landmarks != nullptr) + (out->due.count != nullptr);
    if (set != 0 && set != 3) { set_error("invalid argument: out->due is half set: boxes, landmarks and count go together"); return RFD_ERR_INVALID_ARG; }
    if (set == 0 && out->due.total) { set_error("invalid argument: out->due.total without the due slab"); return RFD_ERR_INVALID_ARG; }
    const int bad = track_plan_bad_stream(stream, n, t->cfg.streams);
    if (bad >= 0) {
        set_error("invalid argument: stream[%d] = %d is outside [0, %d)", bad, stream[bad], t->cfg.streams);
        return RFD_ERR_INVALID_ARG;
    }
    return RFD_OK;
}

// plan, copy, launch: all device pointers, enqueued only
static int tracker_enqueue(rfd_tracker *t, const int32_t *stream, const rfd_dets &dets, const float *quality, int n, const rfd_track_out &out)
{
    const hipStream_t s = ctx_stream(t->ctx);
    int32_t *slot;
    RFD_TRY(t->plan_ring.acquire(&slot));
    const int groups = track_plan(stream, n, slot);
    RFD_HIP(hipMemcpyAsync(t->plan.p, slot, track_plan_ints(n) * sizeof(int32_t), hipMemcpyHostToDevice, s));
    RFD_TRY(t->plan_ring.record(s));
    TrackParams p;
    memset(&p, 0, sizeof p);
    p.plan = (const int32_t *)t->plan.p;
    p.n = n; p.max_det = t->max_det;
    p.boxes = dets.boxes; p.lmk = dets.landmarks; p.count = dets.count; p.quality = quality;
    p.iou_min = t->cfg.iou_min; p.min_score = t->cfg.min_score; p.new_score = t->cfg.new_score; p.improve = t->cfg.improve;
    p.max_missed = t->cfg.max_missed; p.min_hits = t->cfg.min_hits; p.max_tracks = t->cfg.max_tracks;
    p.slots = (TrackSlot *)t->slots.p;
    p.next_serial = (int32_t *)t->next_serial.p;
    p.track = out.track; p.flags = out.flags; p.stats = out.stats; p.ended = out.ended;
    p.due_boxes = out.due.boxes; p.due_lmk = out.due.landmarks; p.due_count = out.due.count; p.due_total = out.due.total;
    p.due_track = out.due_track;
    return launch_track_update(p, groups, s);
}

int rfd_tracker_update_device(rfd_tracker *t, const int32_t *stream, const rfd_dets *dets, const float *quality, int n,
                              const rfd_track_out *out, int async)
{
    RFD_TRY(tracker_check_update(t, stream, dets, n, out));
    if (n == 0) return RFD_OK;
    RFD_HIP(hipSetDevice(ctx_device(t->ctx)));
    RFD_TRY(tracker_enqueue(t, stream, *dets, quality, n, *out));
    if (async) return RFD_OK;
    RFD_HIP(hipStreamSynchronize(ctx_stream(t->ctx)));
    return RFD_OK;
}

int rfd_tracker_update(rfd_tracker *t, const int32_t *stream, const rfd_dets *dets, const float *quality, int n, const rfd_track_out *out)
{
    RFD_TRY(tracker_check_update(t, stream, dets, n, out));
    if (n == 0) return RFD_OK;
    RFD_HIP(hipSetDevice(ctx_device(t->ctx)));
    const hipStream_t s = ctx_stream(t->ctx);
    const size_t N = (size_t)n, MD = (size_t)t->max_det, MT = (size_t)t->cfg.max_tracks;
    // every array with its device twin; the outputs go up too, so that what they hold past the counts comes back as it was
    struct Twin { DevBuf *dev; const void *in; void *back; size_t bytes; };
    const Twin twins[] = {
        {&t->h_boxes, dets->boxes, nullptr, N * MD * 5 * sizeof(float)},
        {&t->h_lmk, dets->landmarks, nullptr, N * MD * 10 * sizeof(float)},
        {&t->h_count, dets->count, nullptr, N * sizeof(int32_t)},
        {&t->h_quality, quality, nullptr, N * MD * sizeof(float)},
        {&t->h_track, out->track, out->track, N * MD * sizeof(int32_t)},
        {&t->h_flags, out->flags, out->flags, N * MD * sizeof(uint32_t)},
        {&t->h_stats, out->stats, out->stats, N * 4 * sizeof(int32_t)},
        {&t->h_ended, out->ended, out->ended, N * MT * sizeof(int32_t)},
        {&t->h_due_boxes, out->due.boxes, out->due.boxes, N * MD * 5 * sizeof(float)},
        {&t->h_due_lmk, out->due.landmarks, out->due.landmarks, N * MD * 10 * sizeof(float)},
        {&t->h_due_count, out->due.count, out->due.count, N * sizeof(int32_t)},
        {&t->h_due_total, out->due.total, out->due.total, N * sizeof(int32_t)},
        {&t->h_due_track, out->due_track, out->due_track, N * MD * sizeof(int32_t)},
    };
    for (const Twin &w : twins)
        if (w.in) RFD_TRY(w.dev->reserve(w.bytes));
    for (const Twin &w : twins)
        if (w.in) RFD_HIP(hipMemcpyAsync(w.dev->p, w.in, w.bytes, hipMemcpyHostToDevice, s));
    auto dev = [&](int i) -> void * { return twins[i].in ? twins[i].dev->p : nullptr; };
    rfd_dets d = {(float *)dev(0), (float *)dev(1), (int32_t *)dev(2), nullptr};
    rfd_track_out o;
    memset(&o, 0, sizeof o);
    o.track = (int32_t *)dev(4); o.flags = (uint32_t *)dev(5); o.stats = (int32_t *)dev(6); o.ended = (int32_t *)dev(7);
    o.due = rfd_dets{(float *)dev(8), (float *)dev(9), (int32_t *)dev(10), (int32_t *)dev(11)};
    o.due_track = (int32_t *)dev(12);
    RFD_TRY(tracker_enqueue(t, stream, d, (const float *)dev(3), n, o));
    for (const Twin &w : twins)
        if (w.back) RFD_HIP(hipMemcpyAsync(w.back, w.dev->p, w.bytes, hipMemcpyDeviceToHost, s));
    RFD_HIP(hipStreamSynchronize(s));
    return RFD_OK;
}

int rfd_tracker_reset(rfd_tracker *t, int stream)
{
    RFD_CHECK_ARG(t != nullptr, "tracker is null");
    if (stream < -1 || stream >= t->cfg.streams) {
        set_error("invalid argument: stream %d is outside [0, %d) and not -1", stream, t->cfg.streams);
        return RFD_ERR_INVALID_ARG;
    }
    RFD_HIP(hipSetDevice(ctx_device(t->ctx)));
    const size_t per = (size_t)t->cfg.max_tracks * sizeof(TrackSlot);
    char *base = (char *)t->slots.p;
    if (stream < 0) RFD_HIP(hipMemsetAsync(base, 0, per * t->cfg.streams, ctx_stream(t->ctx)));
    else RFD_HIP(hipMemsetAsync(base + per * stream, 0, per, ctx_stream(t->ctx)));
    return RFD_OK;
}

int rfd_tracker_get_tracks(rfd_tracker *t, int stream, rfd_track *out, int cap, int *count)
{
    RFD_CHECK_ARG(t != nullptr, "tracker is null");
    RFD_CHECK_ARG(count != nullptr, "count is null");
    RFD_CHECK_ARG(cap >= 0 && (out || cap == 0), "out is null with a cap");
    if (stream < 0 || stream >= t->cfg.streams) {
        set_error("invalid argument: stream %d is outside [0, %d)", stream, t->cfg.streams);
        return RFD_ERR_INVALID_ARG;
    }
    RFD_HIP(hipSetDevice(ctx_device(t->ctx)));
    const hipStream_t s = ctx_stream(t->ctx);
    std::vector<TrackSlot> host((size_t)t->cfg.max_tracks);
    RFD_HIP(hipMemcpyAsync(host.data(), (const TrackSlot *)t->slots.p + (size_t)stream * t->cfg.max_tracks,
                           host.size() * sizeof(TrackSlot), hipMemcpyDeviceToHost, s));
    RFD_HIP(hipStreamSynchronize(s));
    int live = 0;
    for (int i = 0; i < t->cfg.max_tracks; ++i) {
        const TrackSlot &k = host[(size_t)i];
        if (k.serial == 0) continue;
        if (live < cap) {
            rfd_track &o = out[live];
            o.slot = i; o.serial = k.serial;
            memcpy(o.box, k.box, sizeof o.box);
            o.missed = k.missed; o.hits = k.hits; o.shot_q = k.shot_q;
        }
        ++live;
    }
    *count = live;
    return RFD_OK;
}
