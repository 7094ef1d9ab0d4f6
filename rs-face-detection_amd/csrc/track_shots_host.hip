// track_shots_host.hip -- every entry of include/rfd.h's "track shots".  What the state owns is track_shots_host.h, the host
// decisions are track_shots_plan.h, the kernels are kernels_track_shots.hip.  The tracker itself (its slots, its update) is
// tracker_host.hip and is only read here; so are the identities' heads (track_identity_host.hip), for the records.
#include "tracker_host.h"

#include <vector>

using namespace rfd;

int rfd_track_shot_config_default(rfd_track_shot_config *cfg)
{
    RFD_CHECK_ARG(cfg != nullptr, "cfg is null");
    memset(cfg, 0, sizeof *cfg);
    cfg->crop_w = 112; // rfd_alignment_config's default out_w, out_h
    cfg->crop_h = 112;
    return RFD_OK;
}

static const char kShotsOff[] = "invalid argument: track shots are not enabled on this tracker (rfd_tracker_shots_enable)";

int rfd_tracker_shots_enable(rfd_tracker *t, const rfd_track_shot_config *cfg)
{
    rfd_track_shot_config def;
    if (!cfg) { RFD_TRY(rfd_track_shot_config_default(&def)); cfg = &def; }
    char msg[128];
    // the config is judged first: its refusals need no tracker
    if (!track_shot_config_ok(*cfg, msg, sizeof msg)) { set_error("invalid argument: track shot config: %s", msg); return RFD_ERR_INVALID_ARG; }
    RFD_CHECK_ARG(t != nullptr, "tracker is null");
    if (t->shots.enabled) { set_error("invalid argument: track shots are already enabled on this tracker"); return RFD_ERR_INVALID_ARG; }
    if (!track_shot_fits(t->cfg.streams, t->cfg.max_tracks, cfg->crop_w, cfg->crop_h)) {
        set_error("track shots: %d streams x %d tracks x %d x %d x 3 bytes exceed 1 GiB", t->cfg.streams, t->cfg.max_tracks, cfg->crop_w, cfg->crop_h);
        return RFD_ERR_CAPACITY;
    }
    RFD_HIP(hipSetDevice(ctx_device(t->ctx)));
    const hipStream_t s = ctx_stream(t->ctx);
    TrackShotState &sh = t->shots;
    const size_t head_bytes = (size_t)t->cfg.streams * t->cfg.max_tracks * sizeof(TrackShotHead);
    const size_t items = track_shot_item_capacity(t->max_batch, t->cfg.max_tracks);
    int rc = RFD_OK;
    if (rc == RFD_OK) rc = sh.heads.reserve(head_bytes);
    if (rc == RFD_OK) rc = sh.bank.reserve(track_shot_bank_bytes(t->cfg.streams, t->cfg.max_tracks, cfg->crop_w, cfg->crop_h));
    if (rc == RFD_OK) rc = sh.ring.ensure(track_shot_ring_bytes(t->max_batch));
    if (rc == RFD_OK) rc = sh.call.reserve(track_shot_ring_bytes(t->max_batch));
    if (rc == RFD_OK) rc = sh.items.reserve(items * sizeof(ShotCopyItem));
    if (rc == RFD_OK) rc = sh.seg_count.reserve((size_t)t->max_batch * sizeof(int32_t));
    if (rc == RFD_OK) rc = sh.scratch.reserve((2 * (size_t)t->max_batch + 1 + items) * sizeof(int32_t));
    // the bank needs no fill: a crop is read only through a head that a keep has written
    if (rc == RFD_OK && hipMemsetAsync(sh.heads.p, 0, head_bytes, s) != hipSuccess) {
        set_error("the fill of the track shots' state failed");
        (void)hipStreamSynchronize(s); // a fill that was enqueued has run before its buffer is freed
        rc = RFD_ERR_HIP;
    }
    if (rc != RFD_OK) {
        sh.heads.release(); sh.bank.release(); sh.call.release(); sh.items.release(); sh.seg_count.release(); sh.scratch.release();
        return rc;
    }
    sh.cfg = *cfg;
    sh.row_bytes = track_shot_row_bytes(cfg->crop_w, cfg->crop_h);
    sh.enabled = true;
    return RFD_OK;
}

// what every call of this section checks first
static int shots_check_call(const rfd_tracker *t, const int32_t *stream, int n)
{
    RFD_CHECK_ARG(t != nullptr, "tracker is null");
    if (!t->shots.enabled) { set_error("%s", kShotsOff); return RFD_ERR_INVALID_ARG; }
    RFD_CHECK_ARG(n >= 0, "n < 0");
    if (n > t->max_batch) {
        set_error("track shots: a call of %d frames exceeds max_batch_size %d", n, t->max_batch);
        return RFD_ERR_CAPACITY;
    }
    if (n == 0) return RFD_OK;
    RFD_CHECK_ARG(stream != nullptr, "stream is null");
    const int bad = track_plan_bad_stream(stream, n, t->cfg.streams);
    if (bad >= 0) {
        set_error("invalid argument: stream[%d] = %d is outside [0, %d)", bad, stream[bad], t->cfg.streams);
        return RFD_ERR_INVALID_ARG;
    }
    return RFD_OK;
}

static int shots_check_keep(const rfd_tracker *t, const int32_t *stream, int n, const rfd_track_obs *obs, int m, const uint8_t *crops,
                            const int32_t *status)
{
    RFD_TRY(shots_check_call(t, stream, n));
    RFD_CHECK_ARG(m >= 0, "m < 0");
    RFD_CHECK_ARG(obs && obs->first && obs->row && obs->serial, "obs: first, row or serial is null");
    if (n == 0 || m == 0) return RFD_OK;
    RFD_CHECK_ARG(crops != nullptr, "crops is null");
    RFD_CHECK_ARG(status != nullptr, "status is null");
    return RFD_OK;
}

static int shots_check_collect(const rfd_tracker *t, const int32_t *stream, int n, const int32_t *stats, const int32_t *ended, int cap,
                               const rfd_track_records *out)
{
    RFD_TRY(shots_check_call(t, stream, n));
    RFD_CHECK_ARG(cap >= 1, "cap < 1");
    if (n == 0) return RFD_OK;
    RFD_CHECK_ARG(stats != nullptr, "stats is null");
    RFD_CHECK_ARG(ended != nullptr, "ended is null");
    RFD_CHECK_ARG(out && out->total && out->first && out->rec, "out: total, first or rec is null");
    RFD_CHECK_ARG((uintptr_t)out->rec % 8 == 0, "out: rec is not 8-byte aligned");
    return RFD_OK;
}

// the work list (keep: the plan; collect: the stream list) and the stamps of a call, through this state's ring
static int shots_send_call(rfd_tracker *t, const int32_t *stream, const int64_t *stamp, int n, bool plan, int *groups)
{
    const hipStream_t s = ctx_stream(t->ctx);
    TrackShotState &sh = t->shots;
    char *slot;
    RFD_TRY(sh.ring.acquire(&slot));
    int32_t *ints = reinterpret_cast<int32_t *>(slot);
    if (plan) {
        *groups = track_plan(stream, n, ints);
    } else {
        memcpy(ints, stream, (size_t)n * sizeof(int32_t));
        for (size_t i = (size_t)n; i < track_plan_ints(n); ++i) ints[i] = 0; // the slot is copied whole
    }
    memset(slot + track_plan_ints(n) * sizeof(int32_t), 0, track_shot_ring_stamp_offset(n) - track_plan_ints(n) * sizeof(int32_t));
    track_shot_ring_stamps(slot, stamp, n);
    RFD_HIP(hipMemcpyAsync(sh.call.p, slot, track_shot_ring_bytes(n), hipMemcpyHostToDevice, s));
    RFD_TRY(sh.ring.record(s));
    return RFD_OK;
}

static TrackShotCommon shots_common(rfd_tracker *t, int n)
{
    TrackShotState &sh = t->shots;
    TrackShotCommon c;
    memset(&c, 0, sizeof c);
    c.plan = (const int32_t *)sh.call.p;
    c.stamp = (const int64_t *)((const char *)sh.call.p + track_shot_ring_stamp_offset(n));
    c.n = n; c.max_det = t->max_det; c.max_tracks = t->cfg.max_tracks;
    c.slots = (const TrackSlot *)t->slots.p;
    c.heads = (TrackShotHead *)sh.heads.p;
    c.items = (ShotCopyItem *)sh.items.p;
    c.seg_count = (int32_t *)sh.seg_count.p;
    return c;
}

static int keep_enqueue(rfd_tracker *t, const int32_t *stream, const int64_t *stamp, int n, const rfd_track_obs &obs, int m,
                        const uint8_t *crops, const int32_t *face_status, const float *q, int32_t *status)
{
    const hipStream_t s = ctx_stream(t->ctx);
    TrackShotState &sh = t->shots;
    int groups = 0;
    RFD_TRY(shots_send_call(t, stream, stamp, n, true, &groups));
    TrackShotDecideParams p;
    memset(&p, 0, sizeof p);
    p.c = shots_common(t, n);
    p.total = obs.total; p.first = obs.first; p.row = obs.row; p.serial = obs.serial;
    p.m = m; p.face_status = face_status; p.q = q; p.status = status;
    RFD_TRY(launch_track_shot_decide(p, groups, s));
    ShotCopyParams cp;
    memset(&cp, 0, sizeof cp);
    cp.src = crops; cp.dst = (uint8_t *)sh.bank.p; cp.row_bytes = (uint32_t)sh.row_bytes;
    cp.items = p.c.items; cp.seg_count = p.c.seg_count; cp.segments = groups; cp.seg_stride = t->cfg.max_tracks;
    return launch_shot_copy(cp, track_shot_keep_bound(m, groups, t->cfg.max_tracks), s);
}

static int collect_enqueue(rfd_tracker *t, const int32_t *stream, const int64_t *stamp, int n, const int32_t *stats, const int32_t *ended,
                           int cap, const rfd_track_records &out)
{
    const hipStream_t s = ctx_stream(t->ctx);
    TrackShotState &sh = t->shots;
    int groups = 0;
    RFD_TRY(shots_send_call(t, stream, stamp, n, false, &groups));
    TrackRecordListParams p;
    memset(&p, 0, sizeof p);
    p.c = shots_common(t, n);
    p.stats = stats; p.ended = ended; p.cap = cap;
    p.id_heads = t->ident.enabled ? (const TrackIdHead *)t->ident.heads.p : nullptr;
    p.scratch = (int32_t *)sh.scratch.p;
    p.total = out.total; p.first = out.first; p.rec = out.rec;
    RFD_TRY(launch_track_record_list(p, s));
    if (!out.crops) return RFD_OK;
    ShotCopyParams cp;
    memset(&cp, 0, sizeof cp);
    cp.src = (const uint8_t *)sh.bank.p; cp.dst = out.crops; cp.row_bytes = (uint32_t)sh.row_bytes;
    cp.items = p.c.items; cp.seg_count = p.c.seg_count; cp.segments = 1; cp.seg_stride = 0;
    return launch_shot_copy(cp, track_shot_collect_bound(cap, n, t->cfg.max_tracks), s);
}

int rfd_tracker_keep_shots_device(rfd_tracker *t, const int32_t *stream, const int64_t *stamp, int n, const rfd_track_obs *obs, int m,
                                  const uint8_t *crops, const int32_t *face_status, const float *q, int32_t *status, int async)
{
    RFD_TRY(shots_check_keep(t, stream, n, obs, m, crops, status));
    if (n == 0 || m == 0) return RFD_OK;
    RFD_HIP(hipSetDevice(ctx_device(t->ctx)));
    RFD_TRY(keep_enqueue(t, stream, stamp, n, *obs, m, crops, face_status, q, status));
    if (async) return RFD_OK;
    RFD_HIP(hipStreamSynchronize(ctx_stream(t->ctx)));
    return RFD_OK;
}

int rfd_tracker_collect_ended_device(rfd_tracker *t, const int32_t *stream, const int64_t *stamp, int n, const int32_t *stats,
                                     const int32_t *ended, int cap, const rfd_track_records *out, int async)
{
    RFD_TRY(shots_check_collect(t, stream, n, stats, ended, cap, out));
    if (n == 0) return RFD_OK;
    RFD_HIP(hipSetDevice(ctx_device(t->ctx)));
    RFD_TRY(collect_enqueue(t, stream, stamp, n, stats, ended, cap, *out));
    if (async) return RFD_OK;
    RFD_HIP(hipStreamSynchronize(ctx_stream(t->ctx)));
    return RFD_OK;
}

namespace {
// a caller's host array with its device twin: `in` goes up when set, `back` comes down
struct Twin {
    DevBuf *dev;
    const void *in;
    void *back;
    size_t bytes;
};

int twins_up(const Twin *twins, size_t count, hipStream_t s)
{
    for (size_t i = 0; i < count; ++i)
        if (twins[i].in) RFD_TRY(twins[i].dev->reserve(twins[i].bytes));
    for (size_t i = 0; i < count; ++i)
        if (twins[i].in) RFD_HIP(hipMemcpyAsync(twins[i].dev->p, twins[i].in, twins[i].bytes, hipMemcpyHostToDevice, s));
    return RFD_OK;
}

int twins_back(const Twin *twins, size_t count, hipStream_t s)
{
    for (size_t i = 0; i < count; ++i)
        if (twins[i].back) RFD_HIP(hipMemcpyAsync(twins[i].back, twins[i].dev->p, twins[i].bytes, hipMemcpyDeviceToHost, s));
    RFD_HIP(hipStreamSynchronize(s));
    return RFD_OK;
}
} // namespace

int rfd_tracker_keep_shots(rfd_tracker *t, const int32_t *stream, const int64_t *stamp, int n, const rfd_track_obs *obs, int m,
                           const uint8_t *crops, const int32_t *face_status, const float *q, int32_t *status)
{
    RFD_TRY(shots_check_keep(t, stream, n, obs, m, crops, status));
    if (n == 0 || m == 0) return RFD_OK;
    RFD_HIP(hipSetDevice(ctx_device(t->ctx)));
    const hipStream_t s = ctx_stream(t->ctx);
    TrackShotState &sh = t->shots;
    const size_t N = (size_t)n, M = (size_t)m, MD = (size_t)t->max_det;
    // the output goes up too, so that what it holds past the count comes back as it was
    const Twin twins[] = {
        {&sh.h_total, obs->total, nullptr, sizeof(int32_t)},
        {&sh.h_first, obs->first, nullptr, (N + 1) * sizeof(int32_t)},
        {&sh.h_row, obs->row, nullptr, M * sizeof(int32_t)},
        {&sh.h_serial, obs->serial, nullptr, N * MD * sizeof(int32_t)},
        {&sh.h_crops, crops, nullptr, M * sh.row_bytes},
        {&sh.h_face_status, face_status, nullptr, M * sizeof(int32_t)},
        {&sh.h_q, q, nullptr, M * sizeof(float)},
        {&sh.h_status, status, status, M * sizeof(int32_t)},
    };
    constexpr size_t K = sizeof twins / sizeof twins[0];
    RFD_TRY(twins_up(twins, K, s));
    auto dev = [&](int i) -> void * { return twins[i].in ? twins[i].dev->p : nullptr; };
    const rfd_track_obs o = {(const int32_t *)dev(0), (const int32_t *)dev(1), (const int32_t *)dev(2), (const int32_t *)dev(3)};
    RFD_TRY(keep_enqueue(t, stream, stamp, n, o, m, (const uint8_t *)dev(4), (const int32_t *)dev(5), (const float *)dev(6), (int32_t *)dev(7)));
    return twins_back(twins, K, s);
}

int rfd_tracker_collect_ended(rfd_tracker *t, const int32_t *stream, const int64_t *stamp, int n, const int32_t *stats, const int32_t *ended,
                              int cap, const rfd_track_records *out)
{
    RFD_TRY(shots_check_collect(t, stream, n, stats, ended, cap, out));
    if (n == 0) return RFD_OK;
    RFD_HIP(hipSetDevice(ctx_device(t->ctx)));
    const hipStream_t s = ctx_stream(t->ctx);
    TrackShotState &sh = t->shots;
    const size_t N = (size_t)n, MT = (size_t)t->cfg.max_tracks, CAP = (size_t)cap;
    const Twin twins[] = {
        {&sh.h_stats, stats, nullptr, N * 4 * sizeof(int32_t)},
        {&sh.h_ended, ended, nullptr, N * MT * sizeof(int32_t)},
        {&sh.h_rtotal, out->total, out->total, sizeof(int32_t)},
        {&sh.h_rfirst, out->first, out->first, (N + 1) * sizeof(int32_t)},
        {&sh.h_rec, out->rec, out->rec, CAP * sizeof(rfd_track_record)},
        {&sh.h_rcrops, out->crops, out->crops, CAP * sh.row_bytes},
    };
    constexpr size_t K = sizeof twins / sizeof twins[0];
    RFD_TRY(twins_up(twins, K, s));
    auto dev = [&](int i) -> void * { return twins[i].in ? twins[i].dev->p : nullptr; };
    const rfd_track_records o = {(int32_t *)dev(2), (int32_t *)dev(3), (rfd_track_record *)dev(4), (uint8_t *)dev(5)};
    RFD_TRY(collect_enqueue(t, stream, stamp, n, (const int32_t *)dev(0), (const int32_t *)dev(1), cap, o));
    return twins_back(twins, K, s);
}

// the slots and heads of a stream on the host, after the stream has drained
static int shots_read_stream(rfd_tracker *t, int stream, std::vector<TrackSlot> &slots, std::vector<TrackShotHead> &heads)
{
    RFD_CHECK_ARG(t != nullptr, "tracker is null");
    if (!t->shots.enabled) { set_error("%s", kShotsOff); return RFD_ERR_INVALID_ARG; }
    if (stream < 0 || stream >= t->cfg.streams) {
        set_error("invalid argument: stream %d is outside [0, %d)", stream, t->cfg.streams);
        return RFD_ERR_INVALID_ARG;
    }
    RFD_HIP(hipSetDevice(ctx_device(t->ctx)));
    const hipStream_t s = ctx_stream(t->ctx);
    const size_t mt = (size_t)t->cfg.max_tracks;
    slots.resize(mt);
    heads.resize(mt);
    RFD_HIP(hipMemcpyAsync(slots.data(), (const TrackSlot *)t->slots.p + (size_t)stream * mt, mt * sizeof(TrackSlot), hipMemcpyDeviceToHost, s));
    RFD_HIP(hipMemcpyAsync(heads.data(), (const TrackShotHead *)t->shots.heads.p + (size_t)stream * mt, mt * sizeof(TrackShotHead), hipMemcpyDeviceToHost, s));
    RFD_HIP(hipStreamSynchronize(s));
    return RFD_OK;
}

int rfd_tracker_get_shots(rfd_tracker *t, int stream, rfd_track_shot *out, int cap, int *count)
{
    RFD_CHECK_ARG(t != nullptr, "tracker is null");
    RFD_CHECK_ARG(count != nullptr, "count is null");
    RFD_CHECK_ARG(cap >= 0 && (out || cap == 0), "out is null with a cap");
    std::vector<TrackSlot> slots;
    std::vector<TrackShotHead> heads;
    RFD_TRY(shots_read_stream(t, stream, slots, heads));
    int live = 0;
    for (int i = 0; i < t->cfg.max_tracks; ++i) {
        const TrackShotHead &h = heads[(size_t)i];
        if (slots[(size_t)i].serial == 0 || h.serial != slots[(size_t)i].serial) continue;
        if (live < cap) {
            rfd_track_shot &o = out[live];
            o.slot = i; o.serial = h.serial; o.shots = h.shots; o.kept = h.kept; o.q = h.q; o.reserved = 0;
            o.first_stamp = h.first_stamp; o.best_stamp = h.best_stamp;
        }
        ++live;
    }
    *count = live;
    return RFD_OK;
}

int rfd_tracker_get_shot_crop(rfd_tracker *t, int stream, int32_t serial, uint8_t *out)
{
    RFD_CHECK_ARG(t != nullptr, "tracker is null");
    RFD_CHECK_ARG(out != nullptr, "out is null");
    std::vector<TrackSlot> slots;
    std::vector<TrackShotHead> heads;
    RFD_TRY(shots_read_stream(t, stream, slots, heads));
    int slot = -1;
    for (int i = 0; i < t->cfg.max_tracks && slot < 0 && serial != 0; ++i)
        if (slots[(size_t)i].serial == serial) slot = i;
    if (slot < 0 || heads[(size_t)slot].serial != serial) {
        set_error("invalid argument: no such track: stream %d has no track with a kept shot and serial %d", stream, serial);
        return RFD_ERR_INVALID_ARG;
    }
    const size_t row = t->shots.row_bytes;
    const uint8_t *src = (const uint8_t *)t->shots.bank.p + ((size_t)stream * t->cfg.max_tracks + slot) * row;
    RFD_HIP(hipMemcpyAsync(out, src, row, hipMemcpyDeviceToHost, ctx_stream(t->ctx)));
    RFD_HIP(hipStreamSynchronize(ctx_stream(t->ctx)));
    return RFD_OK;
}
