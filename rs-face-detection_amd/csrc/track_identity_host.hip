// track_identity_host.hip -- every entry of include/rfd.h's "track identities".  What the state owns is track_identity_host.h,
// the host decisions are track_identity_plan.h, the kernels are kernels_track_identity.hip.  The tracker itself (its slots, its
// update) is tracker_host.hip and is only read here.
#include "tracker_host.h"

#include <vector>

using namespace rfd;

int rfd_track_identity_config_default(rfd_track_identity_config *cfg)
{
    RFD_CHECK_ARG(cfg != nullptr, "cfg is null");
    memset(cfg, 0, sizeof *cfg);
    // chosen values, not tuned on data (rfd.h)
    cfg->dim = 512;
    cfg->accept = 0.5f;
    cfg->release = 0.4f;
    cfg->margin = 0.05f;
    return RFD_OK;
}

int rfd_tracker_identity_enable(rfd_tracker *t, const rfd_track_identity_config *cfg)
{
    rfd_track_identity_config def;
    if (!cfg) { RFD_TRY(rfd_track_identity_config_default(&def)); cfg = &def; }
    char msg[128];
    // the config is judged first: its refusals need no tracker
    if (!track_identity_config_ok(*cfg, msg, sizeof msg)) { set_error("invalid argument: track identity config: %s", msg); return RFD_ERR_INVALID_ARG; }
    RFD_CHECK_ARG(t != nullptr, "tracker is null");
    if (t->ident.enabled) { set_error("invalid argument: track identities are already enabled on this tracker"); return RFD_ERR_INVALID_ARG; }
    if (!track_identity_fits(t->cfg.streams, t->cfg.max_tracks, cfg->dim)) {
        set_error("track identities: %d streams x %d tracks x dim %d x 4 bytes exceed 1 GiB", t->cfg.streams, t->cfg.max_tracks, cfg->dim);
        return RFD_ERR_CAPACITY;
    }
    RFD_HIP(hipSetDevice(ctx_device(t->ctx)));
    const hipStream_t s = ctx_stream(t->ctx);
    TrackIdentityState &id = t->ident;
    const size_t head_bytes = (size_t)t->cfg.streams * t->cfg.max_tracks * sizeof(TrackIdHead);
    const size_t tmpl_bytes = track_identity_template_bytes(t->cfg.streams, t->cfg.max_tracks, cfg->dim);
    RFD_TRY(id.heads.reserve(head_bytes));
    RFD_TRY(id.templates.reserve(tmpl_bytes));
    if (hipMemsetAsync(id.heads.p, 0, head_bytes, s) != hipSuccess || hipMemsetAsync(id.templates.p, 0, tmpl_bytes, s) != hipSuccess) {
        set_error("the fill of the track identities' state failed");
        (void)hipStreamSynchronize(s); // a fill that was enqueued has run before its buffer is freed
        id.heads.release();
        id.templates.release();
        return RFD_ERR_HIP;
    }
    id.cfg = *cfg;
    id.enabled = true;
    return RFD_OK;
}

// what every call of this section checks first
static int identity_check_call(const rfd_tracker *t, const int32_t *stream, int n)
{
    RFD_CHECK_ARG(t != nullptr, "tracker is null");
    if (!t->ident.enabled) { set_error("invalid argument: track identities are not enabled on this tracker (rfd_tracker_identity_enable)"); return RFD_ERR_INVALID_ARG; }
    RFD_CHECK_ARG(n >= 0, "n < 0");
    if (n > t->max_batch) {
        set_error("track identities: a call of %d frames exceeds max_batch_size %d", n, t->max_batch);
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

static int identity_check_obs(const rfd_track_obs *obs, int m)
{
    RFD_CHECK_ARG(m >= 0, "m < 0");
    RFD_CHECK_ARG(obs && obs->first && obs->row && obs->serial, "obs: first, row or serial is null");
    return RFD_OK;
}

static int identity_check_fuse(const rfd_tracker *t, const int32_t *stream, int n, const rfd_track_obs *obs, int m, const float *emb,
                               const float *query, const int32_t *status)
{
    RFD_TRY(identity_check_call(t, stream, n));
    RFD_TRY(identity_check_obs(obs, m));
    if (n == 0 || m == 0) return RFD_OK;
    RFD_CHECK_ARG(emb != nullptr, "emb is null");
    RFD_CHECK_ARG(query != nullptr, "query is null");
    RFD_CHECK_ARG(status != nullptr, "status is null");
    return RFD_OK;
}

static int identity_check_label(const rfd_tracker *t, const int32_t *stream, int n, const rfd_track_obs *obs, int m, int k,
                                const float *scores, const int32_t *rows, const int32_t *status_in)
{
    RFD_TRY(identity_check_call(t, stream, n));
    RFD_TRY(identity_check_obs(obs, m));
    if (k < 1 || k > kTrackIdentityMaxK) { set_error("invalid argument: k = %d is outside 1..%d", k, kTrackIdentityMaxK); return RFD_ERR_INVALID_ARG; }
    if (n == 0 || m == 0) return RFD_OK;
    RFD_CHECK_ARG(scores != nullptr, "scores is null");
    RFD_CHECK_ARG(rows != nullptr, "rows is null");
    RFD_CHECK_ARG(status_in != nullptr, "status_in is null");
    return RFD_OK;
}

static int identity_check_who(const rfd_tracker *t, const int32_t *stream, int n, const int32_t *track, const int32_t *count,
                              const uint32_t *who)
{
    RFD_TRY(identity_check_call(t, stream, n));
    if (n == 0) return RFD_OK;
    RFD_CHECK_ARG(track != nullptr, "track is null");
    RFD_CHECK_ARG(count != nullptr, "count is null");
    RFD_CHECK_ARG(who != nullptr, "who is null");
    return RFD_OK;
}

static TrackIdCommon identity_common(rfd_tracker *t, int n)
{
    TrackIdCommon c;
    memset(&c, 0, sizeof c);
    c.plan = (const int32_t *)t->plan.p;
    c.n = n; c.max_det = t->max_det; c.max_tracks = t->cfg.max_tracks; c.dim = t->ident.cfg.dim;
    c.slots = (const TrackSlot *)t->slots.p;
    c.heads = (TrackIdHead *)t->ident.heads.p;
    c.templates = (float *)t->ident.templates.p;
    return c;
}

// the stream list of a fuse or label call as its plan, through the tracker's ring; returns the groups
static int identity_send_plan(rfd_tracker *t, const int32_t *stream, int n, int *groups)
{
    const hipStream_t s = ctx_stream(t->ctx);
    int32_t *slot;
    RFD_TRY(t->plan_ring.acquire(&slot));
    *groups = track_identity_plan(stream, n, slot);
    RFD_HIP(hipMemcpyAsync(t->plan.p, slot, track_identity_plan_ints(n) * sizeof(int32_t), hipMemcpyHostToDevice, s));
    RFD_TRY(t->plan_ring.record(s));
    return RFD_OK;
}

static int fuse_enqueue(rfd_tracker *t, const int32_t *stream, int n, const rfd_track_obs &obs, int m, const float *emb,
                        const float *weight, float *query, int32_t *status)
{
    int groups = 0;
    RFD_TRY(identity_send_plan(t, stream, n, &groups));
    TrackFuseParams p;
    memset(&p, 0, sizeof p);
    p.c = identity_common(t, n);
    p.total = obs.total; p.first = obs.first; p.row = obs.row; p.serial = obs.serial;
    p.m = m; p.emb = emb; p.weight = weight; p.query = query; p.status = status;
    return launch_track_fuse(p, groups, ctx_stream(t->ctx));
}

static int label_enqueue(rfd_tracker *t, const int32_t *stream, int n, const rfd_track_obs &obs, int m, int k, const float *scores,
                         const int32_t *rows, const int32_t *ids, const int32_t *status_in)
{
    int groups = 0;
    RFD_TRY(identity_send_plan(t, stream, n, &groups));
    TrackLabelParams p;
    memset(&p, 0, sizeof p);
    p.c = identity_common(t, n);
    p.total = obs.total; p.first = obs.first; p.row = obs.row; p.serial = obs.serial;
    p.m = m; p.k = k; p.scores = scores; p.rows = rows; p.ids = ids; p.status_in = status_in;
    p.accept = t->ident.cfg.accept; p.release = t->ident.cfg.release; p.margin = t->ident.cfg.margin;
    return launch_track_label(p, groups, ctx_stream(t->ctx));
}

static int who_enqueue(rfd_tracker *t, const int32_t *stream, int n, const int32_t *track, const int32_t *count, const uint32_t *flags_in,
                       uint32_t *who, int32_t *identity, float *id_score)
{
    const hipStream_t s = ctx_stream(t->ctx);
    int32_t *slot;
    RFD_TRY(t->plan_ring.acquire(&slot));
    memcpy(slot, stream, (size_t)n * sizeof(int32_t)); // no order to keep: the stream list as it stands
    RFD_HIP(hipMemcpyAsync(t->plan.p, slot, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, s));
    RFD_TRY(t->plan_ring.record(s));
    TrackWhoParams p;
    memset(&p, 0, sizeof p);
    p.c = identity_common(t, n);
    p.track = track; p.count = count; p.flags_in = flags_in; p.who = who; p.identity = identity; p.id_score = id_score;
    return launch_track_who(p, s);
}

int rfd_tracker_fuse_device(rfd_tracker *t, const int32_t *stream, int n, const rfd_track_obs *obs, int m, const float *emb,
                            const float *weight, float *query, int32_t *status, int async)
{
    RFD_TRY(identity_check_fuse(t, stream, n, obs, m, emb, query, status));
    if (n == 0 || m == 0) return RFD_OK;
    RFD_HIP(hipSetDevice(ctx_device(t->ctx)));
    RFD_TRY(fuse_enqueue(t, stream, n, *obs, m, emb, weight, query, status));
    if (async) return RFD_OK;
    RFD_HIP(hipStreamSynchronize(ctx_stream(t->ctx)));
    return RFD_OK;
}

int rfd_tracker_label_device(rfd_tracker *t, const int32_t *stream, int n, const rfd_track_obs *obs, int m, int k, const float *scores,
                             const int32_t *rows, const int32_t *ids, const int32_t *status_in, int async)
{
    RFD_TRY(identity_check_label(t, stream, n, obs, m, k, scores, rows, status_in));
    if (n == 0 || m == 0) return RFD_OK;
    RFD_HIP(hipSetDevice(ctx_device(t->ctx)));
    RFD_TRY(label_enqueue(t, stream, n, *obs, m, k, scores, rows, ids, status_in));
    if (async) return RFD_OK;
    RFD_HIP(hipStreamSynchronize(ctx_stream(t->ctx)));
    return RFD_OK;
}

int rfd_tracker_who_device(rfd_tracker *t, const int32_t *stream, int n, const int32_t *track, const int32_t *count,
                           const uint32_t *flags_in, uint32_t *who, int32_t *identity, float *id_score, int async)
{
    RFD_TRY(identity_check_who(t, stream, n, track, count, who));
    if (n == 0) return RFD_OK;
    RFD_HIP(hipSetDevice(ctx_device(t->ctx)));
    RFD_TRY(who_enqueue(t, stream, n, track, count, flags_in, who, identity, id_score));
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

int rfd_tracker_fuse(rfd_tracker *t, const int32_t *stream, int n, const rfd_track_obs *obs, int m, const float *emb, const float *weight,
                     float *query, int32_t *status)
{
    RFD_TRY(identity_check_fuse(t, stream, n, obs, m, emb, query, status));
    if (n == 0 || m == 0) return RFD_OK;
    RFD_HIP(hipSetDevice(ctx_device(t->ctx)));
    const hipStream_t s = ctx_stream(t->ctx);
    TrackIdentityState &id = t->ident;
    const size_t N = (size_t)n, M = (size_t)m, MD = (size_t)t->max_det, D = (size_t)id.cfg.dim;
    // the outputs go up too, so that what they hold past the count comes back as it was
    const Twin twins[] = {
        {&id.h_total, obs->total, nullptr, sizeof(int32_t)},
        {&id.h_first, obs->first, nullptr, (N + 1) * sizeof(int32_t)},
        {&id.h_row, obs->row, nullptr, M * sizeof(int32_t)},
        {&id.h_serial, obs->serial, nullptr, N * MD * sizeof(int32_t)},
        {&id.h_emb, emb, nullptr, M * D * sizeof(float)},
        {&id.h_weight, weight, nullptr, M * sizeof(float)},
        {&id.h_query, query, query, M * D * sizeof(float)},
        {&id.h_status, status, status, M * sizeof(int32_t)},
    };
    constexpr size_t K = sizeof twins / sizeof twins[0];
    RFD_TRY(twins_up(twins, K, s));
    auto dev = [&](int i) -> void * { return twins[i].in ? twins[i].dev->p : nullptr; };
    const rfd_track_obs o = {(const int32_t *)dev(0), (const int32_t *)dev(1), (const int32_t *)dev(2), (const int32_t *)dev(3)};
    RFD_TRY(fuse_enqueue(t, stream, n, o, m, (const float *)dev(4), (const float *)dev(5), (float *)dev(6), (int32_t *)dev(7)));
    return twins_back(twins, K, s);
}

int rfd_tracker_label(rfd_tracker *t, const int32_t *stream, int n, const rfd_track_obs *obs, int m, int k, const float *scores,
                      const int32_t *rows, const int32_t *ids, const int32_t *status_in)
{
    RFD_TRY(identity_check_label(t, stream, n, obs, m, k, scores, rows, status_in));
    if (n == 0 || m == 0) return RFD_OK;
    RFD_HIP(hipSetDevice(ctx_device(t->ctx)));
    const hipStream_t s = ctx_stream(t->ctx);
    TrackIdentityState &id = t->ident;
    const size_t N = (size_t)n, M = (size_t)m, MD = (size_t)t->max_det, KK = (size_t)k;
    const Twin twins[] = {
        {&id.h_total, obs->total, nullptr, sizeof(int32_t)},
        {&id.h_first, obs->first, nullptr, (N + 1) * sizeof(int32_t)},
        {&id.h_row, obs->row, nullptr, M * sizeof(int32_t)},
        {&id.h_serial, obs->serial, nullptr, N * MD * sizeof(int32_t)},
        {&id.h_scores, scores, nullptr, M * KK * sizeof(float)},
        {&id.h_rows, rows, nullptr, M * KK * sizeof(int32_t)},
        {&id.h_ids, ids, nullptr, M * KK * sizeof(int32_t)},
        {&id.h_status, status_in, nullptr, M * sizeof(int32_t)},
    };
    constexpr size_t K = sizeof twins / sizeof twins[0];
    RFD_TRY(twins_up(twins, K, s));
    auto dev = [&](int i) -> void * { return twins[i].in ? twins[i].dev->p : nullptr; };
    const rfd_track_obs o = {(const int32_t *)dev(0), (const int32_t *)dev(1), (const int32_t *)dev(2), (const int32_t *)dev(3)};
    RFD_TRY(label_enqueue(t, stream, n, o, m, k, (const float *)dev(4), (const int32_t *)dev(5), (const int32_t *)dev(6), (const int32_t *)dev(7)));
    return twins_back(twins, K, s);
}

int rfd_tracker_who(rfd_tracker *t, const int32_t *stream, int n, const int32_t *track, const int32_t *count, const uint32_t *flags_in,
                    uint32_t *who, int32_t *identity, float *id_score)
{
    RFD_TRY(identity_check_who(t, stream, n, track, count, who));
    if (n == 0) return RFD_OK;
    RFD_HIP(hipSetDevice(ctx_device(t->ctx)));
    const hipStream_t s = ctx_stream(t->ctx);
    TrackIdentityState &id = t->ident;
    const size_t N = (size_t)n, MD = (size_t)t->max_det;
    const bool in_place = flags_in != nullptr && (const void *)flags_in == (const void *)who;
    const Twin twins[] = {
        {&id.h_track, track, nullptr, N * MD * sizeof(int32_t)},
        {&id.h_count, count, nullptr, N * sizeof(int32_t)},
        {&id.h_flags, in_place ? nullptr : flags_in, nullptr, N * MD * sizeof(uint32_t)},
        {&id.h_who, who, who, N * MD * sizeof(uint32_t)},
        {&id.h_identity, identity, identity, N * MD * sizeof(int32_t)},
        {&id.h_id_score, id_score, id_score, N * MD * sizeof(float)},
    };
    constexpr size_t K = sizeof twins / sizeof twins[0];
    RFD_TRY(twins_up(twins, K, s));
    auto dev = [&](int i) -> void * { return twins[i].in ? twins[i].dev->p : nullptr; };
    const uint32_t *d_flags = in_place ? (const uint32_t *)dev(3) : (const uint32_t *)dev(2); // in place on the device as well
    RFD_TRY(who_enqueue(t, stream, n, (const int32_t *)dev(0), (const int32_t *)dev(1), d_flags, (uint32_t *)dev(3), (int32_t *)dev(4),
                        (float *)dev(5)));
    return twins_back(twins, K, s);
}

// the slots and heads of a stream on the host, after the stream has drained
static int identity_read_stream(rfd_tracker *t, int stream, std::vector<TrackSlot> &slots, std::vector<TrackIdHead> &heads)
{
    RFD_CHECK_ARG(t != nullptr, "tracker is null");
    if (!t->ident.enabled) { set_error("invalid argument: track identities are not enabled on this tracker (rfd_tracker_identity_enable)"); return RFD_ERR_INVALID_ARG; }
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
    RFD_HIP(hipMemcpyAsync(heads.data(), (const TrackIdHead *)t->ident.heads.p + (size_t)stream * mt, mt * sizeof(TrackIdHead), hipMemcpyDeviceToHost, s));
    RFD_HIP(hipStreamSynchronize(s));
    return RFD_OK;
}

int rfd_tracker_get_identities(rfd_tracker *t, int stream, rfd_track_identity *out, int cap, int *count)
{
    RFD_CHECK_ARG(t != nullptr, "tracker is null");
    RFD_CHECK_ARG(count != nullptr, "count is null");
    RFD_CHECK_ARG(cap >= 0 && (out || cap == 0), "out is null with a cap");
    std::vector<TrackSlot> slots;
    std::vector<TrackIdHead> heads;
    RFD_TRY(identity_read_stream(t, stream, slots, heads));
    int live = 0;
    for (int i = 0; i < t->cfg.max_tracks; ++i) {
        const TrackIdHead &h = heads[(size_t)i];
        if (slots[(size_t)i].serial == 0 || h.serial != slots[(size_t)i].serial) continue;
        if (live < cap) {
            rfd_track_identity &o = out[live];
            o.slot = i; o.serial = h.serial; o.identity = h.identity; o.row = h.row; o.score = h.score;
            o.named = h.named; o.shots = h.shots; o.weight = h.weight;
        }
        ++live;
    }
    *count = live;
    return RFD_OK;
}

int rfd_tracker_get_template(rfd_tracker *t, int stream, int32_t serial, float *out)
{
    RFD_CHECK_ARG(t != nullptr, "tracker is null");
    RFD_CHECK_ARG(out != nullptr, "out is null");
    std::vector<TrackSlot> slots;
    std::vector<TrackIdHead> heads;
    RFD_TRY(identity_read_stream(t, stream, slots, heads));
    int slot = -1;
    for (int i = 0; i < t->cfg.max_tracks && slot < 0 && serial != 0; ++i)
        if (slots[(size_t)i].serial == serial) slot = i;
    if (slot < 0 || heads[(size_t)slot].serial != serial) {
        set_error("invalid argument: no such track: stream %d has no fused track with serial %d", stream, serial);
        return RFD_ERR_INVALID_ARG;
    }
    const size_t dim = (size_t)t->ident.cfg.dim;
    const float *src = (const float *)t->ident.templates.p + ((size_t)stream * t->cfg.max_tracks + slot) * dim;
    RFD_HIP(hipMemcpyAsync(out, src, dim * sizeof(float), hipMemcpyDeviceToHost, ctx_stream(t->ctx)));
    RFD_HIP(hipStreamSynchronize(ctx_stream(t->ctx)));
    return RFD_OK;
}
