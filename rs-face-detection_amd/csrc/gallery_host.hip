// gallery_host.hip -- the host side of the face gallery (include/rfd.h, "gallery"): every rfd_gallery_* entry.  What a call
// changes in the bookkeeping is decided by the gallery's GalleryBook (gallery_book.h); this file checks the arguments, enqueues
// the copies and the kernels of kernels_gallery.hip and kernels_gallery_nearest.hip (as gallery_nearest_plan.h plans them) on
// the context's stream, and reads and writes the gallery file (gallery_file.h).
#include "gallery_host.h"

#include <algorithm>
#include <functional>
#include <memory>
#include <string>

#include "gallery_file.h"
#include "kernels.h"

using namespace rfd;

static int gallery_host_stage(rfd_gallery *g)
{
    if (g->pin) return RFD_OK;
    RFD_TRY(g->stage.reserve(rfd_gallery::kStageBytes));
    return g->pin.alloc(rfd_gallery::kStageBytes);
}

// The host forms move rows of `dim` floats through the one staging buffer, in chunks that fit it; a chunk has left the buffer
// (the stream is drained) before the next one enters.  With `src`, rows [first, first + count) of it are copied in before
// `op(first, count)` is enqueued; with `dst`, op fills the device buffer and the rows are copied out behind it.
static int gallery_staged(rfd_gallery *g, const float *src, float *dst, int n, const std::function<int(int, int)> &op)
{
    RFD_TRY(gallery_host_stage(g));
    const hipStream_t s = ctx_stream(g->ctx);
    const int dim = g->book.dim(), chunk = (int)(rfd_gallery::kStageBytes / ((size_t)dim * sizeof(float)));
    for (int i = 0; i < n; i += chunk) {
        const int m = std::min(chunk, n - i);
        const size_t bytes = (size_t)m * dim * sizeof(float);
        if (src) {
            memcpy(g->pin, src + (size_t)i * dim, bytes);
            RFD_HIP(hipMemcpyAsync(g->stage.p, g->pin, bytes, hipMemcpyHostToDevice, s));
        }
        RFD_TRY(op(i, m));
        if (dst) RFD_HIP(hipMemcpyAsync(g->pin, g->stage.p, bytes, hipMemcpyDeviceToHost, s));
        RFD_HIP(hipStreamSynchronize(s));
        if (dst) memcpy(dst + (size_t)i * dim, g->pin, bytes);
    }
    return RFD_OK;
}

// ---- argument checks: those of the values here, those of the rows in the book ----
// first non-finite value of x [n][dim], named in the error message (`what` = "row" / "query")
static int gallery_check_finite(const float *x, int n, int dim, const char *what)
{
    for (int i = 0; i < n; ++i)
        for (int d = 0; d < dim; ++d) {
            uint32_t u;
            memcpy(&u, &x[(size_t)i * dim + d], 4);
            if ((u & 0x7f800000u) == 0x7f800000u) {
                set_error("invalid argument: %s %d holds a non-finite value (%g) at element %d", what, i, (double)x[(size_t)i * dim + d], d);
                return RFD_ERR_INVALID_ARG;
            }
        }
    return RFD_OK;
}

static int gallery_check_k(int k)
{
    RFD_CHECK_ARG(k >= 1, "k < 1");
    if (k > RFD_GALLERY_MAX_K) { set_error("k = %d exceeds RFD_GALLERY_MAX_K (%d)", k, RFD_GALLERY_MAX_K); return RFD_ERR_CAPACITY; }
    return RFD_OK;
}

static int gallery_check_min_score(float min_score)
{
    RFD_CHECK_ARG(min_score == min_score, "min_score is NaN");
    return RFD_OK;
}

// the status of a check of the book; what it refused becomes the call's error
static int book_status(int st, const char *msg)
{
    if (st != RFD_OK) set_error("%s", msg);
    return st;
}
static int gallery_check_room(const rfd_gallery *g, int n) { char msg[256]; return book_status(g->book.check_room(n, msg, sizeof msg), msg); }
static int gallery_check_rows(const rfd_gallery *g, const int32_t *rows, int n) { char msg[256]; return book_status(g->book.check_rows(rows, n, msg, sizeof msg), msg); }
static int gallery_check_distinct(const int32_t *rows, int n) { char msg[256]; return book_status(GalleryBook::check_distinct(rows, n, msg, sizeof msg), msg); }
static int gallery_check_identities(const rfd_gallery *g, const int32_t *rows, const int32_t *ids, int n)
{
    char msg[256];
    return book_status(g->book.check_identities(rows, ids, n, msg, sizeof msg), msg);
}
static int gallery_check_tags(const rfd_gallery *g, const int32_t *rows, int n) { char msg[256]; return book_status(g->book.check_tags(rows, n, msg, sizeof msg), msg); }

// ---- the device's live words and the row lists ----
// brings the device's live words up to the rows added since they were last written or read
static int gallery_live_sync(rfd_gallery *g, hipStream_t s)
{
    const GalleryBook::Rows behind = g->book.unsynced();
    if (!behind.empty()) RFD_TRY(launch_gallery_live_range((uint16_t *)g->live.p, behind.row0, behind.row1, s));
    g->book.mark_synced();
    return RFD_OK;
}

// what a search passes for `live`: null while no row is removed (the scan without the mask), else the device's words
static int gallery_search_mask(rfd_gallery *g, hipStream_t s, const uint16_t **live)
{
    *live = nullptr;
    if (g->book.removed() == 0) return RFD_OK;
    RFD_TRY(gallery_live_sync(g, s));
    *live = (const uint16_t *)g->live.p;
    return RFD_OK;
}

// the ring of page-locked list slots and their device twin, allocated by the first call that sends a list
static int gallery_edit_lists(rfd_gallery *g)
{
    RFD_TRY(g->edit_ring.ensure((size_t)kEditInts * sizeof(int32_t)));
    return g->edit.reserve((size_t)kEditInts * sizeof(int32_t));
}

// Rows `rows` (host, checked) take bf16(emb[i]) and become live (emb: device [n][dim]), or are erased and become removed (emb
// null).  Enqueued in chunks of kEditRows, each planned by the book into the next ring slot; no synchronisation with the stream.
static int gallery_edit(rfd_gallery *g, const int32_t *rows, const float *emb, int n)
{
    const hipStream_t s = ctx_stream(g->ctx);
    const int dim = g->book.dim();
    RFD_TRY(gallery_edit_lists(g)); // first call on this gallery
    RFD_TRY(gallery_live_sync(g, s));
    for (int at = 0; at < n; at += kEditRows) {
        int32_t *slot;
        RFD_TRY(g->edit_ring.acquire(&slot));
        const GalleryEditPlan p = g->book.plan_edit(rows + at, std::min(kEditRows, n - at), emb != nullptr, slot);
        RFD_HIP(hipMemcpyAsync(g->edit.p, slot, (size_t)p.ints() * sizeof(int32_t), hipMemcpyHostToDevice, s));
        RFD_TRY(g->edit_ring.record(s));
        const int32_t *d = (const int32_t *)g->edit.p, *blk = d + p.m, *word = blk + p.nb, *unlabel = word + p.nb;
        RFD_TRY(launch_gallery_put(emb ? emb + (size_t)at * dim : nullptr, d, p.m, dim, (bf16_t *)g->store.p, blk, word, p.nb, (uint16_t *)g->live.p, s));
        if (p.nu > 0) RFD_TRY(launch_gallery_set_identities((int32_t *)g->ids.p, unlabel, nullptr, p.nu, s));
        if (!emb && g->tags.p) RFD_TRY(launch_gallery_set_tags((uint32_t *)g->tags.p, d, nullptr, p.m, s)); // a removed row's tag is 0
    }
    return RFD_OK;
}

int64_t rfd_debug_gallery_offset(int dim, int row, int d)
{
    if (dim < 32 || dim > 1024 || dim % 32 != 0 || row < 0 || d < 0 || d >= dim) return -1;
    return (int64_t)gallery_offset(dim, row, d);
}

// ---- create, destroy, size, clear ----
int rfd_gallery_create(rfd_ctx *c, int dim, int capacity, rfd_gallery **out)
{
    RFD_CHECK_ARG(c && out, "null argument");
    *out = nullptr;
    RFD_CHECK_ARG(dim >= 32 && dim <= 1024 && dim % 32 == 0, "dim must be a multiple of 32 in 32..1024");
    RFD_CHECK_ARG(capacity >= 1 && capacity <= (1 << 30), "capacity out of range");
    RFD_HIP(hipSetDevice(ctx_device(c)));
    const hipStream_t s = ctx_stream(c);
    std::unique_ptr<rfd_gallery> g(new rfd_gallery()); // an early return frees whatever was built so far
    g->ctx = c;
    g->book.init(dim, capacity);
    g->cus = device_cus();
    g->groups_max = 2 * g->cus; // two workgroups of four waves per CU: what the scan's registers admit
    const size_t bytes = (size_t)ceil_div(capacity, 16) * 16 * dim * sizeof(bf16_t);
    RFD_TRY(g->store.reserve(bytes));
    RFD_TRY(g->ws.reserve((size_t)g->groups_max * kGalleryMaxQueries * RFD_GALLERY_MAX_K * sizeof(uint2)));
    const size_t live_bytes = (size_t)ceil_div(ceil_div(capacity, 16), 2) * 2 * sizeof(uint16_t); // the masked scan loads aligned pairs of words
    RFD_TRY(g->live.reserve(live_bytes));
    // rows that were never added read as zeros (the tail of the last block is scored, then masked by its row index)
    if (hipMemsetAsync(g->store.p, 0, bytes, s) != hipSuccess || hipMemsetAsync(g->live.p, 0, live_bytes, s) != hipSuccess) {
        set_error("hipMemsetAsync of the gallery failed");
        (void)hipStreamSynchronize(s); // a fill that was enqueued has run before its buffer is freed
        return RFD_ERR_HIP;
    }
    *out = g.release();
    return RFD_OK;
}

void rfd_gallery_destroy(rfd_gallery *g)
{
    if (!g) return;
    (void)hipSetDevice(ctx_device(g->ctx));
    (void)hipStreamSynchronize(ctx_stream(g->ctx));
    delete g;
}

int rfd_gallery_size(const rfd_gallery *g, int *rows, int *capacity, int *dim)
{
    RFD_CHECK_ARG(g, "gallery is null");
    if (rows) *rows = g->book.rows();
    if (capacity) *capacity = g->book.capacity();
    if (dim) *dim = g->book.dim();
    return RFD_OK;
}

int rfd_gallery_clear(rfd_gallery *g)
{
    RFD_CHECK_ARG(g, "gallery is null");
    RFD_HIP(hipSetDevice(ctx_device(g->ctx)));
    const hipStream_t s = ctx_stream(g->ctx);
    const int rows = g->book.rows(), synced = g->book.unsynced().row0;
    if (rows > 0) RFD_HIP(hipMemsetAsync(g->store.p, 0, (size_t)ceil_div(rows, 16) * 16 * g->book.dim() * sizeof(bf16_t), s));
    if (synced > 0) RFD_HIP(hipMemsetAsync(g->live.p, 0, (size_t)ceil_div(synced, 16) * sizeof(uint16_t), s));
    if (g->ids.p && rows > 0) RFD_HIP(hipMemsetAsync(g->ids.p, 0xff, (size_t)rows * sizeof(int32_t), s)); // all -1 again
    if (g->tags.p && rows > 0) RFD_HIP(hipMemsetAsync(g->tags.p, 0, (size_t)rows * sizeof(uint32_t), s));
    g->book.clear();
    return RFD_OK;
}

// ---- add, get ----
int rfd_gallery_add_device(rfd_gallery *g, const float *emb, int n, int *first_row)
{
    RFD_CHECK_ARG(g && n >= 0, "gallery is null or n < 0");
    if (first_row) *first_row = g->book.rows();
    if (n == 0) return RFD_OK;
    RFD_CHECK_ARG(emb && (uintptr_t)emb % 16 == 0, "emb is null or not 16-byte aligned");
    RFD_TRY(gallery_check_room(g, n));
    RFD_HIP(hipSetDevice(ctx_device(g->ctx)));
    RFD_TRY(launch_gallery_add(emb, n, g->book.dim(), g->book.rows(), (bf16_t *)g->store.p, ctx_stream(g->ctx)));
    g->book.add(n);
    return RFD_OK;
}

int rfd_gallery_add(rfd_gallery *g, const float *emb, int n, int *first_row)
{
    RFD_CHECK_ARG(g && n >= 0, "gallery is null or n < 0");
    if (first_row) *first_row = g->book.rows();
    if (n == 0) return RFD_OK;
    RFD_CHECK_ARG(emb, "emb is null");
    RFD_TRY(gallery_check_room(g, n));
    RFD_TRY(gallery_check_finite(emb, n, g->book.dim(), "row"));
    RFD_HIP(hipSetDevice(ctx_device(g->ctx)));
    RFD_TRY(gallery_staged(g, emb, nullptr, n, [&](int i, int m) {
        return launch_gallery_add((const float *)g->stage.p, m, g->book.dim(), g->book.rows() + i, (bf16_t *)g->store.p, ctx_stream(g->ctx));
    }));
    g->book.add(n);
    return RFD_OK;
}

int rfd_gallery_get_rows(rfd_gallery *g, int row0, int n, float *out)
{
    RFD_CHECK_ARG(g && n >= 0, "gallery is null or n < 0");
    if (n == 0) return RFD_OK;
    RFD_CHECK_ARG(out, "out is null");
    RFD_CHECK_ARG(row0 >= 0 && n <= g->book.rows() - row0, "rows [row0, row0 + n) are not all in the gallery");
    RFD_HIP(hipSetDevice(ctx_device(g->ctx)));
    return gallery_staged(g, nullptr, out, n, [&](int i, int m) {
        return launch_gallery_get((const bf16_t *)g->store.p, row0 + i, m, g->book.dim(), (float *)g->stage.p, ctx_stream(g->ctx));
    });
}

// the first tags of a gallery, or its first filtered search: the device array, all zero, in stream order ahead of every use
static int gallery_tag_array(rfd_gallery *g, hipStream_t s)
{
    if (g->tags.p) return RFD_OK;
    const size_t bytes = (size_t)ceil_div(g->book.capacity(), 16) * 16 * sizeof(uint32_t); // whole blocks: the scan reads a block's 16 words
    RFD_TRY(g->tags.reserve(bytes));
    if (hipMemsetAsync(g->tags.p, 0, bytes, s) != hipSuccess) {
        set_error("hipMemsetAsync of the gallery's tags failed");
        (void)hipStreamSynchronize(s);
        g->tags.release();
        return RFD_ERR_HIP;
    }
    return RFD_OK;
}

// ---- search: the k best rows, or with `ids` (rfd.h, "identities") the k best identities, or with a filter (rfd.h, "tags") the
//      k best identities among each query's eligible rows, in both forms of each ----
// the filter of the queries of a call or of a pass: one mask and one value per query, on the device; null: no filter
struct GalleryFilter {
    const uint32_t *mask = nullptr, *value = nullptr;
    explicit operator bool() const { return mask != nullptr; }
    GalleryFilter from(int i) const { return mask ? GalleryFilter{mask + i, value + i} : GalleryFilter{}; }
};

// one pass over the gallery for m <= kGalleryMaxQueries queries on the device; results on the device
static int gallery_search_pass(rfd_gallery *g, hipStream_t s, const uint16_t *live, const float *queries, int m, int k, float min_score, float *scores,
                               int32_t *rows, int32_t *ids, GalleryFilter f = {})
{
    const GalleryBook &b = g->book;
    if (f)
        return launch_gallery_search_filtered((const bf16_t *)g->store.p, live, (const int32_t *)g->ids.p, (const uint32_t *)g->tags.p, f.mask, f.value, b.rows(),
                                              b.dim(), queries, m, k, min_score, (uint2 *)g->ws.p, g->groups_max, scores, rows, ids, s);
    if (!ids) return launch_gallery_search((const bf16_t *)g->store.p, live, b.rows(), b.dim(), queries, m, k, (uint2 *)g->ws.p, g->groups_max, scores, rows, s);
    return launch_gallery_search_identities((const bf16_t *)g->store.p, live, (const int32_t *)g->ids.p, b.rows(), b.dim(), queries, m, k, min_score,
                                            (uint2 *)g->ws.p, g->groups_max, scores, rows, ids, s);
}

// n >= 1 queries and their results on the device; ids null: the rows alone; f: device lists of n
static int gallery_search_device(rfd_gallery *g, const float *queries, int n, int k, float min_score, float *scores, int32_t *rows, int32_t *ids, int async,
                                 GalleryFilter f = {})
{
    RFD_CHECK_ARG((uintptr_t)queries % 16 == 0, "queries are not 16-byte aligned");
    RFD_HIP(hipSetDevice(ctx_device(g->ctx)));
    const hipStream_t s = ctx_stream(g->ctx);
    const uint16_t *live = nullptr;
    RFD_TRY(gallery_search_mask(g, s, &live));
    if (f) RFD_TRY(gallery_tag_array(g, s));
    for (int i = 0; i < n; i += kGalleryMaxQueries) // one pass over the gallery per group of queries; the passes share the workspace in stream order
        RFD_TRY(gallery_search_pass(g, s, live, queries + (size_t)i * g->book.dim(), std::min(kGalleryMaxQueries, n - i), k, min_score, scores + (size_t)i * k,
                                    rows + (size_t)i * k, ids ? ids + (size_t)i * k : nullptr, f.from(i)));
    if (!async) RFD_HIP(hipStreamSynchronize(s));
    return RFD_OK;
}

// n >= 1 queries and their results on the host; ids null: the rows alone; f: host lists of n
static int gallery_search_host(rfd_gallery *g, const float *queries, int n, int k, float min_score, float *scores, int32_t *rows, int32_t *ids,
                               GalleryFilter f = {})
{
    const int dim = g->book.dim();
    RFD_TRY(gallery_check_finite(queries, n, dim, "query"));
    RFD_HIP(hipSetDevice(ctx_device(g->ctx)));
    const hipStream_t s = ctx_stream(g->ctx);
    RFD_TRY(gallery_host_stage(g));
    const uint16_t *live = nullptr;
    RFD_TRY(gallery_search_mask(g, s, &live));
    if (f) RFD_TRY(gallery_tag_array(g, s));
    // the staging buffer holds one group: its queries (with a filter: and behind them its masks | values, in the same copy), then
    // its scores, its rows and (with ids) its identities
    const size_t fcap = f ? (size_t)kGalleryMaxQueries * 2 * sizeof(uint32_t) : 0;
    const size_t qcap = (size_t)kGalleryMaxQueries * dim * sizeof(float) + fcap, rcap = (size_t)kGalleryMaxQueries * RFD_GALLERY_MAX_K * sizeof(float);
    char *d = (char *)g->stage.p, *h = (char *)g->pin;
    float *d_q = (float *)d, *d_s = (float *)(d + qcap);
    int32_t *d_r = (int32_t *)(d + qcap + rcap), *d_i = ids ? (int32_t *)(d + qcap + 2 * rcap) : nullptr;
    for (int i = 0; i < n; i += kGalleryMaxQueries) {
        const int m = std::min(kGalleryMaxQueries, n - i);
        const size_t qbytes = (size_t)m * dim * sizeof(float), rbytes = (size_t)m * k * sizeof(float);
        const size_t fbytes = f ? (size_t)m * sizeof(uint32_t) : 0;
        memcpy(h, queries + (size_t)i * dim, qbytes);
        if (f) {
            memcpy(h + qbytes, f.mask + i, fbytes);
            memcpy(h + qbytes + fbytes, f.value + i, fbytes);
        }
        RFD_HIP(hipMemcpyAsync(d_q, h, qbytes + 2 * fbytes, hipMemcpyHostToDevice, s));
        const uint32_t *d_f = (const uint32_t *)(d + qbytes);
        RFD_TRY(gallery_search_pass(g, s, live, d_q, m, k, min_score, d_s, d_r, d_i, f ? GalleryFilter{d_f, d_f + m} : GalleryFilter{}));
        if (ids) {
            RFD_HIP(hipMemcpyAsync(h + qcap, d_s, 3 * rcap, hipMemcpyDeviceToHost, s)); // the three results lie side by side
        } else {
            RFD_HIP(hipMemcpyAsync(h + qcap, d_s, rbytes, hipMemcpyDeviceToHost, s));
            RFD_HIP(hipMemcpyAsync(h + qcap + rcap, d_r, rbytes, hipMemcpyDeviceToHost, s));
        }
        RFD_HIP(hipStreamSynchronize(s));
        memcpy(scores + (size_t)i * k, h + qcap, rbytes);
        memcpy(rows + (size_t)i * k, h + qcap + rcap, rbytes);
        if (ids) memcpy(ids + (size_t)i * k, h + qcap + 2 * rcap, rbytes);
    }
    return RFD_OK;
}

int rfd_gallery_search_device(rfd_gallery *g, const float *queries, int n, int k, float *scores, int32_t *rows, int async)
{
    RFD_CHECK_ARG(g && n >= 0, "gallery is null or n < 0");
    RFD_TRY(gallery_check_k(k));
    if (n == 0) return RFD_OK;
    RFD_CHECK_ARG(queries && scores && rows, "null argument");
    return gallery_search_device(g, queries, n, k, 0.f, scores, rows, nullptr, async);
}

int rfd_gallery_search(rfd_gallery *g, const float *queries, int n, int k, float *scores, int32_t *rows)
{
    RFD_CHECK_ARG(g && n >= 0, "gallery is null or n < 0");
    RFD_TRY(gallery_check_k(k));
    if (n == 0) return RFD_OK;
    RFD_CHECK_ARG(queries && scores && rows, "null argument");
    return gallery_search_host(g, queries, n, k, 0.f, scores, rows, nullptr);
}

int rfd_gallery_search_identities_device(rfd_gallery *g, const float *queries, int n, int k, float min_score, float *scores, int32_t *rows, int32_t *ids,
                                         int async)
{
    RFD_CHECK_ARG(g && n >= 0, "gallery is null or n < 0");
    RFD_TRY(gallery_check_k(k));
    RFD_TRY(gallery_check_min_score(min_score));
    if (n == 0) return RFD_OK;
    RFD_CHECK_ARG(queries && scores && rows && ids, "null argument");
    return gallery_search_device(g, queries, n, k, min_score, scores, rows, ids, async);
}

int rfd_gallery_search_identities(rfd_gallery *g, const float *queries, int n, int k, float min_score, float *scores, int32_t *rows, int32_t *ids)
{
    RFD_CHECK_ARG(g && n >= 0, "gallery is null or n < 0");
    RFD_TRY(gallery_check_k(k));
    RFD_TRY(gallery_check_min_score(min_score));
    if (n == 0) return RFD_OK;
    RFD_CHECK_ARG(queries && scores && rows && ids, "null argument");
    return gallery_search_host(g, queries, n, k, min_score, scores, rows, ids);
}

int rfd_gallery_search_filtered_device(rfd_gallery *g, const float *queries, int n, int k, float min_score, const uint32_t *mask, const uint32_t *value,
                                       float *scores, int32_t *rows, int32_t *ids, int async)
{
    RFD_CHECK_ARG(g && n >= 0, "gallery is null or n < 0");
    RFD_TRY(gallery_check_k(k));
    RFD_TRY(gallery_check_min_score(min_score));
    if (n == 0) return RFD_OK;
    RFD_CHECK_ARG(queries && scores && rows && ids, "null argument");
    RFD_CHECK_ARG(mask && value, "mask or value is null");
    return gallery_search_device(g, queries, n, k, min_score, scores, rows, ids, async, GalleryFilter{mask, value});
}

int rfd_gallery_search_filtered(rfd_gallery *g, const float *queries, int n, int k, float min_score, const uint32_t *mask, const uint32_t *value, float *scores,
                                int32_t *rows, int32_t *ids)
{
    RFD_CHECK_ARG(g && n >= 0, "gallery is null or n < 0");
    RFD_TRY(gallery_check_k(k));
    RFD_TRY(gallery_check_min_score(min_score));
    if (n == 0) return RFD_OK;
    RFD_CHECK_ARG(queries && scores && rows && ids, "null argument");
    RFD_CHECK_ARG(mask && value, "mask or value is null");
    return gallery_search_host(g, queries, n, k, min_score, scores, rows, ids, GalleryFilter{mask, value});
}

// ---- remove and replace (rfd.h, "remove and replace") ----
int rfd_gallery_remove(rfd_gallery *g, const int32_t *rows, int n)
{
    RFD_CHECK_ARG(g && n >= 0, "gallery is null or n < 0");
    if (n == 0) return RFD_OK;
    RFD_CHECK_ARG(rows, "rows is null");
    RFD_TRY(gallery_check_rows(g, rows, n));
    RFD_HIP(hipSetDevice(ctx_device(g->ctx)));
    return gallery_edit(g, rows, nullptr, n);
}

int rfd_gallery_replace_device(rfd_gallery *g, const int32_t *rows, const float *emb, int n)
{
    RFD_CHECK_ARG(g && n >= 0, "gallery is null or n < 0");
    if (n == 0) return RFD_OK;
    RFD_CHECK_ARG(rows, "rows is null");
    RFD_CHECK_ARG(emb && (uintptr_t)emb % 16 == 0, "emb is null or not 16-byte aligned");
    RFD_TRY(gallery_check_rows(g, rows, n));
    RFD_TRY(gallery_check_distinct(rows, n));
    RFD_HIP(hipSetDevice(ctx_device(g->ctx)));
    return gallery_edit(g, rows, emb, n);
}

int rfd_gallery_replace(rfd_gallery *g, const int32_t *rows, const float *emb, int n)
{
    RFD_CHECK_ARG(g && n >= 0, "gallery is null or n < 0");
    if (n == 0) return RFD_OK;
    RFD_CHECK_ARG(rows && emb, "rows or emb is null");
    RFD_TRY(gallery_check_rows(g, rows, n));
    RFD_TRY(gallery_check_distinct(rows, n));
    RFD_TRY(gallery_check_finite(emb, n, g->book.dim(), "row"));
    RFD_HIP(hipSetDevice(ctx_device(g->ctx)));
    return gallery_staged(g, emb, nullptr, n, [&](int i, int m) { return gallery_edit(g, rows + i, (const float *)g->stage.p, m); });
}

int rfd_gallery_live(const rfd_gallery *g, int *live_rows)
{
    RFD_CHECK_ARG(g && live_rows, "null argument");
    *live_rows = g->book.rows() - g->book.removed();
    return RFD_OK;
}

int rfd_gallery_removed(const rfd_gallery *g, int32_t *out, int cap, int *count)
{
    RFD_CHECK_ARG(g && count && cap >= 0 && (out || cap == 0), "null argument or cap < 0");
    *count = g->book.removed();
    (void)g->book.removed_rows(out, cap);
    return RFD_OK;
}

// ---- identities (rfd.h, "identities") ----
// the first labels of a gallery: the device array, all unlabelled, in stream order ahead of every use
static int gallery_identity_array(rfd_gallery *g, hipStream_t s)
{
    if (g->ids.p) return RFD_OK;
    const size_t bytes = (size_t)ceil_div(g->book.capacity(), 16) * 16 * sizeof(int32_t); // whole blocks: the scan reads a block's 16 words
    RFD_TRY(g->ids.reserve(bytes));
    if (hipMemsetAsync(g->ids.p, 0xff, bytes, s) != hipSuccess) {
        set_error("hipMemsetAsync of the gallery's identities failed");
        (void)hipStreamSynchronize(s);
        g->ids.release();
        return RFD_ERR_HIP;
    }
    return RFD_OK;
}

int rfd_gallery_set_identities(rfd_gallery *g, const int32_t *rows, const int32_t *ids, int n)
{
    RFD_CHECK_ARG(g && n >= 0, "gallery is null or n < 0");
    if (n == 0) return RFD_OK;
    RFD_CHECK_ARG(rows && ids, "rows or ids is null");
    RFD_TRY(gallery_check_rows(g, rows, n));
    RFD_TRY(gallery_check_identities(g, rows, ids, n));
    RFD_TRY(gallery_check_distinct(rows, n));
    RFD_HIP(hipSetDevice(ctx_device(g->ctx)));
    const hipStream_t s = ctx_stream(g->ctx);
    RFD_TRY(gallery_edit_lists(g));
    RFD_TRY(gallery_identity_array(g, s));
    for (int at = 0; at < n; at += kEditRows) {
        const int m = std::min(kEditRows, n - at);
        int32_t *slot;
        RFD_TRY(g->edit_ring.acquire(&slot));
        g->book.plan_identities(rows + at, ids + at, m, slot);
        RFD_HIP(hipMemcpyAsync(g->edit.p, slot, (size_t)2 * m * sizeof(int32_t), hipMemcpyHostToDevice, s));
        RFD_TRY(g->edit_ring.record(s));
        const int32_t *d = (const int32_t *)g->edit.p;
        RFD_TRY(launch_gallery_set_identities((int32_t *)g->ids.p, d, d + m, m, s));
    }
    return RFD_OK;
}

int rfd_gallery_get_identities(const rfd_gallery *g, int row0, int n, int32_t *out)
{
    RFD_CHECK_ARG(g && n >= 0, "gallery is null or n < 0");
    if (n == 0) return RFD_OK;
    RFD_CHECK_ARG(out, "out is null");
    RFD_CHECK_ARG(row0 >= 0 && n <= g->book.rows() - row0, "rows [row0, row0 + n) are not all in the gallery");
    g->book.identities(row0, n, out);
    return RFD_OK;
}

int rfd_gallery_identities(const rfd_gallery *g, int *labelled_rows)
{
    RFD_CHECK_ARG(g && labelled_rows, "null argument");
    *labelled_rows = g->book.labelled();
    return RFD_OK;
}

// ---- tags (rfd.h, "tags") ----
int rfd_gallery_set_tags(rfd_gallery *g, const int32_t *rows, const uint32_t *tags, int n)
{
    RFD_CHECK_ARG(g && n >= 0, "gallery is null or n < 0");
    if (n == 0) return RFD_OK;
    RFD_CHECK_ARG(rows && tags, "rows or tags is null");
    RFD_TRY(gallery_check_rows(g, rows, n));
    RFD_TRY(gallery_check_tags(g, rows, n));
    RFD_TRY(gallery_check_distinct(rows, n));
    RFD_HIP(hipSetDevice(ctx_device(g->ctx)));
    const hipStream_t s = ctx_stream(g->ctx);
    RFD_TRY(gallery_edit_lists(g));
    RFD_TRY(gallery_tag_array(g, s));
    for (int at = 0; at < n; at += kEditRows) {
        const int m = std::min(kEditRows, n - at);
        int32_t *slot;
        RFD_TRY(g->edit_ring.acquire(&slot));
        g->book.plan_tags(rows + at, tags + at, m, slot);
        RFD_HIP(hipMemcpyAsync(g->edit.p, slot, (size_t)2 * m * sizeof(int32_t), hipMemcpyHostToDevice, s));
        RFD_TRY(g->edit_ring.record(s));
        const int32_t *d = (const int32_t *)g->edit.p;
        RFD_TRY(launch_gallery_set_tags((uint32_t *)g->tags.p, d, (const uint32_t *)(d + m), m, s));
    }
    return RFD_OK;
}

int rfd_gallery_get_tags(const rfd_gallery *g, int row0, int n, uint32_t *out)
{
    RFD_CHECK_ARG(g && n >= 0, "gallery is null or n < 0");
    if (n == 0) return RFD_OK;
    RFD_CHECK_ARG(out, "out is null");
    RFD_CHECK_ARG(row0 >= 0 && n <= g->book.rows() - row0, "rows [row0, row0 + n) are not all in the gallery");
    g->book.tags(row0, n, out);
    return RFD_OK;
}

// ---- nearest (rfd.h, "nearest"; gallery_nearest_plan.h, kernels_gallery_nearest.hip) ----
void rfd_gallery_nearest_config_default(rfd_gallery_nearest_config *cfg)
{
    if (!cfg) return;
    memset(cfg, 0, sizeof *cfg);
    cfg->mode = RFD_GALLERY_NEAREST_OTHER_ROW;
    cfg->min_score = -INFINITY;
    cfg->tag_mask = 0u;
}

int rfd_debug_gallery_nearest_plan(int rows, int row0, int n, int dim, int cus, rfd_gallery_nearest_plan *out)
{
    RFD_CHECK_ARG(out, "out is null");
    memset(out, 0, sizeof *out);
    RFD_CHECK_ARG(dim >= 32 && dim <= 1024 && dim % 32 == 0, "dim must be a multiple of 32 in 32..1024");
    RFD_CHECK_ARG(rows >= 0 && row0 >= 0 && n >= 0 && n <= rows - row0 && cus >= 1, "rows [row0, row0 + n) are not all in the gallery, or cus < 1");
    const GalleryNearestPlan p = gallery_nearest_plan(rows, row0, n, dim, cus); // n = 0: nothing to launch, grid 0
    *out = {p.form, p.tile_rows, p.tiles, p.splits, p.blocks, p.blocks_per_split, p.grid, p.ws_bytes};
    return RFD_OK;
}

// the checks of both forms, in the contract's order; *cfg: the call's configuration (the default where the caller passed none)
static int gallery_nearest_check(const rfd_gallery *g, int row0, int n, const rfd_gallery_nearest_config *in, rfd_gallery_nearest_config *cfg)
{
    RFD_CHECK_ARG(g, "gallery is null");
    RFD_CHECK_ARG(row0 >= 0 && n >= 0 && n <= g->book.rows() - row0, "rows [row0, row0 + n) are not all in the gallery");
    rfd_gallery_nearest_config_default(cfg);
    if (in) *cfg = *in;
    RFD_CHECK_ARG(cfg->mode == RFD_GALLERY_NEAREST_OTHER_ROW || cfg->mode == RFD_GALLERY_NEAREST_OTHER_IDENTITY, "unknown mode");
    for (int i = 0; i < 5; ++i) RFD_CHECK_ARG(cfg->reserved[i] == 0, "a reserved word is not 0");
    return RFD_OK;
}

static int gallery_nearest_outputs(const float *scores, const int32_t *rows, const int32_t *ids)
{
    RFD_CHECK_ARG(scores && rows, "scores or rows is null");
    RFD_CHECK_ARG((uintptr_t)scores % 4 == 0 && (uintptr_t)rows % 4 == 0 && (uintptr_t)ids % 4 == 0, "an output is not 4-byte aligned");
    return RFD_OK;
}

// rows [row0, row0 + n), n >= 1, checked: the scan and the merge on the stream, outputs on the device
static int gallery_nearest_enqueue(rfd_gallery *g, hipStream_t s, int row0, int n, const rfd_gallery_nearest_config &cfg, float *scores, int32_t *rows,
                                   int32_t *ids)
{
    const GalleryBook &b = g->book;
    RFD_TRY(g->nearest_ws.reserve((size_t)gallery_nearest_ws_bound(b.capacity(), b.dim(), g->cus))); // first call on this gallery
    const uint16_t *live = nullptr;
    RFD_TRY(gallery_search_mask(g, s, &live));
    const GalleryNearestPlan plan = gallery_nearest_plan(b.rows(), row0, n, b.dim(), g->cus);
    return launch_gallery_nearest((const bf16_t *)g->store.p, live, (const int32_t *)g->ids.p, (const uint32_t *)g->tags.p, b.rows(), b.dim(), row0, n, cfg.mode,
                                  cfg.min_score, cfg.tag_mask, plan, (uint2 *)g->nearest_ws.p, scores, rows, ids, s);
}

int rfd_gallery_nearest_device(rfd_gallery *g, int row0, int n, const rfd_gallery_nearest_config *cfg, float *scores, int32_t *rows, int32_t *ids, int async)
{
    rfd_gallery_nearest_config c;
    RFD_TRY(gallery_nearest_check(g, row0, n, cfg, &c));
    if (n == 0) return RFD_OK;
    RFD_TRY(gallery_nearest_outputs(scores, rows, ids));
    RFD_HIP(hipSetDevice(ctx_device(g->ctx)));
    const hipStream_t s = ctx_stream(g->ctx);
    RFD_TRY(gallery_nearest_enqueue(g, s, row0, n, c, scores, rows, ids));
    if (!async) RFD_HIP(hipStreamSynchronize(s));
    return RFD_OK;
}

int rfd_gallery_nearest(rfd_gallery *g, int row0, int n, const rfd_gallery_nearest_config *cfg, float *scores, int32_t *rows, int32_t *ids)
{
    rfd_gallery_nearest_config c;
    RFD_TRY(gallery_nearest_check(g, row0, n, cfg, &c));
    if (n == 0) return RFD_OK;
    RFD_TRY(gallery_nearest_outputs(scores, rows, ids));
    RFD_HIP(hipSetDevice(ctx_device(g->ctx)));
    const hipStream_t s = ctx_stream(g->ctx);
    RFD_TRY(gallery_host_stage(g));
    // the staging buffer holds a chunk's scores, rows and identities side by side; a chunk has left it before the next enters
    const int chunk = (int)(rfd_gallery::kStageBytes / (3 * sizeof(float)));
    for (int i = 0; i < n; i += chunk) {
        const int m = std::min(chunk, n - i);
        const size_t bytes = (size_t)m * sizeof(float);
        float *d_s = (float *)g->stage.p;
        int32_t *d_r = (int32_t *)(d_s + m), *d_i = d_r + m;
        RFD_TRY(gallery_nearest_enqueue(g, s, row0 + i, m, c, d_s, d_r, d_i));
        RFD_HIP(hipMemcpyAsync(g->pin, g->stage.p, 3 * bytes, hipMemcpyDeviceToHost, s));
        RFD_HIP(hipStreamSynchronize(s));
        memcpy(scores + i, g->pin, bytes);
        memcpy(rows + i, g->pin + bytes, bytes);
        if (ids) memcpy(ids + i, g->pin + 2 * bytes, bytes);
    }
    return RFD_OK;
}

// ---- the gallery file (rfd.h, "gallery file"; gallery_file.h) ----
int rfd_gallery_file_info(const char *path, int *dim, int *rows, int *live)
{
    RFD_CHECK_ARG(path, "path is null");
    char msg[256];
    const int st = gallery_file_info(path, dim, rows, live, msg, sizeof msg);
    if (st != RFD_OK) set_error("%s", msg);
    return st;
}

int rfd_gallery_save(rfd_gallery *g, const char *path)
{
    RFD_CHECK_ARG(g && path, "null argument");
    RFD_HIP(hipSetDevice(ctx_device(g->ctx)));
    const hipStream_t s = ctx_stream(g->ctx);
    RFD_TRY(gallery_host_stage(g));
    RFD_HIP(hipStreamSynchronize(s));
    const std::string tmp = std::string(path) + ".tmp";
    FILE *f = fopen(tmp.c_str(), "wb");
    if (!f) { set_error("cannot open %s for writing", tmp.c_str()); return RFD_ERR_IO; }
    const int dim = g->book.dim(), rows = g->book.rows();
    bool ok = gallery_file_write_head(f, dim, rows, g->book.file_bits().data());
    int st = RFD_OK;
    const int chunk = (int)(rfd_gallery::kStageBytes / ((size_t)dim * sizeof(bf16_t)));
    for (int i = 0; ok && st == RFD_OK && i < rows; i += chunk) {
        const int m = std::min(chunk, rows - i);
        const size_t bytes = (size_t)m * dim * sizeof(bf16_t);
        st = launch_gallery_export((const bf16_t *)g->store.p, i, m, dim, (bf16_t *)g->stage.p, s);
        if (st == RFD_OK && (hipMemcpyAsync(g->pin, g->stage.p, bytes, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)) {
            set_error("copying rows %d..%d of the gallery to the host failed", i, i + m - 1);
            st = RFD_ERR_HIP;
        }
        if (st == RFD_OK) ok = gallery_file_write_values(f, (const uint16_t *)g->pin.p, (size_t)m * dim);
    }
    ok = (fclose(f) == 0) && ok;
    if (st == RFD_OK && !ok) { set_error("short write to %s", tmp.c_str()); st = RFD_ERR_IO; }
    if (st == RFD_OK && rename(tmp.c_str(), path) != 0) { set_error("cannot rename %s to %s", tmp.c_str(), path); st = RFD_ERR_IO; }
    if (st != RFD_OK) (void)remove(tmp.c_str());
    return st;
}

// the rows of an opened file into the store of a new gallery, through the staging buffer
static int gallery_load_rows(rfd_gallery *g, hipStream_t s, GalleryFileReader &r, const char *path)
{
    RFD_TRY(gallery_host_stage(g));
    const int chunk = (int)(rfd_gallery::kStageBytes / ((size_t)r.dim * sizeof(bf16_t)));
    uint16_t *h = (uint16_t *)g->pin.p;
    for (int i = 0; i < r.rows; i += chunk) {
        const int m = std::min(chunk, r.rows - i);
        if (int st = r.read_rows(m, h)) { set_error("%s", r.msg); return st; }
        for (int j = 0; j < m; ++j) // a removed row is erased whatever the file holds for it
            if (!r.is_live(i + j)) memset(h + (size_t)j * r.dim, 0, (size_t)r.dim * sizeof(uint16_t));
        if (hipMemcpyAsync(g->stage.p, h, (size_t)m * r.dim * sizeof(bf16_t), hipMemcpyHostToDevice, s) != hipSuccess) {
            set_error("copying rows of %s to the device failed", path);
            return RFD_ERR_HIP;
        }
        RFD_TRY(launch_gallery_import((const bf16_t *)g->stage.p, m, r.dim, i, (bf16_t *)g->store.p, s));
        if (hipStreamSynchronize(s) != hipSuccess) { set_error("loading rows of %s failed", path); return RFD_ERR_HIP; }
    }
    return RFD_OK;
}

// the book's live words to the device, through the staging buffer
static int gallery_load_live_words(rfd_gallery *g, hipStream_t s, const char *path)
{
    const std::vector<uint16_t> &words = g->book.live_words();
    const size_t bytes = words.size() * sizeof(uint16_t); // <= ceil(2^30 / 16) * 2 = 128 MiB: in pieces
    for (size_t at = 0; at < bytes; at += rfd_gallery::kStageBytes) {
        const size_t m = std::min(rfd_gallery::kStageBytes, bytes - at);
        memcpy(g->pin, (const char *)words.data() + at, m);
        if (hipMemcpyAsync((char *)g->live.p + at, g->pin, m, hipMemcpyHostToDevice, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) {
            set_error("copying the live words of %s to the device failed", path);
            return RFD_ERR_HIP;
        }
    }
    return RFD_OK;
}

int rfd_gallery_load(rfd_ctx *c, const char *path, int capacity, rfd_gallery **out)
{
    RFD_CHECK_ARG(c && path && out && capacity >= 0, "null argument or capacity < 0");
    *out = nullptr;
    RFD_TRY(rfd_gallery_file_info(path, nullptr, nullptr, nullptr)); // the whole validation, before anything is allocated
    GalleryFileReader r;
    if (int st = r.open(path)) { set_error("%s", r.msg); return st; }
    if (capacity == 0) capacity = std::max(r.rows, 1);
    if (capacity < r.rows) { set_error("%s holds %d rows: a capacity of %d does not fit them", path, r.rows, capacity); return RFD_ERR_CAPACITY; }
    rfd_gallery *g = nullptr;
    RFD_TRY(rfd_gallery_create(c, r.dim, capacity, &g));
    const hipStream_t s = ctx_stream(c);
    int st = gallery_load_rows(g, s, r, path);
    if (st == RFD_OK && r.rows > 0) {
        g->book.from_file(r.rows, r.live, r.bits);
        st = gallery_load_live_words(g, s, path);
    }
    if (st != RFD_OK) { rfd_gallery_destroy(g); return st; }
    *out = g;
    return RFD_OK;
}
