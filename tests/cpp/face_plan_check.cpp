// face_plan_check.cpp -- csrc/face_plan.h alone, built by the host compiler under AddressSanitizer and UBSan
// (tests/test_face_plan_cpu.py).  Every piece of the plan against a model written here, independently of the header: the resize
// flag against "the source is exactly twice the destination", the four buffer layouts against the documented order and the
// sizes the entries reserved before the plan existed, the fused / rest split against its definition over every pattern, the
// liveness tile table against a loop over the pixels, the list bound in 64 bits, every check on both sides of every boundary
// with the message the ABI tests see, and the defaults.
#include <climits>
#include <cfloat>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../rs-face-detection_amd/csrc/face_plan.h"

using namespace rfd;

static long steps = 0, checks = 0, failures = 0;

#define CHECK(cond, ...)                                  \
    do {                                                  \
        ++checks;                                         \
        if (!(cond)) {                                    \
            if (++failures <= 20) {                       \
                std::printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); \
                std::printf(__VA_ARGS__);                 \
                std::printf("\n");                        \
            }                                             \
        }                                                 \
    } while (0)

// ---- resize ----
static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd(uint32_t lo, uint32_t hi) // lo .. hi inclusive (xorshift64*)
{
    rng_state ^= rng_state >> 12; rng_state ^= rng_state << 25; rng_state ^= rng_state >> 27;
    return lo + (uint32_t)(((rng_state * 0x2545f4914f6cdd1dull) >> 33) % (hi - lo + 1));
}

static void resize_one(int sw, int sh, int dw, int dh)
{
    ++steps;
    const ResizeScale r = resize_scale(sw, sh, dw, dh);
    const double mx = 1.0 / ((double)dw / sw), my = 1.0 / ((double)dh / sh);
    CHECK(std::memcmp(&r.scale_x, &mx, sizeof mx) == 0 && std::memcmp(&r.scale_y, &my, sizeof my) == 0, "scale of %dx%d -> %dx%d", sw, sh, dw, dh);
    CHECK(r.area_fast == (sw == 2 * dw && sh == 2 * dh ? 1 : 0), "area_fast %d of %dx%d -> %dx%d", r.area_fast, sw, sh, dw, dh);
}

static void resize()
{
    for (int sw = 1; sw <= 64; ++sw)
        for (int dw = 1; dw <= 64; ++dw)
            for (int sh = 1; sh <= 64; ++sh)
                for (int dh = 1; dh <= 64; ++dh) resize_one(sw, sh, dw, dh);
    for (int i = 0; i < 4000; ++i) {
        const int dw = (int)rnd(1, 4096), dh = (int)rnd(1, 4096);
        resize_one((int)rnd(1, 8192), (int)rnd(1, 8192), (int)rnd(1, 8192), (int)rnd(1, 8192));
        resize_one(2 * dw, 2 * dh, dw, dh);                                   // the fast path itself
        resize_one(2 * dw + (int)rnd(0, 2) - 1, 2 * dh, dw, dh);              // and its nearest misses
        resize_one(2 * dw, 2 * dh + (int)rnd(0, 2) - 1, dw, dh);
        resize_one(2 * dw, (int)rnd(1, 8192), dw, dh);
        resize_one(dw, dh, 2 * dw, 2 * dh);                                   // twice as large, not half
    }
    resize_one(8192, 8192, 4096, 4096);
    resize_one(8191, 8192, 4096, 4096);
    resize_one(8192, 8192, 4096, 4095);
}

// ---- layouts: the regions in the documented order, each of the documented size, contiguous from word 0 to the total ----
struct Region { const char *name; size_t at, words; };

static void regions_tile(const char *what, const std::vector<Region> &r, size_t total, size_t formula, int a, int b, int c)
{
    ++steps;
    size_t at = 0;
    for (const Region &g : r) {
        CHECK(g.at == at, "%s (%d, %d, %d): %s starts at word %zu, the regions before it end at %zu", what, a, b, c, g.name, g.at, at);
        CHECK((g.at * 4) % 4 == 0 && g.words > 0, "%s (%d, %d, %d): %s is empty or not on a word", what, a, b, c, g.name);
        at = g.at + g.words;
    }
    CHECK(at == total, "%s (%d, %d, %d): the regions end at word %zu, the total is %zu", what, a, b, c, at, total);
    CHECK(total == formula, "%s (%d, %d, %d): %zu words, the entries reserved %zu", what, a, b, c, total, formula);
}

static void layouts()
{
    for (int n = 1; n <= 33; ++n) {
        const size_t N = (size_t)n;
        const SelLayout s = sel_layout(n);
        regions_tile("sel_out", {{"box", s.box, 5 * N}, {"kps", s.kps, 10 * N}, {"found", s.found, N}}, s.words, 16 * N, n, 0, 0);
        for (int bound = 1; bound <= 70; ++bound) {
            const size_t B = (size_t)bound;
            const ListLayout l = list_layout(n, bound);
            regions_tile("list_out", {{"total", l.total, 1}, {"first", l.first, N + 1}, {"frame", l.frame, B}, {"row", l.row, B}, {"status", l.status, B},
                                      {"box", l.box, 5 * B}, {"kps", l.kps, 10 * B}}, l.words, N + 2 + 18 * B, n, bound, 0);
        }
        for (int k = 1; k <= 4; ++k) {
            const size_t K = (size_t)k;
            const LiveTensorLayout t = live_tensor_layout(n, k);
            regions_tile("live_io tensors", {{"box", t.box, 5 * N}, {"found", t.found, N}, {"weights", t.weights, N * K}, {"rois", t.rois, 4 * N * K},
                                             {"status", t.status, N}}, t.words, N * (7 + 5 * K), n, k, 0);
            for (int classes = 2; classes <= 5; ++classes) {
                const size_t C = (size_t)classes;
                const LiveDecideLayout d = live_decide_layout(n, k, classes);
                regions_tile("live_io decide", {{"logits", d.logits, K * N * C}, {"weights", d.weights, N * K}, {"score", d.score, N}, {"live", d.live, N}},
                             d.words, K * N * C + N * K + 2 * N, n, k, classes);
            }
        }
    }
    // sizes whose byte count passes 2^32: the offsets are size_t all the way
    const ListLayout big = list_layout(INT_MAX, INT_MAX);
    CHECK(big.words == (size_t)INT_MAX + 2 + 18 * (size_t)INT_MAX && big.kps == (size_t)INT_MAX + 2 + 8 * (size_t)INT_MAX, "list_out of INT_MAX frames and faces");
    const LiveDecideLayout bd = live_decide_layout(1 << 20, 64, 1 << 10);
    CHECK(bd.weights == ((size_t)64 << 30) && bd.words == ((size_t)64 << 30) + ((size_t)64 << 20) + ((size_t)2 << 20), "a decide call of 2^36 logits");
}

// ---- split ----
static void split()
{
    const int sizes[3][2] = {{112, 112}, {96, 128}, {1, 4096}};
    for (const auto &a : sizes)
        for (int k = 0; k <= 4; ++k)
            for (int pattern = 0; pattern < (1 << k); ++pattern)
                for (int other = 0; other < 3; ++other) { // what a config that is not of the crop's size differs in
                    ++steps;
                    rfd_face_tensor_config cfgs[4];
                    std::memset(cfgs, 0, sizeof cfgs);
                    for (int j = 0; j < k; ++j) {
                        const bool same = (pattern >> j) & 1;
                        cfgs[j].out_w = same || other == 1 ? a[0] : other == 0 ? a[0] + 1 : a[1] == a[0] ? a[0] + 2 : a[1];
                        cfgs[j].out_h = same || other == 0 ? a[1] : other == 1 ? a[1] + 1 : a[1] == a[0] ? a[1] + 2 : a[0];
                    }
                    const FaceSplit s = face_split(a[0], a[1], cfgs, k);
                    CHECK(s.n_fused + s.n_rest == k && s.n_fused >= 0 && s.n_rest >= 0, "k %d pattern %d: %d fused, %d rest", k, pattern, s.n_fused, s.n_rest);
                    if (s.n_fused < 0 || s.n_rest < 0 || s.n_fused > 4 || s.n_rest > 4) continue;
                    int seen = 0;
                    for (int q = 0; q < s.n_fused; ++q) {
                        const int j = s.fused[q];
                        CHECK(j >= 0 && j < k && ((pattern >> j) & 1) == 1, "k %d pattern %d: fused holds %d", k, pattern, j);
                        CHECK(q == 0 || s.fused[q - 1] < j, "k %d pattern %d: fused is not in the order of j", k, pattern);
                        if (j >= 0 && j < k) seen |= 1 << j;
                    }
                    for (int q = 0; q < s.n_rest; ++q) {
                        const int j = s.rest[q];
                        CHECK(j >= 0 && j < k && ((pattern >> j) & 1) == 0, "k %d pattern %d: rest holds %d", k, pattern, j);
                        CHECK(q == 0 || s.rest[q - 1] < j, "k %d pattern %d: rest is not in the order of j", k, pattern);
                        if (j >= 0 && j < k) seen |= 1 << j;
                    }
                    CHECK(seen == (1 << k) - 1, "k %d pattern %d: the union is 0x%x", k, pattern, seen);
                }
}

// ---- tile prefix ----
static void tiles()
{
    const int wh[][2] = {{1, 1}, {16, 16}, {16, 17}, {17, 16}, {80, 80}, {255, 1}, {256, 1}, {257, 1}, {256, 128}, {4096, 4096}, {4096, 4095}, {1, 4096}};
    const int nwh = (int)(sizeof wh / sizeof wh[0]);
    for (int k = 1; k <= 4; ++k)
        for (int first = 0; first < nwh; ++first)
            for (int step = 1; step <= 5; ++step) {
                ++steps;
                rfd_liveness_config cfg;
                std::memset(&cfg, 0, sizeof cfg);
                cfg.k = k;
                for (int j = 0; j < k; ++j) { cfg.out_w[j] = wh[(first + j * step) % nwh][0]; cfg.out_h[j] = wh[(first + j * step) % nwh][1]; }
                const LiveTiles t = live_tiles(cfg);
                long long at = 0;
                for (int j = 0; j < k; ++j) {
                    CHECK(t.tile0[j] == at, "k %d first %d step %d: tile0[%d] is %d, the loop says %lld", k, first, step, j, t.tile0[j], at);
                    for (long long p = 0; p < (long long)cfg.out_w[j] * cfg.out_h[j]; p += 256) ++at; // one tile per 256 pixels begun
                }
                CHECK(t.total == at, "k %d first %d step %d: total %d, the loop says %lld", k, first, step, t.total, at);
            }
    rfd_liveness_config def;
    liveness_config_default(&def);
    const LiveTiles t = live_tiles(def);
    CHECK(t.tile0[0] == 0 && t.tile0[1] == 25 && t.tile0[2] == 50 && t.tile0[3] == 306 && t.total == 370, "the default models: %d tiles", t.total);
}

// ---- face_list_bound ----
static void bound()
{
    const int v[] = {1, 2, 5, 31, 32, 33, 1024, 46341, INT_MAX / 2, INT_MAX - 1, INT_MAX};
    for (int n : v)
        for (int max_faces : v)
            for (int max_det : v)
                for (int cap : v) {
                    ++steps;
                    const int64_t per = max_faces < max_det ? max_faces : max_det, all = (int64_t)n * per, want = all < cap ? all : (int64_t)cap;
                    const int got = face_list_bound(n, max_faces, max_det, cap);
                    CHECK(got == want, "n %d max_faces %d max_det %d cap %d: %d, in 64 bits %lld", n, max_faces, max_det, cap, got, (long long)want);
                }
}

// ---- the checks ----
static void expect(int status, const char *msg, int want, const std::string &text, const char *what)
{
    ++steps;
    CHECK(status == want, "%s: status %d, expected %d", what, status, want);
    if (want != RFD_OK) CHECK(text == msg, "%s: message \"%s\", expected \"%s\"", what, msg, text.c_str());
    else CHECK(std::strcmp(msg, "untouched") == 0, "%s: an accepting check wrote \"%s\"", what, msg);
}

#define EXPECT(want, text, what, check, ...)                            \
    do {                                                                \
        const int want_ = (want);                                       \
        const std::string text_ = (text);                               \
        char msg_[256] = "untouched";                                   \
        expect(check(__VA_ARGS__, msg_, sizeof msg_), msg_, want_, text_, what); \
    } while (0)

static std::string fmt(const char *f, ...) __attribute__((format(printf, 1, 2)));
static std::string fmt(const char *f, ...)
{
    char b[256];
    va_list ap;
    va_start(ap, f);
    vsnprintf(b, sizeof b, f, ap);
    va_end(ap);
    return b;
}

static void the_checks()
{
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const int sides[] = {INT_MIN, -1, 0, 1, 2, 112, 4095, 4096, 4097, INT_MAX};
    // alignment and tensor sizes, crop sizes: 1 .. 4096 on both sides
    for (int w : sides)
        for (int h : sides) {
            const bool ok = w >= 1 && w <= 4096 && h >= 1 && h <= 4096;
            rfd_alignment_config a;
            alignment_config_default(&a);
            a.out_w = w; a.out_h = h;
            EXPECT(ok ? RFD_OK : RFD_ERR_INVALID_ARG, fmt("alignment output size %dx%d out of range", w, h), "alignment size", check_align_cfg, a);
            rfd_face_tensor_config t;
            face_tensor_config_quality(&t);
            t.out_w = w; t.out_h = h;
            for (int j : {0, 3})
                EXPECT(ok ? RFD_OK : RFD_ERR_INVALID_ARG, fmt("tensor config %d: size %dx%d out of range", j, w, h), "tensor size", check_face_tensor_size, t, j);
            EXPECT(ok ? RFD_OK : RFD_ERR_INVALID_ARG, "invalid argument: crop size out of range (crop_w >= 1 && crop_h >= 1 && crop_w <= 4096 && crop_h <= 4096)",
                   "crop size", check_crop_size, w, h);
        }
    // the number of tensor configs: k_min .. 4
    for (int k : {INT_MIN, -1, 0, 1, 2, 4, 5, 6, INT_MAX})
        for (int k_min : {0, 1}) {
            const int want = k > 4 ? RFD_ERR_CAPACITY : k < k_min ? RFD_ERR_INVALID_ARG : RFD_OK;
            EXPECT(want, k > 4 ? fmt("%d tensor configs exceed RFD_MAX_FACE_TENSORS (4)", k) : "invalid argument: too few tensor configs (k >= k_min)", "tensor count",
                   check_face_tensor_count, k, k_min);
        }
    // the list config: the first field that is wrong is the one named
    rfd_face_list_config l;
    face_list_config_default(&l);
    EXPECT(RFD_OK, "", "list default", check_list_cfg, l, 1);
    EXPECT(RFD_OK, "", "list default, a large cap", check_list_cfg, l, INT_MAX);
    for (int cap : {INT_MIN, -1, 0}) EXPECT(RFD_ERR_INVALID_ARG, fmt("invalid argument: cap %d < 1", cap), "list cap", check_list_cfg, l, cap);
    for (int mf : {INT_MIN, -1, 0, 1, INT_MAX}) {
        l.max_faces = mf;
        EXPECT(mf >= 1 ? RFD_OK : RFD_ERR_INVALID_ARG, fmt("invalid argument: max_faces %d < 1", mf), "list max_faces", check_list_cfg, l, 1);
        if (mf < 1) EXPECT(RFD_ERR_INVALID_ARG, fmt("invalid argument: max_faces %d < 1", mf), "list max_faces before cap", check_list_cfg, l, 0);
    }
    l.max_faces = 1;
    for (float px : {0.0f, -0.0f, 1.0f, FLT_MIN, FLT_MAX, -FLT_MIN, -1.0f, inf, -inf, nan}) {
        l.min_face_px = px;
        const bool ok = px >= 0.0f && px <= FLT_MAX;
        EXPECT(ok ? RFD_OK : RFD_ERR_INVALID_ARG, fmt("invalid argument: min_face_px %g is negative or not finite", (double)px), "list min_face_px", check_list_cfg, l, 1);
    }
    l.min_face_px = 0.0f;
    for (float sc : {0.0f, -0.0f, -1.0f, -FLT_MAX, FLT_MAX, inf, -inf, nan}) {
        l.min_score = sc;
        const bool ok = sc >= -FLT_MAX && sc <= FLT_MAX;
        EXPECT(ok ? RFD_OK : RFD_ERR_INVALID_ARG, fmt("invalid argument: min_score %g is not finite", (double)sc), "list min_score", check_list_cfg, l, 1);
        if (!ok) {
            l.min_face_px = -1.0f; // min_face_px is looked at first
            EXPECT(RFD_ERR_INVALID_ARG, "invalid argument: min_face_px -1 is negative or not finite", "list field order", check_list_cfg, l, 1);
            l.min_face_px = 0.0f;
        }
    }
    // the liveness config
    rfd_liveness_config v;
    liveness_config_default(&v);
    EXPECT(RFD_OK, "", "liveness default", check_liveness_cfg, v);
    for (int k : {INT_MIN, -1, 0, 1, 4, 5, INT_MAX}) {
        v.k = k;
        const int want = k > 4 ? RFD_ERR_CAPACITY : k < 1 ? RFD_ERR_INVALID_ARG : RFD_OK;
        EXPECT(want, k > 4 ? fmt("liveness config: k = %d exceeds RFD_MAX_FACE_TENSORS (4)", k) : fmt("invalid argument: liveness config: k = %d, at least one model is needed", k),
               "liveness k", check_liveness_cfg, v);
    }
    for (int j = 0; j < 4; ++j) {
        for (int side : sides) {
            const bool ok = side >= 1 && side <= 4096;
            liveness_config_default(&v);
            v.out_w[j] = side;
            EXPECT(ok ? RFD_OK : RFD_ERR_INVALID_ARG, fmt("invalid argument: liveness config: out_w[%d] = %d out of range", j, side), "liveness out_w", check_liveness_cfg, v);
            v.k = j; // a model past k is not looked at
            if (j >= 1) EXPECT(RFD_OK, "", "liveness out_w past k", check_liveness_cfg, v);
            liveness_config_default(&v);
            v.out_h[j] = side;
            EXPECT(ok ? RFD_OK : RFD_ERR_INVALID_ARG, fmt("invalid argument: liveness config: out_h[%d] = %d out of range", j, side), "liveness out_h", check_liveness_cfg, v);
        }
        for (float sc : {FLT_MIN, 1.0f, 2.7f, FLT_MAX, 0.0f, -0.0f, -1.0f, -FLT_MAX, inf, -inf, nan}) {
            const bool ok = sc > 0.0f && sc <= FLT_MAX;
            liveness_config_default(&v);
            v.scale[j] = sc;
            EXPECT(ok ? RFD_OK : RFD_ERR_INVALID_ARG, fmt("invalid argument: liveness config: scale[%d] = %g is not finite and positive", j, (double)sc), "liveness scale",
                   check_liveness_cfg, v);
        }
    }
    liveness_config_default(&v); // the first wrong field of the first wrong model
    v.out_h[1] = 0; v.out_w[2] = 0; v.scale[1] = nan;
    EXPECT(RFD_ERR_INVALID_ARG, "invalid argument: liveness config: out_h[1] = 0 out of range", "liveness field order", check_liveness_cfg, v);
    // the counts of the three rules
    for (int n : {INT_MIN, -1, 0, 1, 2, INT_MAX})
        for (int m : {INT_MIN, -1, 0, 1, 2, 3, INT_MAX}) {
            EXPECT(n >= 1 && m >= 1 ? RFD_OK : RFD_ERR_INVALID_ARG, "invalid argument: n < 1 or classes < 1 (n >= 1 && classes >= 1)", "quality counts", check_quality_counts, n, m);
            EXPECT(n >= 1 && m >= 1 ? RFD_OK : RFD_ERR_INVALID_ARG, "invalid argument: n < 1 or dim < 1 (n >= 1 && dim >= 1)", "normalise counts", check_normalize_counts, n, m);
            for (int k : {INT_MIN, -1, 0, 1, 4, 5, 9, INT_MAX})
                EXPECT(k >= 1 && n >= 1 && m >= 2 ? RFD_OK : RFD_ERR_INVALID_ARG, "invalid argument: k < 1, n < 1 or classes < 2 (k >= 1 && n >= 1 && classes >= 2)",
                       "liveness decide counts", check_liveness_decide_counts, k, n, m);
        }
}

// ---- defaults ----
static void defaults()
{
    ++steps;
    rfd_selection_config s;
    selection_config_default(&s);
    CHECK(s.margin_center_left_ratio == 0.3f && s.margin_center_right_ratio == 0.3f && s.margin_edge_ratio == 0.1f && s.minimum_face_ratio == 0.0075f, "selection");
    rfd_alignment_config a;
    std::memset(&a, 0xff, sizeof a);
    alignment_config_default(&a);
    const float tmpl[10] = {38.2946f, 51.6963f, 73.5318f, 51.5014f, 56.0252f, 71.7366f, 41.5493f, 92.3655f, 70.7299f, 92.2041f};
    CHECK(a.out_w == 112 && a.out_h == 112 && std::memcmp(a.standard_landmarks, tmpl, sizeof tmpl) == 0, "alignment");
    for (int r : a.reserved) CHECK(r == 0, "alignment reserved");
    rfd_face_tensor_config t;
    std::memset(&t, 0xff, sizeof t);
    face_tensor_config_quality(&t);
    CHECK(t.out_w == 112 && t.out_h == 112 && t.mean[0] == 123.675f && t.mean[1] == 116.28f && t.mean[2] == 103.53f && t.scale[0] == 0.01712475f &&
          t.scale[1] == 0.017507f && t.scale[2] == 0.01742919f && t.reserved[0] == 0 && t.reserved[3] == 0, "quality tensors");
    std::memset(&t, 0xff, sizeof t);
    face_tensor_config_extraction(&t);
    for (int c = 0; c < 3; ++c) CHECK(t.mean[c] == 127.5f && t.scale[c] == 0.0078125f, "extraction tensors");
    CHECK(t.out_w == 112 && t.out_h == 112 && t.reserved[0] == 0 && t.reserved[3] == 0, "extraction tensors");
    std::memset(&t, 0xff, sizeof t);
    face_tensor_config_quality_assessment(&t, 96, 64);
    for (int c = 0; c < 3; ++c) CHECK(t.mean[c] == 127.5f && t.scale[c] == 0.00784313725f, "quality assessment tensors");
    CHECK(t.out_w == 96 && t.out_h == 64 && t.reserved[0] == 0 && t.reserved[3] == 0, "quality assessment tensors");
    rfd_face_list_config l;
    std::memset(&l, 0xff, sizeof l);
    face_list_config_default(&l);
    CHECK(l.max_faces == 32 && l.min_face_px == 0.0f && l.min_score == 0.0f && l.reserved[0] == 0 && l.reserved[3] == 0, "face list");
    rfd_liveness_config v;
    std::memset(&v, 0xff, sizeof v);
    liveness_config_default(&v);
    const float scale[4] = {4.0f, 2.7f, 2.0f, 1.0f};
    const int size[4] = {80, 80, 256, 128};
    CHECK(v.k == 4 && v.reserved[0] == 0 && v.reserved[3] == 0, "liveness");
    for (int j = 0; j < 4; ++j) CHECK(v.scale[j] == scale[j] && v.out_w[j] == size[j] && v.out_h[j] == size[j], "liveness model %d", j);
}

int main()
{
    resize();
    layouts();
    split();
    tiles();
    bound();
    the_checks();
    defaults();
    std::printf("%ld steps, %ld checks, %ld failures\n", steps, checks, failures);
    return failures ? 1 : 0;
}
