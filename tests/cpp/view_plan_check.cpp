// view_plan_check.cpp -- csrc/view_plan.h alone, built by the host compiler under AddressSanitizer and UBSan
// (tests/test_view_plan_cpu.py).  Every frame of 1 .. 2 t + 3 pixels on each axis, three tile sizes t, every legal overlap, with
// and without the full view: by brute force over the pixels the tiles cover the frame, lie inside it, overlap their neighbours by
// at least the overlap and end at the border; the count is the formula's; the `inner` bits are the geometry's.  The plan is
// written into a heap array of exactly `count` views, so a view too many is an out-of-bounds write the sanitizers name.  Then
// the refusals, the 1080p plan the documents quote, and view_slots.
#include <cstdio>
#include <vector>

#include "../../rs-face-detection_amd/csrc/view_plan.h"

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

static int tiles_of(int W, int t, int o) { return W <= t ? 1 : (W - o + (t - o) - 1) / (t - o); }

static void one(int W, int H, int tw, int th, int o, int full)
{
    ++steps;
#define WHERE "frame %dx%d tile %dx%d overlap %d full %d", W, H, tw, th, o, full
    const rfd_view_config cfg = {tw, th, o, full, 4.0f};
    const int nx = tiles_of(W, tw, o), ny = tiles_of(H, th, o);
    const int want = nx * ny + (full && nx * ny > 1 ? 1 : 0);
    int count = -1;
    CHECK(view_plan(3, W, H, &cfg, nullptr, 0, &count) == RFD_ERR_CAPACITY && count == want, WHERE); // the count query
    std::vector<rfd_view> out((size_t)want);
    count = -1;
    CHECK(view_plan(3, W, H, &cfg, out.data(), want, &count) == RFD_OK && count == want, WHERE);
    if (count != want) return;
    size_t k = 0;
    if (full && nx * ny > 1) {
        const rfd_view &v = out[k++];
        CHECK(v.frame == 3 && v.x == 0 && v.y == 0 && v.w == W && v.h == H && v.inner == 0u, WHERE);
    }
    const int w = W <= tw ? W : tw, h = H <= th ? H : th;
    std::vector<int> seen((size_t)W * H, 0);
    for (int j = 0; j < ny; ++j)
        for (int i = 0; i < nx; ++i) {
            const rfd_view &v = out[k++];
            CHECK(v.frame == 3 && v.w == w && v.h == h, WHERE);
            CHECK(v.x >= 0 && v.y >= 0 && v.x + v.w <= W && v.y + v.h <= H, WHERE);
            CHECK(v.x == (nx > 1 ? (int)((long long)i * (W - tw) / (nx - 1)) : 0) && v.y == (ny > 1 ? (int)((long long)j * (H - th) / (ny - 1)) : 0), WHERE);
            const uint32_t inner = (v.x > 0 ? 1u : 0u) | (v.y > 0 ? 2u : 0u) | (v.x + v.w < W ? 4u : 0u) | (v.y + v.h < H ? 8u : 0u);
            CHECK(v.inner == inner, WHERE);
            CHECK(((v.inner & 1u) != 0) == (i > 0) && ((v.inner & 4u) != 0) == (i + 1 < nx), WHERE); // only the outermost tiles touch the border
            CHECK(((v.inner & 2u) != 0) == (j > 0) && ((v.inner & 8u) != 0) == (j + 1 < ny), WHERE);
            if (i + 1 == nx) CHECK(v.x + v.w == W, WHERE);
            if (j + 1 == ny) CHECK(v.y + v.h == H, WHERE);
            if (i > 0) { // the left neighbour: same row, previous view
                const rfd_view &l = out[k - 2];
                CHECK(l.y == v.y && l.x < v.x && l.x + l.w - v.x >= o, WHERE);
            }
            if (j > 0) {
                const rfd_view &u = out[k - 1 - (size_t)nx];
                CHECK(u.x == v.x && u.y < v.y && u.y + u.h - v.y >= o, WHERE);
            }
            if (v.x >= 0 && v.y >= 0 && v.x + v.w <= W && v.y + v.h <= H)
                for (int y = v.y; y < v.y + v.h; ++y)
                    for (int x = v.x; x < v.x + v.w; ++x) ++seen[(size_t)y * W + x];
        }
    int holes = 0;
    for (int s : seen) holes += s == 0;
    CHECK(holes == 0, WHERE);
    if (want > 1) { // one view too few: refused, the count told, nothing written
        std::vector<rfd_view> small((size_t)want - 1, rfd_view{-7, -7, -7, -7, -7, 77u});
        count = -1;
        CHECK(view_plan(3, W, H, &cfg, small.data(), want - 1, &count) == RFD_ERR_CAPACITY && count == want, WHERE);
        bool touched = false;
        for (const rfd_view &v : small) touched |= v.frame != -7 || v.inner != 77u;
        CHECK(!touched, WHERE);
    }
#undef WHERE
}

static void refusals()
{
    ++steps;
    rfd_view out[16];
    int count = 5;
    for (int t : {1, 4, 9})
        for (int o : {-1, t, t + 1, 1000}) {
            const rfd_view_config cfg = {t, t, o, 1, 4.0f};
            count = 5;
            CHECK(view_plan(0, 20, 20, &cfg, out, 16, &count) == RFD_ERR_INVALID_ARG && count == 0, "tile %d overlap %d", t, o);
        }
    const rfd_view_config wide = {8, 3, 3, 1, 4.0f}; // the overlap must be below BOTH tile extents
    CHECK(view_plan(0, 20, 20, &wide, out, 16, &count) == RFD_ERR_INVALID_ARG && count == 0, "overlap == tile_h");
    const rfd_view_config ok = {8, 8, 2, 1, 4.0f};
    CHECK(view_plan(0, 0, 20, &ok, out, 16, &count) == RFD_ERR_INVALID_ARG, "frame_w 0");
    CHECK(view_plan(0, 20, -1, &ok, out, 16, &count) == RFD_ERR_INVALID_ARG, "frame_h -1");
    CHECK(view_plan(-1, 20, 20, &ok, out, 16, &count) == RFD_ERR_INVALID_ARG, "frame -1");
    CHECK(view_plan(0, 20, 20, nullptr, out, 16, &count) == RFD_ERR_INVALID_ARG, "cfg null");
    CHECK(view_plan(0, 20, 20, &ok, out, 16, nullptr) == RFD_ERR_INVALID_ARG, "count null");
    CHECK(view_plan(0, 20, 20, &ok, nullptr, 16, &count) == RFD_ERR_INVALID_ARG, "out null with a cap");
    const rfd_view_config zero = {0, 8, 0, 1, 4.0f};
    CHECK(view_plan(0, 20, 20, &zero, out, 16, &count) == RFD_ERR_INVALID_ARG, "tile_w 0");
    // a plan whose count does not fit an int is refused, not wrapped
    const rfd_view_config dense = {2, 2, 1, 0, 4.0f};
    CHECK(view_plan(0, 0x7fffffff, 0x7fffffff, &dense, nullptr, 0, &count) == RFD_ERR_CAPACITY && count == 0x7fffffff, "count %d", count);
}

static void documented()
{
    ++steps;
    rfd_view_config cfg;
    view_config_default(&cfg, 640, 640);
    CHECK(cfg.tile_w == 640 && cfg.tile_h == 640 && cfg.overlap == 128 && cfg.full_view == 1 && cfg.edge_margin == 4.0f, "defaults");
    view_config_default(&cfg, 128, 96);
    CHECK(cfg.tile_w == 128 && cfg.tile_h == 96 && cfg.overlap == 25, "defaults 128x96");
    view_config_default(&cfg, 640, 640);
    rfd_view v[9];
    int count = 0;
    CHECK(view_plan(0, 1920, 1080, &cfg, v, 9, &count) == RFD_OK && count == 9, "1080p: %d views", count);
    CHECK(v[0].w == 1920 && v[0].h == 1080 && v[0].inner == 0u, "1080p full view");
    const int xs[4] = {0, 426, 853, 1280}, ys[2] = {0, 440};
    for (int j = 0; j < 2; ++j)
        for (int i = 0; i < 4; ++i) {
            const rfd_view &t = v[1 + j * 4 + i];
            CHECK(t.x == xs[i] && t.y == ys[j] && t.w == 640 && t.h == 640, "1080p tile %d,%d at %d,%d", i, j, t.x, t.y);
        }
    CHECK(v[1].inner == (4u | 8u) && v[8].inner == (1u | 2u) && v[2].inner == (1u | 4u | 8u), "1080p inner bits");
    // W <= t on one axis, on both, and a frame of exactly one tile: a single tile makes no full view
    CHECK(view_plan(0, 1920, 600, &cfg, v, 9, &count) == RFD_OK && count == 5 && v[1].h == 600 && v[1].inner == 4u && v[4].inner == 1u, "one row of tiles");
    CHECK(view_plan(0, 300, 200, &cfg, v, 9, &count) == RFD_OK && count == 1 && v[0].w == 300 && v[0].h == 200 && v[0].inner == 0u, "a small frame");
    CHECK(view_plan(0, 640, 640, &cfg, v, 9, &count) == RFD_OK && count == 1 && v[0].inner == 0u, "exactly one tile");
    cfg.full_view = 0;
    CHECK(view_plan(0, 1920, 1080, &cfg, v, 9, &count) == RFD_OK && count == 8 && v[0].w == 640, "no full view");
    // 4K at the defaults: 8 x 4 tiles and the full view
    cfg.full_view = 1;
    CHECK(view_plan(0, 3840, 2160, &cfg, nullptr, 0, &count) == RFD_ERR_CAPACITY && count == 33, "4K: %d views", count);
}

static void slots()
{
    ++steps;
    const rfd_view v[6] = {{0, 0, 0, 4, 4, 0u}, {0, 2, 0, 4, 4, 1u}, {0, 4, 0, 4, 4, 15u}, {2, 0, 0, 1, 1, 0u}, {3, 0, 0, 9, 9, 0u}, {3, 1, 1, 2, 2, 0u}};
    std::vector<int32_t> slot(6, -1);
    int vmax = -1, bad = 7;
    CHECK(view_slots(v, 6, 4, slot.data(), &vmax, &bad) == kViewOk && vmax == 3 && bad == -1, "vmax %d", vmax);
    const int want[6] = {0, 1, 2, 0, 0, 1};
    for (int i = 0; i < 6; ++i) CHECK(slot[i] == want[i], "slot %d is %d", i, slot[i]);
    CHECK(view_slots(v, 0, 4, slot.data(), &vmax, &bad) == kViewOk && vmax == 0, "no views");
    CHECK(view_slots(v, 6, 3, slot.data(), &vmax, &bad) == kViewFrameRange && bad == 4, "frame 3 of 3");
    rfd_view u[3] = {v[0], v[3], v[1]};
    CHECK(view_slots(u, 3, 4, slot.data(), &vmax, &bad) == kViewFrameOrder && bad == 2, "unsorted");
    u[2] = rfd_view{2, 0, 0, 0, 5, 0u};
    CHECK(view_slots(u, 3, 4, slot.data(), &vmax, &bad) == kViewEmpty && bad == 2, "empty");
    u[2] = rfd_view{2, -1, 0, 5, 5, 0u};
    CHECK(view_slots(u, 3, 4, slot.data(), &vmax, &bad) == kViewOrigin && bad == 2, "negative corner");
    u[2] = rfd_view{2, 0, 0, 5, 5, 16u};
    CHECK(view_slots(u, 3, 4, slot.data(), &vmax, &bad) == kViewInnerBits && bad == 2, "inner bit 4");
    u[0].frame = -1;
    CHECK(view_slots(u, 3, 4, slot.data(), &vmax, &bad) == kViewFrameRange && bad == 0, "frame -1");
    CHECK(view_inside(rfd_view{0, 3, 2, 5, 6, 0u}, 8, 8) && !view_inside(rfd_view{0, 4, 2, 5, 6, 0u}, 8, 8) && !view_inside(rfd_view{0, 3, 3, 5, 6, 0u}, 8, 8), "inside");
    CHECK(!view_inside(rfd_view{0, 0x7fffffff, 0, 0x7fffffff, 1, 0u}, 0x7fffffff, 8), "x + w beyond int");
}

int main()
{
    for (int t : {4, 7, 12})
        for (int o = 0; o < t; ++o)
            for (int W = 1; W <= 2 * t + 3; ++W)
                for (int H = 1; H <= 2 * t + 3; ++H)
                    for (int full = 0; full < 2; ++full) one(W, H, t, t, o, full);
    for (int o = 0; o < 5; ++o) // tile_w != tile_h
        for (int W = 1; W <= 25; ++W)
            for (int H = 1; H <= 13; ++H) one(W, H, 11, 5, o, 1);
    refusals();
    documented();
    slots();
    std::printf("%ld steps, %ld checks, %ld failures\n", steps, checks, failures);
    return failures ? 1 : 0;
}
