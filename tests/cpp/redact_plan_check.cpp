// redact_plan_check.cpp -- csrc/redact_plan.h alone, built by the host compiler, plain and under AddressSanitizer and UBSan
// (tests/test_redact_cpu.py).  The region of boxes at the int32 and f32 extremes, infinities and NaNs in every coordinate (an
// overflow anywhere is a UBSan report); the ellipse rule against 128-bit arithmetic, for every pixel of every region up to
// 48 x 48 and at the rims of 32768 x 32768, where a term reaches 2^60; the tiles: for every cell 2 .. 64 the tile side is a
// multiple of the cell within 33 .. 64, and for every frame side 1 .. 200 the tiles partition the pixels and no cell lies in two
// tiles; the kernel's walk from a group's first pixel to the cells of its four pixels; the bounds of the config and of a frame.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <limits>

#include "../../rs-face-detection_amd/csrc/redact_plan.h"

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

static const float kInf = std::numeric_limits<float>::infinity(), kNan = std::numeric_limits<float>::quiet_NaN(), kMax = std::numeric_limits<float>::max();

// skipped, or the region
static void region(float x1, float y1, float x2, float y2, float mx, float mt, float mb, int W, int H, bool skipped, int X0 = 0, int Y0 = 0, int X1 = 0, int Y1 = 0)
{
    ++steps;
    const RdRegion g = rd_region(x1, y1, x2, y2, mx, mt, mb, W, H);
    CHECK(g.skipped == skipped, "box %g %g %g %g margins %g %g %g: skipped %d", x1, y1, x2, y2, mx, mt, mb, (int)g.skipped);
    if (!skipped && !g.skipped) {
        CHECK(g.x0 == X0 && g.y0 == Y0 && g.x1 == X1 && g.y1 == Y1, "box %g %g %g %g: region %d %d %d %d", x1, y1, x2, y2, g.x0, g.y0, g.x1, g.y1);
        CHECK(0 <= g.x0 && g.x0 <= g.x1 && g.x1 < W && 0 <= g.y0 && g.y0 <= g.y1 && g.y1 < H, "box %g %g %g %g: region leaves the frame", x1, y1, x2, y2);
    }
}

static bool covers128(int dx, int dy, int w, int h)
{
    const __int128 a = (__int128)dx * dx * h * h, b = (__int128)dy * dy * w * w, c = (__int128)w * w * h * h;
    return a + b <= c;
}

static void ellipse_pixel(int x, int y, int w, int h)
{
    const int dx = 2 * x + 1 - w, dy = 2 * y + 1 - h;
    CHECK(rd_ellipse_covers(dx, dy, w, h) == covers128(dx, dy, w, h), "%d x %d: pixel %d, %d", w, h, x, y);
    CHECK(rd_sq(dy) * rd_sq(w) <= rd_sq(w) * rd_sq(h), "%d x %d: row %d: the right-hand side wraps", w, h, y);
}

static void ellipse(int w, int h)
{
    ++steps;
    if ((long long)w * h <= 48 * 48) {
        int covered = 0;
        for (int y = 0; y < h; ++y)
            for (int x = 0; x < w; ++x) {
                ellipse_pixel(x, y, w, h);
                covered += rd_ellipse_covers(2 * x + 1 - w, 2 * y + 1 - h, w, h) ? 1 : 0;
                CHECK(rd_ellipse_covers(2 * x + 1 - w, 2 * y + 1 - h, w, h) == rd_ellipse_covers(2 * (w - 1 - x) + 1 - w, 2 * (h - 1 - y) + 1 - h, w, h),
                      "%d x %d: pixel %d, %d and its mirror differ", w, h, x, y);
            }
        CHECK(covered >= 1 && rd_ellipse_covers(2 * (w / 2) + 1 - w, 2 * (h / 2) + 1 - h, w, h), "%d x %d: the centre is not covered", w, h);
        if (w == 1 || h == 1) CHECK(covered == w * h, "%d x %d: a line is not full", w, h);
    } else { // the rims and the diagonal, where the terms are largest
        const int xs[] = {0, 1, 2, w / 7, w / 4, w / 2 - 1, w / 2, w - 3, w - 2, w - 1}, ys[] = {0, 1, 2, h / 7, h / 4, h / 2 - 1, h / 2, h - 3, h - 2, h - 1};
        for (int x : xs)
            for (int y : ys)
                if (x >= 0 && x < w && y >= 0 && y < h) ellipse_pixel(x, y, w, h);
        for (int t = 0; t < 4096; ++t) { // along the rim of the ellipse: the pixels next to where the row's chord ends
            const int y = (int)((long long)t * (h - 1) / 4095);
            const double dy = (2.0 * y + 1 - h) / h, half = 0.5 * w * std::sqrt(std::fmax(0.0, 1.0 - dy * dy));
            for (int d = -2; d <= 2; ++d) {
                const int x = (int)(0.5 * w - half) + d;
                if (x >= 0 && x < w) ellipse_pixel(x, y, w, h);
            }
        }
    }
}

static void tiles_of(int cell)
{
    ++steps;
    const int T = rd_tile_side(cell);
    CHECK(T % cell == 0 && T >= 33 && T <= kRdTileTarget, "cell %d: tile %d", cell, T);
    CHECK((T / cell) * (T / cell) <= kRdMaxTileCells, "cell %d: %d cells a side", cell, T / cell);
    for (int len = 1; len <= 200; ++len) {
        const int nt = rd_tiles(len, T);
        int sum = 0;
        for (int t = 0; t < nt; ++t) {
            const int tw = (T < len - t * T) ? T : len - t * T;
            CHECK(tw >= 1 && tw <= T, "cell %d, side %d: tile %d holds %d pixels", cell, len, t, tw);
            sum += tw;
        }
        CHECK(sum == len, "cell %d, side %d: the tiles hold %d pixels", cell, len, sum);
        for (int x = 0; x < len; ++x) { // the cell of a pixel lies in the pixel's tile, whole (up to the frame's edge)
            const int c0 = (x / cell) * cell, c1 = c0 + cell - 1;
            CHECK(c0 / T == x / T && (c1 < len ? c1 : len - 1) / T == x / T, "cell %d, side %d: the cell of pixel %d lies in two tiles", cell, len, x);
        }
    }
    // the kernel's walk: a group's first pixel lx0 = 4 g by one division, the other three by stepping the remainder
    for (int g = 0; g < 16; ++g) {
        int cx = (4 * g) / cell, rem = (4 * g) - cx * cell;
        for (int j = 0; j < 4; ++j) {
            if (4 * g + j < T) CHECK(cx == (4 * g + j) / cell && cx < T / cell, "cell %d: pixel %d walked to cell %d", cell, 4 * g + j, cx);
            if (++rem == cell) { ++cx; rem = 0; }
        }
    }
}

static rfd_image image(int w, int h, ptrdiff_t stride, const uint8_t *data)
{
    rfd_image im;
    std::memset(&im, 0, sizeof im);
    im.data = data; im.width = w; im.height = h; im.stride = stride;
    return im;
}

int main()
{
    // ---- as_i32 ----
    const float in[] = {1.75f, -1.75f, kNan, kInf, -kInf, 2147483648.0f, -2147483648.0f, 2147483520.0f, -0.5f, 0.99f, kMax, -kMax};
    const int32_t out[] = {1, -1, 0, 2147483647, -2147483647 - 1, 2147483647, -2147483647 - 1, 2147483520, 0, 0, 2147483647, -2147483647 - 1};
    for (int i = 0; i < 12; ++i) { ++steps; CHECK(rd_as_i32(in[i]) == out[i], "as_i32(%g) = %d", in[i], rd_as_i32(in[i])); }

    // ---- regions ----
    region(10.7f, 3.2f, 20.9f, 8.0f, 0, 0, 0, 100, 80, false, 10, 3, 20, 8);
    region(-0.5f, -0.99f, 2.9f, 0.5f, 0, 0, 0, 100, 80, false, 0, 0, 2, 0);
    region(99.9f, 79.9f, 500.0f, 500.0f, 0, 0, 0, 100, 80, false, 99, 79, 99, 79);
    region(8, 8, 12, 12, 0.25f, 0.5f, 0.75f, 20, 20, false, 7, 6, 13, 15);
    region(4, 4, 7, 6, 4, 4, 4, 12, 10, false, 0, 0, 11, 9);
    region(100.0f, 0, 120, 5, 0, 0, 0, 100, 80, true);    // right of the frame
    region(0, 80.0f, 5, 90, 0, 0, 0, 100, 80, true);      // below
    region(-9, 0, -1.0f, 5, 0, 0, 0, 100, 80, true);      // left
    region(0, -9, 5, -1.0f, 0, 0, 0, 100, 80, true);      // above
    region(5, 0, 4.5f, 5, 0, 0, 0, 100, 80, true);        // inverted
    region(0, 6, 5, 5.5f, 0, 0, 0, 100, 80, true);
    region(5, 5, 5, 5, 4, 4, 4, 100, 80, false, 5, 5, 5, 5); // an empty box is one pixel
    // the int32 ends: no side is ever computed for a skipped row, and a kept one lies in the frame
    region(2147483648.0f, 0, 4294967296.0f, 5, 0, 0, 0, 32768, 32768, true);
    region(-4294967296.0f, 0, -2147483904.0f, 5, 0, 0, 0, 32768, 32768, true);
    region(-4294967296.0f, -4294967296.0f, 4294967296.0f, 4294967296.0f, 0, 0, 0, 32768, 32768, false, 0, 0, 32767, 32767);
    region(-4294967296.0f, -4294967296.0f, 4294967296.0f, 4294967296.0f, 4, 4, 4, 32768, 32768, false, 0, 0, 32767, 32767);
    region(2147483520.0f, 2147483520.0f, 2147483520.0f, 2147483520.0f, 4, 4, 4, 32768, 32768, true);
    // the f32 ends: bw overflows to +inf; with a margin of 0 its product is a NaN and the row is skipped, with any other the
    // region is the whole frame; a box at +max alone keeps a finite bw
    region(-kMax, -kMax, kMax, kMax, 0, 0, 0, 1920, 1080, true);
    region(-kMax, -kMax, kMax, kMax, 0.1f, 0.2f, 0.1f, 1920, 1080, false, 0, 0, 1919, 1079);
    region(-kMax, 0, kMax, 5, 0.1f, 0, 0, 1920, 1080, false, 0, 0, 1919, 5);
    region(-kMax, 0, kMax, 5, 0, 0.5f, 0.5f, 1920, 1080, true);
    region(0, 0, kMax, kMax, 4, 4, 4, 1920, 1080, false, 0, 0, 1919, 1079);
    region(kMax, kMax, kMax, kMax, 4, 4, 4, 1920, 1080, true);
    region(-kMax, -kMax, -kMax, -kMax, 4, 4, 4, 1920, 1080, true);
    for (int k = 0; k < 4; ++k)
        for (float bad : {kNan, kInf, -kInf}) {
            float b[4] = {2, 3, 6, 7};
            b[k] = bad;
            region(b[0], b[1], b[2], b[3], 0.1f, 0.2f, 0.1f, 100, 80, true);
            region(b[0], b[1], b[2], b[3], 0, 0, 0, 100, 80, true);
        }

    // ---- the ellipse ----
    for (int w = 1; w <= 48; ++w)
        for (int h = 1; h <= 48; ++h) ellipse(w, h);
    for (int w : {1, 2, 3, 1000, 32767, 32768})
        for (int h : {1, 2, 3, 1000, 32767, 32768})
            if ((long long)w * h > 48 * 48) ellipse(w, h);
    CHECK(rd_sq(32768) * rd_sq(32768) == (1ull << 60), "w^2 h^2 at the limit");
    CHECK(!rd_ellipse_covers(-32767, -32767, 32768, 32768) && rd_ellipse_covers(-32767, 1, 32768, 32768) && !rd_ellipse_covers(-32767, 257, 32768, 32768),
          "the corner and the rim at the limit");

    // ---- the tiles ----
    for (int cell = kRdMinCell; cell <= kRdMaxCell; ++cell) tiles_of(cell);
    CHECK(rd_frame_tiles(32768, 32768, 33) == 993 * 993, "the tiles of the largest frame: %d", rd_frame_tiles(32768, 32768, 33));
    {
        ++steps;
        const uint8_t px = 0;
        const rfd_image fr[3] = {image(200, 150, 600, &px), image(1920, 1080, 5760, &px), image(1, 1, 3, &px)};
        const RdGrid g = rd_grid(fr, 3, 16);
        CHECK(g.x == 30u * 17u && g.y == 3u, "grid %u x %u", g.x, g.y);
        const RdGrid g3 = rd_grid(fr, 3, 3); // tiles of 63
        CHECK(g3.x == 31u * 18u && g3.y == 3u, "grid %u x %u", g3.x, g3.y);
        const RdGrid g1 = rd_grid(fr + 2, 1, 64);
        CHECK(g1.x == 1u && g1.y == 1u, "grid %u x %u", g1.x, g1.y);
    }

    // ---- the bounds ----
    {
        char msg[160];
        rfd_redact_config c;
        std::memset(&c, 0, sizeof c);
        c.mode = RFD_REDACT_PIXELATE; c.shape = RFD_REDACT_ELLIPSE; c.cell = 16; c.margin_x = 0.1f; c.margin_top = 0.2f; c.margin_bottom = 0.1f;
        ++steps;
        CHECK(rd_config_ok(c, msg, sizeof msg), "the default: %s", msg);
        auto bad = [&](const char *field, auto change) {
            ++steps;
            rfd_redact_config d = c;
            change(d);
            msg[0] = 0;
            CHECK(!rd_config_ok(d, msg, sizeof msg) && std::strstr(msg, field), "%s: %s", field, msg);
        };
        bad("mode", [](rfd_redact_config &d) { d.mode = 2; });
        bad("mode", [](rfd_redact_config &d) { d.mode = -1; });
        bad("shape", [](rfd_redact_config &d) { d.shape = 2; });
        bad("cell", [](rfd_redact_config &d) { d.cell = 1; });
        bad("cell", [](rfd_redact_config &d) { d.cell = 65; });
        bad("fill", [](rfd_redact_config &d) { d.fill[3] = 1; });
        bad("margin_x", [](rfd_redact_config &d) { d.margin_x = -0.1f; });
        bad("margin_x", [](rfd_redact_config &d) { d.margin_x = kNan; });
        bad("margin_top", [](rfd_redact_config &d) { d.margin_top = 4.5f; });
        bad("margin_top", [](rfd_redact_config &d) { d.margin_top = kInf; });
        bad("margin_bottom", [](rfd_redact_config &d) { d.margin_bottom = -kInf; });
        bad("reserved", [](rfd_redact_config &d) { d.reserved[5] = 1; });
        for (int cell : {2, 64}) { ++steps; rfd_redact_config d = c; d.cell = cell; d.margin_x = 4.0f; d.margin_top = 0.0f; CHECK(rd_config_ok(d, msg, sizeof msg), "cell %d: %s", cell, msg); }
        const uint8_t px = 0;
        auto frame = [&](rfd_image im, const char *why) {
            ++steps;
            msg[0] = 0;
            const bool ok = rd_frame_ok(im, "frame", 3, msg, sizeof msg);
            if (why) CHECK(!ok && std::strstr(msg, why) && std::strstr(msg, "frame 3"), "%s: %s", why, msg);
            else CHECK(ok, "%s", msg);
        };
        frame(image(32768, 32768, 98304, &px), nullptr);
        frame(image(1, 1, 3, &px), nullptr);
        frame(image(10, 10, 30, nullptr), "data");
        frame(image(0, 10, 30, &px), "non-positive");
        frame(image(10, -1, 30, &px), "non-positive");
        frame(image(32769, 10, 98307, &px), "exceeds 32768");
        frame(image(10, 10, 29, &px), "stride");
        ++steps;
        CHECK(rd_dst_ok(image(10, 8, 31, &px), image(10, 8, 30, &px), 0, msg, sizeof msg), "%s", msg);
        CHECK(!rd_dst_ok(image(10, 9, 31, &px), image(10, 8, 30, &px), 2, msg, sizeof msg) && std::strstr(msg, "dst 2: size"), "%s", msg);
        CHECK(!rd_dst_ok(image(10, 8, 29, &px), image(10, 8, 30, &px), 1, msg, sizeof msg) && std::strstr(msg, "dst 1: stride"), "%s", msg);
    }

    std::printf("%ld steps, %ld checks, %ld failures\n", steps, checks, failures);
    return failures ? 1 : 0;
}
