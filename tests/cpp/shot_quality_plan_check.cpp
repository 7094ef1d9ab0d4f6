// shot_quality_plan_check.cpp -- csrc/shot_quality_plan.h alone, built by the host compiler, plain and under AddressSanitizer
// and UBSan (tests/test_shot_quality_cpu.py).  The inverse cell map against the edges for every side of 32 .. 4096 pixels and
// every pixel of it (and for sampled sides up to the limit of 32768, the limit included): the edges start at 0, end at the side,
// leave no cell empty, and pixel `rel` lies in [edge(cell), edge(cell + 1)); the kernel's stepping of the remainder by 32 per
// pixel lands on the same cell.  Then the region of boxes at the int32 extremes, infinities and NaNs (an overflow anywhere is
// a UBSan report), and the bounds of the config and of a frame.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>

#include "../../rs-face-detection_amd/csrc/shot_quality_plan.h"

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

static void side(int len)
{
    ++steps;
    int32_t edge[kSqGrid + 1];
    for (int k = 0; k <= kSqGrid; ++k) edge[k] = sq_edge(k, len);
    CHECK(edge[0] == 0 && edge[kSqGrid] == len, "len %d: edges run %d .. %d", len, edge[0], edge[kSqGrid]);
    for (int k = 0; k < kSqGrid; ++k) CHECK(edge[k] < edge[k + 1], "len %d: cell %d is empty", len, k);
    // every pixel: the inverse, and the kernel's way to it (one division per group of four, then the remainder stepped)
    uint32_t col = 0, rem = 0;
    for (int rel = 0; rel < len; ++rel) {
        const int c = sq_cell(rel, len);
        CHECK(c >= 0 && c < kSqGrid && edge[c] <= rel && rel < edge[c + 1], "len %d: pixel %d in cell %d", len, rel, c);
        if ((rel & 3) == 0) {
            const uint32_t num = 32u * (uint32_t)(rel + 1) - 1u;
            col = num / (uint32_t)len;
            rem = num - col * (uint32_t)len;
        } else {
            rem += 32u;
            if (rem >= (uint32_t)len) { rem -= (uint32_t)len; ++col; }
        }
        CHECK((int)col == c, "len %d: pixel %d stepped to cell %u, not %d", len, rel, col, c);
    }
}

static void region(float x1, float y1, float x2, float y2, int W, int H, int32_t X0, int32_t Y0, int32_t X1, int32_t Y1, long long w, long long h)
{
    ++steps;
    const SqRegion g = sq_region(x1, y1, x2, y2, W, H);
    CHECK(g.x0 == X0 && g.y0 == Y0 && g.x1 == X1 && g.y1 == Y1, "box %g %g %g %g: region %d %d %d %d", x1, y1, x2, y2, g.x0, g.y0, g.x1, g.y1);
    CHECK((long long)g.w == w && (long long)g.h == h, "box %g %g %g %g: sides %lld %lld", x1, y1, x2, y2, (long long)g.w, (long long)g.h);
    CHECK(g.measured == (w >= 32 && h >= 32), "box %g %g %g %g: measured %d", x1, y1, x2, y2, (int)g.measured);
    if (g.measured) CHECK(g.x0 >= 0 && g.y0 >= 0 && g.x1 < W && g.y1 < H, "a measured region leaves the frame");
}

int main()
{
    for (int len = 32; len <= 4096; ++len) side(len);
    for (int len = 4097; len < kSqMaxSide; len += 331) side(len);
    for (int len = kSqMaxSide - 3; len <= kSqMaxSide; ++len) side(len);
    static const int more[] = {1080, 1920, 3840, 8192, 16384, 16385};
    for (int len : more) side(len);

    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const int32_t imax = std::numeric_limits<int32_t>::max(), imin = std::numeric_limits<int32_t>::min();
    // as_i32: toward zero, saturating, NaN -> 0
    CHECK(sq_as_i32(1.75f) == 1 && sq_as_i32(-1.75f) == -1 && sq_as_i32(-0.0f) == 0, "truncation");
    CHECK(sq_as_i32(2147483648.0f) == imax && sq_as_i32(2147483520.0f) == 2147483520 && sq_as_i32(inf) == imax && sq_as_i32(3e38f) == imax, "upper end");
    CHECK(sq_as_i32(-2147483648.0f) == imin && sq_as_i32(-2147483904.0f) == imin && sq_as_i32(-inf) == imin && sq_as_i32(-3e38f) == imin, "lower end");
    CHECK(sq_as_i32(nan) == 0 && sq_as_i32(-nan) == 0, "NaN");
    // regions: ordinary, clipped at each side, outside, and the extremes, whose sides need more than 32 bits
    region(3.5f, 2.25f, 40.75f, 50.5f, 100, 100, 3, 2, 40, 50, 38, 49);
    region(-10.f, 20.f, 50.f, 70.f, 100, 100, 0, 20, 50, 70, 51, 51);
    region(20.f, -10.5f, 70.f, 50.f, 100, 100, 20, 0, 70, 50, 51, 51);
    region(60.f, 20.f, 200.f, 70.f, 100, 100, 60, 20, 99, 70, 40, 51);
    region(20.f, 60.f, 70.f, 200.f, 100, 100, 20, 60, 70, 99, 51, 40);
    region(200.f, 20.f, 300.f, 70.f, 100, 100, 200, 20, 99, 70, -100, 51);
    region(nan, nan, nan, nan, 100, 100, 0, 0, 0, 0, 1, 1);
    region(-inf, -inf, inf, inf, 100, 80, 0, 0, 99, 79, 100, 80);
    region(inf, inf, -inf, -inf, 100, 80, imax, imax, imin, imin, (long long)imin - imax + 1, (long long)imin - imax + 1);
    region(10.f, 20.f, -inf, 70.f, 100, 100, 10, 20, imin, 70, (long long)imin - 10 + 1, 51);
    region(inf, 20.f, 50.f, 70.f, 100, 100, imax, 20, 50, 70, 50ll - imax + 1, 51);
    region(-3e38f, -3e38f, 3e38f, 3e38f, kSqMaxSide, kSqMaxSide, 0, 0, kSqMaxSide - 1, kSqMaxSide - 1, kSqMaxSide, kSqMaxSide);
    region(0.f, 0.f, 30.f, 31.f, 100, 100, 0, 0, 30, 31, 31, 32);
    region(0.f, 0.f, 31.f, 31.f, 100, 100, 0, 0, 31, 31, 32, 32);
    region(0.f, 0.f, 31.f, 31.f, 31, 100, 0, 0, 30, 31, 31, 32);   // the frame is the narrower one

    // the config bounds: the default passes, every field refuses by name
    char msg[128];
    rfd_shot_quality_config c;
    auto fresh = [&]() {
        std::memset(&c, 0, sizeof c);
        c.dark = 30; c.bright = 225; c.pitch0 = 0.495f; c.w_yaw = 1.f; c.w_roll = 1.f; c.w_pitch = 2.f; c.sharp_ref = 64.f; c.size_ref = 112.f;
    };
    auto refused = [&](const char *field) {
        ++steps;
        msg[0] = 0;
        const bool ok = sq_config_ok(c, msg, sizeof msg);
        CHECK(!ok && std::strstr(msg, field) != nullptr, "%s: ok %d, \"%s\"", field, (int)ok, msg);
        fresh();
    };
    fresh();
    CHECK(sq_config_ok(c, msg, sizeof msg), "the default is refused: %s", msg);
    c.dark = 0; c.bright = 255; c.w_yaw = c.w_roll = c.w_pitch = 0.f;
    CHECK(sq_config_ok(c, msg, sizeof msg), "the widest thresholds and zero weights are refused: %s", msg);
    fresh();
    c.dark = -1; refused("dark");
    c.dark = 256; c.bright = 300; refused("dark");
    c.bright = 256; refused("bright");
    c.bright = -1; refused("bright");
    c.dark = 100; c.bright = 100; refused("dark");
    c.dark = 101; c.bright = 100; refused("dark");
    const float bad[] = {nan, inf, -inf};
    for (float b : bad) {
        c.pitch0 = b; refused("pitch0");
        c.w_yaw = b; refused("w_yaw");
        c.w_roll = b; refused("w_roll");
        c.w_pitch = b; refused("w_pitch");
        c.sharp_ref = b; refused("sharp_ref");
        c.size_ref = b; refused("size_ref");
    }
    c.w_yaw = -1.f; refused("w_yaw");
    c.w_roll = -1.f; refused("w_roll");
    c.w_pitch = -0.5f; refused("w_pitch");
    c.sharp_ref = 0.f; refused("sharp_ref");
    c.sharp_ref = -1.f; refused("sharp_ref");
    c.size_ref = 0.f; refused("size_ref");
    c.times_score = 2; refused("times_score");
    c.times_score = -1; refused("times_score");

    // the frame bounds
    static const uint8_t px[3] = {0, 0, 0};
    auto frame = [&](const uint8_t *data, int h, int w, ptrdiff_t stride, const char *what) {
        ++steps;
        const rfd_image im = {data, h, w, stride};
        msg[0] = 0;
        const bool ok = sq_frame_ok(im, 7, msg, sizeof msg);
        if (what) CHECK(!ok && std::strstr(msg, what) != nullptr && std::strstr(msg, "frame 7") != nullptr, "%s: ok %d, \"%s\"", what, (int)ok, msg);
        else CHECK(ok, "a good frame is refused: %s", msg);
    };
    frame(px, 1, 1, 3, nullptr);
    frame(px, kSqMaxSide, kSqMaxSide, (ptrdiff_t)kSqMaxSide * 3 + 5, nullptr);
    frame(nullptr, 10, 10, 30, "data");
    frame(px, 0, 10, 30, "size");
    frame(px, 10, -1, 30, "size");
    frame(px, kSqMaxSide + 1, 10, 30, "32768");
    frame(px, 10, kSqMaxSide + 1, (ptrdiff_t)(kSqMaxSide + 1) * 3, "32768");
    frame(px, 10, 10, 29, "stride");
    frame(px, 10, 10, -30, "stride");

    std::printf("%ld steps, %ld checks, %ld failures\n", steps, checks, failures);
    return failures == 0 ? 0 : 1;
}
