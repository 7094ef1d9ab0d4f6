// annotate_plan_check.cpp -- csrc/annotate_plan.h alone, built by the host compiler, plain and under AddressSanitizer and UBSan
// (tests/test_annotate_cpu.py).  The box at the int32 and f32 ends (an overflow anywhere is a UBSan report); an_layer on CLAMPED rows
// against the rule of rfd.h written here once more in int64 on the UNCLAMPED values -- over an exhaustive small sweep, where the
// extent must also hold every covered pixel, and over coordinates around +-2^20 and at the int32 ends with pixels at both ends of a
// 32768-pixel side for every legal thickness, radius and scale (the clamp proof); the formatting of every value 0 .. 999, of the
// value part at its rounding and its ends, and of labels at the int32 ends; the font; the styles, the blend, the grid and the
// bounds of the config.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <limits>
#include <string>
#include <vector>

#include "../../rs-face-detection_amd/csrc/annotate_plan.h"

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
static const int32_t kIMax = std::numeric_limits<int32_t>::max(), kIMin = std::numeric_limits<int32_t>::min();

// ---- the box ----
static void box(float x1, float y1, float x2, float y2, float mx, float mt, float mb, bool skipped, int32_t XA = 0, int32_t YA = 0, int32_t XB = 0, int32_t YB = 0)
{
    ++steps;
    const AnBox g = an_box(x1, y1, x2, y2, mx, mt, mb);
    CHECK(g.skipped == skipped, "box %g %g %g %g margins %g %g %g: skipped %d", x1, y1, x2, y2, mx, mt, mb, (int)g.skipped);
    if (!skipped && !g.skipped)
        CHECK(g.xa == XA && g.ya == YA && g.xb == XB && g.yb == YB, "box %g %g %g %g: %d %d %d %d", x1, y1, x2, y2, g.xa, g.ya, g.xb, g.yb);
}

// ---- the rule of rfd.h in int64 on unclamped values ----
struct Row {
    int64_t xa, ya, xb, yb;
    int64_t mx[5], my[5];
    bool on[5];
    std::vector<int> text;
};

static int rule_layer(const Row &r, int64_t t, int64_t rad, int64_t s, int64_t x, int64_t y)
{
    int layer = 0;
    if (t > 0 && r.xa <= x && x <= r.xb && r.ya <= y && y <= r.yb && (x < r.xa + t || x > r.xb - t || y < r.ya + t || y > r.yb - t)) layer = 1;
    if (rad > 0)
        for (int m = 0; m < 5; ++m)
            if (r.on[m]) {
                const __int128 dx = x - r.mx[m], dy = y - r.my[m];
                if (dx * dx + dy * dy <= (__int128)(rad * rad)) layer = 2;
            }
    const int64_t len = (int64_t)r.text.size();
    if (len > 0) {
        const int64_t pw = s * (6 * len + 1), ph = 9 * s, px = r.xa, py = r.ya - ph >= 0 ? r.ya - ph : r.ya;
        if (x >= px && x < px + pw && y >= py && y < py + ph) {
            layer = 3;
            const int64_t fx = (x - px) / s, fy = (y - py) / s;
            if (fx >= 1 && fy >= 1) {
                const int64_t k = (fx - 1) / 6, u = (fx - 1) % 6, v = fy - 1;
                if (k < len && u < 5 && v < 7 && ((kAnFont[r.text[(size_t)k]][v] >> (4 - u)) & 1)) layer = 4;
            }
        }
    }
    return layer;
}

static AnRow clamped(const Row &r, int rad)
{
    AnRow c;
    const AnBox b = {(int32_t)r.xa, (int32_t)r.ya, (int32_t)r.xb, (int32_t)r.yb, false};
    an_row_box(c, b);
    for (int m = 0; m < 5; ++m) {
        const bool on = r.on[m] && rad > 0;
        c.mx[m] = on ? an_clamp((int32_t)r.mx[m]) : kAnNoMark;
        c.my[m] = on ? an_clamp((int32_t)r.my[m]) : kAnNoMark;
    }
    c.text.glyphs = 0;
    c.text.len = 0;
    for (int g : r.text) an_put(c.text, (uint32_t)g);
    return c;
}

// pixel (x, y) of a frame: the clamped row gives the rule's layer, and a covered pixel lies in the extent
static void pixel(const Row &r, const AnRow &c, const AnExtent &e, int t, int rad, int s, int32_t x, int32_t y)
{
    const int want = rule_layer(r, t, rad, s, x, y), got = an_layer(c, t, rad, s, kAnFont, x, y);
    CHECK(want == got, "box %lld %lld %lld %lld t %d r %d s %d len %d: pixel %d, %d: layer %d, the rule says %d", (long long)r.xa, (long long)r.ya,
          (long long)r.xb, (long long)r.yb, t, rad, s, (int)r.text.size(), x, y, got, want);
    if (want) CHECK(e.x0 <= x && x <= e.x1 && e.y0 <= y && y <= e.y1, "pixel %d, %d is covered outside the extent %d %d %d %d", x, y, e.x0, e.y0, e.x1, e.y1);
}

static Row plain_row(int64_t xa, int64_t ya, int64_t xb, int64_t yb)
{
    Row r;
    r.xa = xa; r.ya = ya; r.xb = xb; r.yb = yb;
    for (int m = 0; m < 5; ++m) { r.mx[m] = r.my[m] = 0; r.on[m] = false; }
    return r;
}

// every pixel of a small frame, for small boxes around and across it
static void small_sweep()
{
    const int W = 26, H = 22;
    for (int t : {0, 1, 3})
        for (int rad : {0, 2})
            for (int s : {1, 2})
                for (int len : {0, 2})
                    for (int xa = -4; xa <= W + 1; xa += 3)
                        for (int ya = -4; ya <= H + 1; ya += 3)
                            for (int bw : {0, 1, 4, 40})
                                for (int bh : {0, 2, 40}) {
                                    ++steps;
                                    Row r = plain_row(xa, ya, xa + bw, ya + bh);
                                    r.mx[0] = xa + 2; r.my[0] = ya + 1; r.on[0] = true;
                                    r.mx[3] = xa + bw; r.my[3] = ya - 3; r.on[3] = true;
                                    for (int k = 0; k < len; ++k) r.text.push_back((7 * k + xa + 40) % kAnGlyphs);
                                    const AnRow c = clamped(r, rad);
                                    const AnExtent e = an_extent(c, t, rad, s);
                                    for (int y = 0; y < H; ++y)
                                        for (int x = 0; x < W; ++x) pixel(r, c, e, t, rad, s, x, y);
                                }
}

// The clamp: coordinates around +-2^20, at the int32 ends and near a 32768-pixel frame, against pixels at both ends of the frame
// and next to every plate, mark and band that could reach them, for every legal thickness, radius and scale.
static void clamp_proof()
{
    const int64_t C = kAnClamp;
    std::vector<int64_t> far = {kIMin, kIMin + 1, -C - 400, -C - 1, -C, -C + 1, -C + 16, -C + 364, -40000, -364, -17, -1, 0, 5, 16, 363, 32750,
                                32767, 32768, 33200, C - 364, C - 17, C - 1, C, C + 1, C + 400, kIMax - 1, kIMax};
    const std::vector<int64_t> ys = {kIMin, -C - 1, -17, 0, 36, 32767, C + 1, kIMax};
    const std::vector<int32_t> px = {0, 1, 8, 15, 16, 17, 35, 36, 363, 364, 32767 - 364, 32767 - 16, 32766, 32767};
    const std::vector<int32_t> py = {0, 16, 36, 32767 - 16, 32767};
    for (int t = 0; t <= kAnMaxThickness; ++t)                       // the outline
        for (int64_t xa : far)
            for (int64_t xb : far)
                for (int64_t ya : ys)
                    for (int64_t yb : ys) {
                        if (xb < xa || yb < ya) continue;
                        ++steps;
                        const Row r = plain_row(xa, ya, xb, yb);
                        const AnRow c = clamped(r, 0);
                        const AnExtent e = an_extent(c, t, 0, 1);
                        for (int32_t y : py)
                            for (int32_t x : px) pixel(r, c, e, t, 0, 1, x, y);
                    }
    for (int rad = 0; rad <= kAnMaxRadius; ++rad)                    // the marks
        for (int64_t cx : far)
            for (int64_t cy : far) {
                ++steps;
                Row r = plain_row(-5, -5, -4, -4);
                r.mx[2] = cx; r.my[2] = cy; r.on[2] = true;
                r.mx[4] = cy; r.my[4] = 3; r.on[4] = true;
                const AnRow c = clamped(r, rad);
                const AnExtent e = an_extent(c, 0, rad, 1);
                for (int32_t y : px)
                    for (int32_t x : px) pixel(r, c, e, 0, rad, 1, x, y);
            }
    for (int s = 1; s <= kAnMaxScale; ++s)                           // the plate and the text
        for (int len : {1, 2, kAnMaxGlyphs})
            for (int64_t xa : far)
                for (int64_t ya : far) {
                    ++steps;
                    Row r = plain_row(xa, ya, xa < kIMax - 50 ? xa + 50 : kIMax, ya < kIMax - 50 ? ya + 50 : kIMax);
                    for (int k = 0; k < len; ++k) r.text.push_back((k + 8) % kAnGlyphs);
                    const AnRow c = clamped(r, 0);
                    const AnExtent e = an_extent(c, 0, 0, s);
                    for (int32_t y : px)
                        for (int32_t x : px) pixel(r, c, e, 0, 0, s, x, y);
                }
}

// ---- text ----
static std::string decode(const AnText &t)
{
    std::string s;
    for (int k = 0; k < t.len; ++k) s += "0123456789-?% "[(t.glyphs >> (4 * k)) & 15u];
    return s;
}

static void text(int label_source, int32_t label, int value_source, float value, const char *want)
{
    ++steps;
    const AnText t = an_text(label_source, label, value_source, value);
    CHECK(decode(t) == want && t.len <= kAnMaxGlyphs && (t.len == 15 || (t.glyphs >> (4 * t.len)) == 0), "label %d value %g: \"%s\", want \"%s\"", label, value,
          decode(t).c_str(), want);
}

static void texts()
{
    char buf[32];
    for (uint32_t v = 0; v <= 999; ++v) {                           // every value the value part can print, and the same as a label
        ++steps;
        AnText t = {0, 0};
        an_put_decimal(t, v);
        std::snprintf(buf, sizeof buf, "%u", v);
        CHECK(decode(t) == buf, "%u prints \"%s\"", v, decode(t).c_str());
        std::snprintf(buf, sizeof buf, "%u 7%%", v);
        text(RFD_ANNOTATE_ARRAY, (int32_t)v, RFD_ANNOTATE_ARRAY, 0.07f, buf);
    }
    const int A = RFD_ANNOTATE_ARRAY, N = RFD_ANNOTATE_NONE, S = RFD_ANNOTATE_SCORE;
    text(N, 5, N, 0.5f, "");
    text(A, 0, N, 0.5f, "0");
    text(A, -1, N, 0.5f, "?");
    text(A, kIMin, N, 0.5f, "?");
    text(A, kIMax, N, 0.5f, "2147483647");
    text(A, kIMax, A, 50.0f, "2147483647 999%");                    // 15 glyphs, the longest
    text(A, kIMin, S, kNan, "? --%");
    text(A, 7, S, 0.5f, "7 50%");
    const float half = 0.005f;
    struct { float v; const char *want; } values[] = {
        {0.0f, "0%"}, {-0.0f, "0%"}, {0.004f, "0%"}, {std::nextafter(half, 0.0f), "0%"}, {half, "1%"}, {std::nextafter(half, 1.0f), "1%"}, {0.5f, "50%"},
        {0.83f, "83%"}, {1.0f, "100%"}, {9.98f, "998%"}, {9.99f, "999%"}, {10.0f, "999%"}, {1e30f, "999%"}, {kMax, "999%"}, {3e7f, "999%"},
        {kInf, "--%"}, {-kInf, "--%"}, {kNan, "--%"}, {-1e-30f, "--%"}, {-1.0f, "--%"},
    };
    for (const auto &c : values) {
        text(N, 0, A, c.v, c.want);
        text(N, 0, S, c.v, c.want);
    }
}

static void font()
{
    for (int g = 0; g < kAnGlyphs; ++g) {
        ++steps;
        for (int v = 0; v < 7; ++v) CHECK(kAnFont[g][v] < 32, "glyph %d row %d leaves 5 columns", g, v);
        for (int h = 0; h < g; ++h) CHECK(std::memcmp(kAnFont[g], kAnFont[h], 7) != 0, "glyphs %d and %d are the same", g, h);
    }
}

static void styles_blend_grid()
{
    const uint32_t mask[4] = {3, 3, 4, 0}, value[4] = {1, 2, 4, 0};
    ++steps;
    CHECK(an_style(1, 4, mask, value) == 0 && an_style(2, 4, mask, value) == 1 && an_style(7, 4, mask, value) == 2 && an_style(0, 4, mask, value) == 3, "first match");
    CHECK(an_style(0, 3, mask, value) == -1 && an_style(4, 2, mask, value) == -1 && an_style(5, 4, mask, value) == 0, "no match, n_styles");
    for (uint32_t a = 1; a <= 256; ++a)
        for (uint32_t c : {0u, 1u, 128u, 255u})
            for (uint32_t p : {0u, 1u, 127u, 255u}) {
                const uint32_t got = an_blend(c, p, a);
                CHECK(got <= 255u && got == (a == 256 ? c : (uint32_t)std::floor((a * c + (256.0 - a) * p + 128.0) / 256.0)), "blend %u %u %u", c, p, a);
                if (c == p) CHECK(got == c, "a blend of equals moves: %u at %u -> %u", c, a, got);
            }
    rfd_image imgs[3];
    std::memset(imgs, 0, sizeof imgs);
    imgs[0].width = 1; imgs[0].height = 1;
    imgs[1].width = 65; imgs[1].height = 128;
    imgs[2].width = 1920; imgs[2].height = 1080;
    ++steps;
    CHECK(an_grid(imgs, 1).x == 1 && an_grid(imgs, 2).x == 4 && an_grid(imgs, 3).x == 30 * 17 && an_grid(imgs, 3).y == 3, "grid");
}

static void config()
{
    char msg[160];
    rfd_annotate_config ok;
    std::memset(&ok, 0, sizeof ok);
    ok.n_styles = 1; ok.thickness = 2; ok.mark_radius = 2; ok.value_source = RFD_ANNOTATE_SCORE; ok.text_scale = 2; ok.alpha = 256;
    ++steps;
    CHECK(an_config_ok(ok, msg, sizeof msg), "the default is refused: %s", msg);
    auto refused = [&](const char *field, void (*change)(rfd_annotate_config &)) {
        ++steps;
        rfd_annotate_config c = ok;
        change(c);
        msg[0] = 0;
        CHECK(!an_config_ok(c, msg, sizeof msg) && std::strstr(msg, field), "%s: \"%s\"", field, msg);
    };
    refused("n_styles", [](rfd_annotate_config &c) { c.n_styles = 0; });
    refused("n_styles", [](rfd_annotate_config &c) { c.n_styles = 5; });
    refused("style", [](rfd_annotate_config &c) { c.style[1].sel_mask = 1; });
    refused("style", [](rfd_annotate_config &c) { c.style[3].colour[2] = 1; });
    refused("colour[3]", [](rfd_annotate_config &c) { c.style[0].colour[3] = 1; });
    refused("thickness", [](rfd_annotate_config &c) { c.thickness = -1; });
    refused("thickness", [](rfd_annotate_config &c) { c.thickness = 17; });
    refused("mark_radius", [](rfd_annotate_config &c) { c.mark_radius = -1; });
    refused("mark_radius", [](rfd_annotate_config &c) { c.mark_radius = 9; });
    refused("label_source", [](rfd_annotate_config &c) { c.label_source = RFD_ANNOTATE_SCORE; });
    refused("label_source", [](rfd_annotate_config &c) { c.label_source = -1; });
    refused("value_source", [](rfd_annotate_config &c) { c.value_source = 3; });
    refused("text_scale", [](rfd_annotate_config &c) { c.text_scale = 0; });
    refused("text_scale", [](rfd_annotate_config &c) { c.text_scale = 5; });
    refused("text_colour", [](rfd_annotate_config &c) { c.text_colour[3] = 9; });
    refused("alpha", [](rfd_annotate_config &c) { c.alpha = 0; });
    refused("alpha", [](rfd_annotate_config &c) { c.alpha = 257; });
    refused("margin_x", [](rfd_annotate_config &c) { c.margin_x = std::numeric_limits<float>::quiet_NaN(); });
    refused("margin_top", [](rfd_annotate_config &c) { c.margin_top = 4.5f; });
    refused("margin_bottom", [](rfd_annotate_config &c) { c.margin_bottom = -0.5f; });
    refused("reserved", [](rfd_annotate_config &c) { c.reserved[3] = 1; });
    for (int t : {0, 16})
        for (int a : {1, 256}) {
            rfd_annotate_config c = ok;
            c.thickness = t; c.alpha = a; c.mark_radius = t / 2; c.text_scale = 1 + t / 6; c.n_styles = 4;
            CHECK(an_config_ok(c, msg, sizeof msg), "a legal config is refused: %s", msg);
        }
}

int main()
{
    // the box: the redaction's region line without the clip
    box(3.0f, 2.0f, 9.5f, 7.25f, 0, 0, 0, false, 3, 2, 9, 7);
    box(-0.5f, -0.5f, 2.9f, 3.0f, 0, 0, 0, false, 0, 0, 2, 3);
    box(8, 8, 12, 12, 0.25f, 0.5f, 0.75f, false, 7, 6, 13, 15);
    box(-3e9f, -3e9f, 3e9f, 3e9f, 0, 0, 0, false, kIMin, kIMin, kIMax, kIMax);
    box(3e9f, 1, 3e9f, 5, 0, 0, 0, false, kIMax, 1, kIMax, 5);
    box(-kMax, -kMax, kMax, kMax, 0, 0, 0, true);                                   // bw = +inf, inf * 0 = NaN
    box(-kMax, -kMax, kMax, kMax, 0.1f, 0.2f, 0.1f, false, kIMin, kIMin, kIMax, kIMax);
    box(2147483520.0f, 0, 2147483648.0f, 5, 0, 0, 0, false, 2147483520, 0, kIMax, 5);
    box(-2147483648.0f, 0, -2147483520.0f, 5, 4, 0, 0, false, kIMin, 0, -2147483008, 5);
    box(5, 2, 4.5f, 6, 0, 0, 0, true);
    box(2, 6, 5, 5.5f, 4, 4, 4, true);
    for (int k = 0; k < 4; ++k)
        for (float bad : {kNan, kInf, -kInf}) {
            float r[4] = {2, 3, 6, 7};
            r[k] = bad;
            box(r[0], r[1], r[2], r[3], 0.1f, 0.1f, 0.1f, true);
        }
    small_sweep();
    clamp_proof();
    texts();
    font();
    styles_blend_grid();
    config();
    std::printf("%ld steps, %ld checks, %ld failures\n", steps, checks, failures);
    return failures ? 1 : 0;
}
