// annotate_plan.h -- the geometry, the text and the argument checks of the annotation (include/rfd.h, "annotation"): the box of a
// row (the redaction's region, not clipped), the string of a row and its 5 x 7 font, the layer of a pixel, the extent a row can
// touch, the clamp of coordinates before they enter LDS, the tiles and the grid of a call, which bounds a config must keep.
// Plain code with nothing of HIP in it: tests/cpp/annotate_plan_check.cpp builds it with the host compiler alone, and
// kernels_annotate.hip compiles the very same functions for the device (AN_HD), so what the check program proves of the box, the
// extent, the clamp and the text holds for the kernel.  annotate_host.hip does the checks.
#pragma once
#include "redact_plan.h" // rd_as_i32, rd_finite, rd_tiles, the frame and dst checks: the annotation's are the redaction's

#define AN_HD RD_HD

namespace rfd {

constexpr int kAnTile = 64;            // a workgroup owns 64 x 64 pixels, cut by the frame's right and bottom edge
constexpr int kAnMaxThickness = 16, kAnMaxRadius = 8, kAnMaxScale = 4, kAnMaxGlyphs = 15, kAnGlyphs = 14;
constexpr int32_t kAnClamp = 1 << 20;  // coordinates in LDS lie in -2^20 .. 2^20 (an_clamp)
enum { kAnMinus = 10, kAnQuestion = 11, kAnPercent = 12, kAnSpace = 13 };

// The font: glyph g (0 .. 9 the digits, then - ? % space), row 0 .. 6 from the top, bit 4 the left column.  This initialiser
// is the only copy: the host table below, and the kernel's __constant__ table (kernels_annotate.hip) are built from it, and tests
// read it through rfd_debug_annotate_glyph.
#define AN_FONT_INIT                                                                                                               \
    {                                                                                                                              \
        {0x0E, 0x11, 0x13, 0x15, 0x19, 0x11, 0x0E}, /* 0 */ {0x04, 0x0C, 0x04, 0x04, 0x04, 0x04, 0x0E}, /* 1 */                    \
        {0x0E, 0x11, 0x01, 0x02, 0x04, 0x08, 0x1F}, /* 2 */ {0x1F, 0x02, 0x04, 0x02, 0x01, 0x11, 0x0E}, /* 3 */                    \
        {0x02, 0x06, 0x0A, 0x12, 0x1F, 0x02, 0x02}, /* 4 */ {0x1F, 0x10, 0x1E, 0x01, 0x01, 0x11, 0x0E}, /* 5 */                    \
        {0x06, 0x08, 0x10, 0x1E, 0x11, 0x11, 0x0E}, /* 6 */ {0x1F, 0x01, 0x02, 0x04, 0x08, 0x08, 0x08}, /* 7 */                    \
        {0x0E, 0x11, 0x11, 0x0E, 0x11, 0x11, 0x0E}, /* 8 */ {0x0E, 0x11, 0x11, 0x0F, 0x01, 0x02, 0x0C}, /* 9 */                    \
        {0x00, 0x00, 0x00, 0x1F, 0x00, 0x00, 0x00}, /* - */ {0x0E, 0x11, 0x01, 0x02, 0x04, 0x00, 0x04}, /* ? */                    \
        {0x18, 0x19, 0x02, 0x04, 0x08, 0x13, 0x03}, /* % */ {0x00, 0x00, 0x00, 0x00, 0x00, 0x00, 0x00}, /* space */                \
    }
typedef uint8_t AnFont[kAnGlyphs][7];
static const AnFont kAnFont = AN_FONT_INIT;

// The box of a row grown by its margins: the redaction's region line and skip conditions (rd_region), NOT clipped to the frame.
struct AnBox {
    int32_t xa, ya, xb, yb;
    bool skipped;
};

AN_HD inline AnBox an_box(float bx1, float by1, float bx2, float by2, float margin_x, float margin_top, float margin_bottom)
{
    AnBox g = {0, 0, -1, -1, true};
    if (!(rd_finite(bx1) && rd_finite(by1) && rd_finite(bx2) && rd_finite(by2))) return g;
    const float bw = bx2 - bx1, bh = by2 - by1;
    if (!(bw >= 0.0f) || !(bh >= 0.0f)) return g;
    const float gx = bw * margin_x, gt = bh * margin_top, gb = bh * margin_bottom;
    const float xa = bx1 - gx, xb = bx2 + gx, ya = by1 - gt, yb = by2 + gb;
    if (xa != xa || xb != xb || ya != ya || yb != yb) return g;
    g.xa = rd_as_i32(xa); g.ya = rd_as_i32(ya); g.xb = rd_as_i32(xb); g.yb = rd_as_i32(yb);
    g.skipped = g.xb < g.xa || g.yb < g.ya;
    return g;
}

// The string of a row: glyph k is bits 4 k .. 4 k + 3 of `glyphs`, len <= 15 (10 digits, a space, three digits, %).
struct AnText {
    uint64_t glyphs;
    int32_t len;
};

AN_HD inline void an_put(AnText &t, uint32_t glyph) { t.glyphs |= (uint64_t)glyph << (4 * t.len); ++t.len; }
AN_HD inline void an_put_decimal(AnText &t, uint32_t v)
{
    int nd = 1;
    for (uint32_t q = v; q >= 10u; q /= 10u) ++nd;
    for (int d = nd - 1; d >= 0; --d) {
        t.glyphs |= (uint64_t)(v % 10u) << (4 * (t.len + d));
        v /= 10u;
    }
    t.len += nd;
}
// what the value part prints before its %: 0 .. 999, or -1 for "--"
AN_HD inline int32_t an_percent(float v)
{
    if (!rd_finite(v) || !(v >= 0.0f)) return -1;
    const float scaled = v * 100.0f;
    const int32_t p = rd_as_i32(scaled + 0.5f);
    return p < 999 ? p : 999;
}
AN_HD inline AnText an_text(int label_source, int32_t label, int value_source, float value)
{
    AnText t = {0, 0};
    if (label_source == RFD_ANNOTATE_ARRAY) {
        if (label < 0) an_put(t, kAnQuestion);
        else an_put_decimal(t, (uint32_t)label);
    }
    if (value_source != RFD_ANNOTATE_NONE) {
        if (t.len) an_put(t, kAnSpace);
        const int32_t p = an_percent(value);
        if (p < 0) { an_put(t, kAnMinus); an_put(t, kAnMinus); }
        else an_put_decimal(t, (uint32_t)p);
        an_put(t, kAnPercent);
    }
    return t;
}

// A mark centre that no pixel of a frame can reach: what a non-finite landmark, or any landmark at radius 0, becomes.
constexpr int32_t kAnNoMark = -kAnClamp;

AN_HD inline int32_t an_clamp(int32_t v) { return v < -kAnClamp ? -kAnClamp : v > kAnClamp ? kAnClamp : v; }

// What a row carries into LDS, every coordinate clamped: for frames up to 32768 a side, thickness <= 16, radius <= 8 and scale
// <= 4 no in-frame pixel's layer changes by the clamp (annotate_plan_check.cpp sweeps it; a plate is at most 364 x 36).
struct AnRow {
    int32_t xa, ya, xb, yb;
    int32_t mx[5], my[5];
    AnText text;
};

AN_HD inline void an_row_box(AnRow &r, const AnBox &b) { r.xa = an_clamp(b.xa); r.ya = an_clamp(b.ya); r.xb = an_clamp(b.xb); r.yb = an_clamp(b.yb); }
AN_HD inline void an_row_mark(AnRow &r, int m, float lx, float ly, int radius)
{
    const bool on = radius > 0 && rd_finite(lx) && rd_finite(ly);
    r.mx[m] = on ? an_clamp(rd_as_i32(lx)) : kAnNoMark;
    r.my[m] = on ? an_clamp(rd_as_i32(ly)) : kAnNoMark;
}

// The plate of a row, from its (clamped) box.
struct AnPlate {
    int32_t px, py, pw, ph;
};
AN_HD inline AnPlate an_plate(int32_t xa, int32_t ya, int32_t len, int32_t scale)
{
    AnPlate p;
    p.pw = scale * (6 * len + 1);
    p.ph = 9 * scale;
    p.px = xa;
    p.py = ya - p.ph >= 0 ? ya - p.ph : ya;
    return p;
}

// The layer of pixel (x, y) of a frame under a row: 0 none, 1 outline, 2 mark, 3 plate, 4 text -- the highest that holds.
// x, y in 0 .. 32767 and clamped coordinates: every difference is below 2^21 + 2^15, and a square is taken only of |d| <= radius.
AN_HD inline int an_layer(const AnRow &r, int32_t thickness, int32_t radius, int32_t scale, const AnFont &font, int32_t x, int32_t y)
{
    if (r.text.len > 0) {
        const AnPlate p = an_plate(r.xa, r.ya, r.text.len, scale);
        if (x >= p.px && x < p.px + p.pw && y >= p.py && y < p.py + p.ph) {
            const int32_t fx = (int32_t)((uint32_t)(x - p.px) / (uint32_t)scale), fy = (int32_t)((uint32_t)(y - p.py) / (uint32_t)scale);
            if (fx >= 1 && fy >= 1) {
                const int32_t k = (fx - 1) / 6, u = (fx - 1) % 6, v = fy - 1;
                if (k < r.text.len && u < 5 && v < 7) {
                    const uint32_t glyph = (uint32_t)(r.text.glyphs >> (4 * k)) & 15u;
                    if ((font[glyph][v] >> (4 - u)) & 1) return 4;
                }
            }
            return 3;
        }
    }
    if (radius > 0) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int m = 0; m < 5; ++m) {
            const int32_t dx = x - r.mx[m], dy = y - r.my[m];
            if (dx >= -radius && dx <= radius && dy >= -radius && dy <= radius && dx * dx + dy * dy <= radius * radius) return 2;
        }
    }
    if (thickness > 0 && x >= r.xa && x <= r.xb && y >= r.ya && y <= r.yb &&
        (x < r.xa + thickness || x > r.xb - thickness || y < r.ya + thickness || y > r.yb - thickness))
        return 1;
    return 0;
}

// The extent of a row: the bounding box of outline, plate and mark squares, a conservative test of "may touch".  Empty
// (x1 < x0) when the row draws nothing.
struct AnExtent {
    int32_t x0, y0, x1, y1;
};
AN_HD inline AnExtent an_extent(const AnRow &r, int32_t thickness, int32_t radius, int32_t scale)
{
    AnExtent e = {kAnClamp * 2, kAnClamp * 2, -kAnClamp * 2, -kAnClamp * 2};
    auto grow = [&](int32_t x0, int32_t y0, int32_t x1, int32_t y1) {
        e.x0 = x0 < e.x0 ? x0 : e.x0; e.y0 = y0 < e.y0 ? y0 : e.y0;
        e.x1 = x1 > e.x1 ? x1 : e.x1; e.y1 = y1 > e.y1 ? y1 : e.y1;
    };
    if (thickness > 0) grow(r.xa, r.ya, r.xb, r.yb);
    if (r.text.len > 0) {
        const AnPlate p = an_plate(r.xa, r.ya, r.text.len, scale);
        grow(p.px, p.py, p.px + p.pw - 1, p.py + p.ph - 1);
    }
    if (radius > 0)
        for (int m = 0; m < 5; ++m)
            if (r.mx[m] != kAnNoMark || r.my[m] != kAnNoMark) grow(r.mx[m] - radius, r.my[m] - radius, r.mx[m] + radius, r.my[m] + radius);
    return e;
}

// The first style a selection word matches, or -1: the row is not drawn.
AN_HD inline int an_style(uint32_t word, int n_styles, const uint32_t mask[RFD_ANNOTATE_MAX_STYLES], const uint32_t value[RFD_ANNOTATE_MAX_STYLES])
{
    int k = -1;
    for (int i = RFD_ANNOTATE_MAX_STYLES - 1; i >= 0; --i)
        if (i < n_styles && (word & mask[i]) == value[i]) k = i;
    return k;
}

// The blend of a covered pixel's channel.
AN_HD inline uint32_t an_blend(uint32_t c, uint32_t p, uint32_t alpha) { return alpha == 256u ? c : (alpha * c + (256u - alpha) * p + 128u) >> 8; }

// The grid of a call: x = the tiles of its largest frame (workgroups past a smaller frame's tiles leave at once), y = the frame.
inline RdGrid an_grid(const rfd_image *imgs, int n)
{
    RdGrid g = {1, (uint32_t)n};
    for (int i = 0; i < n; ++i) {
        const uint32_t t = (uint32_t)rd_frame_tiles(imgs[i].width, imgs[i].height, kAnTile);
        if (t > g.x) g.x = t;
    }
    return g;
}

// The bounds of rfd_annotate_config; a refusal names its field in msg.
inline bool an_config_ok(const rfd_annotate_config &c, char *msg, size_t cap)
{
    auto no = [&](const char *what) { snprintf(msg, cap, "%s", what); return false; };
    auto margin = [](float m) { return rd_finite(m) && m >= 0.0f && m <= 4.0f; };
    auto source = [](int32_t s, bool score) { return s == RFD_ANNOTATE_NONE || s == RFD_ANNOTATE_ARRAY || (score && s == RFD_ANNOTATE_SCORE); };
    if (c.n_styles < 1 || c.n_styles > RFD_ANNOTATE_MAX_STYLES) return no("n_styles outside 1..4");
    for (int k = 0; k < RFD_ANNOTATE_MAX_STYLES; ++k) {
        const rfd_annotate_style &s = c.style[k];
        if (s.colour[3] != 0) return no("style: colour[3] is not 0");
        if (k >= c.n_styles && (s.sel_mask || s.sel_value || s.colour[0] || s.colour[1] || s.colour[2])) return no("style at or past n_styles is not zero");
    }
    if (c.thickness < 0 || c.thickness > kAnMaxThickness) return no("thickness outside 0..16");
    if (c.mark_radius < 0 || c.mark_radius > kAnMaxRadius) return no("mark_radius outside 0..8");
    if (!source(c.label_source, false)) return no("label_source is not NONE or ARRAY");
    if (!source(c.value_source, true)) return no("value_source is not NONE, ARRAY or SCORE");
    if (c.text_scale < 1 || c.text_scale > kAnMaxScale) return no("text_scale outside 1..4");
    if (c.text_colour[3] != 0) return no("text_colour[3] is not 0");
    if (c.alpha < 1 || c.alpha > 256) return no("alpha outside 1..256");
    if (!margin(c.margin_x)) return no("margin_x is not finite and in 0..4");
    if (!margin(c.margin_top)) return no("margin_top is not finite and in 0..4");
    if (!margin(c.margin_bottom)) return no("margin_bottom is not finite and in 0..4");
    for (int i = 0; i < 4; ++i)
        if (c.reserved[i] != 0) return no("reserved is not zero");
    return true;
}

} // namespace rfd
