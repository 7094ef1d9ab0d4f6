// frame_plan_check.cpp -- csrc/frame_plan.h alone, built by the host compiler, plain and under AddressSanitizer and UBSan
// (tests/test_frame_cpu.py).  The layout of every format at widths and heights 1 .. 9 and 4095 .. 4097 against the sizes
// written out here; every refusal of include/rfd.h ("frames in camera and decoder formats") with its status, its frame number
// and its cause in the message, and the FramePlan left as it was; the work items and first workgroups of mixed batches
// against sums written out by hand; a 32768-wide frame whose byte counts leave 32 bits (an overflow anywhere is a UBSan
// report).
#include <cstdio>
#include <cstring>
#include <initializer_list>

#include "../../rs-face-detection_amd/csrc/frame_plan.h"

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

static const uint8_t kBytes[64] = {0}; // planes are never read by the plan: any non-null address will do
static uint8_t kOut[64];

static rfd_frame frame(int format, int w, int h, int color = 0)
{
    rfd_frame f;
    memset(&f, 0, sizeof f);
    rfd_frame_layout l;
    memset(&l, 0, sizeof l);
    frame_layout(format, w, h, &l);
    for (int k = 0; k < 3; ++k) { f.plane[k] = kBytes; f.stride[k] = l.row_bytes[k]; }
    f.width = w; f.height = h; f.format = format; f.color = color;
    return f;
}
static rfd_image image(int w, int h) { return rfd_image{kOut, h, w, (ptrdiff_t)w * 3}; }

static void layouts()
{
    const int sides[] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 4095, 4096, 4097};
    for (int format = 0; format < kFrameFormats; ++format)
        for (int w : sides)
            for (int h : sides) {
                ++steps;
                rfd_frame_layout l;
                memset(&l, 0xEE, sizeof l);
                CHECK(frame_layout(format, w, h, &l), "%s %d x %d refused", frame_format_name(format), w, h);
                const int cw = w / 2 + w % 2, ch = h / 2 + h % 2; // ceil, written the other way
                int planes = 1, rb[3] = {0, 0, 0}, rows[3] = {h, 0, 0};
                switch (format) {
                case 0: case 1: rb[0] = w + w + w; break;
                case 2: case 3: rb[0] = w * 4; break;
                case 4: rb[0] = w; break;
                case 5: case 6: planes = 2; rb[0] = w; rb[1] = cw + cw; rows[1] = ch; break;
                case 7: planes = 3; rb[0] = w; rb[1] = rb[2] = cw; rows[1] = rows[2] = ch; break;
                default: rb[0] = cw * 4; break;
                }
                CHECK(l.planes == planes && l.reserved == 0, "%s %d x %d: %d planes", frame_format_name(format), w, h, l.planes);
                for (int k = 0; k < 3; ++k)
                    CHECK(l.row_bytes[k] == rb[k] && l.rows[k] == rows[k], "%s %d x %d plane %d: %d x %d, not %d x %d", frame_format_name(format), w, h, k,
                          l.rows[k], l.row_bytes[k], rows[k], rb[k]);
                // and its plan: one frame, quads and item rows
                rfd_frame f = frame(format, w, h);
                rfd_image o = image(w, h);
                FrameDesc d;
                FramePlan p;
                char msg[256] = "";
                CHECK(frame_plan(&f, 1, &o, 4097, 4097, &d, &p, msg, sizeof msg) == RFD_OK, "%s", msg);
                const bool two = format >= 5 && format <= 7;
                const long long quads = (w + 3) / 4, item_rows = two ? ch : h, items = quads * item_rows;
                CHECK(d.quads == quads && d.item_rows == item_rows && d.group0 == 0, "%s %d x %d: %d quads, %d item rows", frame_format_name(format), w, h, d.quads, d.item_rows);
                CHECK(p.items == items && p.groups == (items + 255) / 256, "%s %d x %d: %lld items in %d groups", frame_format_name(format), w, h, (long long)p.items, p.groups);
                CHECK(p.out_bytes == (size_t)w * 3 * h, "%s %d x %d: %zu output bytes", frame_format_name(format), w, h, p.out_bytes);
                // the last item of the last workgroup's tail lies past the frame, the last real item inside it
                CHECK((long long)p.groups * 256 >= items && (long long)(p.groups - 1) * 256 < items, "%s %d x %d: tail", frame_format_name(format), w, h);
            }
    rfd_frame_layout l;
    memset(&l, 0x5A, sizeof l);
    const rfd_frame_layout before = l;
    const int bad[][3] = {{-1, 4, 4}, {10, 4, 4}, {0, 0, 4}, {0, 4, 0}, {0, -3, 4}, {2, (1 << 28) + 1, 1}, {2, 1, (1 << 28) + 1}};
    for (const auto &b : bad) {
        ++steps;
        CHECK(!frame_layout(b[0], b[1], b[2], &l) && memcmp(&l, &before, sizeof l) == 0, "format %d %d x %d accepted or written", b[0], b[1], b[2]);
    }
    CHECK(frame_layout(RFD_PIXEL_BGRA, 1 << 28, 1, &l) && l.row_bytes[0] == (1 << 30), "the widest frame: %d", l.row_bytes[0]);
}

// one refusal: the status, "frame <i>: " and the cause in the message, and *plan as it was
static void refused(const char *what, const rfd_frame *src, int n, const rfd_image *out, int status, int at, const char *cause)
{
    ++steps;
    FrameDesc d[8];
    FramePlan p;
    memset(&p, 0x77, sizeof p);
    const FramePlan before = p;
    char msg[256] = "", head[32];
    const int got = frame_plan(src, n, out, 4096, 2048, d, &p, msg, sizeof msg);
    snprintf(head, sizeof head, "frame %d: ", at);
    CHECK(got == status, "%s: status %d, not %d (%s)", what, got, status, msg);
    CHECK(strncmp(msg, head, strlen(head)) == 0 && strstr(msg, cause), "%s: message \"%s\" lacks \"%s\" or \"%s\"", what, msg, head, cause);
    CHECK(memcmp(&p, &before, sizeof p) == 0, "%s: the plan was written", what);
}

static void refusals()
{
    rfd_frame src[3];
    rfd_image out[3];
    auto fresh = [&]() {
        src[0] = frame(RFD_PIXEL_NV12, 65, 33, RFD_COLOR_BT709_FULL); out[0] = image(65, 33);
        src[1] = frame(RFD_PIXEL_I420, 7, 5); out[1] = image(7, 5);
        src[2] = frame(RFD_PIXEL_BGRA, 16, 2, 99); out[2] = image(16, 2); // the colour of a byte format is ignored
    };
    FrameDesc d[3];
    FramePlan p;
    char msg[256] = "";
    fresh();
    CHECK(frame_plan(src, 3, out, 4096, 2048, d, &p, msg, sizeof msg) == RFD_OK, "the untouched batch: %s", msg);
    for (int i = 0; i < 3; ++i) {
        fresh(); out[i].width += 1; refused("width differs", src, 3, out, RFD_ERR_INVALID_ARG, i, "the output frame is");
        fresh(); out[i].height -= 1; refused("height differs", src, 3, out, RFD_ERR_INVALID_ARG, i, "the output frame is");
        fresh(); out[i].stride = 3 * out[i].width - 1; refused("output stride", src, 3, out, RFD_ERR_INVALID_ARG, i, "stride < 3 * width");
        fresh(); out[i].data = nullptr; refused("output null", src, 3, out, RFD_ERR_INVALID_ARG, i, "data is null");
        fresh(); src[i].format = 10; refused("format 10", src, 3, out, RFD_ERR_INVALID_ARG, i, "unknown pixel format 10");
        fresh(); src[i].format = -1; refused("format -1", src, 3, out, RFD_ERR_INVALID_ARG, i, "unknown pixel format -1");
        fresh(); src[i].width = 0; refused("zero width", src, 3, out, RFD_ERR_INVALID_ARG, i, "non-positive size");
        fresh(); src[i].height = -4; refused("negative height", src, 3, out, RFD_ERR_INVALID_ARG, i, "non-positive size");
        fresh(); src[i].width = 4097; refused("too wide", src, 3, out, RFD_ERR_CAPACITY, i, "exceeds max_src 4096 x 2048");
        fresh(); src[i].height = 2049; refused("too high", src, 3, out, RFD_ERR_CAPACITY, i, "exceeds max_src 4096 x 2048");
        for (int k = 0; k < 4; ++k) { fresh(); src[i].reserved[k] = 1; refused("reserved", src, 3, out, RFD_ERR_INVALID_ARG, i, "reserved is not zero"); }
    }
    // planes and strides: each plane the format has, and only those
    const int planes[3] = {2, 3, 1};
    const char *names[3] = {"nv12", "i420", "bgra"};
    for (int i = 0; i < 3; ++i)
        for (int k = 0; k < 3; ++k) {
            char cause[64];
            fresh(); src[i].plane[k] = nullptr;
            if (k < planes[i]) {
                snprintf(cause, sizeof cause, "plane %d of a %s frame is null", k, names[i]);
                refused("plane null", src, 3, out, RFD_ERR_INVALID_ARG, i, cause);
            } else { ++steps; CHECK(frame_plan(src, 3, out, 4096, 2048, d, &p, msg, sizeof msg) == RFD_OK, "an unused plane was looked at: %s", msg); }
            fresh(); src[i].stride[k] -= 1;
            if (k < planes[i]) {
                snprintf(cause, sizeof cause, "of plane %d is below", k);
                refused("plane stride", src, 3, out, RFD_ERR_INVALID_ARG, i, cause);
            } else { ++steps; CHECK(frame_plan(src, 3, out, 4096, 2048, d, &p, msg, sizeof msg) == RFD_OK, "an unused stride was looked at: %s", msg); }
        }
    // the colour: checked for the YUV formats only
    for (int color : {-1, 4, 1000}) {
        fresh(); src[0].color = color; refused("colour", src, 3, out, RFD_ERR_INVALID_ARG, 0, "unknown colour");
        fresh(); src[1].color = color; refused("colour", src, 3, out, RFD_ERR_INVALID_ARG, 1, "unknown colour");
        fresh(); src[2].color = color;
        ++steps; CHECK(frame_plan(src, 3, out, 4096, 2048, d, &p, msg, sizeof msg) == RFD_OK, "the colour of a bgra frame was looked at: %s", msg);
    }
    // the first bad frame is the one named
    fresh(); src[1].reserved[0] = 1; src[2].format = 77; refused("two bad frames", src, 3, out, RFD_ERR_INVALID_ARG, 1, "reserved");
}

static void batches()
{
    // six frames of six formats; items and workgroups summed by hand:
    //   0 nv12 1920 x 1080: 480 quads x 540 item rows = 259200 items, 1013 groups (1012.5)      group0    0
    //   1 bgra    5 x    3:   2 x   3                 =      6          1                                1013
    //   2 i420   65 x   33:  17 x  17                 =    289          2                                1014
    //   3 yuyv  641 x  481: 161 x 481                 =  77441        303 (302.5...)                     1016
    //   4 gray    1 x    1:   1 x   1                 =      1          1                                1319
    //   5 nv21 4096 x 2047: 1024 x 1024               = 1048576       4096                               1320
    //   sum                                            1385513       5416
    const int fmt[6] = {RFD_PIXEL_NV12, RFD_PIXEL_BGRA, RFD_PIXEL_I420, RFD_PIXEL_YUYV, RFD_PIXEL_GRAY, RFD_PIXEL_NV21};
    const int w[6] = {1920, 5, 65, 641, 1, 4096}, h[6] = {1080, 3, 33, 481, 1, 2047};
    const int quads[6] = {480, 2, 17, 161, 1, 1024}, item_rows[6] = {540, 3, 17, 481, 1, 1024}, group0[6] = {0, 1013, 1014, 1016, 1319, 1320};
    rfd_frame src[6];
    rfd_image out[6];
    for (int i = 0; i < 6; ++i) { src[i] = frame(fmt[i], w[i], h[i], i % 4); out[i] = image(w[i], h[i]); out[i].stride += i; }
    FrameDesc d[6];
    FramePlan p;
    char msg[256] = "";
    ++steps;
    CHECK(frame_plan(src, 6, out, 4096, 2160, d, &p, msg, sizeof msg) == RFD_OK, "%s", msg);
    CHECK(p.items == 1385513 && p.groups == 5416, "%lld items, %d groups", (long long)p.items, p.groups);
    for (int i = 0; i < 6; ++i) {
        CHECK(d[i].quads == quads[i] && d[i].item_rows == item_rows[i] && d[i].group0 == group0[i], "frame %d: %d x %d from %d", i, d[i].quads, d[i].item_rows, d[i].group0);
        CHECK(d[i].width == w[i] && d[i].height == h[i] && d[i].format == fmt[i] && d[i].out == kOut && d[i].out_stride == 3LL * w[i] + i, "frame %d: fields", i);
        CHECK(d[i].plane[0] == kBytes && d[i].stride[0] == src[i].stride[0], "frame %d: plane 0", i);
        if (i) CHECK(d[i].group0 > d[i - 1].group0, "frame %d: first groups do not ascend", i);
    }
    // src_bytes: each plane's start rounded up to 16.  nv12: 2073600 + 1036800 = 3110400 (both multiples of 16); bgra 5 x 3:
    // 60 -> 3110460; i420: at 3110464, 65 * 33 = 2145 -> 3112609, U at 3112624 + 33 * 17 = 561 -> 3113185, V at 3113200 + 561 ->
    // 3113761; yuyv: at 3113776 + 1284 * 481 = 617604 -> 3731380; gray: at 3731392 + 1 -> 3731393; nv21: at 3731408 + 4096 * 2047 =
    // 8384512 -> 12115920 (a multiple of 16) + 4096 * 1024 = 4194304 -> 16310224
    CHECK(p.src_bytes == 16310224, "%zu source bytes", p.src_bytes);
    CHECK(p.out_bytes == 3 * (1920ull * 1080 + 15 + 65 * 33 + 641 * 481 + 1 + 4096ull * 2047), "%zu output bytes", p.out_bytes);
    // the coefficients by colour: frames 0, 2, 3, 5 are YUV with colours 0, 2, 3, 1
    CHECK(d[0].coef.cy == 1220542 && d[0].coef.cvr == 1673527 && d[0].coef.cug == -409993 && d[0].coef.cvg == -852492 && d[0].coef.cub == 2116026 && d[0].coef.y0 == 16, "BT.601 limited");
    CHECK(d[5].coef.cy == 1048576 && d[5].coef.cvr == 1470104 && d[5].coef.cug == -360853 && d[5].coef.cvg == -748826 && d[5].coef.cub == 1858077 && d[5].coef.y0 == 0, "BT.601 full");
    CHECK(d[2].coef.cy == 1220542 && d[2].coef.cvr == 1880097 && d[2].coef.cug == -223347 && d[2].coef.cvg == -558891 && d[2].coef.cub == 2214593 && d[2].coef.y0 == 16, "BT.709 limited");
    CHECK(d[3].coef.cy == 1048576 && d[3].coef.cvr == 1651297 && d[3].coef.cug == -196423 && d[3].coef.cvg == -490864 && d[3].coef.cub == 1945738 && d[3].coef.y0 == 0, "BT.709 full");
    // 32 equal frames: the prefix is a multiple
    rfd_frame s32[32];
    rfd_image o32[32];
    FrameDesc d32[32];
    for (int i = 0; i < 32; ++i) { s32[i] = frame(RFD_PIXEL_UYVY, 1921, 1081); o32[i] = image(1921, 1081); }
    ++steps;
    CHECK(frame_plan(s32, 32, o32, 4096, 2160, d32, &p, msg, sizeof msg) == RFD_OK, "%s", msg);
    // 481 quads x 1081 rows = 519961 items = 2031.1 -> 2032 groups
    for (int i = 0; i < 32; ++i) CHECK(d32[i].group0 == 2032 * i, "frame %d starts at %d", i, d32[i].group0);
    CHECK(p.groups == 65024 && p.items == 16638752, "%d groups, %lld items", p.groups, (long long)p.items);
}

static void large()
{
    // 32768 x 32768: a bgra plane is 4 GiB, the frame 2^28 quads in 2^20 workgroups; two of them and an nv12 one
    rfd_frame src[3] = {frame(RFD_PIXEL_BGRA, 32768, 32768), frame(RFD_PIXEL_BGRA, 32768, 32768), frame(RFD_PIXEL_NV12, 32768, 32767)};
    rfd_image out[3] = {image(32768, 32768), image(32768, 32768), image(32768, 32767)};
    for (rfd_image &o : out) o.stride = (ptrdiff_t)1 << 33;
    FrameDesc d[3];
    FramePlan p;
    char msg[256] = "";
    ++steps;
    CHECK(frame_plan(src, 3, out, 32768, 32768, d, &p, msg, sizeof msg) == RFD_OK, "%s", msg);
    CHECK(d[0].quads == 8192 && d[0].item_rows == 32768 && d[1].group0 == 1048576 && d[2].group0 == 2097152, "first groups %d, %d", d[1].group0, d[2].group0);
    CHECK(d[2].item_rows == 16384 && p.groups == 2097152 + 524288, "%d groups", p.groups);
    CHECK(p.items == 2 * 268435456ll + 134217728ll, "%lld items", (long long)p.items);
    CHECK(p.src_bytes == 2 * 4294967296ull + 32768ull * 32767 + 32768ull * 16384, "%zu source bytes", p.src_bytes);
    CHECK(p.out_bytes == 2 * 3221225472ull + 3ull * 32768 * 32767, "%zu output bytes", p.out_bytes);
    CHECK(d[0].out_stride == (1ll << 33) && d[0].stride[0] == 131072, "strides %lld, %lld", d[0].out_stride, d[0].stride[0]);
    // the kernel numbers a frame's items, the tail of its last workgroup included, in int: a gray frame of 2^28 x 31 is 2^26 quads
    // x 31 rows = 2^31 - 2^26 items and passes, 2^28 x 32 = 2^31 items is refused, and so is whatever lies within one workgroup of 2^31
    rfd_frame wide = frame(RFD_PIXEL_GRAY, 1 << 28, 31);
    rfd_image wide_out = image(1 << 28, 31);
    ++steps;
    CHECK(frame_plan(&wide, 1, &wide_out, 1 << 28, 1 << 28, d, &p, msg, sizeof msg) == RFD_OK && p.items == 2147483648ll - 67108864ll, "%s", msg);
    wide = frame(RFD_PIXEL_GRAY, 1 << 28, 32); wide_out = image(1 << 28, 32);
    memset(&p, 0x77, sizeof p);
    const FramePlan before = p;
    ++steps;
    CHECK(frame_plan(&wide, 1, &wide_out, 1 << 28, 1 << 28, d, &p, msg, sizeof msg) == RFD_ERR_CAPACITY && strstr(msg, "frame 0: gray") && strstr(msg, "2^31 work items"), "%s", msg);
    CHECK(memcmp(&p, &before, sizeof p) == 0, "the plan was written");
    // 2047 quads x 1049088 rows = 2147483136 = 2^31 - 512 items passes (2^31 - 1 - 256 = 2147483391 is the most); one row more does not
    wide = frame(RFD_PIXEL_GRAY, 8188, 1049088); wide_out = image(8188, 1049088);
    ++steps;
    CHECK(frame_plan(&wide, 1, &wide_out, 1 << 28, 1 << 28, d, &p, msg, sizeof msg) == RFD_OK && p.items == 2147483136ll && p.groups == 8388606, "%s (%d groups)", msg, p.groups);
    wide = frame(RFD_PIXEL_GRAY, 8188, 1049089); wide_out = image(8188, 1049089);
    ++steps;
    CHECK(frame_plan(&wide, 1, &wide_out, 1 << 28, 1 << 28, d, &p, msg, sizeof msg) == RFD_ERR_CAPACITY, "2^31 - 512 + 2047 items accepted: %s", msg);
}

int main()
{
    layouts();
    refusals();
    batches();
    large();
    std::printf("%ld steps, %ld checks, %ld failures\n", steps, checks, failures);
    return failures ? 1 : 0;
}
