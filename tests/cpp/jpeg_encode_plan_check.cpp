// jpeg_encode_plan_check.cpp -- csrc/jpeg_encode_plan.h alone, with the host compiler and no HIP: the geometry and the bound at
// 1 x 1 and at 65535 x 65535, every quality's tables against the formula, the code tables against Annex K's counts, the header's
// fixed points, the checks that refuse a call, and the proof that the kernel's reciprocal multiplication IS the division: every
// |c| below 2^15 against every divisor 8 .. 2040.  tests/test_jpeg_encode_cpu.py builds it plain and under the sanitizers.
#include <stdio.h>

#include <vector>

#include "../../rs-face-detection_amd/csrc/jpeg_encode_plan.h"

using namespace rfd;

static long long g_checks = 0, g_failures = 0;
#define CHECK(cond)                                                       \
    do {                                                                  \
        ++g_checks;                                                       \
        if (!(cond)) {                                                    \
            if (++g_failures <= 20) printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
        }                                                                 \
    } while (0)

static rfd_jpeg_encode_config config(int quality, int sampling, int restart_rows)
{
    rfd_jpeg_encode_config c;
    jpeg_encode_config_default(&c);
    c.quality = quality; c.sampling = sampling; c.restart_rows = restart_rows;
    return c;
}

static void division()
{
    for (uint32_t d = 8; d <= 2040; ++d) { // every divisor, whether 8 * a table entry or not
        const uint32_t m = jpeg_encode_recip(d), half = d / 2;
        for (uint32_t c = 0; c < 32768; ++c) {
            ++g_checks;
            if (jpeg_encode_divide(c + half, m) != (c + half) / d) {
                if (++g_failures <= 20) printf("FAILED: (%u + %u) / %u\n", c, half, d);
            }
        }
    }
    CHECK(jpeg_encode_divide(65535u, jpeg_encode_recip(8)) == 65535u / 8);
}

static void tables()
{
    for (int q = 1; q <= 100; ++q) {
        uint8_t t[2][64];
        jpeg_encode_quant(q, t);
        const int scale = q < 50 ? 5000 / q : 200 - 2 * q;
        for (int k = 0; k < 2; ++k)
            for (int i = 0; i < 64; ++i) {
                long v = ((long)kEncBaseQuant[k][i] * scale + 50) / 100;
                v = v < 1 ? 1 : v > 255 ? 255 : v;
                CHECK(t[k][i] == v);
            }
        EncTables e;
        const rfd_jpeg_encode_config c = config(q, RFD_JPEG_420, 1);
        jpeg_encode_tables(c, &e);
        for (int k = 0; k < 2; ++k)
            for (int i = 0; i < 64; ++i) CHECK(e.half[k][i] == 4u * t[k][i] && e.recip[k][i] == jpeg_encode_recip(8u * t[k][i]));
        CHECK(e.header_len == 629 && e.header_len <= kEncHeaderMax && e.size_at > 0 && e.dri_at > e.size_at);
    }
    uint8_t t[2][64];
    jpeg_encode_quant(50, t);
    for (int i = 0; i < 64; ++i) CHECK(t[0][i] == kEncBaseQuant[0][i] && t[1][i] == kEncBaseQuant[1][i]);
    jpeg_encode_quant(100, t);
    for (int i = 0; i < 64; ++i) CHECK(t[0][i] == 1 && t[1][i] == 1);
    // the zigzag order is a permutation whose first steps are the known ones
    int seen[64] = {0};
    for (int k = 0; k < 64; ++k) seen[kEncNatural[k]]++;
    for (int k = 0; k < 64; ++k) CHECK(seen[k] == 1);
    CHECK(kEncNatural[1] == 1 && kEncNatural[2] == 8 && kEncNatural[3] == 16 && kEncNatural[63] == 63);
    // code tables: 162 AC symbols and 12 DC categories each, prefix-free by construction; the known codes of Annex K
    EncTables e;
    jpeg_encode_tables(config(90, RFD_JPEG_420, 0), &e);
    for (int k = 0; k < 2; ++k) {
        int ac = 0, dc = 0, longest = 0;
        for (int s = 0; s < 256; ++s)
            if (e.ac[k][s]) { ++ac; if ((int)(e.ac[k][s] & 255) > longest) longest = (int)(e.ac[k][s] & 255); }
        for (int s = 0; s < 12; ++s) dc += e.dc[k][s] != 0;
        CHECK(ac == 162 && dc == 12 && longest == 16);
        for (int run = 0; run < 16; ++run)
            for (int size = 1; size <= 10; ++size) CHECK(e.ac[k][run << 4 | size] != 0);
        CHECK(e.ac[k][0x00] != 0 && e.ac[k][0xF0] != 0);
        int dc_longest = 0;
        for (int s = 0; s < 12; ++s) dc_longest = (int)(e.dc[k][s] & 255) > dc_longest ? (int)(e.dc[k][s] & 255) : dc_longest;
        CHECK(dc_longest == (k == 0 ? 9 : 11) && dc_longest + 11 + 63 * (longest + 10) <= kEncMaxBlockBits); // no block is longer than the bound's unit
    }
    CHECK(e.ac[0][0x00] == (0xAu << 8 | 4) && e.ac[0][0xF0] == (0x7F9u << 8 | 11) && e.ac[1][0x00] == (0x0u << 8 | 2) && e.dc[0][0] == (0x0u << 8 | 2));
    CHECK(e.dri_at == 0 && e.header_len == 623);
    jpeg_encode_tables(config(90, RFD_JPEG_GRAY, 1), &e);
    CHECK(e.header_len == 2 + 18 + 69 + 13 + 33 + 183 + 6 + 10);
}

static void geometry()
{
    char msg[200];
    EncImage d;
    // 1 x 1
    for (int s = RFD_JPEG_GRAY; s <= RFD_JPEG_420; ++s) {
        memset(&d, 0, sizeof d);
        CHECK(jpeg_encode_geometry(1, 1, config(90, s, 1), &d, msg, sizeof msg));
        const EncSampling sm = jpeg_encode_sampling(s);
        CHECK(d.mcus == 1 && d.intervals == 1 && d.interval == 1 && d.dri == 1);
        CHECK(d.blocks == (sm.ncomp == 1 ? 1 : sm.h * sm.v + 2));
        CHECK(d.wb[0] == 1 && d.hb[0] == 1 && d.bw[0] == sm.h && d.bh[0] == sm.v && d.ch[0] == 1);
        CHECK(jpeg_encode_bound_of(d, 629) == 629u + 2u * (((size_t)d.blocks * kEncMaxBlockBits + 7) / 8) + 2u);
    }
    // 65535 x 65535
    memset(&d, 0, sizeof d);
    CHECK(jpeg_encode_geometry(65535, 65535, config(90, RFD_JPEG_420, 1), &d, msg, sizeof msg));
    CHECK(d.mcux == 4096 && d.mcus == 4096 * 4096 && d.blocks == 4096 * 4096 * 6 && d.intervals == 4096 && d.dri == 4096);
    CHECK(d.bw[0] == 8192 && d.wb[0] == 8192 && d.ch[1] == 32768 && d.wb[1] == 4096 && d.comp0[1] == 8192 * 8192 && d.comp0[2] == 8192 * 8192 + 4096 * 4096);
    CHECK(jpeg_encode_bound_of(d, 629) == 629u + 4096u * (2u * (((size_t)4096 * 6 * kEncMaxBlockBits + 7) / 8) + 2u));
    memset(&d, 0, sizeof d);
    CHECK(jpeg_encode_geometry(65535, 65535, config(90, RFD_JPEG_444, 0), &d, msg, sizeof msg));
    CHECK(d.mcus == 8192 * 8192 && d.intervals == 1 && d.interval == d.mcus && d.dri == 0 && d.blocks == 3 * 8192 * 8192);
    CHECK(!jpeg_encode_geometry(65535, 65535, config(90, RFD_JPEG_444, 8), &d, msg, sizeof msg) && strstr(msg, "restart_rows"));
    CHECK(jpeg_encode_geometry(65535, 65535, config(90, RFD_JPEG_444, 7), &d, msg, sizeof msg) && d.dri == 7 * 8192);
    CHECK(!jpeg_encode_geometry(0, 5, config(90, 1, 0), &d, msg, sizeof msg) && strstr(msg, "width"));
    CHECK(!jpeg_encode_geometry(5, 65536, config(90, 1, 0), &d, msg, sizeof msg) && strstr(msg, "height"));
    // real blocks and rows of the sizes that separate the two bottom-edge rules, at 4:2:0
    CHECK(jpeg_encode_geometry(16, 8, config(90, RFD_JPEG_420, 0), &d, msg, sizeof msg));
    CHECK(d.hb[0] == 1 && d.bh[0] == 2 && d.ch[1] == 4 && d.hb[1] == 1 && d.wb[0] == 2 && d.bw[0] == 2);
    CHECK(jpeg_encode_geometry(33, 17, config(90, RFD_JPEG_422, 2), &d, msg, sizeof msg));
    CHECK(d.mcux == 3 && d.wb[0] == 5 && d.bw[0] == 6 && d.hb[0] == 3 && d.wb[1] == 3 && d.ch[1] == 17 && d.dri == 6 && d.intervals == 2);
    // every interval counted once, whatever the sizes
    for (int w = 1; w <= 70; w += 3)
        for (int h = 1; h <= 70; h += 5)
            for (int s = RFD_JPEG_GRAY; s <= RFD_JPEG_420; ++s)
                for (int r = 0; r <= 3; ++r) {
                    CHECK(jpeg_encode_geometry(w, h, config(90, s, r), &d, msg, sizeof msg));
                    CHECK((int64_t)(d.intervals - 1) * d.interval < d.mcus && (int64_t)d.intervals * d.interval >= d.mcus);
                    CHECK(d.blocks % d.mcus == 0 && d.comp0[0] == 0);
                }
}

static void plan()
{
    char msg[256];
    std::vector<uint8_t> px(64 * 64 * 3);
    rfd_image imgs[3];
    for (int i = 0; i < 3; ++i) { imgs[i].data = px.data(); imgs[i].width = 10 + 20 * i; imgs[i].height = 9 + i; imgs[i].stride = 3 * imgs[i].width + i; }
    EncImage desc[3];
    EncPlan p;
    uint8_t *slots = reinterpret_cast<uint8_t *>(0x1000);
    CHECK(jpeg_encode_plan(imgs, 3, config(90, RFD_JPEG_420, 1), slots, 4096, 629, desc, &p, msg, sizeof msg) == RFD_OK);
    CHECK(desc[0].block0 == 0 && desc[1].block0 == desc[0].blocks && desc[2].block0 == desc[0].blocks + desc[1].blocks && p.blocks == desc[2].block0 + desc[2].blocks);
    CHECK(desc[0].group0 == 0 && desc[1].group0 == 1 && desc[2].group0 == 2 && p.groups == 3 && desc[2].out == slots + 8192);
    CHECK(desc[1].interval0 == desc[0].intervals && p.intervals == desc[0].intervals + desc[1].intervals + desc[2].intervals);
    CHECK(p.coef_bytes == (size_t)p.blocks * 128 && p.interval_bytes == (size_t)p.intervals * 8 && p.max_bound == jpeg_encode_bound_of(desc[2], 629));
    imgs[1].stride = 3 * imgs[1].width - 1;
    CHECK(jpeg_encode_plan(imgs, 3, config(90, RFD_JPEG_420, 1), slots, 4096, 629, desc, &p, msg, sizeof msg) == RFD_ERR_INVALID_ARG && strstr(msg, "image 1") && strstr(msg, "stride"));
    imgs[1].stride = 3 * imgs[1].width;
    imgs[2].data = nullptr;
    CHECK(jpeg_encode_plan(imgs, 3, config(90, RFD_JPEG_420, 1), slots, 4096, 629, desc, &p, msg, sizeof msg) == RFD_ERR_INVALID_ARG && strstr(msg, "image 2"));
    imgs[2].data = px.data();
    const struct { int q, s, r; const char *word; } bad[] = {{0, 3, 1, "quality"}, {101, 3, 1, "quality"}, {90, -1, 1, "sampling"}, {90, 4, 1, "sampling"}, {90, 3, -1, "restart_rows"}};
    for (const auto &b : bad) CHECK(jpeg_encode_plan(imgs, 3, config(b.q, b.s, b.r), slots, 4096, 629, desc, &p, msg, sizeof msg) == RFD_ERR_INVALID_ARG && strstr(msg, b.word));
    rfd_jpeg_encode_config c = config(90, 3, 1);
    c.reserved[4] = 1;
    CHECK(jpeg_encode_plan(imgs, 3, c, slots, 4096, 629, desc, &p, msg, sizeof msg) == RFD_ERR_INVALID_ARG && strstr(msg, "reserved"));
    // a call of more than 2^30 blocks
    rfd_image huge[12];
    for (auto &h : huge) { h.data = px.data(); h.width = 65535; h.height = 65535; h.stride = 3 * 65535; }
    EncImage hd[12];
    CHECK(jpeg_encode_plan(huge, 12, config(90, RFD_JPEG_444, 1), slots, 4096, 629, hd, &p, msg, sizeof msg) == RFD_ERR_CAPACITY);
    CHECK(jpeg_encode_plan(huge, 5, config(90, RFD_JPEG_444, 1), slots, 4096, 629, hd, &p, msg, sizeof msg) == RFD_OK && p.blocks == 5ll * 3 * 8192 * 8192);
}

int main()
{
    division();
    tables();
    geometry();
    plan();
    printf("%lld checks, %lld failures\n", g_checks, g_failures);
    return g_failures ? 1 : 0;
}
