// jpeg_plan_check.cpp -- the planning of a JPEG decode call (csrc/jpeg_plan.h: the layout of the staging, the per-file argument
// check, the descriptor tables of the launches) alone, built with the host compiler under -fsanitize=address,undefined by
// tests/test_jpeg_scaled_cpu.py and run as a program.  The files named on the command line are planned one by one, in pairs and
// all together, with a staging of exactly the batch and of the batch + 3, at scales 1, 2, 4, 8, with the orientation ignored and
// applied, with the caller's frames and with packed ones.  The tables are written into a heap block of exactly the layout's
// total, so a write past it aborts the program; what they hold is compared with sums this file computes itself.
// No HIP, no device, nothing loaded into Python.
//   usage: jpeg_plan_check <file.jpg>...
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../rs-face-detection_amd/csrc/jpeg_plan.h"

using namespace rfd;

static int failures = 0;
static long plans = 0, checks = 0;
static std::string where;
#define CHECK(cond)                                                                        \
    do {                                                                                   \
        ++checks;                                                                          \
        if (!(cond) && ++failures <= 40) std::printf("FAIL %s: %s (line %d)\n", where.c_str(), #cond, __LINE__); \
    } while (0)

struct File { std::vector<uint8_t> bytes; int w, h, orientation; };

static size_t up(size_t a, size_t b) { return (a + b - 1) / b; }
static size_t align16(size_t v) { return (v + 15) / 16 * 16; }
static int row_tiles(int w, int h) { return (int)((up((size_t)w, 4) * (size_t)h + 255) / 256); }

// the regions of the staging against the closed formula of the sizes
static void check_layout(const JpegStageLayout &l, size_t B, int mw, int mh, char *base)
{
    const size_t a8 = up((size_t)mw, 8), b8 = up((size_t)mh, 8), a16 = up((size_t)mw, 16), b16 = up((size_t)mh, 16);
    const size_t blocks = std::max(3 * a8 * b8, std::max(4 * a16 * b8, 6 * a16 * b16));
    const size_t tables = align16(B * sizeof(JpegFrame) + B * blocks * (4 + 64 * 2));
    const size_t scaled = align16(tables + B * (sizeof(JpegOrientedFrame) + sizeof(JpegFrame)));
    CHECK(l.blocks_max == blocks && l.batch == B);
    CHECK(l.total == scaled + B * (sizeof(JpegScaledFrame) + 2 * sizeof(JpegOrientedFrame)));
    CHECK(l.plane_bytes() == B * blocks * 64);
    CHECK(l.rec_off == B * sizeof(JpegFrame) && l.coef_off == l.rec_off + B * blocks * 4);
    CHECK(l.oriented_off == tables && l.oriented_off % 16 == 0 && l.oriented_off >= l.coef_off + B * blocks * 128);
    CHECK(l.scaled_off == scaled && l.scaled_off % 16 == 0);
    CHECK(0 < l.rec_off && l.rec_off < l.coef_off && l.coef_off < l.oriented_off && l.oriented_off < l.scaled_off && l.scaled_off < l.total);
    CHECK((char *)l.frames(base) == base && (char *)l.rec(base) == base + l.rec_off && (char *)l.coef(base) == base + l.coef_off);
    CHECK((char *)l.oriented(base) == base + l.oriented_off && (char *)l.upright(base) == base + l.oriented_off + B * sizeof(JpegOrientedFrame));
    CHECK((char *)(l.upright(base) + B) <= base + l.scaled_off);
    CHECK((char *)l.scaled(base) == base + l.scaled_off && (char *)l.scaled_upright(base) == base + l.scaled_off + B * sizeof(JpegScaledFrame));
    CHECK(l.scaled_oriented(base) == l.scaled_upright(base) + B && (char *)(l.scaled_oriented(base) + B) == base + l.total);
}

static bool untouched(const char *base, size_t from, size_t to)
{
    for (size_t i = from; i < to; ++i)
        if ((unsigned char)base[i] != 0xa5) return false;
    return true;
}

// one call: files `pick` in a staging of max_batch frames
static void plan(const std::vector<File> &files, const std::vector<int> &pick, int max_batch, int scale, bool apply, bool packed)
{
    ++plans;
    const int n = (int)pick.size();
    int mw = 1, mh = 1;
    for (int i : pick) { mw = std::max(mw, files[(size_t)i].w); mh = std::max(mh, files[(size_t)i].h); }
    char tag[160];
    std::snprintf(tag, sizeof tag, "n %d first %d batch %d scale %d apply %d packed %d", n, pick[0], max_batch, scale, (int)apply, (int)packed);
    where = tag;
    const JpegStageLayout l(max_batch, mw, mh);
    std::unique_ptr<char[]> base(new char[l.total]); // exact size: a write past the staging is a heap overflow
    std::memset(base.get(), 0xa5, l.total);
    check_layout(l, (size_t)max_batch, mw, mh, base.get());

    std::vector<const uint8_t *> bytes;
    std::vector<size_t> len;
    std::vector<rfd_image> out((size_t)n);
    std::vector<int> ow((size_t)n), oh((size_t)n), orient((size_t)n);
    static uint8_t pixels[16]; // never written: only its address travels
    for (int i = 0; i < n; ++i) {
        const File &f = files[(size_t)pick[(size_t)i]];
        bytes.push_back(f.bytes.data());
        len.push_back(f.bytes.size());
        const int o = apply ? f.orientation : 1, sw = (f.w + scale - 1) / scale, sh = (f.h + scale - 1) / scale;
        orient[(size_t)i] = o; ow[(size_t)i] = o >= 5 ? sh : sw; oh[(size_t)i] = o >= 5 ? sw : sh;
        out[(size_t)i].data = pixels + i % 16;
        out[(size_t)i].width = ow[(size_t)i]; out[(size_t)i].height = oh[(size_t)i];
        out[(size_t)i].stride = (ptrdiff_t)ow[(size_t)i] * 3 + i % 5;
    }
    std::unique_ptr<JpegCallFrame[]> fr(new JpegCallFrame[(size_t)n]);
    char msg[512] = "";
    int n_oriented = -1;
    const int st = jpeg_plan_frames(bytes.data(), len.data(), n, out.data(), scale, apply, mw, mh, fr.get(), &n_oriented, msg, sizeof msg);
    CHECK(st == RFD_OK); // the oriented scaled size is accepted
    if (st != RFD_OK) { std::printf("  %s\n", msg); return; }
    int want_oriented = 0;
    size_t blocks = 0;
    for (int i = 0; i < n; ++i) {
        want_oriented += orient[(size_t)i] != 1;
        CHECK(fr[i].orientation == orient[(size_t)i] && fr[i].out_w == ow[(size_t)i] && fr[i].out_h == oh[(size_t)i]);
        CHECK(fr[i].rec0 == blocks && fr[i].hdr.nblocks >= 1 && (size_t)fr[i].hdr.nblocks <= l.blocks_max);
        blocks += (size_t)fr[i].hdr.nblocks;
    }
    CHECK(n_oriented == want_oriented);

    size_t out_bytes = 0;
    for (int i = 0; i < n; ++i) out_bytes += (size_t)ow[(size_t)i] * 3 * (size_t)oh[(size_t)i];
    std::vector<uint8_t> packed_frames(out_bytes);
    uint8_t *const pool = packed_frames.data();
    const JpegOutput place = {packed ? nullptr : out.data(), pool};
    const JpegTables t = jpeg_plan_tables(fr.get(), n, scale, n_oriented != 0, place, l, base.get());
    const JpegFrame *f = l.frames(base.get());
    const JpegScaledFrame *sf = l.scaled(base.get());
    int groups = 0, tiles = 0, cgroups = 0;
    size_t out_at = 0;
    for (int i = 0; i < n; ++i) {
        const JpegHeader &h = fr[i].hdr;
        CHECK(f[i].group0 == groups && f[i].tile0 == tiles);
        groups += (int)up((size_t)h.nblocks, 32);
        tiles += row_tiles(h.width, h.height);
        CHECK(f[i].rec0 == fr[i].rec0 && f[i].coef0 == f[i].rec0 * 64 && f[i].plane0 == f[i].rec0 * 64 && f[i].nblocks == h.nblocks);
        CHECK(f[i].width == h.width && f[i].height == h.height && f[i].ncomp == h.ncomp);
        if (i + 1 < n) CHECK(f[i].plane0 + 64 * (size_t)f[i].nblocks <= f[i + 1].plane0); // no two frames' ranges overlap
        if (packed) CHECK(f[i].out == pool + out_at && f[i].stride == (long long)ow[(size_t)i] * 3);
        else CHECK(f[i].out == out[(size_t)i].data && f[i].stride == (long long)out[(size_t)i].stride);
        out_at += (size_t)ow[(size_t)i] * 3 * (size_t)oh[(size_t)i];
        if (scale == 1) continue;
        size_t at = f[i].plane0;
        for (int k = 0; k < h.ncomp; ++k) {
            const int nk = sf[i].n[k], blk = h.comp[k].bw * h.comp[k].bh;
            CHECK(nk == 8 || nk == 4 || nk == 2 || nk == 1);
            CHECK(sf[i].cgroup[k] == cgroups && sf[i].plane[k] == at && sf[i].pitch[k] == h.comp[k].bw * nk);
            cgroups += (int)up((size_t)blk, (size_t)(256 / nk));
            at += (size_t)blk * (size_t)nk * (size_t)nk;
        }
        CHECK(at <= f[i].plane0 + 64 * (size_t)f[i].nblocks); // the three planes lie inside the frame's own share
        CHECK(sf[i].width == (h.width + scale - 1) / scale && sf[i].height == (h.height + scale - 1) / scale);
        CHECK(sf[i].hup == (h.ncomp == 3 && h.hmax == 2 && h.vmax == 1 ? 2 : 1) && sf[i].replicate == (scale == 8));
    }
    CHECK(out_at == out_bytes);
    CHECK(t.groups == groups && t.tiles == tiles && t.cgroups == cgroups && t.blocks == blocks);
    CHECK(blocks * 64 <= l.plane_bytes() && blocks <= (size_t)max_batch * l.blocks_max); // the last frame ends within the pools
    CHECK(l.frames_bytes(n) <= l.rec_off && l.frames_rec_bytes(t.blocks) <= l.coef_off && l.frames_rec_bytes(t.blocks) == l.rec_off + 4 * blocks);

    // the two colour lists
    if (scale == 1 && !n_oriented) { // one colour launch over the frame table: no list is written
        CHECK(t.upright.n == 0 && t.oriented.n == 0 && t.upright.tiles == 0 && t.oriented.tiles == 0 && t.lists_bytes == 0);
        CHECK(untouched(base.get(), l.oriented_off, l.total));
        return;
    }
    CHECK(t.upright.n + t.oriented.n == n && t.oriented.n == n_oriented);
    std::vector<int> seen((size_t)n, 0);
    const JpegOrientedFrame *ol = scale == 1 ? l.oriented(base.get()) : l.scaled_oriented(base.get());
    int at = 0;
    for (int k = 0; k < t.oriented.n; ++k) {
        const JpegOrientedFrame &e = ol[k];
        CHECK(e.frame >= 0 && e.frame < n);
        if (e.frame < 0 || e.frame >= n) return;
        ++seen[(size_t)e.frame];
        const int tx = (ow[(size_t)e.frame] + 63) / 64, ty = (oh[(size_t)e.frame] + 63) / 64;
        CHECK(e.orientation == orient[(size_t)e.frame] && e.orientation != 1 && e.tile0 == at && e.tiles_x == tx && tx * ty >= 1);
        at += tx * ty;
    }
    CHECK(t.oriented.tiles == at);
    at = 0;
    for (int k = 0; k < t.upright.n; ++k) {
        int i;
        if (scale == 1) { // the upright frames again, with tile0 counted in their own launch
            const JpegFrame &u = l.upright(base.get())[k];
            for (i = 0; i < n && f[i].rec0 != u.rec0; ++i) {}
            CHECK(i < n);
            if (i == n) return;
            JpegFrame same = u;
            same.tile0 = f[i].tile0;
            CHECK(std::memcmp(&same, &f[i], sizeof same) == 0 && u.tile0 == at);
        } else {
            const JpegOrientedFrame &e = l.scaled_upright(base.get())[k];
            i = e.frame;
            CHECK(i >= 0 && i < n);
            if (i < 0 || i >= n) return;
            CHECK(e.orientation == 1 && e.tile0 == at && e.tiles_x == 0);
        }
        ++seen[(size_t)i];
        CHECK(orient[(size_t)i] == 1 && row_tiles(ow[(size_t)i], oh[(size_t)i]) >= 1);
        at += row_tiles(ow[(size_t)i], oh[(size_t)i]);
    }
    CHECK(t.upright.tiles == at);
    for (int i = 0; i < n; ++i) CHECK(seen[(size_t)i] == 1); // every frame in exactly one list
    const size_t B = (size_t)max_batch;
    if (scale == 1) {
        CHECK(t.lists_off == l.oriented_off && t.lists_off + t.lists_bytes <= l.scaled_off);
        CHECK(t.lists_bytes == B * sizeof(JpegOrientedFrame) + (size_t)t.upright.n * sizeof(JpegFrame));
        CHECK(untouched(base.get(), l.scaled_off, l.total));
    } else {
        CHECK(t.lists_off == l.scaled_off && t.lists_off + t.lists_bytes <= l.total);
        CHECK(t.lists_bytes == B * (sizeof(JpegScaledFrame) + sizeof(JpegOrientedFrame)) + (size_t)t.oriented.n * sizeof(JpegOrientedFrame));
        CHECK(untouched(base.get(), l.oriented_off, l.scaled_off));
    }
}

// the argument check on one file: a wrong size, a short stride and a null data pointer, each with its message
static void refusals(const File &f, int scale, bool apply)
{
    char tag[120];
    std::snprintf(tag, sizeof tag, "refusals %d x %d orientation %d scale %d apply %d", f.w, f.h, f.orientation, scale, (int)apply);
    where = tag;
    const int o = apply ? f.orientation : 1, sw = (f.w + scale - 1) / scale, sh = (f.h + scale - 1) / scale, ow = o >= 5 ? sh : sw, oh = o >= 5 ? sw : sh;
    const uint8_t *bytes = f.bytes.data();
    const size_t len = f.bytes.size();
    static uint8_t pixel;
    std::unique_ptr<JpegCallFrame[]> fr(new JpegCallFrame[1]);
    char msg[512], want[512];
    int n_oriented = 0;
    auto call = [&](rfd_image im) {
        std::strcpy(msg, "");
        return jpeg_plan_frames(&bytes, &len, 1, &im, scale, apply, f.w, f.h, fr.get(), &n_oriented, msg, sizeof msg);
    };
    const rfd_image good = {&pixel, oh, ow, (ptrdiff_t)ow * 3};
    CHECK(call(good) == RFD_OK);
    rfd_image bad = good;
    bad.width = ow + 1;
    if (scale != 1)
        std::snprintf(want, sizeof want, "invalid argument: output frame 0 is %d x %d, file 0 is %d x %d at scale 1/%d in orientation %d (%d x %d stored)", ow + 1, oh, ow, oh, scale,
                      o, f.w, f.h);
    else if (o == 1) std::snprintf(want, sizeof want, "invalid argument: output frame 0 is %d x %d, file 0 is %d x %d", ow + 1, oh, f.w, f.h);
    else std::snprintf(want, sizeof want, "invalid argument: output frame 0 is %d x %d, file 0 is %d x %d in orientation %d (%d x %d stored)", ow + 1, oh, ow, oh, o, f.w, f.h);
    CHECK(call(bad) == RFD_ERR_INVALID_ARG && std::strcmp(msg, want) == 0);
    if (ow != oh) { // the unoriented size of a transposing orientation is a wrong size too
        bad = good;
        bad.width = oh; bad.height = ow; bad.stride = (ptrdiff_t)oh * 3;
        CHECK(call(bad) == RFD_ERR_INVALID_ARG);
    }
    bad = good;
    bad.stride = (ptrdiff_t)ow * 3 - 1;
    std::snprintf(want, sizeof want, "invalid argument: output frame 0 has stride %td < 3 * width", bad.stride);
    CHECK(call(bad) == RFD_ERR_INVALID_ARG && std::strcmp(msg, want) == 0);
    bad = good;
    bad.data = nullptr;
    CHECK(call(bad) == RFD_ERR_INVALID_ARG && std::strcmp(msg, "invalid argument: output frame 0 has no data pointer") == 0);
    std::strcpy(msg, "");
    const rfd_image im = good;
    CHECK(jpeg_plan_frames(&bytes, &len, 1, &im, scale, apply, f.w - 1, f.h, fr.get(), &n_oriented, msg, sizeof msg) == RFD_ERR_CAPACITY);
    std::snprintf(want, sizeof want, "file 0: %d x %d exceeds max_src %d x %d", f.w, f.h, f.w - 1, f.h);
    CHECK(std::strcmp(msg, want) == 0);
}

// the staging of the device entropy stage against the closed formula of its sizes
static void entropy_layout(int B, int mw, int mh)
{
    where = "entropy layout";
    const JpegStageLayout l(B, mw, mh);
    const JpegEntLayout e(B, mw, mh, l.blocks_max);
    const size_t ivl = 2 * (size_t)B * up((size_t)mw, 8) * up((size_t)mh, 8), pool = std::min((size_t)B * std::max((size_t)65536, 32 * l.blocks_max), (size_t)0xffff0000u);
    CHECK(e.ivl_words() == ivl && e.scan_pool == pool);
    CHECK(e.status_off == (size_t)B * sizeof(JpegEntropyFrame) && e.ivl_off == e.status_off + 4 * (size_t)B && e.scan_off == e.ivl_off + 4 * ivl && e.total == e.scan_off + pool);
    char *base = nullptr;
    CHECK((char *)e.frames(base) == base && (char *)e.status(base) == base + e.status_off && (char *)e.intervals(base) == base + e.ivl_off && (char *)e.scan(base) == base + e.scan_off);
}

int main(int argc, char **argv)
{
    if (argc < 2) { std::fprintf(stderr, "usage: %s <file.jpg>...\n", argv[0]); return 2; }
    std::vector<File> files;
    for (int a = 1; a < argc; ++a) {
        FILE *fp = std::fopen(argv[a], "rb");
        if (!fp) { std::perror(argv[a]); return 2; }
        File f;
        for (int ch; (ch = std::fgetc(fp)) != EOF;) f.bytes.push_back((uint8_t)ch);
        std::fclose(fp);
        std::unique_ptr<JpegHeader> h(new JpegHeader);
        if (jpeg_parse_header(f.bytes.data(), f.bytes.size(), *h) != RFD_OK) { std::printf("FAIL %s: %s\n", argv[a], h->msg); return 1; }
        f.w = h->width; f.h = h->height; f.orientation = h->orientation;
        files.push_back(f);
    }
    const int N = (int)files.size();
    std::vector<std::vector<int>> batches;
    for (int i = 0; i < N; ++i) batches.push_back({i});
    for (int i = 0; i < N; ++i) batches.push_back({i, (i + 1) % N});           // neighbours: the same image, the next orientation
    for (int i = 0; i < N; ++i) batches.push_back({(i * 7 + 3) % N, i});       // and a pair from elsewhere in the list
    std::vector<int> all;
    for (int i = 0; i < N; ++i) all.push_back(i);
    batches.push_back(all);
    static const int kScales[4] = {1, 2, 4, 8};
    for (const std::vector<int> &pick : batches)
        for (int extra = 0; extra <= 3; extra += 3)
            for (int scale : kScales)
                for (int apply = 0; apply < 2; ++apply)
                    for (int packed = 0; packed < 2; ++packed) plan(files, pick, (int)pick.size() + extra, scale, apply != 0, packed != 0);
    for (const File &f : files)
        for (int scale : kScales)
            for (int apply = 0; apply < 2; ++apply) refusals(f, scale, apply != 0);
    entropy_layout(1, 1, 1);
    entropy_layout(3, 130, 70);
    entropy_layout(32, 1920, 1080);
    std::printf("jpeg_plan_check: %d files, %ld plans, %ld checks, %d failures\n", N, plans, checks, failures);
    return failures ? 1 : 0;
}
