// track_shots_plan_check.cpp -- csrc/track_shots_plan.h alone, built by the host compiler under AddressSanitizer and UBSan
// (tests/test_track_shots_cpu.py).  Every config bound refuses with its field named and accepts its edge values; the bank size
// is held at the int32 ends and around 1 GiB; the two grid bounds; the copy path over all 16 x 16 residues of source and
// destination and row sizes 1 .. 100, with the split of every chunk replayed on real heap rows of exactly the row's size, so a
// byte outside a row is an out-of-bounds access the sanitizers name; the chunks of a row cover it exactly once for every row
// size up to 3 x 1024 x 1024; and the ring slot of a call is written into a heap block of exactly track_shot_ring_bytes(n).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../rs-face-detection_amd/csrc/track_shots_plan.h"

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

static void config_bounds()
{
    ++steps;
    const rfd_track_shot_config ok = {112, 112, {0, 0, 0, 0, 0, 0}};
    char msg[128];
    CHECK(track_shot_config_ok(ok, msg, sizeof msg), "the default is refused: %s", msg);
    auto refused = [&](rfd_track_shot_config c, const char *field) {
        msg[0] = 0;
        const bool r = !track_shot_config_ok(c, msg, sizeof msg) && std::string(msg).find(field) != std::string::npos;
        CHECK(r, "%s: '%s'", field, msg);
    };
    const int imin = std::numeric_limits<int>::min(), imax = std::numeric_limits<int>::max();
    for (int bad : {0, -1, 1025, imin, imax}) {
        rfd_track_shot_config c = ok;
        c.crop_w = bad;
        refused(c, "crop_w");
        c = ok;
        c.crop_h = bad;
        refused(c, "crop_h");
    }
    for (int good : {1, 2, 5, 1023, 1024}) {
        rfd_track_shot_config c = ok;
        c.crop_w = good;
        CHECK(track_shot_config_ok(c, msg, sizeof msg), "crop_w %d: %s", good, msg);
        c = ok;
        c.crop_h = good;
        CHECK(track_shot_config_ok(c, msg, sizeof msg), "crop_h %d: %s", good, msg);
    }
    for (int i = 0; i < 6; ++i)
        for (int v : {1, -1, imin}) {
            rfd_track_shot_config c = ok;
            c.reserved[i] = v;
            refused(c, "reserved");
        }
}

static void bank_size()
{
    ++steps;
    const int imin = std::numeric_limits<int>::min(), imax = std::numeric_limits<int>::max();
    CHECK(track_shot_row_bytes(112, 112) == 37632u, "112 x 112");
    CHECK(track_shot_row_bytes(1, 1) == 3u && track_shot_row_bytes(1024, 1024) == 3145728u, "the ends");
    CHECK(track_shot_row_bytes(0, 5) == 0u && track_shot_row_bytes(5, -1) == 0u && track_shot_row_bytes(imin, imin) == 0u, "non-positive sides");
    CHECK(track_shot_row_bytes(imax, imax) == (size_t)imax * (size_t)imax * 3, "no int32 overflow");
    CHECK(track_shot_bank_bytes(imax, 256, 1024, 1024) == (size_t)imax * 256 * 3145728u, "no int32 overflow in streams");
    CHECK(track_shot_bank_bytes(0, 64, 5, 5) == 0u && track_shot_bank_bytes(imin, 64, 5, 5) == 0u && track_shot_bank_bytes(1, -64, 5, 5) == 0u, "non-positive counts");
    // around 1 GiB: 1 GiB / 3 is no integer, so the bound is met from below and passed from above
    CHECK(track_shot_bank_bytes(4096, 256, 16, 16) == 805306368u && track_shot_fits(4096, 256, 16, 16), "768 MiB fits");
    CHECK(track_shot_bank_bytes(4096, 64, 37, 37) == 1076625408u && !track_shot_fits(4096, 64, 37, 37), "1 GiB + 2.7 MiB does not");
    CHECK(track_shot_bank_bytes(4096, 64, 37, 36) == 1047527424u && track_shot_fits(4096, 64, 37, 36), "999 MiB fits");
    CHECK(track_shot_fits(1, 64, 1024, 1024) && track_shot_fits(1, 256, 1024, 1024) && !track_shot_fits(2, 256, 1024, 1024), "1024 x 1024 crops");
    CHECK(track_shot_fits(113, 256, 112, 112) == (113ull * 256 * 37632 <= (1ull << 30)), "112 x 112 crops");
    for (int streams = 1; streams <= 4096; streams *= 2)
        for (int mt : {64, 128, 256})
            for (int side : {1, 5, 16, 112, 333, 1024}) {
                const unsigned long long want = (unsigned long long)streams * mt * side * side * 3;
                CHECK(track_shot_bank_bytes(streams, mt, side, side) == want, "%d %d %d", streams, mt, side);
                CHECK(track_shot_fits(streams, mt, side, side) == (want <= (1ull << 30)), "%d %d %d", streams, mt, side);
            }
}

static void grid_bounds()
{
    ++steps;
    const int imax = std::numeric_limits<int>::max();
    CHECK(track_shot_keep_bound(5, 2, 64) == 5 && track_shot_keep_bound(500, 2, 64) == 128 && track_shot_keep_bound(0, 2, 64) == 0, "keep");
    CHECK(track_shot_keep_bound(-3, 2, 64) == 0 && track_shot_keep_bound(imax, 32, 256) == 8192 && track_shot_keep_bound(imax, imax, 256) == imax, "keep ends");
    CHECK(track_shot_collect_bound(4, 3, 64) == 4 && track_shot_collect_bound(1000, 3, 64) == 192 && track_shot_collect_bound(imax, 32, 256) == 8192, "collect");
    CHECK(track_shot_collect_bound(0, 3, 64) == 0 && track_shot_collect_bound(7, 0, 64) == 0 && track_shot_collect_bound(imax, imax, 256) == imax, "collect ends");
    CHECK(track_shot_item_capacity(32, 256) == 8192u, "the work list");
    for (int m = 0; m <= 300; ++m)
        for (int g = 1; g <= 4; ++g) CHECK(track_shot_keep_bound(m, g, 64) == (m < g * 64 ? m : g * 64), "%d %d", m, g);
}

// one item replayed on the host: the chunks of the row, each split by its path, on heap rows of exactly `bytes` bytes placed at
// the given residues; -> the number of bytes written, each exactly once
static void replay(unsigned sres, unsigned dres, uint32_t bytes)
{
    ++steps;
    // a 16-byte aligned heap block of exactly residue + bytes bytes with the row as its tail: the byte behind the row is outside
    auto place = [&](unsigned res, void **block) {
        if (posix_memalign(block, 16, res + bytes) != 0) std::abort();
        return static_cast<unsigned char *>(*block) + res;
    };
    void *sb = nullptr, *db = nullptr;
    unsigned char *src = place(sres, &sb), *dst = place(dres, &db);
    CHECK((uintptr_t)src % 16 == sres && (uintptr_t)dst % 16 == dres, "placement");
    for (uint32_t i = 0; i < bytes; ++i) {
        src[i] = (unsigned char)(i * 7 + 1);
        dst[i] = 0;
    }
    std::vector<int> written(bytes, 0);
    const int path = track_shot_copy_path((uint64_t)(uintptr_t)src, (uint64_t)(uintptr_t)dst, bytes);
    const int want = bytes >= 16 && sres == 0 && dres == 0 ? kShotCopyVec16 : bytes >= 4 && sres % 4 == dres % 4 ? kShotCopyDword : kShotCopyBytes;
    CHECK(path == want, "path %d, want %d (%u %u %u)", path, want, sres, dres, bytes);
    for (uint32_t c = 0; c < track_shot_row_chunks(bytes); ++c) {
        const uint32_t b = track_shot_chunk_begin(bytes, c), e = track_shot_chunk_end(bytes, c);
        const ShotCopySplit cut = track_shot_copy_split(path, (uint64_t)(uintptr_t)(src + b), e - b);
        CHECK(cut.head + cut.body * cut.unit + cut.tail == e - b, "the split covers the chunk");
        uint32_t at = b;
        for (uint32_t i = 0; i < cut.head; ++i, ++at) { dst[at] = src[at]; ++written[at]; }
        CHECK(cut.body == 0 || ((uintptr_t)(src + at) % cut.unit == 0 && (uintptr_t)(dst + at) % cut.unit == 0), "the body is aligned to its unit");
        for (uint32_t i = 0; i < cut.body; ++i, at += cut.unit) {
            std::memcpy(dst + at, src + at, cut.unit); // in bounds, or the sanitizer says so
            for (uint32_t k = 0; k < cut.unit; ++k) ++written[at + k];
        }
        for (uint32_t i = 0; i < cut.tail; ++i, ++at) { dst[at] = src[at]; ++written[at]; }
        CHECK(at == e, "the split ends at the chunk's end");
    }
    bool once = true, same = true;
    for (uint32_t i = 0; i < bytes; ++i) {
        once = once && written[i] == 1;
        same = same && dst[i] == src[i];
    }
    CHECK(once && same, "every byte of the row once (%u %u %u)", sres, dres, bytes);
    std::free(sb);
    std::free(db);
}

static void copy_paths()
{
    for (unsigned s = 0; s < 16; ++s)
        for (unsigned d = 0; d < 16; ++d)
            for (uint32_t bytes = 1; bytes <= 100; ++bytes) replay(s, d, bytes);
    // rows of more than one chunk, with a partial last chunk, on every path
    for (uint32_t bytes : {4096u, 4097u, 8191u, 8192u + 75u, 37632u})
        for (unsigned s : {0u, 1u, 4u, 6u})
            for (unsigned d : {0u, 2u, 4u, 5u}) replay(s, d, bytes);
}

static void chunks_cover_every_row()
{
    ++steps;
    unsigned long long bad = 0;
    for (uint32_t bytes = 1; bytes <= 3u * 1024 * 1024; ++bytes) {
        const uint32_t n = track_shot_row_chunks(bytes);
        uint32_t at = 0;
        for (uint32_t c = 0; c < n; ++c) {
            const uint32_t b = track_shot_chunk_begin(bytes, c), e = track_shot_chunk_end(bytes, c);
            if (b != at || e <= b || e - b > kTrackShotChunkBytes || b % 16 != 0) ++bad;
            at = e;
        }
        if (at != bytes) ++bad;
        ++checks;
    }
    CHECK(bad == 0, "%llu rows are not covered exactly once", bad);
    CHECK(track_shot_row_chunks(1) == 1 && track_shot_row_chunks(4096) == 1 && track_shot_row_chunks(4097) == 2 && track_shot_row_chunks(3145728) == 768, "counts");
}

static void ring_slot(int n)
{
    ++steps;
    const size_t ints = track_plan_ints(n) * sizeof(int32_t), at = track_shot_ring_stamp_offset(n), bytes = track_shot_ring_bytes(n);
    CHECK(at >= ints && at < ints + 8 && at % 8 == 0, "the stamps start at the next multiple of 8 (n %d)", n);
    CHECK(bytes == at + (size_t)n * 8, "n stamps (n %d)", n);
    for (int pass = 0; pass < 2; ++pass) {
        char *slot = new char[bytes]; // exactly: a byte too many is an out-of-bounds write
        std::memset(slot, 0x5A, bytes);
        std::vector<int32_t> stream((size_t)n);
        std::vector<int64_t> stamp((size_t)n);
        for (int i = 0; i < n; ++i) {
            stream[(size_t)i] = (i * 5) % 3;
            stamp[(size_t)i] = i % 2 ? std::numeric_limits<int64_t>::max() - i : std::numeric_limits<int64_t>::min() + i;
        }
        const int groups = track_plan(stream.data(), n, reinterpret_cast<int32_t *>(slot));
        CHECK(groups >= 1 && groups <= 3, "groups");
        track_shot_ring_stamps(slot, pass ? nullptr : stamp.data(), n);
        int64_t got;
        for (int i = 0; i < n; ++i) {
            std::memcpy(&got, slot + at + (size_t)i * 8, 8);
            CHECK(got == (pass ? 0 : stamp[(size_t)i]), "stamp %d", i);
        }
        delete[] slot;
    }
}

int main()
{
    config_bounds();
    bank_size();
    grid_bounds();
    copy_paths();
    chunks_cover_every_row();
    for (int n : {1, 2, 3, 31, 32, 64}) ring_slot(n);
    std::printf("%ld steps, %ld checks, %ld failures\n", steps, checks, failures);
    return failures ? 1 : 0;
}
