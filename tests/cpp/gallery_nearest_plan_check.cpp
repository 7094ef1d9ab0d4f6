// gallery_nearest_plan_check.cpp -- csrc/gallery_nearest_plan.h alone, built by the host compiler under AddressSanitizer and
// UBSan (tests/test_gallery_nearest_cpu.py): every (rows, row0, n, dim, cus) of a grid around the boundaries must decompose so
// that the tiles cover [row0, row0 + n) exactly once, the splits cover every row block exactly once, the workspace holds
// splits * n keys, the grid is non-zero and within the documented cap, and few rows against many still make at least `cus`
// workgroups.  The coverage is counted in arrays, so an off-by-one in the plan is an out-of-bounds write the sanitizers name.
#include <cstdio>
#include <set>
#include <vector>

#include "../../rs-face-detection_amd/csrc/gallery_nearest_plan.h"

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

static void one(int rows, int row0, int n, int dim, int cus)
{
    ++steps;
    const GalleryNearestPlan p = gallery_nearest_plan(rows, row0, n, dim, cus);
#define WHERE "rows %d row0 %d n %d dim %d cus %d", rows, row0, n, dim, cus
    CHECK(p.form == gallery_nearest_form(dim, n) && p.tile_rows == gallery_nearest_tile_rows(dim, n), WHERE);
    CHECK(p.tile_rows >= 16 && p.tile_rows % 16 == 0 && p.tile_rows <= kNearestMaxTileRows, WHERE);
    CHECK((p.form == kNearestFormRegisters) == (dim == 512 && n >= kNearestRegisterMinRows), WHERE); // the register form is dim 512's alone
    CHECK(p.tile_rows == (p.form == kNearestFormRegisters ? 64 : 32), WHERE);
    if (n == 0 || rows == 0) { // nothing to launch
        CHECK(p.grid == 0 && p.ws_bytes == 0 && p.tiles == 0 && p.splits == 0, WHERE);
        return;
    }
    CHECK(p.grid >= 1 && p.grid == (int64_t)p.tiles * p.splits, WHERE);
    CHECK(p.grid <= gallery_nearest_grid_cap(n, dim, cus) && p.grid <= 0x7fffffffll, WHERE);
    CHECK(p.ws_bytes == (int64_t)p.splits * n * 8, WHERE);
    CHECK(p.ws_bytes <= gallery_nearest_ws_bound(rows, dim, cus), WHERE);
    // the tiles, as the scan addresses them: tile t owns rows row0 + t * tile_rows + i below row0 + n
    std::vector<int> a_seen((size_t)n, 0);
    for (int t = 0; t < p.tiles; ++t) {
        int in_tile = 0;
        for (int i = 0; i < p.tile_rows; ++i) {
            const int64_t a = (int64_t)row0 + (int64_t)t * p.tile_rows + i;
            if (a < (int64_t)row0 + n) { ++a_seen[(size_t)(a - row0)]; ++in_tile; }
        }
        CHECK(in_tile >= 1, WHERE); // no tile is empty: the scan clamps to the call's last row
    }
    bool once = true;
    for (int v : a_seen) once = once && v == 1;
    CHECK(once, WHERE);
    // the splits, as the scan walks them: wave w of split s starts at block 4 s + w and steps by 4 * splits
    CHECK(p.blocks == (rows + 15) / 16 && p.blocks_per_split >= 1 && p.blocks_per_split <= p.blocks, WHERE);
    std::vector<int> b_seen((size_t)p.blocks, 0);
    for (int s = 0; s < p.splits; ++s) {
        int owned = 0;
        for (int w = 0; w < kNearestWaves; ++w)
            for (int64_t b = (int64_t)s * kNearestWaves + w; b < p.blocks; b += (int64_t)p.splits * kNearestWaves) { ++b_seen[(size_t)b]; ++owned; }
        CHECK(owned >= 1 && owned <= p.blocks_per_split, WHERE); // no split is empty
    }
    once = true;
    for (int v : b_seen) once = once && v == 1;
    CHECK(once, WHERE);
    // few rows against many: while the gallery has a group of blocks per workgroup of the target, the chip is filled
    if ((int64_t)p.blocks >= (int64_t)kNearestWaves * kNearestTargetPerCu * cus) CHECK(p.grid >= (int64_t)kNearestTargetPerCu * cus && p.grid >= cus, WHERE);
    // many rows: no split, the gallery is read once per tile
    if (p.tiles >= kNearestTargetPerCu * cus) CHECK(p.splits == 1, WHERE);
#undef WHERE
}

int main()
{
    const int dims[] = {32, 512, 1024}, cuss[] = {1, 8, 256};
    for (int dim : dims) {
        const int tr = gallery_nearest_tile_rows(dim, 1 << 20); // of a large call; 32 and 64 are both in the sets below for every dim
        std::set<int> sizes = {0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, kNearestRegisterMinRows - 1, kNearestRegisterMinRows, tr - 1, tr, tr + 1, 2 * tr - 1, 2 * tr, 2 * tr + 1, 1000, 2999, 3000};
        for (int cus : cuss) {
            for (int rows : sizes)
                for (int n : sizes) {
                    if (n > rows) continue;
                    const std::set<int> starts = {0, 1, 15, 16, 17, tr - 1, tr + 1, rows - n};
                    for (int row0 : starts)
                        if (row0 >= 0 && row0 <= rows - n) one(rows, row0, n, dim, cus);
                }
            // the two regimes of the documents: an enrolment batch and a sweep on a million rows (coverage counted as above)
            one(1 << 20, 0, 32, dim, cus);
            one(1 << 20, (1 << 20) - 33, 33, dim, cus);
            one(1 << 20, 0, 1, dim, cus);
            one(1 << 18, 5, (1 << 18) - 5, dim, cus);
        }
    }
    // the regimes by their numbers: 32 new rows against 2^20 occupy every CU; a sweep is not split
    const GalleryNearestPlan few = gallery_nearest_plan(1 << 20, 0, 32, 512, 256), many = gallery_nearest_plan(1 << 20, 0, 1 << 20, 512, 256);
    CHECK(few.tiles == 1 && few.grid >= 256 && few.splits == few.grid && few.form == kNearestFormLds, "few: grid %lld", (long long)few.grid);
    CHECK(many.splits == 1 && many.tiles == (1 << 20) / many.tile_rows, "many: splits %d", many.splits);
    CHECK(many.form == kNearestFormRegisters && many.tile_rows == 64, "a sweep at dim 512 takes the register form");
    // arguments outside the rules plan nothing
    CHECK(gallery_nearest_plan(10, 0, 11, 512, 8).grid == 0 && gallery_nearest_plan(10, -1, 2, 512, 8).grid == 0, "refusals");
    CHECK(gallery_nearest_plan(10, 0, 5, 48, 8).grid == 0 && gallery_nearest_plan(10, 0, 5, 512, 0).grid == 0, "refusals");
    std::printf("gallery_nearest_plan_check: %ld steps, %ld checks, %ld failures\n", steps, checks, failures);
    return failures ? 1 : 0;
}
