// track_plan_check.cpp -- csrc/track_plan.h alone, built by the host compiler under AddressSanitizer and UBSan
// (tests/test_tracker_ref_cpu.py).  Stream lists of every length up to 9 over up to 4 streams exhaustively, then seeded long ones
// and the hostile orders (interleaved, reversed, one stream with all frames but one): the plan lists each distinct stream once,
// in ascending order, with exactly its frames in call order, and every frame once.  The plan is written into a heap array of
// exactly track_plan_ints(n) ints, so an int too many is an out-of-bounds write the sanitizers name.  Then the stream check and
// the config bounds.
#include <cmath>
#include <cstdio>
#include <limits>
#include <string>
#include <vector>

#include "../../rs-face-detection_amd/csrc/track_plan.h"

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

static void one(const std::vector<int32_t> &stream)
{
    ++steps;
    const int n = (int)stream.size();
    std::vector<int32_t> plan(track_plan_ints(n), -77);
    const int groups = track_plan(stream.data(), n, plan.data());
    const int32_t *gs = track_plan_group_stream(plan.data(), n), *gf = track_plan_group_first(plan.data(), n), *order = track_plan_order(plan.data(), n);
    // by brute force: the distinct streams ascending, each with its frames in call order
    std::vector<int32_t> distinct;
    int32_t top = 0;
    for (int i = 0; i < n; ++i) top = stream[(size_t)i] > top ? stream[(size_t)i] : top;
    for (int s = 0; s <= top; ++s) {
        bool any = false;
        for (int i = 0; i < n; ++i) any |= stream[(size_t)i] == s;
        if (any) distinct.push_back(s);
    }
    CHECK(groups == (int)distinct.size(), "n %d: %d groups", n, groups);
    if (groups != (int)distinct.size()) return;
    CHECK(gf[0] == 0 || n == 0, "first group starts at %d", gf[0]);
    CHECK(gf[groups] == n, "last group ends at %d of %d", gf[groups], n);
    std::vector<int> seen((size_t)n, 0);
    for (int g = 0; g < groups; ++g) {
        CHECK(gs[g] == distinct[(size_t)g], "group %d is stream %d", g, gs[g]);
        CHECK(gf[g] < gf[g + 1], "group %d is empty", g);
        std::vector<int32_t> want;
        for (int i = 0; i < n; ++i)
            if (stream[(size_t)i] == distinct[(size_t)g]) want.push_back(i);
        CHECK(gf[g + 1] - gf[g] == (int)want.size(), "group %d holds %d frames", g, gf[g + 1] - gf[g]);
        for (int k = gf[g]; k < gf[g + 1] && k - gf[g] < (int)want.size(); ++k) {
            CHECK(order[k] == want[(size_t)(k - gf[g])], "group %d frame %d is %d", g, k - gf[g], order[k]);
            if (order[k] >= 0 && order[k] < n) ++seen[(size_t)order[k]];
        }
    }
    for (int i = 0; i < n; ++i) CHECK(seen[(size_t)i] == 1, "frame %d listed %d times", i, seen[(size_t)i]);
    for (int g = groups; g < n; ++g) CHECK(gs[g] == -1 && gf[g + 1] == n, "the unused tail is defined");
    CHECK(track_plan_bad_stream(stream.data(), n, 4096) == -1, "a good list is refused");
}

static void exhaustive()
{
    for (int n = 1; n <= 9; ++n) {
        std::vector<int32_t> s((size_t)n, 0);
        for (;;) {
            one(s);
            int i = 0;
            while (i < n && ++s[(size_t)i] == 4) s[(size_t)i++] = 0;
            if (i == n) break;
        }
    }
}

static void hostile()
{
    uint32_t x = 12345u;
    auto rnd = [&x]() { x = x * 1664525u + 1013904223u; return x >> 8; };
    for (int n : {1, 2, 31, 32, 33, 64, 257})
        for (int streams : {1, 2, 5, 32, 4096}) {
            std::vector<int32_t> s((size_t)n);
            for (int i = 0; i < n; ++i) s[(size_t)i] = i % streams;             // interleaved
            one(s);
            for (int i = 0; i < n; ++i) s[(size_t)i] = (n - 1 - i) % streams;     // reversed
            one(s);
            for (int i = 0; i < n; ++i) s[(size_t)i] = i == n / 2 ? streams - 1 : 0; // one stream with all frames but one
            one(s);
            for (int rep = 0; rep < 20; ++rep) {
                for (int i = 0; i < n; ++i) s[(size_t)i] = (int32_t)(rnd() % (uint32_t)streams);
                one(s);
            }
        }
}

static void refusals()
{
    ++steps;
    const int32_t s[5] = {0, 3, 4, -1, 9};
    CHECK(track_plan_bad_stream(s, 3, 5) == -1, "streams 0 3 4 of 5");
    CHECK(track_plan_bad_stream(s, 3, 4) == 2, "stream 4 of 4");
    CHECK(track_plan_bad_stream(s, 5, 5) == 3, "stream -1");
    CHECK(track_plan_bad_stream(s + 4, 1, 9) == 0, "stream 9 of 9");
    CHECK(track_plan_bad_stream(s, 0, 1) == -1, "no frames");
    const rfd_tracker_config ok = {1, 64, 0.3f, 5, 0.7f, 0.7f, 2, 1.1f, {0, 0, 0, 0}};
    char msg[128];
    CHECK(track_config_ok(ok, msg, sizeof msg), "the default is refused: %s", msg);
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    auto refused = [&](rfd_tracker_config c, const char *field) {
        msg[0] = 0;
        const bool r = !track_config_ok(c, msg, sizeof msg) && std::string(msg).find(field) != std::string::npos;
        CHECK(r, "%s: '%s'", field, msg);
    };
    rfd_tracker_config c;
    for (int v : {0, -1, 4097}) { c = ok; c.streams = v; refused(c, "streams"); }
    for (int v : {0, 32, 65, 192, 512, -64}) { c = ok; c.max_tracks = v; refused(c, "max_tracks"); }
    for (float v : {0.0f, -0.5f, nan, inf}) { c = ok; c.iou_min = v; refused(c, "iou_min"); }
    c = ok; c.max_missed = -1; refused(c, "max_missed");
    c = ok; c.min_score = nan; refused(c, "min_score");
    c = ok; c.new_score = 0.5f; refused(c, "new_score");
    c = ok; c.new_score = nan; refused(c, "new_score");
    for (int v : {0, -3}) { c = ok; c.min_hits = v; refused(c, "min_hits"); }
    for (float v : {0.99f, nan, inf, -2.0f}) { c = ok; c.improve = v; refused(c, "improve"); }
    for (int v : {64, 128, 256}) { c = ok; c.max_tracks = v; c.streams = 4096; c.max_missed = 0; c.min_hits = 1; c.improve = 1.0f; CHECK(track_config_ok(c, msg, sizeof msg), "edge values refused: %s", msg); }
}

int main()
{
    exhaustive();
    hostile();
    refusals();
    std::printf("%ld steps, %ld checks, %ld failures\n", steps, checks, failures);
    return failures ? 1 : 0;
}
