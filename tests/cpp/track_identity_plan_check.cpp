// track_identity_plan_check.cpp -- csrc/track_identity_plan.h alone, built by the host compiler under AddressSanitizer and UBSan
// (tests/test_track_identity_cpu.py).  Every config bound refuses with its field named and accepts its edge values; the size bound
// is held at 1 GiB exactly over every legal (streams, max_tracks, dim); the lane element count covers dim and is one of the
// kernel's instantiations; and the plan of a fuse or label call is the tracker's plan, int for int, written into a heap array of
// exactly track_identity_plan_ints(n) ints, so an int too many is an out-of-bounds write the sanitizers name.
#include <cmath>
#include <cstdio>
#include <limits>
#include <string>
#include <vector>

#include "../../rs-face-detection_amd/csrc/track_identity_plan.h"

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
    const rfd_track_identity_config ok = {512, 0.5f, 0.4f, 0.05f, {0, 0, 0, 0}};
    char msg[128];
    CHECK(track_identity_config_ok(ok, msg, sizeof msg), "the default is refused: %s", msg);
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    auto refused = [&](rfd_track_identity_config c, const char *field) {
        msg[0] = 0;
        const bool r = !track_identity_config_ok(c, msg, sizeof msg) && std::string(msg).find(field) != std::string::npos;
        CHECK(r, "%s: '%s'", field, msg);
    };
    rfd_track_identity_config c;
    for (int v : {0, -32, 16, 31, 33, 48, 100, 1000, 1025, 1056, 2048}) { c = ok; c.dim = v; refused(c, "dim"); }
    for (int v = 32; v <= 1024; v += 32) { c = ok; c.dim = v; CHECK(track_identity_config_ok(c, msg, sizeof msg), "dim %d refused: %s", v, msg); }
    for (float v : {nan, inf, -inf}) { c = ok; c.accept = v; refused(c, "accept"); }
    for (float v : {nan, inf, -inf}) { c = ok; c.release = v; refused(c, "release"); }
    c = ok; c.release = std::nextafter(c.accept, inf); refused(c, "release");
    c = ok; c.release = c.accept; CHECK(track_identity_config_ok(c, msg, sizeof msg), "release == accept refused: %s", msg);
    c = ok; c.accept = -0.5f; c.release = -1.0f; CHECK(track_identity_config_ok(c, msg, sizeof msg), "negative thresholds refused: %s", msg);
    for (float v : {nan, inf, -0.001f, -inf}) { c = ok; c.margin = v; refused(c, "margin"); }
    c = ok; c.margin = 0.0f; CHECK(track_identity_config_ok(c, msg, sizeof msg), "margin 0 refused: %s", msg);
}

static void size_bound()
{
    for (int streams : {1, 2, 255, 256, 257, 1023, 1024, 1025, 2048, 4095, 4096})
        for (int max_tracks : {64, 128, 256})
            for (int dim = 32; dim <= 1024; dim += 32) {
                ++steps;
                const unsigned long long bytes = 4ull * (unsigned long long)streams * (unsigned long long)max_tracks * (unsigned long long)dim;
                CHECK(track_identity_template_bytes(streams, max_tracks, dim) == bytes, "%d %d %d", streams, max_tracks, dim);
                CHECK(track_identity_fits(streams, max_tracks, dim) == (bytes <= (1ull << 30)), "%d %d %d", streams, max_tracks, dim);
                const int j = track_identity_lane_elems(dim);
                CHECK((j == 1 || j == 2 || j == 4 || j == 8 || j == 16) && 64 * j >= dim && (j == 1 || 32 * j < dim), "dim %d: %d", dim, j);
            }
    CHECK(track_identity_fits(4096, 64, 1024) && !track_identity_fits(4096, 128, 1024), "1 GiB is the last that fits");
}

static void plan_is_the_trackers()
{
    uint32_t x = 4711u;
    auto rnd = [&x]() { x = x * 1664525u + 1013904223u; return x >> 8; };
    for (int n : {1, 2, 3, 31, 32, 33, 64})
        for (int streams : {1, 2, 5, 32, 4096})
            for (int rep = 0; rep < 40; ++rep) {
                ++steps;
                std::vector<int32_t> s((size_t)n);
                for (int i = 0; i < n; ++i)
                    s[(size_t)i] = rep == 0 ? i % streams : rep == 1 ? (n - 1 - i) % streams : (int32_t)(rnd() % (uint32_t)streams);
                CHECK(track_identity_plan_ints(n) == track_plan_ints(n), "n %d", n);
                std::vector<int32_t> a(track_identity_plan_ints(n), -77), b(track_plan_ints(n), -77);
                const int ga = track_identity_plan(s.data(), n, a.data()), gb = track_plan(s.data(), n, b.data());
                CHECK(ga == gb && a == b, "n %d streams %d rep %d", n, streams, rep);
                // every frame once, in call order within its stream, streams ascending
                const int32_t *gs = track_plan_group_stream(a.data(), n), *gf = track_plan_group_first(a.data(), n), *order = track_plan_order(a.data(), n);
                int seen = 0;
                for (int g = 0; g < ga; ++g) {
                    CHECK(g == 0 || gs[g] > gs[g - 1], "groups ascend");
                    for (int k = gf[g]; k < gf[g + 1]; ++k, ++seen) {
                        CHECK(order[k] >= 0 && order[k] < n && s[(size_t)order[k]] == gs[g], "frame %d in group %d", order[k], g);
                        CHECK(k == gf[g] || order[k] > order[k - 1], "call order within a stream");
                    }
                }
                CHECK(seen == n, "%d of %d frames listed", seen, n);
            }
}

int main()
{
    config_bounds();
    size_bound();
    plan_is_the_trackers();
    std::printf("%ld steps, %ld checks, %ld failures\n", steps, checks, failures);
    return failures ? 1 : 0;
}
