// gallery_tags_check.cpp -- the tags of the gallery's host bookkeeping (csrc/gallery_book.h; include/rfd.h, "tags") alone, built
// with the host compiler under -fsanitize=address,undefined by tests/test_gallery_filter_cpu.py and run as a program.  Next to
// the book it keeps a model of one word and one bool per row, drives both with the call sequences of rfd_gallery_set_tags /
// _remove / _replace / _clear / _load as csrc/gallery_host.hip makes them, and compares every tag, and the slot a call would
// send, after every step.  No HIP, no device, nothing loaded into Python.
#include <cstdio>
#include <cstring>
#include <random>
#include <set>
#include <string>
#include <vector>

#include "../../rs-face-detection_amd/csrc/gallery_book.h"

using rfd::GalleryBook;
using rfd::kEditInts;
using rfd::kEditRows;

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

static const int32_t kGuard = 0x5a5a5a5a;
static const uint32_t kUnwritten = 0xdeadbeefu;

struct Pair {
    GalleryBook book;
    int cap;
    std::vector<bool> live;     // per row handed out
    std::vector<uint32_t> tag;  // per row handed out
    const char *what;
    std::string last_msg;

    Pair(int capacity, const char *what_) : cap(capacity), what(what_) { book.init(32, capacity); }
    int rows() const { return (int)live.size(); }

    void compare()
    {
        ++steps;
        CHECK(book.rows() == rows(), "%s: rows %d, model %d", what, book.rows(), rows());
        std::vector<uint32_t> got((size_t)rows() + 1, kUnwritten);
        book.tags(0, rows(), got.data());
        CHECK(got[(size_t)rows()] == kUnwritten, "%s: tags() wrote past its rows", what);
        for (int r = 0; r < rows(); ++r) {
            CHECK(got[r] == tag[r], "%s: tag of row %d is 0x%08x, model 0x%08x", what, r, got[r], tag[r]);
            CHECK(live[r] || tag[r] == 0, "%s: the removed row %d has a tag in the model", what, r);
            CHECK(book.is_live(r) == live[r], "%s: live bit of row %d", what, r);
        }
        if (rows() > 2) { // a window that begins inside the gallery
            uint32_t w[3] = {kUnwritten, kUnwritten, kUnwritten};
            book.tags(rows() - 2, 2, w);
            CHECK(w[0] == tag[(size_t)rows() - 2] && w[1] == tag[(size_t)rows() - 1] && w[2] == kUnwritten, "%s: tags(rows - 2, 2)", what);
        }
    }

    void add(int n)
    {
        char msg[256] = "";
        if (book.check_room(n, msg, sizeof msg) == RFD_OK) {
            book.add(n);
            live.insert(live.end(), (size_t)n, true);
            tag.insert(tag.end(), (size_t)n, 0u); // a new row has tag 0
        }
        compare();
    }

    // rfd_gallery_set_tags: the checks in its order, then the chunk loop
    int set_tags(const std::vector<int32_t> &list, const std::vector<uint32_t> &tags)
    {
        char msg[256] = "";
        const int n = (int)list.size();
        int st = book.check_rows(list.data(), n, msg, sizeof msg);
        if (st == RFD_OK) st = book.check_tags(list.data(), n, msg, sizeof msg);
        if (st == RFD_OK) st = GalleryBook::check_distinct(list.data(), n, msg, sizeof msg);
        bool fine = std::set<int32_t>(list.begin(), list.end()).size() == list.size();
        for (int i = 0; i < n; ++i) fine = fine && list[i] >= 0 && list[i] < rows() && live[list[i]];
        CHECK((st == RFD_OK) == fine, "%s: the tag checks say %d (\"%s\")", what, st, msg);
        if (st != RFD_OK) {
            CHECK(st == RFD_ERR_INVALID_ARG && msg[0], "%s: a refused list has status %d", what, st);
            last_msg = msg;
            compare(); // nothing changed
            return st;
        }
        for (int at = 0; at < n; at += kEditRows) {
            const int m = n - at < kEditRows ? n - at : kEditRows;
            std::vector<int32_t> slot((size_t)kEditInts + 1, kGuard);
            book.plan_tags(list.data() + at, tags.data() + at, m, slot.data());
            for (int i = 0; i < m; ++i) {
                uint32_t sent;
                std::memcpy(&sent, &slot[(size_t)m + i], 4);
                CHECK(slot[i] == list[at + i] && sent == tags[at + i], "%s: tag slot entry %d is (%d, 0x%08x)", what, i, slot[i], sent);
                tag[list[at + i]] = tags[at + i];
            }
            for (size_t i = (size_t)2 * m; i <= (size_t)kEditInts; ++i)
                if (slot[i] != kGuard) { CHECK(false, "%s: the tag slot was written at %zu, behind its %d ints", what, i, 2 * m); break; }
            ++checks;
            compare();
        }
        return RFD_OK;
    }

    // rfd_gallery_remove (revive false) / rfd_gallery_replace_device (revive true): gallery_edit's chunk loop.  On the device a
    // remove zeroes the tags of the slot's first m ints, the listed rows.
    void edit(const std::vector<int32_t> &list, bool revive)
    {
        const int n = (int)list.size();
        for (int at = 0; at < n; at += kEditRows) {
            const int m = n - at < kEditRows ? n - at : kEditRows;
            std::vector<int32_t> slot((size_t)kEditInts + 1, kGuard);
            const rfd::GalleryEditPlan p = book.plan_edit(list.data() + at, m, revive, slot.data());
            CHECK(p.m == m && slot[(size_t)kEditInts] == kGuard, "%s: plan_edit of %d rows", what, m);
            for (int i = 0; i < m; ++i) {
                const int r = list[at + i];
                CHECK(slot[i] == r, "%s: slot row %d is %d, listed %d", what, i, slot[i], r);
                if (revive) live[r] = true; // the tag stays: 0 for a reused hole, its own for a corrected enrolment
                else { live[r] = false; tag[r] = 0; }
            }
            compare();
        }
    }

    void clear()
    {
        book.clear();
        live.clear();
        tag.clear();
        compare();
    }

    // rfd_gallery_save -> rfd_gallery_load: tags are not in the file
    void file_round_trip()
    {
        const std::vector<unsigned char> bits = book.file_bits();
        int nlive = 0;
        for (int r = 0; r < rows(); ++r) nlive += live[r];
        Pair back(cap, what);
        back.book.from_file(rows(), nlive, bits);
        back.live = live;
        back.tag.assign((size_t)rows(), 0u);
        back.compare();
        if (rows() > 0 && back.live[0]) back.set_tags({0}, {0x80000001u}); // a loaded gallery takes tags like any other
        compare();
        // and from_file on a book that holds tags forgets them
        GalleryBook again = book;
        again.from_file(rows(), nlive, bits);
        std::vector<uint32_t> got((size_t)rows(), kUnwritten);
        again.tags(0, rows(), got.data());
        for (int r = 0; r < rows(); ++r) CHECK(got[r] == 0, "%s: from_file left tag 0x%08x on row %d", what, got[r], r);
    }
};

static std::vector<int32_t> range(int from, int n, int step = 1)
{
    std::vector<int32_t> v;
    for (int i = 0; i < n; ++i) v.push_back(from + i * step);
    return v;
}

static std::vector<uint32_t> words(int n, uint32_t seed)
{
    std::vector<uint32_t> v;
    std::mt19937 gen(seed);
    for (int i = 0; i < n; ++i) v.push_back(i % 5 == 0 ? 0x80000000u | (uint32_t)i : i % 7 == 0 ? 0xffffffffu : (uint32_t)gen());
    return v;
}

static void constructed_life_cycle()
{
    Pair p(64, "life cycle");
    p.compare(); // empty
    p.add(20);
    p.set_tags({3, 4, 19}, {0xffffffffu, 0x80000000u, 7u}); // every bit, the top bit
    p.add(20);
    p.set_tags({39, 20, 3}, {5u, 0u, 1u}); // rows beyond the tags so far; 0 is a tag like any other; a row tagged again
    p.edit({4, 39, 4}, false);             // remove zeroes, also a row named twice
    p.edit({19}, true);                    // replace of a live row keeps its tag
    CHECK(p.tag[19] == 7u, "life cycle: replace changed a tag");
    p.edit({4}, true);                     // a reused hole has tag 0
    CHECK(p.tag[4] == 0u && p.live[4], "life cycle: a reused hole");
    p.set_tags({4}, {9u});
    p.file_round_trip();
    p.clear();
    p.add(5);
    CHECK(p.tag[3] == 0u, "life cycle: clear kept a tag");
    p.set_tags({4}, {1u});
    p.file_round_trip();
    // a gallery on which no tag was ever set: removes and replaces touch nothing
    Pair q(40, "never tagged");
    q.add(33);
    q.edit({0, 32}, false);
    q.edit({0}, true);
    q.file_round_trip();
}

static void constructed_refusals()
{
    Pair p(64, "refusals");
    p.add(40);
    p.set_tags(range(0, 40), words(40, 3));
    p.edit({4}, false);
    CHECK(p.set_tags({5, 4}, {1u, 1u}) == RFD_ERR_INVALID_ARG && p.last_msg == "invalid argument: rows[1] = 4 is a removed row", "refusals: \"%s\"", p.last_msg.c_str());
    CHECK(p.set_tags({5, 6, 5}, {1u, 1u, 1u}) == RFD_ERR_INVALID_ARG && p.last_msg == "invalid argument: row 5 is listed more than once", "refusals: \"%s\"",
          p.last_msg.c_str());
    CHECK(p.set_tags({40}, {1u}) == RFD_ERR_INVALID_ARG && p.last_msg == "invalid argument: rows[0] = 40 is not in [0, 40)", "refusals: \"%s\"", p.last_msg.c_str());
    CHECK(p.set_tags({1, -1}, {1u, 1u}) == RFD_ERR_INVALID_ARG && p.last_msg == "invalid argument: rows[1] = -1 is not in [0, 40)", "refusals: \"%s\"", p.last_msg.c_str());
    CHECK(p.set_tags({}, {}) == RFD_OK, "refusals: the empty list");
    // refused on a book that never had a tag: it still has none
    Pair q(8, "refusals, untagged");
    q.add(8);
    q.edit({2}, false);
    CHECK(q.set_tags({1, 2}, {3u, 3u}) == RFD_ERR_INVALID_ARG, "refusals: a removed row on an untagged book");
}

static void constructed_chunks()
{
    Pair p(4097, "chunks");
    p.add(4097);
    for (int m : {1, 1023, 1024, 1025}) { // 1025: split by the caller's loop
        p.set_tags(range(5, m), words(m, (uint32_t)m));
        p.edit(range(5, m), false);
        p.edit(range(5, m), true);
        p.set_tags(range(4096, m, -1), words(m, (uint32_t)m + 1)); // descending rows, the gallery's last row first
    }
    std::vector<int32_t> twice = range(100, 1024);
    twice.push_back(100); // the second mention would land in the second chunk: refused before anything is planned
    CHECK(p.set_tags(twice, words(1025, 9)) == RFD_ERR_INVALID_ARG, "chunks: a row listed twice across chunks");
    p.edit(twice, false); // a remove may name it twice
    CHECK(p.set_tags(range(0, 4097), words(4097, 11)) == RFD_ERR_INVALID_ARG && p.last_msg == "invalid argument: rows[100] = 100 is a removed row",
          "chunks: a removed row in the first chunk of five: \"%s\"", p.last_msg.c_str());
    p.edit(range(0, 4097), true);
    CHECK(p.set_tags(range(0, 4097), words(4097, 11)) == RFD_OK, "chunks: every row, five chunks");
}

static void random_sequences()
{
    for (int cap : {1, 16, 17, 100, 1500})
        for (unsigned seed = 1; seed <= 3; ++seed) {
            std::mt19937 gen(seed * 104729u + (unsigned)cap);
            auto rnd = [&](int n) { return (int)(gen() % (unsigned)n); };
            Pair p(cap, "random");
            const int nsteps = cap > 1000 ? 100 : 250;
            for (int s = 0; s < nsteps; ++s) {
                const int op = rnd(100), rows = p.rows();
                auto some_rows = [&](bool distinct) {
                    std::vector<int32_t> v;
                    const int n = 1 + rnd(rnd(4) == 0 ? 2 * rows : 8);
                    for (int i = 0; i < n; ++i) v.push_back(rnd(rows));
                    if (distinct) {
                        std::set<int32_t> u(v.begin(), v.end());
                        v.assign(u.begin(), u.end());
                        for (size_t i = v.size(); i > 1; --i) std::swap(v[i - 1], v[(size_t)rnd((int)i)]);
                    }
                    return v;
                };
                if (op < 25 || rows == 0) p.add(rnd(4) == 0 ? rnd(cap + 2) : rnd(20));
                else if (op < 45) p.edit(some_rows(false), false);
                else if (op < 58) p.edit(some_rows(true), true);
                else if (op < 90) {
                    std::vector<int32_t> v = some_rows(rnd(8) != 0);
                    if (rnd(3)) {
                        std::vector<int32_t> kept;
                        for (int32_t r : v)
                            if (p.live[r]) kept.push_back(r);
                        v = kept;
                    }
                    std::vector<uint32_t> t;
                    for (size_t i = 0; i < v.size(); ++i) t.push_back(rnd(3) == 0 ? (uint32_t)gen() : (uint32_t)rnd(4) << (rnd(2) ? 30 : 0));
                    if (!v.empty()) p.set_tags(v, t);
                } else if (op < 94) p.clear();
                else p.file_round_trip();
            }
        }
}

int main()
{
    constructed_life_cycle();
    constructed_refusals();
    constructed_chunks();
    random_sequences();
    std::printf("gallery_tags_check: %ld steps, %ld checks, %ld failures\n", steps, checks, failures);
    return failures ? 1 : 0;
}
