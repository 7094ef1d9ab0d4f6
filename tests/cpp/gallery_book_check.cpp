// gallery_book_check.cpp -- the gallery's host bookkeeping (csrc/gallery_book.h) alone, built with the host compiler under
// -fsanitize=address,undefined by tests/test_gallery_book_cpu.py and run as a program.  Next to the book it keeps a naive model,
// one bool and one int per row, and an image of the device's live words as the calls of csrc/gallery_host.hip would leave them;
// it drives book and model with the call sequences of the rfd_gallery_* entries -- constructed cases first, then seeded random
// ones -- and compares everything after every step.  No HIP, no device, nothing loaded into Python.
#include <algorithm>
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

// The book, the model, and the image of the device's words.
struct Pair {
    GalleryBook book;
    int cap;
    std::vector<bool> live; // per row handed out
    std::vector<int> id;    // per row handed out, -1 = unlabelled
    int synced = 0;         // rows the device's words were last brought up to
    std::vector<uint16_t> dev; // the device's live words: ceil(cap / 16), as live_range / put / the clear's memset leave them
    const char *what;

    Pair(int capacity, const char *what_) : cap(capacity), dev((size_t)(capacity + 15) / 16, 0), what(what_) { book.init(32, capacity); }
    int rows() const { return (int)live.size(); }
    uint16_t word(int b) const
    {
        unsigned w = 0;
        for (int i = 0; i < 16 && 16 * b + i < rows(); ++i) w |= (unsigned)live[(size_t)16 * b + i] << i;
        return (uint16_t)w;
    }

    void compare()
    {
        ++steps;
        int removed = 0, labelled = 0;
        for (int r = 0; r < rows(); ++r) { removed += !live[r]; labelled += id[r] >= 0; }
        CHECK(book.rows() == rows() && book.capacity() == cap && book.dim() == 32, "%s: rows %d, model %d", what, book.rows(), rows());
        CHECK(book.removed() == removed, "%s: removed %d, model %d", what, book.removed(), removed);
        CHECK(book.labelled() == labelled, "%s: labelled %d, model %d", what, book.labelled(), labelled);
        CHECK(book.live_words().size() == (size_t)(rows() + 15) / 16, "%s: %zu words for %d rows", what, book.live_words().size(), rows());
        std::vector<int32_t> ids((size_t)rows() + 1, 12345);
        book.identities(0, rows(), ids.data());
        CHECK(ids[(size_t)rows()] == 12345, "%s: identities() wrote past its rows", what);
        std::vector<int32_t> gone;
        for (int r = 0; r < rows(); ++r) {
            CHECK(book.is_live(r) == live[r], "%s: live bit of row %d is %d", what, r, (int)book.is_live(r));
            CHECK(ids[r] == id[r], "%s: identity of row %d is %d, model %d", what, r, ids[r], id[r]);
            CHECK(live[r] || id[r] < 0, "%s: the removed row %d is labelled in the model", what, r);
            if (!live[r]) gone.push_back(r);
        }
        for (size_t b = 0; b < book.live_words().size(); ++b) CHECK(book.live_words()[b] == word((int)b), "%s: word %zu is 0x%04x, model 0x%04x", what, b, book.live_words()[b], word((int)b));
        std::vector<int32_t> got(gone.size() + 1, kGuard);
        CHECK(book.removed_rows(got.data(), (int)gone.size()) == (int)gone.size() && got.back() == kGuard, "%s: removed_rows count", what);
        got.pop_back();
        CHECK(got == gone, "%s: removed_rows differ from the model's", what);
        if (gone.size() > 1) { // a cap below the count: the first rows only
            std::vector<int32_t> few(2, kGuard);
            CHECK(book.removed_rows(few.data(), 1) == 1 && few[0] == gone[0] && few[1] == kGuard, "%s: removed_rows with cap 1", what);
        }
        const GalleryBook::Rows u = book.unsynced();
        CHECK(u.row0 == synced && u.row1 == rows() && u.empty() == (synced >= rows()), "%s: unsynced [%d, %d), model [%d, %d)", what, u.row0, u.row1, synced, rows());
        // the device's words: right for the blocks of rows [0, synced) but for the bits of rows added since, zero behind them
        for (size_t b = 0; b < dev.size(); ++b) {
            unsigned want = 0;
            for (int i = 0; i < 16; ++i) {
                const int r = 16 * (int)b + i;
                if (r < synced && r < rows() && live[r]) want |= 1u << i;
            }
            CHECK(dev[b] == want, "%s: device word %zu is 0x%04x, expected 0x%04x (synced %d, rows %d)", what, b, dev[b], want, synced, rows());
        }
    }

    // gallery_live_sync: launch_gallery_live_range sets the bits of the range
    void sync()
    {
        const GalleryBook::Rows u = book.unsynced();
        CHECK(u.row0 == synced && u.row1 == rows(), "%s: sync of [%d, %d), model [%d, %d)", what, u.row0, u.row1, synced, rows());
        for (int r = u.row0; r < u.row1; ++r) dev[(size_t)r >> 4] |= (uint16_t)(1u << (r & 15));
        book.mark_synced();
        synced = rows();
    }

    // rfd_gallery_add_device
    int add(int n)
    {
        char msg[256] = "";
        const int st = book.check_room(n, msg, sizeof msg);
        CHECK((st == RFD_OK) == (n <= cap - rows()), "%s: check_room(%d) with %d of %d rows says %d", what, n, rows(), cap, st);
        if (st != RFD_OK) {
            char want[256];
            std::snprintf(want, sizeof want, "the gallery holds %d of %d rows: %d more do not fit", rows(), cap, n);
            CHECK(st == RFD_ERR_CAPACITY && !std::strcmp(msg, want), "%s: check_room message \"%s\"", what, msg);
        } else {
            const int first = book.add(n);
            CHECK(first == rows(), "%s: add(%d) returned row %d, model %d", what, n, first, rows());
            live.insert(live.end(), (size_t)n, true);
            id.insert(id.end(), (size_t)n, -1);
        }
        compare();
        return st;
    }

    // rfd_gallery_remove (revive false) / rfd_gallery_replace_device (revive true): the checks, then gallery_edit's chunk loop
    int edit(const std::vector<int32_t> &list, bool revive)
    {
        char msg[256] = "";
        const int n = (int)list.size();
        int st = book.check_rows(list.data(), n, msg, sizeof msg);
        bool in_range = true;
        for (int32_t r : list) in_range = in_range && r >= 0 && r < rows();
        CHECK((st == RFD_OK) == in_range, "%s: check_rows says %d (\"%s\")", what, st, msg);
        if (st == RFD_OK && revive) {
            st = GalleryBook::check_distinct(list.data(), n, msg, sizeof msg);
            CHECK((st == RFD_OK) == (std::set<int32_t>(list.begin(), list.end()).size() == list.size()), "%s: check_distinct says %d (\"%s\")", what, st, msg);
        }
        if (st != RFD_OK) { CHECK(st == RFD_ERR_INVALID_ARG && msg[0], "%s: a refused list has status %d", what, st); compare(); return st; }
        sync();
        for (int at = 0; at < n; at += kEditRows) edit_chunk(list.data() + at, n - at < kEditRows ? n - at : kEditRows, revive);
        return RFD_OK;
    }

    void edit_chunk(const int32_t *list, int m, bool revive)
    {
        std::vector<int32_t> lost; // the model first: what the chunk must have done
        std::set<int32_t> blocks;
        for (int i = 0; i < m; ++i) {
            const int r = list[i];
            blocks.insert(r >> 4);
            if (revive) live[r] = true;
            else if (live[r]) {
                live[r] = false;
                if (id[r] >= 0) { id[r] = -1; lost.push_back(r); }
            }
        }
        std::vector<int32_t> slot((size_t)kEditInts + 1, kGuard);
        const rfd::GalleryEditPlan p = book.plan_edit(list, m, revive, slot.data());
        CHECK(p.m == m && p.nb == (int)blocks.size() && p.nu == (int)lost.size(), "%s: plan {%d, %d, %d}, model {%d, %zu, %zu}", what, p.m, p.nb, p.nu, m, blocks.size(), lost.size());
        CHECK(p.ints() == p.m + 2 * p.nb + p.nu && p.ints() <= kEditInts, "%s: a slot of %d ints", what, p.ints());
        CHECK(slot[(size_t)kEditInts] == kGuard, "%s: the word behind the slot was overwritten", what);
        // the blocks are sorted in place, m of them before they are made unique: the book may touch 2 m ints, or its result if longer
        for (int i = p.ints() > 2 * m ? p.ints() : 2 * m; i < kEditInts; ++i)
            if (slot[(size_t)i] != kGuard) { CHECK(false, "%s: the slot was written at %d, behind its %d ints", what, i, p.ints()); break; }
        ++checks;
        if (p.nb != (int)blocks.size() || p.nu != (int)lost.size()) { compare(); return; }
        const int32_t *blk = slot.data() + m, *word_ = blk + p.nb, *unlabel = word_ + p.nb;
        for (int i = 0; i < m; ++i) CHECK(slot[i] == list[i], "%s: slot row %d is %d, listed %d", what, i, slot[i], list[i]);
        int j = 0;
        for (int32_t b : blocks) { // std::set iterates ascending: the slot's blocks must be exactly these, so strictly ascending
            CHECK(blk[j] == b, "%s: block %d of the slot is %d, expected %d", what, j, blk[j], b);
            CHECK(j == 0 || blk[j] > blk[j - 1], "%s: the slot's blocks do not ascend at %d", what, j);
            CHECK(word_[j] == (int32_t)word(b), "%s: word of block %d is 0x%x, model 0x%x", what, b, word_[j], word(b));
            if (blk[j] >= 0 && (size_t)blk[j] < dev.size()) dev[(size_t)blk[j]] = (uint16_t)word_[j]; // gallery_put_kernel's words
            ++j;
        }
        for (size_t i = 0; i < lost.size(); ++i) CHECK(unlabel[i] == lost[i], "%s: unlabel %zu is %d, expected %d", what, i, unlabel[i], lost[i]);
        compare();
    }

    // rfd_gallery_set_identities: the checks in its order, then the chunk loop
    int set_ids(const std::vector<int32_t> &list, const std::vector<int32_t> &ids)
    {
        char msg[256] = "";
        const int n = (int)list.size();
        int st = book.check_rows(list.data(), n, msg, sizeof msg);
        if (st == RFD_OK) st = book.check_identities(list.data(), ids.data(), n, msg, sizeof msg);
        if (st == RFD_OK) st = GalleryBook::check_distinct(list.data(), n, msg, sizeof msg);
        bool fine = std::set<int32_t>(list.begin(), list.end()).size() == list.size();
        for (int i = 0; i < n; ++i) fine = fine && list[i] >= 0 && list[i] < rows() && live[list[i]] && ids[i] >= -1;
        CHECK((st == RFD_OK) == fine, "%s: the identity checks say %d (\"%s\")", what, st, msg);
        if (st != RFD_OK) { CHECK(st == RFD_ERR_INVALID_ARG && msg[0], "%s: refused identities have status %d", what, st); last_msg = msg; compare(); return st; }
        for (int at = 0; at < n; at += kEditRows) {
            const int m = n - at < kEditRows ? n - at : kEditRows;
            std::vector<int32_t> slot((size_t)kEditInts + 1, kGuard);
            book.plan_identities(list.data() + at, ids.data() + at, m, slot.data());
            for (int i = 0; i < m; ++i) {
                CHECK(slot[i] == list[at + i] && slot[m + i] == ids[at + i], "%s: identity slot entry %d is (%d, %d)", what, i, slot[i], slot[m + i]);
                id[list[at + i]] = ids[at + i];
            }
            CHECK(slot[(size_t)2 * m] == kGuard && slot[(size_t)kEditInts] == kGuard, "%s: the identity slot was written behind its %d ints", what, 2 * m);
            compare();
        }
        return RFD_OK;
    }
    std::string last_msg;

    // rfd_gallery_clear: the memset of the device's words covers the blocks of the synced rows
    void clear()
    {
        const int was = book.unsynced().row0;
        for (int b = 0; b < (was + 15) / 16; ++b) dev[(size_t)b] = 0;
        book.clear();
        live.clear();
        id.clear();
        synced = 0;
        compare();
    }

    // rfd_gallery_save -> rfd_gallery_load: the bytes of the file and a new book from them
    void file_round_trip()
    {
        const std::vector<unsigned char> bits = book.file_bits();
        CHECK(bits.size() == (size_t)(rows() + 7) / 8, "%s: %zu liveness bytes for %d rows", what, bits.size(), rows());
        int nlive = 0;
        for (size_t i = 0; i < bits.size(); ++i)
            for (int b = 0; b < 8; ++b) {
                const int r = 8 * (int)i + b;
                const bool want = r < rows() && live[r];
                nlive += want;
                CHECK((bool)((bits[i] >> b) & 1) == want, "%s: file bit of row %d", what, r);
            }
        Pair back(cap, what);
        back.book.from_file(rows(), nlive, bits);
        back.live = live;
        back.id.assign((size_t)rows(), -1); // identities are not in the file
        back.synced = rows();
        for (size_t b = 0; b < back.book.live_words().size(); ++b) back.dev[b] = back.book.live_words()[b]; // rfd_gallery_load copies them
        back.compare();
        if (rows() < cap) back.add(1); // a loaded gallery goes on like any other
        compare();
    }
};

static std::vector<int32_t> range(int from, int n, int step = 1)
{
    std::vector<int32_t> v;
    for (int i = 0; i < n; ++i) v.push_back(from + i * step);
    return v;
}

static void constructed_sizes()
{
    for (int rows : {1, 15, 16, 17, 31, 32, 33, 4097}) {
        Pair p(rows, "sizes");
        p.file_round_trip(); // the empty gallery
        // capacity reached exactly, in pieces that end inside, at and behind a block boundary; then exceeded by one
        for (int piece : {1, 14, 1, 1, 14, 1, 1, 4064}) p.add(piece < rows - p.rows() ? piece : rows - p.rows());
        CHECK(p.rows() == rows, "sizes: %d rows after filling %d", p.rows(), rows);
        CHECK(p.add(1) == RFD_ERR_CAPACITY && p.add(0) == RFD_OK, "sizes: one row too many, then none");
        p.file_round_trip();
        p.set_ids(range(0, rows), std::vector<int32_t>((size_t)rows, 7));
        p.edit({rows - 1}, false); // the last row, labelled
        p.edit({0, rows - 1, 0}, false); // a row twice and a row that is already removed
        p.file_round_trip();
        p.edit(range(0, rows), true); // a replace of every row revives the removed ones
        p.edit(range(0, rows), false);
        p.file_round_trip(); // no live row
        p.clear();
        p.add(rows); // clear, then add: capacity is whole again
        CHECK(p.add(1) == RFD_ERR_CAPACITY, "sizes: full again after clear and add");
        p.file_round_trip();
    }
    {
        Pair one(40, "one add across blocks");
        one.add(3);
        one.add(30); // begins and ends inside a block, covers a whole one
        one.add(7);
    }
}

static void constructed_chunks()
{
    Pair p(4097, "chunks");
    p.add(4097);
    for (int m : {1, 1023, 1024}) {
        p.edit(range(5, m), false);
        p.edit(range(5, m), true);
    }
    p.edit(range(3, 1025), false); // 1024 + 1: split by the caller's loop
    p.edit(range(3, 1025, 3), true); // revives some of them, and rewrites live rows, in two chunks
    std::vector<int32_t> twice = range(100, 1024);
    twice.push_back(100); // the second mention lands in the second chunk
    p.edit(twice, false);
    CHECK(p.edit(twice, true) == RFD_ERR_INVALID_ARG, "chunks: a replace names a row twice");
    CHECK(p.edit({4097}, false) == RFD_ERR_INVALID_ARG && p.edit({-1}, false) == RFD_ERR_INVALID_ARG, "chunks: rows outside the gallery");
    p.set_ids(range(2000, 1025), range(0, 1025)); // identities in two chunks
    p.edit(range(1990, 1025), false);             // some labelled, some not
}

static void constructed_worst_slot()
{
    // 1024 rows, each in a block of its own, each labelled: m + 2 nb + nu = 4 * 1024 ints, the whole slot
    Pair p(16 * kEditRows, "worst slot");
    p.add(16 * kEditRows);
    std::vector<int32_t> list;
    for (int i = 0; i < kEditRows; ++i) list.push_back(16 * i + (i * 7) % 16);
    p.set_ids(list, range(1000, kEditRows));
    const long before = failures;
    p.edit(list, false);
    CHECK(p.book.labelled() == 0 && p.book.removed() == kEditRows && failures == before, "worst slot: %d labelled, %d removed", p.book.labelled(), p.book.removed());
    std::vector<int32_t> slot((size_t)kEditInts + 1, kGuard); // once more by hand, for the count itself
    p.edit(list, true);
    p.set_ids(list, range(0, kEditRows));
    const rfd::GalleryEditPlan plan = p.book.plan_edit(list.data(), kEditRows, false, slot.data());
    CHECK(plan.ints() == kEditInts && plan.nb == kEditRows && plan.nu == kEditRows && slot[(size_t)kEditInts] == kGuard && slot[(size_t)kEditInts - 1] == list.back(),
          "worst slot: %d ints, last %d", plan.ints(), slot[(size_t)kEditInts - 1]);
}

static void constructed_identities()
{
    Pair p(64, "identities");
    p.add(20);
    p.set_ids({3, 4}, {9, 9});
    p.add(20);
    p.set_ids({39, 20, 3}, {5, 0, -1}); // rows beyond the identities so far, and an unlabel
    p.set_ids({20}, {0}); // identity 0 is a label like any other: relabelling it counts nothing twice
    p.set_ids({20}, {4});
    p.edit({4, 39}, false);
    CHECK(p.set_ids({5, 4}, {1, 1}) == RFD_ERR_INVALID_ARG && p.last_msg == "invalid argument: rows[1] = 4 is a removed row", "identities: \"%s\"", p.last_msg.c_str());
    CHECK(p.set_ids({5, 6}, {1, -2}) == RFD_ERR_INVALID_ARG &&
              p.last_msg == "invalid argument: ids[1] = -2 is neither an identity (>= 0) nor RFD_GALLERY_NO_IDENTITY",
          "identities: \"%s\"", p.last_msg.c_str());
    CHECK(p.set_ids({5, 6, 5}, {1, 1, 1}) == RFD_ERR_INVALID_ARG && p.last_msg == "invalid argument: row 5 is listed more than once", "identities: \"%s\"", p.last_msg.c_str());
    CHECK(p.set_ids({40}, {1}) == RFD_ERR_INVALID_ARG && p.last_msg == "invalid argument: rows[0] = 40 is not in [0, 40)", "identities: \"%s\"", p.last_msg.c_str());
    p.edit({4}, true);
    p.set_ids({4}, {2}); // a revived row takes a label again
    p.clear();
    p.add(5);
    p.set_ids({4}, {1});
}

static void random_sequences()
{
    for (int cap : {1, 15, 16, 17, 31, 32, 33, 100, 1500, 4097})
        for (unsigned seed = 1; seed <= 4; ++seed) {
            std::mt19937 gen(seed * 7919u + (unsigned)cap);
            auto rnd = [&](int n) { return (int)(gen() % (unsigned)n); };
            Pair p(cap, "random");
            const int nsteps = cap > 1000 ? 120 : 300;
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
                if (op < 30 || rows == 0) p.add(rnd(4) == 0 ? rnd(cap + 2) : rnd(20));
                else if (op < 50) p.edit(some_rows(false), false);
                else if (op < 65) p.edit(some_rows(rnd(8) != 0), true);
                else if (op < 90) {
                    std::vector<int32_t> v = some_rows(rnd(8) != 0), ids;
                    if (rnd(3)) v.erase(std::remove_if(v.begin(), v.end(), [&](int32_t r) { return !p.live[r]; }), v.end());
                    for (size_t i = 0; i < v.size(); ++i) ids.push_back(rnd(6) - 1 - (rnd(40) == 0));
                    if (!v.empty()) p.set_ids(v, ids);
                } else if (op < 94) p.clear();
                else if (op < 97) p.sync();
                else p.file_round_trip();
            }
        }
}

int main()
{
    constructed_sizes();
    constructed_chunks();
    constructed_worst_slot();
    constructed_identities();
    random_sequences();
    std::printf("gallery_book_check: %ld steps, %ld checks, %ld failures\n", steps, checks, failures);
    return failures ? 1 : 0;
}
