// gallery_book.h -- GalleryBook: the host bookkeeping of a face gallery (include/rfd.h, "gallery"): which rows exist, which are
// live, which carry an identity or a tag, what the device's live words still lack, and what a remove / replace / set-identities
// / set-tags call sends to the device.  Plain host C++ with no HIP in it: gallery_host.hip owns one book per gallery and enqueues what it plans,
// and tests/cpp/gallery_book_check.cpp builds it with the host compiler alone.  A check that refuses leaves its reason in the
// caller's msg and the book unchanged.
#ifndef RFD_GALLERY_BOOK_H
#define RFD_GALLERY_BOOK_H
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../include/rfd.h"

namespace rfd {

// A list of rows travels to the device in chunks of at most kEditRows, each through one slot of kEditInts ints:
//   remove / replace (plan_edit):        rows [m] | blocks [nb] | their new live words [nb] | rows that lose an identity [nu]
//   set identities (plan_identities):    rows [m] | identities [m]
//   set tags (plan_tags):                rows [m] | tags [m] (the 32 bits of each, carried in an int)
// nb <= m (a block per row at most) and nu <= m (each row once), so m + 2 nb + nu <= 4 m <= kEditInts.
constexpr int kEditRows = 1024, kEditInts = 4 * kEditRows;
static_assert(kEditInts >= 4 * kEditRows, "a slot holds the worst case of plan_edit: every row in a block of its own, every row labelled");

struct GalleryEditPlan {
    int m, nb, nu; // rows, distinct blocks, rows that lose an identity
    int ints() const { return m + 2 * nb + nu; }
};

class GalleryBook {
public:
    void init(int dim, int capacity) { dim_ = dim; capacity_ = capacity; clear(); }
    int dim() const { return dim_; }
    int capacity() const { return capacity_; }
    int rows() const { return rows_; }         // slots handed out so far, removed ones included
    int removed() const { return removed_; }
    int labelled() const { return labelled_; } // live rows with an identity >= 0
    // one word per block of 16 rows enrolled so far, bit i = row 16 b + i is live: what the device's twin holds once synced
    const std::vector<uint16_t> &live_words() const { return live_words_; }
    bool is_live(int row) const { return (live_words_[(size_t)row >> 4] >> (row & 15)) & 1; }

    // ---- argument checks ----
    int check_room(int n, char *msg, size_t cap) const
    {
        if (n <= capacity_ - rows_) return RFD_OK;
        snprintf(msg, cap, "the gallery holds %d of %d rows: %d more do not fit", rows_, capacity_, n);
        return RFD_ERR_CAPACITY;
    }
    int check_rows(const int32_t *rows, int n, char *msg, size_t cap) const
    {
        for (int i = 0; i < n; ++i)
            if (rows[i] < 0 || rows[i] >= rows_) {
                snprintf(msg, cap, "invalid argument: rows[%d] = %d is not in [0, %d)", i, rows[i], rows_);
                return RFD_ERR_INVALID_ARG;
            }
        return RFD_OK;
    }
    static int check_distinct(const int32_t *rows, int n, char *msg, size_t cap)
    {
        std::vector<int32_t> sorted(rows, rows + n);
        std::sort(sorted.begin(), sorted.end());
        for (int i = 1; i < n; ++i)
            if (sorted[i] == sorted[i - 1]) {
                snprintf(msg, cap, "invalid argument: row %d is listed more than once", sorted[i]);
                return RFD_ERR_INVALID_ARG;
            }
        return RFD_OK;
    }
    // rows (all in the gallery: check_rows) that may take the identities ids: none removed, every id an identity or "none"
    int check_identities(const int32_t *rows, const int32_t *ids, int n, char *msg, size_t cap) const
    {
        for (int i = 0; i < n; ++i) {
            if (!is_live(rows[i])) {
                snprintf(msg, cap, "invalid argument: rows[%d] = %d is a removed row", i, rows[i]);
                return RFD_ERR_INVALID_ARG;
            }
            if (ids[i] < RFD_GALLERY_NO_IDENTITY) {
                snprintf(msg, cap, "invalid argument: ids[%d] = %d is neither an identity (>= 0) nor RFD_GALLERY_NO_IDENTITY", i, ids[i]);
                return RFD_ERR_INVALID_ARG;
            }
        }
        return RFD_OK;
    }

    // rows (all in the gallery: check_rows) that may take a tag: none removed.  Every 32-bit value is a tag.
    int check_tags(const int32_t *rows, int n, char *msg, size_t cap) const
    {
        for (int i = 0; i < n; ++i)
            if (!is_live(rows[i])) {
                snprintf(msg, cap, "invalid argument: rows[%d] = %d is a removed row", i, rows[i]);
                return RFD_ERR_INVALID_ARG;
            }
        return RFD_OK;
    }

    // n more rows (check_room), all live; returns the first of them
    int add(int n)
    {
        const int row0 = rows_, row1 = rows_ + n;
        live_words_.resize((size_t)(row1 + 15) / 16, 0);
        for (int r = row0; r < row1;) {
            const int b = r >> 4, end = std::min(row1, (b + 1) * 16);
            live_words_[b] |= (uint16_t)((0xffffu >> (16 - (end - b * 16))) & (0xffffu << (r & 15)));
            r = end;
        }
        rows_ = row1;
        return row0;
    }

    // The device's live words are read by the masked scan only, which runs while removed() > 0, so they are brought up to date
    // lazily: they are right for rows [0, row0) of unsynced(), the rows [row0, row1) added since are all live, and the caller
    // sets their bits (launch_gallery_live_range) before the words are next written or read, then calls mark_synced().  A
    // gallery that never removes a row never touches them.
    struct Rows {
        int row0, row1;
        bool empty() const { return row0 >= row1; }
    };
    Rows unsynced() const { return {live_synced_, rows_}; }
    void mark_synced() { live_synced_ = rows_; }

    // One chunk of a replace (revive: the rows become live) or a remove (they become removed and lose their identity): m <=
    // kEditRows rows, all in the gallery.  Updates the book and fills slot [kEditInts] as laid out above; the blocks ascend.  A
    // removed row is always unlabelled, so the rows that lose an identity are the listed ones that still have one; a row's
    // second mention finds it gone, and each is listed once.  A remove also zeroes the rows' tags in the book; on the device
    // the caller zeroes the tags of all m listed rows (the slot's first m ints).
    GalleryEditPlan plan_edit(const int32_t *rows, int m, bool revive, int32_t *slot)
    {
        int32_t *blk = slot + m;
        for (int i = 0; i < m; ++i) {
            const int r = rows[i];
            slot[i] = r;
            blk[i] = r >> 4;
            if (!revive && (size_t)r < tag_.size()) tag_[r] = 0;
            if (is_live(r) == revive) continue;
            live_words_[(size_t)r >> 4] ^= (uint16_t)(1u << (r & 15));
            removed_ += revive ? -1 : 1;
        }
        std::sort(blk, blk + m);
        const int nb = (int)(std::unique(blk, blk + m) - blk);
        int32_t *word = blk + nb, *unlabel = word + nb;
        for (int j = 0; j < nb; ++j) word[j] = live_words_[blk[j]];
        int nu = 0;
        for (int i = 0; !revive && i < m; ++i) {
            const int r = rows[i];
            if ((size_t)r >= ident_.size() || ident_[r] < 0) continue;
            ident_[r] = RFD_GALLERY_NO_IDENTITY;
            --labelled_;
            unlabel[nu++] = r;
        }
        return {m, nb, nu};
    }

    // One chunk of a set-identities call: m <= kEditRows distinct live rows and their identities (check_identities).  Updates the
    // book and fills slot with rows | identities.
    void plan_identities(const int32_t *rows, const int32_t *ids, int m, int32_t *slot)
    {
        if (ident_.size() < (size_t)rows_) ident_.resize((size_t)rows_, RFD_GALLERY_NO_IDENTITY);
        for (int i = 0; i < m; ++i) {
            int32_t &have = ident_[rows[i]];
            labelled_ += (ids[i] >= 0) - (have >= 0);
            have = slot[m + i] = ids[i];
            slot[i] = rows[i];
        }
    }

    // One chunk of a set-tags call: m <= kEditRows distinct live rows and their tags (check_tags).  Updates the book and fills
    // slot with rows | tags.
    void plan_tags(const int32_t *rows, const uint32_t *tags, int m, int32_t *slot)
    {
        if (tag_.size() < (size_t)rows_) tag_.resize((size_t)rows_, 0u);
        for (int i = 0; i < m; ++i) {
            tag_[rows[i]] = tags[i];
            slot[i] = rows[i];
            slot[m + i] = (int32_t)tags[i];
        }
    }

    void clear() // no rows; dim and capacity stay
    {
        rows_ = removed_ = live_synced_ = labelled_ = 0;
        live_words_.clear();
        ident_.clear();
        tag_.clear();
    }

    // the liveness bytes of the gallery file (gallery_file.h): bit (r & 7) of byte r >> 3 is set while row r is live
    std::vector<unsigned char> file_bits() const
    {
        std::vector<unsigned char> bits((size_t)(rows_ + 7) / 8, 0);
        for (size_t i = 0; i < bits.size(); ++i) bits[i] = (unsigned char)(live_words_[i >> 1] >> (8 * (i & 1)));
        return bits;
    }
    // the book of a file of `rows` rows <= capacity, `live` of them live by `bits`; no identities, no tags.  The caller copies
    // live_words() to the device: the book counts them as synced.
    void from_file(int rows, int live, const std::vector<unsigned char> &bits)
    {
        clear();
        rows_ = live_synced_ = rows;
        removed_ = rows - live;
        live_words_.assign((size_t)(rows + 15) / 16, 0);
        for (size_t i = 0; i < bits.size(); ++i) live_words_[i >> 1] |= (uint16_t)(bits[i] << (8 * (i & 1)));
    }

    // the first min(cap, removed()) removed rows, ascending; returns how many were written
    int removed_rows(int32_t *out, int cap) const
    {
        int at = 0;
        for (int r = 0; r < rows_ && at < cap && at < removed_; ++r)
            if (!is_live(r)) out[at++] = r;
        return at;
    }
    // identities of rows [row0, row0 + n), all in the gallery; the rows behind the last one ever labelled are unlabelled
    void identities(int row0, int n, int32_t *out) const
    {
        for (int i = 0; i < n; ++i) out[i] = (size_t)(row0 + i) < ident_.size() ? ident_[row0 + i] : RFD_GALLERY_NO_IDENTITY;
    }
    // tags of rows [row0, row0 + n), all in the gallery; the rows behind the last one ever tagged have tag 0
    void tags(int row0, int n, uint32_t *out) const
    {
        for (int i = 0; i < n; ++i) out[i] = (size_t)(row0 + i) < tag_.size() ? tag_[row0 + i] : 0u;
    }

private:
    int dim_ = 0, capacity_ = 0, rows_ = 0;
    int removed_ = 0, live_synced_ = 0, labelled_ = 0;
    std::vector<uint16_t> live_words_; // the truth about liveness; the device's words follow it (unsynced)
    std::vector<int32_t> ident_;       // the truth about identities: rows [0, size()), shorter than rows_ until a label is set
    std::vector<uint32_t> tag_;        // the truth about tags: rows [0, size()), shorter than rows_ until a tag is set; 0 beyond
};

} // namespace rfd
#endif
