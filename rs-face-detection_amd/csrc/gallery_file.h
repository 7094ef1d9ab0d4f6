// gallery_file.h -- the gallery file "RFDG" (include/rfd.h, "gallery file"): the one statement of the format and all of its
// validation.  Plain host C++ with no HIP in it: gallery_host.hip includes it for rfd_gallery_save / _load / _file_info, and
// tests/cpp/gallery_file_check.cpp builds it with the host compiler alone.
//
// Version 1, little-endian, in LOGICAL row order (not the fragment-major layout of the storage, so a file survives a change of
// gallery_offset):
//   bytes 0..19   "RFDG", u32 version = 1, u32 dim, u32 rows, u32 reserved = 0
//   then          ceil(rows / 8) bytes of liveness: bit (r & 7) of byte r >> 3 is set while row r is live; bits past `rows` are 0
//   then          rows x dim bf16 values (u16 each), row-major; a removed row is present, as zeros
#ifndef RFD_GALLERY_FILE_H
#define RFD_GALLERY_FILE_H
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/rfd.h"

namespace rfd {

constexpr size_t kGalleryFileHeader = 20;
constexpr uint32_t kGalleryFileVersion = 1;
constexpr int kGalleryFileMaxRows = 1 << 30; // rfd_gallery_create's largest capacity

inline bool gallery_dim_ok(int64_t dim) { return dim >= 32 && dim <= 1024 && dim % 32 == 0; }

// Reads and validates a gallery file front to back.  Every failing call leaves its reason in msg.
struct GalleryFileReader {
    FILE *f = nullptr;
    int dim = 0, rows = 0, live = 0;
    std::vector<unsigned char> bits; // the liveness bytes
    int next_row = 0;                // the row the next read_rows starts at
    char msg[256] = "";

    GalleryFileReader() = default;
    GalleryFileReader(const GalleryFileReader &) = delete;
    GalleryFileReader &operator=(const GalleryFileReader &) = delete;
    ~GalleryFileReader() { close(); }
    void close() { if (f) fclose(f); f = nullptr; }

    int fail(int status, const char *fmt, ...)
    {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(msg, sizeof msg, fmt, ap);
        va_end(ap);
        close();
        return status;
    }

    bool is_live(int row) const { return (bits[(size_t)row >> 3] >> (row & 7)) & 1; }

    // header, file length and liveness; the values follow through read_rows
    int open(const char *path)
    {
        close();
        next_row = 0;
        f = fopen(path, "rb");
        if (!f) return fail(RFD_ERR_IO, "cannot open %s", path);
        if (fseeko(f, 0, SEEK_END) != 0) return fail(RFD_ERR_IO, "cannot seek in %s", path);
        const int64_t len = (int64_t)ftello(f);
        if (len < 0 || fseeko(f, 0, SEEK_SET) != 0) return fail(RFD_ERR_IO, "cannot seek in %s", path);
        unsigned char h[kGalleryFileHeader];
        if (len < (int64_t)sizeof h) return fail(RFD_ERR_INVALID_ARG, "%s: file length %lld is shorter than the %zu-byte header", path, (long long)len, sizeof h);
        if (fread(h, 1, sizeof h, f) != sizeof h) return fail(RFD_ERR_IO, "cannot read the header of %s", path);
        auto u32 = [&](int at) { return (uint32_t)h[at] | (uint32_t)h[at + 1] << 8 | (uint32_t)h[at + 2] << 16 | (uint32_t)h[at + 3] << 24; };
        if (memcmp(h, "RFDG", 4) != 0) return fail(RFD_ERR_INVALID_ARG, "%s: wrong magic (not an RFDG gallery file)", path);
        if (u32(4) != kGalleryFileVersion) return fail(RFD_ERR_INVALID_ARG, "%s: unsupported version %u (this library reads version %u)", path, u32(4), kGalleryFileVersion);
        if (!gallery_dim_ok(u32(8))) return fail(RFD_ERR_INVALID_ARG, "%s: dim %u is not a multiple of 32 in 32..1024", path, u32(8));
        if (u32(12) > (uint32_t)kGalleryFileMaxRows) return fail(RFD_ERR_INVALID_ARG, "%s: rows %u exceed %d", path, u32(12), kGalleryFileMaxRows);
        if (u32(16) != 0) return fail(RFD_ERR_INVALID_ARG, "%s: the reserved field is %u, not 0", path, u32(16));
        dim = (int)u32(8);
        rows = (int)u32(12);
        const int64_t nbits = ((int64_t)rows + 7) / 8, want = (int64_t)sizeof h + nbits + (int64_t)rows * dim * 2;
        if (len != want)
            return fail(RFD_ERR_INVALID_ARG, "%s: file length %lld, but dim %d and rows %d imply %lld", path, (long long)len, dim, rows, (long long)want);
        bits.assign((size_t)nbits, 0);
        if (nbits && fread(bits.data(), 1, (size_t)nbits, f) != (size_t)nbits) return fail(RFD_ERR_IO, "cannot read the liveness bytes of %s", path);
        if (rows & 7) {
            const unsigned beyond = bits.back() >> (rows & 7);
            if (beyond) return fail(RFD_ERR_INVALID_ARG, "%s: liveness bits are set beyond row %d", path, rows - 1);
        }
        live = 0;
        for (unsigned char b : bits) live += __builtin_popcount(b);
        return RFD_OK;
    }

    // the next n rows' bf16 bits -> out [n][dim]; refuses a non-finite value, naming row and element
    int read_rows(int n, uint16_t *out)
    {
        if (!f || n < 0 || n > rows - next_row) return fail(RFD_ERR_INVALID_ARG, "read_rows(%d) at row %d of %d", n, next_row, rows);
        const size_t count = (size_t)n * dim;
        if (count && fread(out, 2, count, f) != count) return fail(RFD_ERR_IO, "cannot read rows %d..%d", next_row, next_row + n - 1);
        for (size_t i = 0; i < count; ++i) {
            const unsigned char *p = reinterpret_cast<const unsigned char *>(out + i);
            const uint16_t v = (uint16_t)(p[0] | p[1] << 8);
            out[i] = v;
            if ((v & 0x7f80u) == 0x7f80u)
                return fail(RFD_ERR_INVALID_ARG, "row %d holds a non-finite value (bf16 bits 0x%04x) at element %d", next_row + (int)(i / dim), v, (int)(i % dim));
        }
        next_row += n;
        return RFD_OK;
    }
};

// header and liveness of a file of `rows` rows; bits: ceil(rows / 8) bytes
inline bool gallery_file_write_head(FILE *f, int dim, int rows, const unsigned char *bits)
{
    unsigned char h[kGalleryFileHeader] = {'R', 'F', 'D', 'G'};
    const uint32_t w[4] = {kGalleryFileVersion, (uint32_t)dim, (uint32_t)rows, 0u};
    for (int i = 0; i < 4; ++i)
        for (int b = 0; b < 4; ++b) h[4 + 4 * i + b] = (unsigned char)(w[i] >> (8 * b));
    const size_t nbits = ((size_t)rows + 7) / 8;
    return fwrite(h, 1, sizeof h, f) == sizeof h && (nbits == 0 || fwrite(bits, 1, nbits, f) == nbits);
}

// count bf16 values, little-endian whatever the host
inline bool gallery_file_write_values(FILE *f, const uint16_t *v, size_t count)
{
    unsigned char buf[4096];
    for (size_t at = 0; at < count;) {
        const size_t m = count - at < sizeof buf / 2 ? count - at : sizeof buf / 2;
        for (size_t i = 0; i < m; ++i) { buf[2 * i] = (unsigned char)(v[at + i] & 0xff); buf[2 * i + 1] = (unsigned char)(v[at + i] >> 8); }
        if (fwrite(buf, 2, m, f) != m) return false;
        at += m;
    }
    return true;
}

// the whole validation, no device: rfd_gallery_file_info
inline int gallery_file_info(const char *path, int *dim, int *rows, int *live, char *msg, size_t msg_cap)
{
    GalleryFileReader r;
    int st = r.open(path);
    std::vector<uint16_t> buf;
    if (st == RFD_OK) {
        const int chunk = (1 << 16) / r.dim; // 128 KiB of values at a time
        buf.resize((size_t)chunk * r.dim);
        while (st == RFD_OK && r.next_row < r.rows) st = r.read_rows(r.rows - r.next_row < chunk ? r.rows - r.next_row : chunk, buf.data());
    }
    if (st != RFD_OK) {
        snprintf(msg, msg_cap, "%s", r.msg);
        return st;
    }
    if (dim) *dim = r.dim;
    if (rows) *rows = r.rows;
    if (live) *live = r.live;
    return RFD_OK;
}

} // namespace rfd
#endif
