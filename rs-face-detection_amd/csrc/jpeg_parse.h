// jpeg_parse.h -- the serial half of the baseline JPEG decoder (include/rfd.h, "JPEG decode"): marker parsing, all of the
// validation, and the Huffman decoder that turns a file into quantised coefficients.  Plain host C++ with no HIP in it:
// detector.hip includes it for rfd_jpeg_info / rfd_debug_jpeg_coefficients, jpeg_plan.h and jpeg_host.hip for
// rfd_decode_jpeg_batch*, and tests/cpp/jpeg_parse_check.cpp builds it with the host compiler alone.  The parser and the scan decoder allocate nothing,
// take no lock and touch no shared state, so one frame per worker thread decodes without any synchronisation.
//
// Supported: SOF0 / SOF1 with 8-bit samples, Huffman coding, ONE interleaved scan of one component (grey) or of three with
// luma 1x1, 2x1 or 2x2 and chroma 1x1.  Everything else is refused with RFD_ERR_UNSUPPORTED (a well-formed file of a kind
// this decoder does not do) or RFD_ERR_INVALID_ARG (a malformed file), and the message names the cause and the byte.
//
// Lenient on purpose, as libjpeg is (it warns and goes on): the Ss / Se / Ah / Al bytes of the SOS header are not compared with
// 0 / 63 / 0 (a sequential scan has no other meaning for them); whole unread bytes in front of a restart marker are dropped, so
// garbage between the last MCU of an interval and its RSTn is accepted; a file may end without EOI after its last MCU.  None of
// this lets the decoder read or write outside its buffers.
//
// What the decoder writes, per block in the order (component, block row, block column) of planes padded to whole MCUs:
//   rec[block]  = (offset << 7) | count     offset: index of the block's first value in coef[]; count: 0..64
//   coef[offset .. offset + count)          the QUANTISED coefficients in zigzag order up to the last non-zero one
// The blocks of an MCU are consecutive in coef[] (decode order), which is why every block carries its own offset.
// A reduced-size decode (rfd.h, "JPEG decode, reduced size") tells the decoder each component's inverse-DCT size n; `count` is
// then 1 + the zigzag position of the last non-zero coefficient that an n x n inverse DCT READS (jpeg_idct_reads), so the run
// ends earlier; values at unread positions inside the run still travel.
#ifndef RFD_JPEG_PARSE_H
#define RFD_JPEG_PARSE_H
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "../../include/rfd.h"

namespace rfd {

// natural (row-major) index of zigzag position k
constexpr uint8_t kJpegNatural[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                      41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                      30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
constexpr int kJpegRecCountBits = 7;                          // rec = offset << 7 | count
constexpr uint32_t kJpegMaxCoefs = 1u << (32 - kJpegRecCountBits); // a frame's coefficient slots (64 per block) must stay below this

struct JpegHuff {
    bool present = false;
    uint8_t vals[256];
    uint16_t fast[512];  // the next 9 bits -> length << 8 | symbol; 0: the code is longer than 9 bits (or absent)
    int32_t maxcode[17]; // largest code of length l, -1: none
    int32_t valoff[17];  // vals index of a code of length l = valoff[l] + code
};

struct JpegComponent {
    int id, h, v, tq, td, ta;
    int bw, bh; // blocks per row / per column of the plane, padded to whole MCUs
    int blk0;   // the plane's first block in the frame's block order
};

struct JpegHeader {
    int width = 0, height = 0, ncomp = 0, sampling = 0, restart_interval = 0;
    int hmax = 1, vmax = 1, mcux = 0, mcuy = 0, nblocks = 0;
    JpegComponent comp[3] = {};
    uint16_t quant[4][64]; // zigzag order, as the file holds them
    bool have_quant[4] = {false, false, false, false};
    JpegHuff dc[4], ac[4];
    size_t scan = 0; // the first entropy-coded byte
    int orientation = 1; // the EXIF orientation tag, 1..8 (jpeg_exif_orientation); 1 where the file has none
    char msg[200] = "";

    int fail(int status, const char *fmt, ...)
    {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(msg, sizeof msg, fmt, ap);
        va_end(ap);
        return status;
    }
};

// the code lengths and symbols of one DHT table -> the decoding tables; false: the lengths do not form a prefix code
inline bool jpeg_build_huff(JpegHuff &t, const uint8_t bits[17], const uint8_t *vals, int count)
{
    memset(t.fast, 0, sizeof t.fast);
    memset(t.vals, 0, sizeof t.vals);
    memcpy(t.vals, vals, (size_t)count);
    uint32_t code = 0;
    int k = 0;
    for (int l = 1; l <= 16; ++l) {
        t.valoff[l] = k - (int32_t)code;
        for (int i = 0; i < bits[l]; ++i, ++k, ++code) {
            if (l <= 9)
                for (uint32_t f = code << (9 - l), e = f + (1u << (9 - l)); f < e && f < 512; ++f) t.fast[f] = (uint16_t)(l << 8 | vals[k]);
        }
        if (code > (1u << l)) return false;
        t.maxcode[l] = bits[l] ? (int32_t)code - 1 : -1;
        code <<= 1;
    }
    t.maxcode[0] = -1;
    t.valoff[0] = 0;
    t.present = true;
    return true;
}

// The orientation tag (0x0112) of an Exif APP1 payload p[0 .. n), which begins with "Exif\0\0": a TIFF header (byte order, 42,
// the offset of IFD0 from the start of the header) and IFD0, a 16-bit count of 12-byte entries (tag, type, count, value).  The
// first entry with the tag counts, if it is one SHORT or one LONG with a value of 1..8; 1 in every other case -- EXIF damage is
// never a reason to refuse a file (libjpeg, OpenCV and Pillow agree).  Every read is checked against the payload first, in size_t
// sums of values below 2^32 + 2^20, which cannot wrap.
inline int jpeg_exif_orientation(const uint8_t *p, size_t n)
{
    if (n < 6 + 8) return 1;
    const uint8_t *t = p + 6; // the TIFF block: offsets count from here
    const size_t tn = n - 6;
    const bool le = t[0] == 'I' && t[1] == 'I';
    if (!le && !(t[0] == 'M' && t[1] == 'M')) return 1;
    auto u16 = [&](size_t at) -> uint32_t { return le ? (uint32_t)t[at] | (uint32_t)t[at + 1] << 8 : (uint32_t)t[at] << 8 | t[at + 1]; };
    auto u32 = [&](size_t at) -> uint32_t { return le ? u16(at) | u16(at + 2) << 16 : u16(at) << 16 | u16(at + 2); };
    if (u16(2) != 42) return 1;
    const size_t ifd = u32(4);
    if (ifd > tn || tn - ifd < 2) return 1;
    const size_t entries = u16(ifd);
    for (size_t e = 0; e < entries; ++e) {
        const size_t at = ifd + 2 + 12 * e; // below 2^32 + 2 + 12 * 65535
        if (at > tn || tn - at < 12) return 1; // the directory runs past the payload
        if (u16(at) != 0x0112) continue;
        const uint32_t type = u16(at + 2), count = u32(at + 4);
        if (count != 1 || (type != 3 && type != 4)) return 1;
        const uint32_t v = type == 3 ? u16(at + 8) : u32(at + 8);
        return v >= 1 && v <= 8 ? (int)v : 1;
    }
    return 1;
}

// Walks the markers from SOI to the end of the SOS header and validates every one of them.
inline int jpeg_parse_header(const uint8_t *d, size_t len, JpegHeader &h)
{
    if (!d) return h.fail(RFD_ERR_INVALID_ARG, "invalid argument: the JPEG data pointer is null");
    if (len < 2 || d[0] != 0xff || d[1] != 0xd8) return h.fail(RFD_ERR_INVALID_ARG, "not a JPEG file: no SOI marker at byte 0");
    size_t pos = 2;
    bool have_sof = false, have_exif = false;
    for (;;) {
        if (pos >= len) return h.fail(RFD_ERR_INVALID_ARG, "truncated: the data ends at byte %zu, before any SOS marker", len);
        if (d[pos] != 0xff) return h.fail(RFD_ERR_INVALID_ARG, "expected a marker at byte %zu, found 0x%02x", pos, d[pos]);
        while (pos < len && d[pos] == 0xff) ++pos; // fill bytes in front of a marker
        if (pos >= len) return h.fail(RFD_ERR_INVALID_ARG, "truncated: the data ends at byte %zu inside a marker", len);
        const size_t at = pos - 1;
        const int m = d[pos++];
        if (m == 0x00) return h.fail(RFD_ERR_INVALID_ARG, "a stuffed 0xFF00 at byte %zu, outside entropy-coded data", at);
        if (m == 0xd8) return h.fail(RFD_ERR_INVALID_ARG, "a second SOI marker at byte %zu", at);
        if (m == 0xd9) return h.fail(RFD_ERR_INVALID_ARG, "EOI at byte %zu, before any SOS marker", at);
        if ((m >= 0xd0 && m <= 0xd7) || m == 0x01) return h.fail(RFD_ERR_INVALID_ARG, "marker 0xFF%02X at byte %zu, outside a scan", m, at);
        if (pos + 2 > len) return h.fail(RFD_ERR_INVALID_ARG, "truncated: the length field of marker 0xFF%02X at byte %zu is cut off", m, at);
        const size_t L = (size_t)d[pos] << 8 | d[pos + 1];
        if (L < 2) return h.fail(RFD_ERR_INVALID_ARG, "marker 0xFF%02X at byte %zu has length %zu, less than 2", m, at, L);
        if (pos + L > len) return h.fail(RFD_ERR_INVALID_ARG, "the length field of marker 0xFF%02X at byte %zu points past the end (%zu > %zu)", m, at, pos + L, len);
        const uint8_t *seg = d + pos + 2;
        size_t n = L - 2;
        switch (m) {
        case 0xdb: // DQT
            while (n > 0) {
                const int pq = seg[0] >> 4, tq = seg[0] & 15;
                if (pq > 1 || tq > 3) return h.fail(RFD_ERR_INVALID_ARG, "DQT at byte %zu: precision %d / table %d out of range", at, pq, tq);
                const size_t need = 1 + 64 * (size_t)(pq + 1);
                if (n < need) return h.fail(RFD_ERR_INVALID_ARG, "DQT at byte %zu: the segment is too short for its table", at);
                for (int k = 0; k < 64; ++k) h.quant[tq][k] = pq ? (uint16_t)(seg[1 + 2 * k] << 8 | seg[2 + 2 * k]) : seg[1 + k];
                h.have_quant[tq] = true;
                seg += need; n -= need;
            }
            break;
        case 0xc4: // DHT
            while (n > 0) {
                const int tc = seg[0] >> 4, th = seg[0] & 15;
                if (tc > 1 || th > 3) return h.fail(RFD_ERR_INVALID_ARG, "DHT at byte %zu: class %d / table %d out of range", at, tc, th);
                if (n < 17) return h.fail(RFD_ERR_INVALID_ARG, "DHT at byte %zu: the segment is too short for its code lengths", at);
                uint8_t bits[17] = {0};
                int count = 0;
                for (int l = 1; l <= 16; ++l) count += bits[l] = seg[l];
                if (count > 256 || n < 17 + (size_t)count) return h.fail(RFD_ERR_INVALID_ARG, "DHT at byte %zu: %d symbols do not fit the segment", at, count);
                if (tc == 0)
                    for (int i = 0; i < count; ++i)
                        if (seg[17 + i] > 15) return h.fail(RFD_ERR_INVALID_ARG, "DHT at byte %zu: DC symbol %d is above 15", at, seg[17 + i]);
                if (!jpeg_build_huff(tc ? h.ac[th] : h.dc[th], bits, seg + 17, count))
                    return h.fail(RFD_ERR_INVALID_ARG, "DHT at byte %zu: the code lengths of table %d do not form a prefix code", at, th);
                seg += 17 + count; n -= 17 + (size_t)count;
            }
            break;
        case 0xc0: case 0xc1: { // SOF0, SOF1
            if (have_sof) return h.fail(RFD_ERR_INVALID_ARG, "a second SOF marker at byte %zu", at);
            if (n < 6) return h.fail(RFD_ERR_INVALID_ARG, "SOF at byte %zu: the segment is too short", at);
            const int prec = seg[0], nf = seg[5];
            h.height = seg[1] << 8 | seg[2];
            h.width = seg[3] << 8 | seg[4];
            if (prec == 12) return h.fail(RFD_ERR_UNSUPPORTED, "unsupported JPEG: 12-bit precision (SOF at byte %zu)", at);
            if (prec != 8) return h.fail(RFD_ERR_INVALID_ARG, "SOF at byte %zu: sample precision %d", at, prec);
            if (h.width == 0 || h.height == 0) return h.fail(RFD_ERR_INVALID_ARG, "SOF at byte %zu: zero dimensions (%d x %d)", at, h.width, h.height);
            if (nf == 4) return h.fail(RFD_ERR_UNSUPPORTED, "unsupported JPEG: four components (SOF at byte %zu)", at);
            if (nf != 1 && nf != 3) return h.fail(nf == 2 ? RFD_ERR_UNSUPPORTED : RFD_ERR_INVALID_ARG, "SOF at byte %zu: %d components (this decoder does 1 and 3)", at, nf);
            if (n != 6 + 3 * (size_t)nf) return h.fail(RFD_ERR_INVALID_ARG, "SOF at byte %zu: length %zu does not match %d components", at, L, nf);
            h.ncomp = nf;
            for (int c = 0; c < nf; ++c) {
                JpegComponent &k = h.comp[c];
                k.id = seg[6 + 3 * c];
                k.h = seg[7 + 3 * c] >> 4; k.v = seg[7 + 3 * c] & 15;
                k.tq = seg[8 + 3 * c];
                if (k.h < 1 || k.h > 4 || k.v < 1 || k.v > 4 || k.tq > 3)
                    return h.fail(RFD_ERR_INVALID_ARG, "SOF at byte %zu: component %d has sampling %dx%d, table %d", at, c, k.h, k.v, k.tq);
            }
            if (nf == 1) {
                h.comp[0].h = h.comp[0].v = 1; // a single-component scan is not interleaved: one block per MCU whatever the factors say
                h.sampling = 0;
            } else {
                const JpegComponent *k = h.comp;
                const bool chroma = k[1].h == 1 && k[1].v == 1 && k[2].h == 1 && k[2].v == 1;
                if (chroma && k[0].h == 1 && k[0].v == 1) h.sampling = 1;
                else if (chroma && k[0].h == 2 && k[0].v == 1) h.sampling = 2;
                else if (chroma && k[0].h == 2 && k[0].v == 2) h.sampling = 3;
                else
                    return h.fail(RFD_ERR_UNSUPPORTED, "unsupported JPEG: sampling factors %dx%d, %dx%d, %dx%d (SOF at byte %zu)", k[0].h, k[0].v, k[1].h,
                                  k[1].v, k[2].h, k[2].v, at);
            }
            h.hmax = h.comp[0].h; h.vmax = h.comp[0].v;
            h.mcux = (h.width + 8 * h.hmax - 1) / (8 * h.hmax);
            h.mcuy = (h.height + 8 * h.vmax - 1) / (8 * h.vmax);
            h.nblocks = 0;
            for (int c = 0; c < nf; ++c) {
                h.comp[c].bw = h.mcux * h.comp[c].h; h.comp[c].bh = h.mcuy * h.comp[c].v;
                h.comp[c].blk0 = h.nblocks;
                h.nblocks += h.comp[c].bw * h.comp[c].bh;
            }
            have_sof = true;
            break;
        }
        case 0xc2: return h.fail(RFD_ERR_UNSUPPORTED, "unsupported JPEG: progressive (SOF2 at byte %zu)", at);
        case 0xc3: return h.fail(RFD_ERR_UNSUPPORTED, "unsupported JPEG: lossless (SOF3 at byte %zu)", at);
        case 0xc5: case 0xc6: case 0xc7: return h.fail(RFD_ERR_UNSUPPORTED, "unsupported JPEG: hierarchical (SOF%d at byte %zu)", m - 0xc0, at);
        case 0xc9: case 0xca: case 0xcb: case 0xcd: case 0xce: case 0xcf: case 0xcc:
            return h.fail(RFD_ERR_UNSUPPORTED, "unsupported JPEG: arithmetic-coded (marker 0xFF%02X at byte %zu)", m, at);
        case 0xc8: return h.fail(RFD_ERR_INVALID_ARG, "reserved marker 0xFFC8 at byte %zu", at);
        case 0xdd: // DRI
            if (n != 2) return h.fail(RFD_ERR_INVALID_ARG, "DRI at byte %zu has length %zu, not 4", at, L);
            h.restart_interval = seg[0] << 8 | seg[1];
            break;
        case 0xda: { // SOS
            if (!have_sof) return h.fail(RFD_ERR_INVALID_ARG, "SOS at byte %zu, before any SOF marker", at);
            if (n < 1) return h.fail(RFD_ERR_INVALID_ARG, "SOS at byte %zu: the segment is too short", at);
            const int ns = seg[0];
            if (ns >= 1 && ns < h.ncomp) return h.fail(RFD_ERR_UNSUPPORTED, "unsupported JPEG: multi-scan (the scan at byte %zu holds %d of %d components)", at, ns, h.ncomp);
            if (ns != h.ncomp) return h.fail(RFD_ERR_INVALID_ARG, "SOS at byte %zu: %d components in the scan, %d in the frame", at, ns, h.ncomp);
            if (n != 4 + 2 * (size_t)ns) return h.fail(RFD_ERR_INVALID_ARG, "SOS at byte %zu: length %zu does not match %d components", at, L, ns);
            for (int c = 0; c < ns; ++c) {
                JpegComponent &k = h.comp[c];
                if (seg[1 + 2 * c] != k.id) return h.fail(RFD_ERR_INVALID_ARG, "SOS at byte %zu: scan component %d has id %d, the frame's has %d", at, c, seg[1 + 2 * c], k.id);
                k.td = seg[2 + 2 * c] >> 4; k.ta = seg[2 + 2 * c] & 15;
                if (k.td > 3 || k.ta > 3) return h.fail(RFD_ERR_INVALID_ARG, "SOS at byte %zu: Huffman table index out of range", at);
                if (!h.dc[k.td].present) return h.fail(RFD_ERR_INVALID_ARG, "missing table: component %d uses DC Huffman table %d, which no DHT defined (SOS at byte %zu)", c, k.td, at);
                if (!h.ac[k.ta].present) return h.fail(RFD_ERR_INVALID_ARG, "missing table: component %d uses AC Huffman table %d, which no DHT defined (SOS at byte %zu)", c, k.ta, at);
                if (!h.have_quant[k.tq]) return h.fail(RFD_ERR_INVALID_ARG, "missing table: component %d uses quantisation table %d, which no DQT defined (SOS at byte %zu)", c, k.tq, at);
            }
            h.scan = pos + L;
            return RFD_OK;
        }
        case 0xe1: // APP1: the first one that is Exif is asked for the orientation, whatever it answers
            if (!have_exif && n >= 6 && memcmp(seg, "Exif\0\0", 6) == 0) {
                have_exif = true;
                h.orientation = jpeg_exif_orientation(seg, n);
            }
            break;
        default: break; // every other APPn, COM and every other marker with a length: skipped
        }
        pos += L;
    }
}

// The entropy-coded bytes as a bit stream: 0xFF00 gives 0xFF, a marker (or the end of the data) stops the stream, which then
// delivers zeros that are counted, so that the decoder can tell real bits from made-up ones.
struct JpegBits {
    const uint8_t *d;
    size_t pos, end;
    uint64_t acc = 0;
    int n = 0, pad = 0; // bits in acc; how many of them, at the low end, are made up
    int marker = -1;    // the marker that stopped the stream (0: the data ended), -1 while it runs
    size_t marker_at = 0;

    void fill()
    {
        while (n <= 56) {
            unsigned b = 0;
            if (marker < 0) {
                if (pos >= end) { marker = 0; marker_at = end; }
                else if (d[pos] != 0xff) b = d[pos++];
                else {
                    size_t q = pos + 1;
                    while (q < end && d[q] == 0xff) ++q;
                    if (q >= end) { marker = 0; marker_at = end; }
                    else if (d[q] == 0) { b = 0xff; pos = q + 1; }
                    else { marker = d[q]; marker_at = q - 1; pos = q + 1; }
                }
            }
            if (marker >= 0) pad += 8;
            acc = acc << 8 | b;
            n += 8;
        }
    }
    unsigned peek(int k) const { return (unsigned)(acc >> (n - k)) & ((1u << k) - 1); }
    void skip(int k) { n -= k; }
    bool overrun() const { return n < pad; } // made-up bits have been consumed
};

inline int jpeg_huff_decode(JpegBits &br, const JpegHuff &t)
{
    const unsigned e = t.fast[br.peek(9)];
    if (e) { br.skip((int)(e >> 8)); return (int)(e & 255); }
    for (int l = 10; l <= 16; ++l) {
        const int32_t code = (int32_t)br.peek(l);
        if (code <= t.maxcode[l]) { br.skip(l); return t.vals[(t.valoff[l] + code) & 255]; }
    }
    return -1;
}

// s magnitude bits -> the signed value (1 <= s <= 15)
inline int jpeg_receive_extend(JpegBits &br, int s)
{
    const int r = (int)br.peek(s);
    br.skip(s);
    return r < (1 << (s - 1)) ? r - (1 << s) + 1 : r;
}

// ---- reduced-size decode (rfd.h, "JPEG decode, reduced size"): libjpeg's scale_num / scale_denom = 1 / s, s in {1, 2, 4, 8} ----
inline bool jpeg_scale_valid(int denom) { return denom == 1 || denom == 2 || denom == 4 || denom == 8; }
inline int jpeg_scaled_dim(int v, int denom) { return (v + denom - 1) / denom; }

// jdmaster.c: the inverse-DCT size of each component.  With m = 8 / s the minimum size, a component whose sampling factor leaves
// room takes a size doubled (up to 8) instead of being upsampled afterwards: 4:2:0 chroma gets 2 m in both directions.
inline void jpeg_idct_sizes(const JpegHeader &h, int denom, int n[3])
{
    const int m = 8 / denom;
    for (int c = 0; c < 3; ++c) {
        n[c] = m;
        if (c >= h.ncomp) continue;
        while (n[c] < 8 && (h.hmax * m) % (h.comp[c].h * n[c] * 2) == 0 && (h.vmax * m) % (h.comp[c].v * n[c] * 2) == 0) n[c] *= 2;
    }
}

// jidctred.c: does the n x n inverse DCT read the coefficient at natural index nat?  Per axis it reads the frequencies
// n = 8: 0..7    n = 4: 0 1 2 3 5 6 7    n = 2: 0 1 3 5 7    n = 1: 0
constexpr bool jpeg_idct_reads(int n, int nat)
{
    const unsigned axis = n == 8 ? 0xffu : n == 4 ? 0xefu : n == 2 ? 0xabu : 0x01u;
    return (axis >> (nat >> 3) & 1u) && (axis >> (nat & 7) & 1u);
}
// the same by zigzag position, one bit each: what the entropy decoder tests per non-zero coefficient
constexpr uint64_t jpeg_idct_read_mask(int n)
{
    uint64_t m = 0;
    for (int z = 0; z < 64; ++z)
        if (jpeg_idct_reads(n, kJpegNatural[z])) m |= (uint64_t)1 << z;
    return m;
}
constexpr uint64_t kJpegReadMask[4] = {jpeg_idct_read_mask(1), jpeg_idct_read_mask(2), jpeg_idct_read_mask(4), jpeg_idct_read_mask(8)};
static_assert(kJpegReadMask[3] == ~(uint64_t)0 && kJpegReadMask[0] == 1, "8 x 8 reads everything, 1 x 1 the DC alone");
inline uint64_t jpeg_read_mask_of(int n) { return kJpegReadMask[n == 8 ? 3 : n == 4 ? 2 : n == 2 ? 1 : 0]; }

// Decodes the scan of a parsed file.  rec: h.nblocks records; coef: room for 64 * h.nblocks values (never more are written);
// *used = the values written.  h.msg holds the cause of a failure.  idct_n: the inverse-DCT size per component of a reduced-size
// decode, which shortens the runs to what that size reads; null: full size.
inline int jpeg_decode_scan(const uint8_t *d, size_t len, JpegHeader &h, uint32_t *rec, int16_t *coef, uint32_t *used, const int *idct_n = nullptr)
{
    if ((uint64_t)h.nblocks * 64 > kJpegMaxCoefs) return h.fail(RFD_ERR_CAPACITY, "a JPEG frame of %d blocks exceeds the decoder's %u coefficient slots", h.nblocks, kJpegMaxCoefs);
    JpegBits br{d, h.scan, len};
    int pred[3] = {0, 0, 0};
    uint32_t off = 0;
    const int mcus = h.mcux * h.mcuy;
    int rst = 0, todo = h.restart_interval;
    for (int mcu = 0; mcu < mcus; ++mcu) {
        if (h.restart_interval && todo == 0) { // a restart marker stands between the intervals
            if (br.marker < 0) { // the stream has not run into it yet: the marker must be the next thing
                br.acc = 0; br.n = 0; br.pad = 0;
                br.fill();
                if (br.marker < 0 || br.pad < br.n)
                    return h.fail(RFD_ERR_INVALID_ARG, "expected RST%d at byte %zu (MCU %d), found entropy-coded data", rst & 7, br.pos, mcu);
            }
            if (br.marker == 0) return h.fail(RFD_ERR_INVALID_ARG, "truncated: the data ends at byte %zu, before MCU %d of %d", len, mcu, mcus);
            if (br.marker != 0xd0 + (rst & 7))
                return h.fail(RFD_ERR_INVALID_ARG, "RST out of sequence: expected RST%d, found marker 0xFF%02X at byte %zu (MCU %d)", rst & 7, br.marker, br.marker_at, mcu);
            br.acc = 0; br.n = 0; br.pad = 0; br.marker = -1;
            pred[0] = pred[1] = pred[2] = 0;
            ++rst;
            todo = h.restart_interval;
        }
        --todo;
        const int my = mcu / h.mcux, mx = mcu - my * h.mcux;
        for (int c = 0; c < h.ncomp; ++c) {
            const JpegComponent &k = h.comp[c];
            const JpegHuff &dc = h.dc[k.td], &ac = h.ac[k.ta];
            const uint64_t reads = jpeg_read_mask_of(idct_n ? idct_n[c] : 8);
            for (int v = 0; v < k.v; ++v)
                for (int u = 0; u < k.h; ++u) {
                    int16_t *out = coef + off;
                    int count = 0, keep = 0; // values written so far; how many of them travel (full size: all)
                    br.fill();
                    int s = jpeg_huff_decode(br, dc);
                    if (s < 0) return h.fail(RFD_ERR_INVALID_ARG, "a Huffman code not in DC table %d near byte %zu (MCU %d)", k.td, br.pos, mcu);
                    if (s) pred[c] = (int)((unsigned)pred[c] + (unsigned)jpeg_receive_extend(br, s));
                    out[0] = (int16_t)pred[c]; // wraps where a hostile file drives the predictor out of range, as libjpeg's store does
                    if (out[0]) count = keep = 1;
                    for (int i = 1; i < 64;) {
                        br.fill();
                        const int rs = jpeg_huff_decode(br, ac);
                        if (rs < 0) return h.fail(RFD_ERR_INVALID_ARG, "a Huffman code not in AC table %d near byte %zu (MCU %d)", k.ta, br.pos, mcu);
                        s = rs & 15;
                        const int r = rs >> 4;
                        if (s == 0) {
                            if (r != 15) break; // end of block
                            i += 16;
                            if (i > 64) return h.fail(RFD_ERR_INVALID_ARG, "a coefficient index above 63 (a zero run to %d) near byte %zu (MCU %d)", i - 1, br.pos, mcu);
                            continue;
                        }
                        i += r;
                        if (i > 63) return h.fail(RFD_ERR_INVALID_ARG, "a coefficient index above 63 (%d) near byte %zu (MCU %d)", i, br.pos, mcu);
                        for (int z = count ? count : 1; z < i; ++z) out[z] = 0;
                        out[i] = (int16_t)jpeg_receive_extend(br, s);
                        count = ++i;
                        if (reads >> (i - 1) & 1) keep = count;
                    }
                    if (br.overrun()) {
                        if (br.marker > 0) return h.fail(RFD_ERR_INVALID_ARG, "marker 0xFF%02X at byte %zu ends the entropy-coded data before MCU %d of %d is complete", br.marker, br.marker_at, mcu, mcus);
                        return h.fail(RFD_ERR_INVALID_ARG, "truncated: the data ends at byte %zu, before MCU %d of %d is complete", len, mcu, mcus);
                    }
                    const int blk = k.blk0 + (my * k.v + v) * k.bw + mx * k.h + u;
                    rec[blk] = off << kJpegRecCountBits | (uint32_t)keep;
                    off += (uint32_t)keep;
                }
        }
    }
    *used = off;
    return RFD_OK;
}

// the stored size of a w x h file in orientation o -> the size of the oriented frame: 5..8 transpose
inline void jpeg_oriented_size(int o, int w, int h, int *ow, int *oh)
{
    *ow = o >= 5 ? h : w;
    *oh = o >= 5 ? w : h;
}

// the same validation: rfd_jpeg_orientation
inline int jpeg_orientation(const uint8_t *d, size_t len, struct rfd_jpeg_orientation *out, char *msg, size_t msg_cap)
{
    std::unique_ptr<JpegHeader> h(new JpegHeader);
    const int st = jpeg_parse_header(d, len, *h);
    if (st != RFD_OK) {
        snprintf(msg, msg_cap, "%s", h->msg);
        return st;
    }
    if (out) {
        memset(out, 0, sizeof *out);
        out->orientation = h->orientation;
        jpeg_oriented_size(h->orientation, h->width, h->height, &out->width, &out->height);
        out->stored_width = h->width; out->stored_height = h->height;
    }
    return RFD_OK;
}

// the whole header validation, no device: rfd_jpeg_info
inline int jpeg_info(const uint8_t *d, size_t len, struct rfd_jpeg_info *out, char *msg, size_t msg_cap)
{
    std::unique_ptr<JpegHeader> h(new JpegHeader);
    const int st = jpeg_parse_header(d, len, *h);
    if (st != RFD_OK) {
        snprintf(msg, msg_cap, "%s", h->msg);
        return st;
    }
    if (out) {
        memset(out, 0, sizeof *out);
        out->width = h->width; out->height = h->height;
        out->components = h->ncomp;
        out->sampling = h->sampling;
        out->restart_interval = h->restart_interval;
    }
    return RFD_OK;
}

// the same validation: rfd_jpeg_scaled_size
inline int jpeg_scaled_size(const uint8_t *d, size_t len, int denom, int orientation_mode, struct rfd_jpeg_scaled_size *out, char *msg, size_t msg_cap)
{
    std::unique_ptr<JpegHeader> h(new JpegHeader);
    const int st = jpeg_parse_header(d, len, *h);
    if (st != RFD_OK) {
        snprintf(msg, msg_cap, "%s", h->msg);
        return st;
    }
    if (out) {
        memset(out, 0, sizeof *out);
        out->denom = denom;
        out->orientation = orientation_mode == RFD_JPEG_ORIENTATION_APPLY ? h->orientation : 1;
        jpeg_oriented_size(out->orientation, jpeg_scaled_dim(h->width, denom), jpeg_scaled_dim(h->height, denom), &out->width, &out->height);
        out->stored_width = h->width; out->stored_height = h->height;
    }
    return RFD_OK;
}

// records + quantised zigzag runs of a decoded scan -> out [nblocks][64]: dequantised (saturating to i16), natural order
inline void jpeg_dequantise_natural(const JpegHeader &h, const uint32_t *rec, const int16_t *coef, int16_t *out)
{
    memset(out, 0, (size_t)h.nblocks * 64 * sizeof(int16_t));
    for (int c = 0; c < h.ncomp; ++c) {
        const JpegComponent &k = h.comp[c];
        const uint16_t *q = h.quant[k.tq];
        for (int b = k.blk0; b < k.blk0 + k.bw * k.bh; ++b) {
            const int16_t *src = coef + (rec[(size_t)b] >> kJpegRecCountBits);
            const int count = (int)(rec[(size_t)b] & ((1u << kJpegRecCountBits) - 1));
            for (int z = 0; z < count; ++z) {
                const int v = (int)src[z] * (int)q[z];
                out[(size_t)b * 64 + kJpegNatural[z]] = (int16_t)(v < -32768 ? -32768 : v > 32767 ? 32767 : v);
            }
        }
    }
}

// rfd_debug_jpeg_coefficients: parse, decode, dequantise, zigzag -> natural order.  rfd_debug_jpeg_block_counts (count_out): the
// same walk at a denominator, reporting each record's count instead
inline int jpeg_debug_coefficients(const uint8_t *d, size_t len, int16_t *out, size_t cap_blocks, size_t *blocks, char *msg, size_t msg_cap, int denom = 1,
                                   uint8_t *count_out = nullptr)
{
    std::unique_ptr<JpegHeader> h(new JpegHeader);
    int st = jpeg_parse_header(d, len, *h);
    std::vector<uint32_t> rec;
    std::vector<int16_t> coef;
    uint32_t used = 0;
    if (st == RFD_OK) {
        if (blocks) *blocks = (size_t)h->nblocks;
        if ((uint64_t)h->nblocks * 64 > kJpegMaxCoefs) st = h->fail(RFD_ERR_CAPACITY, "a JPEG frame of %d blocks exceeds the decoder's %u coefficient slots", h->nblocks, kJpegMaxCoefs);
        else if ((size_t)h->nblocks > cap_blocks) st = h->fail(RFD_ERR_CAPACITY, "the file has %d blocks, the output holds %zu", h->nblocks, cap_blocks);
    }
    if (st == RFD_OK) {
        rec.resize((size_t)h->nblocks);
        coef.resize((size_t)h->nblocks * 64);
        int n[3];
        jpeg_idct_sizes(*h, denom, n);
        st = jpeg_decode_scan(d, len, *h, rec.data(), coef.data(), &used, denom == 1 ? nullptr : n);
    }
    if (st != RFD_OK) {
        snprintf(msg, msg_cap, "%s", h->msg);
        return st;
    }
    if (count_out)
        for (int b = 0; b < h->nblocks; ++b) count_out[b] = (uint8_t)(rec[(size_t)b] & ((1u << kJpegRecCountBits) - 1));
    else
        jpeg_dequantise_natural(*h, rec.data(), coef.data(), out);
    return RFD_OK;
}

} // namespace rfd
#endif
