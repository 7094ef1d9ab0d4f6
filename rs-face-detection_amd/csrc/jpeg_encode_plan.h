// jpeg_encode_plan.h -- the host half of a JPEG encode call (include/rfd.h, "JPEG encode"): the checks that can refuse a call, the
// geometry of a file, quality -> quantisation tables and their reciprocals, the Huffman code tables, the header bytes, the size
// bound, the descriptor the kernels read for each image and the workspace a call needs.  Plain code with nothing of HIP in it:
// tests/cpp/jpeg_encode_plan_check.cpp builds it with the host compiler alone, jpeg_encode_host.hip runs it before anything is
// enqueued, kernels_jpeg_encode.hip reads the tables and descriptors it fills.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/rfd.h"

namespace rfd {

constexpr int kEncGroup = 256;           // threads of every workgroup of the three kernels
constexpr int kEncBlocksPerGroup = 32;   // block kernel: 8 threads per 8 x 8 block
constexpr int kEncChunk = 256;           // entropy kernel: blocks a workgroup packs at a time, one per thread
constexpr int kEncMaxBlockBits = 22 + 63 * 26; // DC: a code of at most 11 bits (chrominance; 9 for luminance) + 11 bits; each AC: 16-bit code + 10 bits (and no EOB then)
constexpr int kEncHeaderMax = 640;       // SOI .. SOS of a colour file with DRI is 629 bytes
constexpr int kEncMaxSide = 65535;       // what SOF0 can say

// ITU-T T.81 Annex K.1, natural (row-major) order
constexpr uint8_t kEncBaseQuant[2][64] = {
    {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};

// natural index of zigzag position k
constexpr uint8_t kEncNatural[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
                                     35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// Annex K.3: code lengths 1 .. 16 and symbols of the typical tables; [0] luminance, [1] chrominance
constexpr uint8_t kEncDcBits[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
constexpr uint8_t kEncAcBits[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119}};
constexpr uint8_t kEncAcVals[2][162] = {
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1,
     0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26,
     0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56,
     0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85,
     0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa,
     0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6,
     0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
     0xfa},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42,
     0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19,
     0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55,
     0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83,
     0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8,
     0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4,
     0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
     0xfa}};

inline void jpeg_encode_config_default(rfd_jpeg_encode_config *c)
{
    memset(c, 0, sizeof *c);
    c->quality = 90;
    c->sampling = RFD_JPEG_420;
    c->restart_rows = 1;
}

// "" when the config is in range, else the field and its bound
inline bool jpeg_encode_check_config(const rfd_jpeg_encode_config &c, char *msg, size_t cap)
{
    if (c.quality < 1 || c.quality > 100) { snprintf(msg, cap, "quality %d is outside 1 .. 100", (int)c.quality); return false; }
    if (c.sampling < RFD_JPEG_GRAY || c.sampling > RFD_JPEG_420) { snprintf(msg, cap, "sampling %d is no rfd_jpeg_sampling", (int)c.sampling); return false; }
    if (c.restart_rows < 0) { snprintf(msg, cap, "restart_rows %d is negative", (int)c.restart_rows); return false; }
    for (int k = 0; k < 5; ++k)
        if (c.reserved[k] != 0) { snprintf(msg, cap, "reserved is not zero"); return false; }
    return true;
}

// libjpeg's jpeg_set_quality with force_baseline: table t (0 luminance, 1 chrominance), natural order
inline void jpeg_encode_quant(int quality, uint8_t table[2][64])
{
    const int q = quality < 1 ? 1 : quality > 100 ? 100 : quality;
    const int scale = q < 50 ? 5000 / q : 200 - 2 * q;
    for (int t = 0; t < 2; ++t)
        for (int k = 0; k < 64; ++k) {
            const int v = (kEncBaseQuant[t][k] * scale + 50) / 100;
            table[t][k] = (uint8_t)(v < 1 ? 1 : v > 255 ? 255 : v);
        }
}

// The division by a divisor d = 8 * table entry (8 .. 2040) as a multiplication: for every n below 2^16 (the kernel's
// n = |c| + d / 2 with |c| < 2^15), n / d == (n * jpeg_encode_recip(d)) >> 32.  With m = floor(2^32 / d) + 1 the product
// overshoots n * 2^32 / d by n * (m d - 2^32) / d < n, which cannot reach the next multiple as long as n d < 2^32.
// tests/cpp/jpeg_encode_plan_check.cpp tries every pair.
inline uint32_t jpeg_encode_recip(uint32_t d) { return (uint32_t)((uint64_t(1) << 32) / d) + 1u; }
inline uint32_t jpeg_encode_divide(uint32_t n, uint32_t recip) { return (uint32_t)(((uint64_t)n * recip) >> 32); }

// What all images of a call share, read by the kernels from device memory.
struct EncTables {
    uint32_t recip[2][64]; // jpeg_encode_recip of 8 * table, natural order
    uint32_t half[2][64];  // 8 * table / 2
    uint32_t ac[2][256];   // by symbol run << 4 | size: code << 8 | length (0: the table has no such symbol)
    uint32_t dc[2][12];    // by category, likewise
    int32_t header_len;    // bytes of `header`: SOI .. SOS
    int32_t size_at;       // where SOF0's height (2 bytes) and width (2 bytes) lie in it
    int32_t dri_at;        // where DRI's interval (2 bytes) lies in it, 0 without DRI
    int32_t pad;
    uint8_t header[kEncHeaderMax]; // written for a 1 x 1 image with interval 1: the kernel puts each image's own values in
};

inline void jpeg_encode_codes(const uint8_t bits[16], const uint8_t *vals, uint32_t *by_symbol)
{
    uint32_t code = 0;
    int k = 0;
    for (int len = 1; len <= 16; ++len) {
        for (int i = 0; i < bits[len - 1]; ++i) by_symbol[vals[k++]] = code++ << 8 | (uint32_t)len;
        code <<= 1;
    }
}

struct EncSampling {
    int ncomp, h, v; // luma factors; chroma is 1 x 1
};
inline EncSampling jpeg_encode_sampling(int sampling)
{
    switch (sampling) {
    case RFD_JPEG_GRAY: return {1, 1, 1};
    case RFD_JPEG_444: return {3, 1, 1};
    case RFD_JPEG_422: return {3, 2, 1};
    default: return {3, 2, 2};
    }
}

// SOI, APP0 (JFIF 1.01, no units, 1 x 1, no thumbnail), DQT 0 [1], SOF0, DHT DC0 AC0 [DC1 AC1], [DRI], SOS: libjpeg's order.
// `interval`: MCUs per restart interval, 0 = no DRI.  Returns the length; out has kEncHeaderMax bytes.  size_at / dri_at may be null.
inline int jpeg_encode_header(int width, int height, int quality, int sampling, int interval, uint8_t *out, int32_t *size_at, int32_t *dri_at)
{
    const EncSampling s = jpeg_encode_sampling(sampling);
    const int tabs = s.ncomp == 1 ? 1 : 2;
    uint8_t quant[2][64];
    jpeg_encode_quant(quality, quant);
    int n = 0;
    auto put = [&](int b) { out[n++] = (uint8_t)b; };
    auto put16 = [&](int v) { put(v >> 8); put(v & 255); };
    put(0xFF); put(0xD8);
    put(0xFF); put(0xE0); put16(16);
    for (int k = 0; k < 5; ++k) put("JFIF"[k]); // with its terminator
    put(1); put(1); put(0); put16(1); put16(1); put(0); put(0);
    for (int t = 0; t < tabs; ++t) {
        put(0xFF); put(0xDB); put16(67); put(t);
        for (int k = 0; k < 64; ++k) put(quant[t][kEncNatural[k]]);
    }
    put(0xFF); put(0xC0); put16(8 + 3 * s.ncomp); put(8);
    if (size_at) *size_at = n;
    put16(height); put16(width); put(s.ncomp);
    for (int c = 0; c < s.ncomp; ++c) { put(c + 1); put(c == 0 ? s.h << 4 | s.v : 0x11); put(c == 0 ? 0 : 1); }
    for (int t = 0; t < tabs; ++t) {
        put(0xFF); put(0xC4); put16(2 + 1 + 16 + 12); put(t);
        for (int k = 0; k < 16; ++k) put(kEncDcBits[t][k]);
        for (int k = 0; k < 12; ++k) put(k);
        put(0xFF); put(0xC4); put16(2 + 1 + 16 + 162); put(0x10 | t);
        for (int k = 0; k < 16; ++k) put(kEncAcBits[t][k]);
        for (int k = 0; k < 162; ++k) put(kEncAcVals[t][k]);
    }
    if (dri_at) *dri_at = 0;
    if (interval > 0) {
        put(0xFF); put(0xDD); put16(4);
        if (dri_at) *dri_at = n;
        put16(interval);
    }
    put(0xFF); put(0xDA); put16(6 + 2 * s.ncomp); put(s.ncomp);
    for (int c = 0; c < s.ncomp; ++c) { put(c + 1); put(c == 0 ? 0x00 : 0x11); }
    put(0); put(63); put(0);
    return n;
}

inline void jpeg_encode_tables(const rfd_jpeg_encode_config &cfg, EncTables *t)
{
    memset(t, 0, sizeof *t);
    uint8_t quant[2][64];
    jpeg_encode_quant(cfg.quality, quant);
    static const uint8_t dc_vals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
    for (int k = 0; k < 2; ++k) {
        for (int i = 0; i < 64; ++i) {
            t->recip[k][i] = jpeg_encode_recip(8u * quant[k][i]);
            t->half[k][i] = 4u * quant[k][i];
        }
        jpeg_encode_codes(kEncAcBits[k], kEncAcVals[k], t->ac[k]);
        jpeg_encode_codes(kEncDcBits[k], dc_vals, t->dc[k]);
    }
    t->header_len = jpeg_encode_header(1, 1, cfg.quality, cfg.sampling, cfg.restart_rows > 0 ? 1 : 0, t->header, &t->size_at, &t->dri_at);
}

// What the kernels read for image i.  Blocks lie component-major, each component's plane padded to whole MCUs and walked row by
// row (the order of rfd_debug_jpeg_coefficients); [c] is the component, luminance first.
struct EncImage {
    const uint8_t *src;
    long long stride;
    uint8_t *out;         // the image's slot
    int32_t width, height;
    int32_t bw[3], bh[3]; // blocks per row / column of the padded plane
    int32_t wb[3], hb[3]; // of them real: ceil(cw / 8), ceil(ch / 8)
    int32_t ch[3];        // the component's rows, ceil(height * v / vmax): downsampled rows at and past it repeat row ch - 1
    int32_t comp0[3];     // the component's first block within the image
    int32_t blocks;       // of the image
    int32_t mcux, mcus;   // MCUs per row, and all of them
    int32_t interval;     // MCUs per restart interval; mcus where the file has no markers
    int32_t intervals;    // ceil(mcus / interval)
    int32_t dri;          // what the DRI segment says: interval, or 0 without markers
    int32_t block0;       // the image's first block among the call's
    int32_t interval0;    // its first interval among the call's
    int32_t group0;       // its first workgroup of the block kernel; ascends strictly over a call
};

struct EncPlan {
    int64_t blocks, intervals; // of the call
    int32_t groups;            // workgroups of the block kernel
    size_t coef_bytes;         // blocks * 64 i16
    size_t interval_bytes;     // intervals * (length u32 + offset u32)
    size_t src_bytes, max_bound; // host form: the frames with tight rows, each start rounded up to 16; the largest bound of an image
};

// false: a side outside 1 .. 65535, or restart_rows MCU rows are more than 65535 MCUs; the cause is in msg.  d->src / stride / out
// and the three *0 members stay as they are.
inline bool jpeg_encode_geometry(int width, int height, const rfd_jpeg_encode_config &cfg, EncImage *d, char *msg, size_t cap)
{
    if (width < 1 || width > kEncMaxSide) { snprintf(msg, cap, "width %d is outside 1 .. 65535", width); return false; }
    if (height < 1 || height > kEncMaxSide) { snprintf(msg, cap, "height %d is outside 1 .. 65535", height); return false; }
    const EncSampling s = jpeg_encode_sampling(cfg.sampling);
    const int mcux = (width + 8 * s.h - 1) / (8 * s.h), mcuy = (height + 8 * s.v - 1) / (8 * s.v);
    if ((int64_t)cfg.restart_rows * mcux > 65535) {
        snprintf(msg, cap, "restart_rows %d of %d MCUs each is an interval above 65535 MCUs", (int)cfg.restart_rows, mcux);
        return false;
    }
    d->width = width; d->height = height;
    int32_t at = 0;
    for (int c = 0; c < 3; ++c) {
        if (c >= s.ncomp) { d->bw[c] = d->bh[c] = d->wb[c] = d->hb[c] = d->ch[c] = 0; d->comp0[c] = at; continue; }
        const int h = c == 0 ? s.h : 1, v = c == 0 ? s.v : 1;
        const int cw = (width * h + s.h - 1) / s.h, chh = (height * v + s.v - 1) / s.v;
        d->bw[c] = mcux * h; d->bh[c] = mcuy * v;
        d->wb[c] = (cw + 7) / 8; d->hb[c] = (chh + 7) / 8;
        d->ch[c] = chh;
        d->comp0[c] = at;
        at += d->bw[c] * d->bh[c]; // at most 3 * 8192 * 8192 in all, below 2^31
    }
    d->blocks = at;
    d->mcux = mcux; d->mcus = mcux * mcuy;
    d->dri = cfg.restart_rows * mcux;
    d->interval = d->dri > 0 ? d->dri : d->mcus;
    d->intervals = (d->mcus + d->interval - 1) / d->interval;
    return true;
}

// A size no file of this geometry can exceed: the header, and for every restart interval its blocks at kEncMaxBlockBits bits each
// (the code-length limit of the tables: a DC symbol of 11 + 11 bits, 63 AC symbols of 16 + 10 bits), padded to a byte, every byte
// of it stuffed, then the two bytes of RSTn or EOI.
inline size_t jpeg_encode_bound_of(const EncImage &d, int header_len)
{
    const int64_t per_mcu = d.blocks / d.mcus; // whole MCUs only
    auto interval_bytes = [&](int64_t mcus) { return (size_t)(2 * ((mcus * per_mcu * kEncMaxBlockBits + 7) / 8) + 2); };
    const int64_t full = d.mcus / d.interval, rest = d.mcus % d.interval;
    return (size_t)header_len + (size_t)full * interval_bytes(d.interval) + (rest ? interval_bytes(rest) : 0);
}

inline size_t jpeg_encode_round16(size_t v) { return (v + 15) & ~(size_t)15; }

// The checks of one call and its plan.  RFD_OK: desc[0 .. n) and *plan are filled, src / stride as the caller gave them and out =
// slots + i * slot_bytes.  Otherwise the status, the image and the cause in msg, and nothing may be enqueued.  n >= 1.
inline int jpeg_encode_plan(const rfd_image *imgs, int n, const rfd_jpeg_encode_config &cfg, uint8_t *slots, size_t slot_bytes, int header_len, EncImage *desc, EncPlan *plan,
                            char *msg, size_t cap)
{
    if (!jpeg_encode_check_config(cfg, msg, cap)) return RFD_ERR_INVALID_ARG;
    EncPlan p;
    memset(&p, 0, sizeof p);
    int64_t groups = 0;
    for (int i = 0; i < n; ++i) {
        char what[160];
        EncImage &d = desc[i];
        memset(&d, 0, sizeof d);
        if (!imgs[i].data) { snprintf(msg, cap, "image %d: data is null", i); return RFD_ERR_INVALID_ARG; }
        if (!jpeg_encode_geometry(imgs[i].width, imgs[i].height, cfg, &d, what, sizeof what)) { snprintf(msg, cap, "image %d: %s", i, what); return RFD_ERR_INVALID_ARG; }
        if (imgs[i].stride < (ptrdiff_t)imgs[i].width * 3) { snprintf(msg, cap, "image %d: stride %lld < 3 * width", i, (long long)imgs[i].stride); return RFD_ERR_INVALID_ARG; }
        d.src = imgs[i].data;
        d.stride = (long long)imgs[i].stride;
        d.out = slots + (size_t)i * slot_bytes;
        d.block0 = (int32_t)p.blocks;
        d.interval0 = (int32_t)p.intervals;
        d.group0 = (int32_t)groups;
        p.blocks += d.blocks;
        p.intervals += d.intervals;
        groups += (d.blocks + kEncBlocksPerGroup - 1) / kEncBlocksPerGroup;
        if (p.blocks > INT32_MAX / 2 || p.intervals > INT32_MAX / 2) { // the kernels number a call's blocks and intervals in int
            snprintf(msg, cap, "image %d: the call exceeds 2^30 blocks or restart intervals", i);
            return RFD_ERR_CAPACITY;
        }
        p.src_bytes = jpeg_encode_round16(p.src_bytes) + (size_t)d.width * 3 * (size_t)d.height;
        const size_t bound = jpeg_encode_bound_of(d, header_len);
        if (bound > p.max_bound) p.max_bound = bound;
    }
    p.groups = (int32_t)groups;
    p.coef_bytes = (size_t)p.blocks * 64 * sizeof(int16_t);
    p.interval_bytes = (size_t)p.intervals * 2 * sizeof(uint32_t);
    *plan = p;
    return RFD_OK;
}

} // namespace rfd
