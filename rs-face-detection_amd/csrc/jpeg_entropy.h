// jpeg_entropy.h -- entropy decoding of restart-interval JPEG files one interval at a time (include/rfd.h, "JPEG decode",
// RFD_JPEG_ENTROPY_DEVICE).  A file with a restart interval (DRI) of R MCUs is cut into pieces that decode independently: after
// every R MCUs the bit stream is byte-aligned, a RSTn marker follows and every DC predictor is zero again.  Three parts:
//   jpeg_prescan            host: finds the intervals of a scan by its markers alone, no Huffman decoding
//   jpeg_device_eligible    host: the rule that decides whether a file takes the interval path at all
//   jpeg_decode_interval    host AND device: ONE inline function that decodes one interval into the dense record layout.
//                           csrc/kernels_jpeg_entropy.hip runs it with one thread per interval; tests/cpp/jpeg_entropy_check.cpp
//                           runs the very same function under the host sanitizers.
// Nothing here allocates, locks or touches shared state.
//
// The interval decoder is STRICT where jpeg_decode_scan (jpeg_parse.h) is lenient: it refuses an interval unless, after its last
// MCU, fewer than 8 bits and no byte of the interval are unread (a stuffed 0xFF00 counts as the two bytes it occupies).  Garbage
// in front of a marker is the host decoder's to judge; a refused frame is simply decoded there.  On what it accepts, the
// coefficients equal jpeg_decode_scan's.  It also refuses a code that is in no table, a coefficient index above 63, a zero run
// past 64 and the use of a bit past the interval's end.  It never reads a byte at or beyond `end`, never writes outside the
// blocks of its own MCUs, and every loop is bounded by the interval's bytes, its MCU count or 64.
//
// Dense record layout (what the device writes): block b's values start at coef[b * 64], rec[b] = (b * 64) << 7 | count.
#ifndef RFD_JPEG_ENTROPY_H
#define RFD_JPEG_ENTROPY_H
#include <cstddef>

#include "jpeg_parse.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define RFD_HD __host__ __device__ __forceinline__
#else
#define RFD_HD inline
#endif

namespace rfd {

constexpr int kJpegDeviceMaxInterval = 128; // MCUs: the longest interval one device thread is given

// what the interval decoder needs of a JpegHuff, in the layout the kernel stages in LDS (a whole number of 32-bit words)
struct JpegDevHuff {
    uint16_t fast[512];
    int32_t maxcode[17];
    int32_t valoff[17];
    uint8_t vals[256];
};
static_assert(sizeof(JpegDevHuff) % 4 == 0, "staged word by word");

// the geometry the block index of (mcu, component, v, u) needs: jpeg_decode_scan's expression
struct JpegScanGeom {
    int ncomp, mcux, mcus, restart;
    int h[3], v[3], bw[3], blk0[3];
};

// ---------------------------------------------------------------- the shared interval decoder
struct JpegIntervalBits {
    const uint8_t *d;
    uint32_t pos, end;
    uint64_t acc;
    int n, pad; // bits in acc; how many of them, at the low end, are made up
    int bad;    // a marker inside the interval: the pre-scan never hands one out
};

RFD_HD void jpeg_interval_fill(JpegIntervalBits &b)
{
    while (b.n <= 56) {
        unsigned v = 0;
        if (b.pos < b.end) {
            v = b.d[b.pos++];
            if (v == 0xff) { // fill 0xFFs, then 0x00: one data byte 0xFF
                uint32_t q = b.pos;
                while (q < b.end && b.d[q] == 0xff) ++q;
                if (q < b.end && b.d[q] == 0) b.pos = q + 1;
                else { b.bad = 1; b.pos = b.end; v = 0; b.pad += 8; }
            }
        } else
            b.pad += 8;
        b.acc = b.acc << 8 | v;
        b.n += 8;
    }
}

RFD_HD unsigned jpeg_interval_peek(const JpegIntervalBits &b, int k) { return (unsigned)(b.acc >> (b.n - k)) & ((1u << k) - 1); }

// -1: the next bits are a code of no symbol
RFD_HD int jpeg_interval_huff(JpegIntervalBits &b, const JpegDevHuff *t)
{
    const unsigned e = t->fast[jpeg_interval_peek(b, 9)];
    if (e) { b.n -= (int)(e >> 8); return (int)(e & 255); }
    // a rolled loop: unrolled, the device compiler fetches maxcode[10 .. 16] as one 128-bit LDS read under a divergent branch
#pragma GCC unroll 1
    for (int l = 10; l <= 16; ++l) {
        const int32_t code = (int32_t)jpeg_interval_peek(b, l);
        if (code <= t->maxcode[l]) { b.n -= l; return t->vals[(t->valoff[l] + code) & 255]; }
    }
    return -1;
}

RFD_HD int jpeg_interval_extend(JpegIntervalBits &b, int s)
{
    const int r = (int)jpeg_interval_peek(b, s);
    b.n -= s;
    return r < (1 << (s - 1)) ? r - (1 << s) + 1 : r;
}

// one block: DC difference, AC run/size pairs -> out[0 .. count), *count; false: refused
RFD_HD bool jpeg_interval_block(JpegIntervalBits &b, const JpegDevHuff *dc, const JpegDevHuff *ac, int &pred, int16_t *out, int *count_out)
{
    int count = 0;
    jpeg_interval_fill(b);
    int s = jpeg_interval_huff(b, dc);
    if (s < 0 || s > 15) return false;
    if (s) pred = (int)((unsigned)pred + (unsigned)jpeg_interval_extend(b, s));
    out[0] = (int16_t)pred; // wraps as jpeg_decode_scan's store does
    if (out[0]) count = 1;
    for (int i = 1; i < 64;) {
        jpeg_interval_fill(b);
        const int rs = jpeg_interval_huff(b, ac);
        if (rs < 0) return false;
        s = rs & 15;
        const int r = rs >> 4;
        if (s == 0) {
            if (r != 15) break; // end of block
            i += 16;
            if (i > 64) return false; // a zero run past 64
            continue;
        }
        i += r;
        if (i > 63) return false; // a coefficient index above 63
        for (int z = count ? count : 1; z < i; ++z) out[z] = 0;
        out[i] = (int16_t)jpeg_interval_extend(b, s);
        count = ++i;
    }
    if (b.n < b.pad) return false; // a made-up bit was consumed
    *count_out = count;
    return true;
}

// the blocks of component C in MCU (mx, my)
RFD_HD bool jpeg_interval_component(JpegIntervalBits &b, int ch, int cv, int bw, int blk0, const JpegDevHuff *dc, const JpegDevHuff *ac, int &pred, int mx,
                                    int my, uint32_t *rec, int16_t *coef)
{
    for (int v = 0; v < cv; ++v)
        for (int u = 0; u < ch; ++u) {
            const int blk = blk0 + (my * cv + v) * bw + mx * ch + u;
            int count = 0;
            if (!jpeg_interval_block(b, dc, ac, pred, coef + (size_t)blk * 64, &count)) return false;
            rec[blk] = ((uint32_t)blk * 64u) << kJpegRecCountBits | (uint32_t)count;
        }
    return true;
}

// Decodes MCUs [mcu0, mcu1) of a frame from bytes [begin, end) of d.  dc / ac: one table per component.  rec / coef: the
// frame's records and coefficient slots (64 per block).  false: refused (some blocks of the interval may have been written).
RFD_HD bool jpeg_decode_interval(const uint8_t *d, uint32_t begin, uint32_t end, int mcu0, int mcu1, const JpegScanGeom &g, const JpegDevHuff *dc,
                                 const JpegDevHuff *ac, uint32_t *rec, int16_t *coef)
{
    JpegIntervalBits b;
    b.d = d; b.pos = begin; b.end = end < begin ? begin : end;
    b.acc = 0; b.n = 0; b.pad = 0; b.bad = 0;
    int pred0 = 0, pred1 = 0, pred2 = 0; // named, not an array: no runtime-indexed private memory on the device
    for (int mcu = mcu0; mcu < mcu1; ++mcu) {
        const int my = mcu / g.mcux, mx = mcu - my * g.mcux;
        if (!jpeg_interval_component(b, g.h[0], g.v[0], g.bw[0], g.blk0[0], dc + 0, ac + 0, pred0, mx, my, rec, coef)) return false;
        if (g.ncomp == 3) {
            if (!jpeg_interval_component(b, g.h[1], g.v[1], g.bw[1], g.blk0[1], dc + 1, ac + 1, pred1, mx, my, rec, coef)) return false;
            if (!jpeg_interval_component(b, g.h[2], g.v[2], g.bw[2], g.blk0[2], dc + 2, ac + 2, pred2, mx, my, rec, coef)) return false;
        }
    }
    // strict: the consumed length is exactly the interval -- every byte taken in, fewer than 8 real bits unread
    return !b.bad && b.pos == b.end && b.n >= b.pad && b.n - b.pad < 8;
}

// ---------------------------------------------------------------- host side: tables, pre-scan, eligibility
inline void jpeg_dev_huff(const JpegHuff &t, JpegDevHuff &o)
{
    memcpy(o.fast, t.fast, sizeof o.fast);
    memcpy(o.maxcode, t.maxcode, sizeof o.maxcode);
    memcpy(o.valoff, t.valoff, sizeof o.valoff);
    memcpy(o.vals, t.vals, sizeof o.vals);
}

inline void jpeg_scan_geom(const JpegHeader &h, JpegScanGeom &g, JpegDevHuff *dc, JpegDevHuff *ac)
{
    memset(&g, 0, sizeof g);
    g.ncomp = h.ncomp; g.mcux = h.mcux; g.mcus = h.mcux * h.mcuy; g.restart = h.restart_interval;
    for (int c = 0; c < h.ncomp; ++c) {
        g.h[c] = h.comp[c].h; g.v[c] = h.comp[c].v; g.bw[c] = h.comp[c].bw; g.blk0[c] = h.comp[c].blk0;
        jpeg_dev_huff(h.dc[h.comp[c].td], dc[c]);
        jpeg_dev_huff(h.ac[h.comp[c].ta], ac[c]);
    }
}

// The marker pre-scan over the entropy-coded bytes d[scan .. len).  At each 0xFF it skips fill 0xFFs and looks at the next
// byte: 0x00 is a stuffed byte (data), 0xD0..0xD7 a restart marker, anything else -- or the end of the data -- ends the scan.
// Interval k is [begin[k], end[k]): end is the first 0xFF of the marker sequence that closes it.  Writes at most cap
// intervals, returns how many there are; *in_sequence: the markers came as RST0, RST1, .. RST7, RST0, ..
inline size_t jpeg_prescan(const uint8_t *d, size_t len, size_t scan, uint32_t *begin, uint32_t *end, size_t cap, bool *in_sequence)
{
    size_t k = 0, pos = scan, first = scan;
    bool seq = true;
    for (;;) {
        const uint8_t *ff = pos < len ? (const uint8_t *)memchr(d + pos, 0xff, len - pos) : nullptr;
        const size_t at = ff ? (size_t)(ff - d) : len;
        size_t q = at + 1;
        while (q < len && d[q] == 0xff) ++q;
        if (ff && q < len && d[q] == 0) { pos = q + 1; continue; }
        if (k < cap) { begin[k] = (uint32_t)first; end[k] = (uint32_t)at; }
        ++k;
        if (!ff || q >= len || d[q] < 0xd0 || d[q] > 0xd7) break;
        if (d[q] != 0xd0 + ((k - 1) & 7)) seq = false;
        pos = first = q + 1;
    }
    *in_sequence = seq;
    return k;
}

// Whether a parsed file takes the interval path, by its structure alone; fills the interval table when it does (cap >= the
// expected count).  *count = the intervals the file must have, ceil(mcus / R), 0 without a restart interval.  false: msg says why.
inline bool jpeg_device_eligible(const uint8_t *d, size_t len, const JpegHeader &h, uint32_t *begin, uint32_t *end, size_t cap, size_t *count, char *msg,
                                 size_t msg_cap)
{
    const int R = h.restart_interval, mcus = h.mcux * h.mcuy;
    *count = 0;
    if (R < 1) { snprintf(msg, msg_cap, "not eligible for device entropy decoding: the file has no restart interval (no DRI marker)"); return false; }
    if (R > kJpegDeviceMaxInterval) {
        snprintf(msg, msg_cap, "not eligible for device entropy decoding: a restart interval of %d MCUs exceeds the limit of %d", R, kJpegDeviceMaxInterval);
        return false;
    }
    if (len > 0xffffffffu) { snprintf(msg, msg_cap, "not eligible for device entropy decoding: a file of %zu bytes", len); return false; }
    const size_t want = ((size_t)mcus + (size_t)R - 1) / (size_t)R;
    *count = want;
    if (want > cap) return true; // the caller sizes the table and asks again
    bool seq = true;
    const size_t found = jpeg_prescan(d, len, h.scan, begin, end, cap, &seq);
    if (found != want) {
        snprintf(msg, msg_cap, "not eligible for device entropy decoding: the scan at byte %zu holds %zu intervals, %d MCUs at %d per interval need %zu", h.scan, found,
                 mcus, R, want);
        return false;
    }
    if (!seq) { snprintf(msg, msg_cap, "not eligible for device entropy decoding: a restart marker out of sequence in the scan at byte %zu", h.scan); return false; }
    return true;
}

} // namespace rfd
#endif
