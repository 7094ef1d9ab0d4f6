// jpeg_plan.h -- what a JPEG decode call (include/rfd.h, "JPEG decode") decides on the host before anything is enqueued: where the
// regions of the two stagings lie, what each frame of the call is and where its blocks go, and the descriptor tables the kernels
// read.  Plain host C++ over jpeg_parse.h, jpeg_entropy.h and jpeg_desc.h: no HIP, no context, no allocation beyond std::vector.
// jpeg_host.hip does what is planned here; tests/cpp/jpeg_plan_check.cpp runs the planning alone under the host sanitizers.
#pragma once
#include <algorithm>

#include "jpeg_desc.h"
#include "jpeg_entropy.h"
#include "jpeg_parse.h"

namespace rfd {

inline int jpeg_div_up(int a, int b) { return (a + b - 1) / b; }
inline size_t jpeg_align16(size_t v) { return (v + 15) & ~(size_t)15; }
template <class T> inline T *jpeg_at(void *base, size_t off) { return (T *)((char *)base + off); }

// blocks of a w x h frame in the sampling that needs most: 4:4:4, 4:2:2 or 4:2:0, each padded to its own MCU
inline size_t jpeg_blocks_bound(int w, int h)
{
    const size_t a8 = (size_t)jpeg_div_up(w, 8), b8 = (size_t)jpeg_div_up(h, 8), a16 = (size_t)jpeg_div_up(w, 16), b16 = (size_t)jpeg_div_up(h, 16);
    return std::max(3 * a8 * b8, std::max(4 * a16 * b8, 6 * a16 * b16));
}

// The page-locked staging of a decoder and its device twin, B = max_batch frames of at most blocks_max blocks each:
//   JpegFrame [B] | block records u32 [B * blocks_max] | coefficients i16 [B * blocks_max * 64]
//   | 16-byte aligned, the tables of the colour launches of an unscaled batch with an oriented frame:
//     JpegOrientedFrame [B] | JpegFrame [B], the second being the upright frames alone
//   | 16-byte aligned, the tables of a scaled batch: JpegScaledFrame [B] | JpegOrientedFrame [B] upright | JpegOrientedFrame [B] oriented
// The one place that knows the offsets: an accessor takes the base of either side.
struct JpegStageLayout {
    size_t batch = 0, blocks_max = 0; // blocks of the largest frame (max_src_w x max_src_h) in its most expensive sampling
    size_t rec_off = 0, coef_off = 0, oriented_off = 0, scaled_off = 0, total = 0;
    JpegStageLayout() = default;
    JpegStageLayout(int max_batch, int max_src_w, int max_src_h) : batch((size_t)max_batch), blocks_max(jpeg_blocks_bound(max_src_w, max_src_h))
    {
        rec_off = batch * sizeof(JpegFrame);
        coef_off = rec_off + batch * blocks_max * sizeof(uint32_t);
        oriented_off = jpeg_align16(coef_off + batch * blocks_max * 64 * sizeof(int16_t));
        scaled_off = jpeg_align16(oriented_off + batch * (sizeof(JpegOrientedFrame) + sizeof(JpegFrame)));
        total = scaled_off + batch * (sizeof(JpegScaledFrame) + 2 * sizeof(JpegOrientedFrame));
    }
    size_t plane_bytes() const { return batch * blocks_max * 64; } // the plane pool, an allocation of its own
    JpegFrame *frames(void *base) const { return jpeg_at<JpegFrame>(base, 0); }
    uint32_t *rec(void *base) const { return jpeg_at<uint32_t>(base, rec_off); }
    int16_t *coef(void *base) const { return jpeg_at<int16_t>(base, coef_off); }
    JpegOrientedFrame *oriented(void *base) const { return jpeg_at<JpegOrientedFrame>(base, oriented_off); }
    JpegFrame *upright(void *base) const { return jpeg_at<JpegFrame>(base, oriented_off + batch * sizeof(JpegOrientedFrame)); }
    JpegScaledFrame *scaled(void *base) const { return jpeg_at<JpegScaledFrame>(base, scaled_off); }
    JpegOrientedFrame *scaled_upright(void *base) const { return jpeg_at<JpegOrientedFrame>(base, scaled_off + batch * sizeof(JpegScaledFrame)); }
    JpegOrientedFrame *scaled_oriented(void *base) const { return scaled_upright(base) + batch; }
    // what one copy from a region's first byte carries: the descriptors of n frames; those of the whole table and the first
    // `blocks` records behind it; the oriented table and n_upright upright frames; the scaled table, the upright list and
    // n_oriented entries of the oriented list
    size_t frames_bytes(int n) const { return (size_t)n * sizeof(JpegFrame); }
    size_t frames_rec_bytes(size_t blocks) const { return rec_off + blocks * sizeof(uint32_t); }
    size_t oriented_bytes(int n_upright) const { return batch * sizeof(JpegOrientedFrame) + (size_t)n_upright * sizeof(JpegFrame); }
    size_t scaled_bytes(int n_oriented) const { return batch * (sizeof(JpegScaledFrame) + sizeof(JpegOrientedFrame)) + (size_t)n_oriented * sizeof(JpegOrientedFrame); }
};

// The staging of the device entropy stage and its device twin, an allocation of their own:
//   JpegEntropyFrame [B] | status u32 [B] | interval tables u32 [2 * B * intervals_max] | scan bytes [scan_pool]
constexpr size_t kJpegScanFloor = 64 * 1024, kJpegScanBytesPerBlock = 32;
struct JpegEntLayout {
    size_t batch = 0, intervals_max = 0, scan_pool = 0; // MCUs of the largest frame at 8 x 8 per MCU; bytes of the scan pool
    size_t status_off = 0, ivl_off = 0, scan_off = 0, total = 0;
    JpegEntLayout() = default;
    JpegEntLayout(int max_batch, int max_src_w, int max_src_h, size_t blocks_max) : batch((size_t)max_batch)
    {
        intervals_max = (size_t)jpeg_div_up(max_src_w, 8) * (size_t)jpeg_div_up(max_src_h, 8);
        // per frame half a byte per coefficient slot of the largest frame, at least 64 KiB; positions in the pool are 32-bit
        scan_pool = std::min(batch * std::max(kJpegScanFloor, kJpegScanBytesPerBlock * blocks_max), (size_t)0xffff0000u);
        status_off = batch * sizeof(JpegEntropyFrame);
        ivl_off = status_off + batch * sizeof(uint32_t);
        scan_off = ivl_off + ivl_words() * sizeof(uint32_t);
        total = scan_off + scan_pool;
    }
    size_t ivl_words() const { return 2 * batch * intervals_max; }
    JpegEntropyFrame *frames(void *base) const { return (JpegEntropyFrame *)base; }
    uint32_t *status(void *base) const { return jpeg_at<uint32_t>(base, status_off); }
    uint32_t *intervals(void *base) const { return jpeg_at<uint32_t>(base, ivl_off); }
    uint8_t *scan(void *base) const { return jpeg_at<uint8_t>(base, scan_off); }
};

// One frame of a decode call.  A call holds its frames as one heap array: JpegHeader is large.
struct JpegCallFrame {
    JpegHeader hdr;            // msg: why the call refuses the frame, or why the frame stays off the device entropy stage
    int32_t orientation = 1;   // what the call applies: the tag in APPLY mode
    int out_w = 0, out_h = 0;  // the size of the frame it writes
    size_t rec0 = 0;           // the frame's first record in the pools; its coefficients and planes start at rec0 * 64
    uint32_t used = 0;         // coefficients the host decoder wrote
    int status = RFD_OK;       // of the host decoder
    int idct_n[3] = {8, 8, 8}; // per component: the inverse-DCT size (jpeg_idct_sizes)
    bool staged = false;       // device entropy stage: its intervals and scan bytes are in the staging, at
    uint32_t scan0 = 0, ivl0 = 0, nint = 0; // scan0 bytes into the scan pool, ivl0 words into the interval pool, nint intervals
};

// The per-file argument check of a call: fills f[0 .. n) -- header, applied orientation, output size, rec0, inverse-DCT sizes --
// and counts the oriented frames, or returns the status with the message in msg.
inline int jpeg_plan_frames(const uint8_t *const *bytes, const size_t *len, int n, const rfd_image *out, int scale, bool apply_orientation, int max_src_w,
                            int max_src_h, JpegCallFrame *f, int *n_oriented, char *msg, size_t cap)
{
    size_t blocks = 0;
    *n_oriented = 0;
    for (int i = 0; i < n; ++i) {
        JpegCallFrame &c = f[i];
        const JpegHeader &h = c.hdr;
        const int st = jpeg_parse_header(bytes[i], len[i], c.hdr);
        if (st != RFD_OK) { snprintf(msg, cap, "file %d: %s", i, h.msg); return st; }
        if (apply_orientation) c.orientation = h.orientation;
        jpeg_oriented_size(c.orientation, jpeg_scaled_dim(h.width, scale), jpeg_scaled_dim(h.height, scale), &c.out_w, &c.out_h);
        *n_oriented += c.orientation != 1;
        if (h.width > max_src_w || h.height > max_src_h) {
            snprintf(msg, cap, "file %d: %d x %d exceeds max_src %d x %d", i, h.width, h.height, max_src_w, max_src_h);
            return RFD_ERR_CAPACITY;
        }
        if (!out[i].data) { snprintf(msg, cap, "invalid argument: output frame %d has no data pointer", i); return RFD_ERR_INVALID_ARG; }
        if (out[i].width != c.out_w || out[i].height != c.out_h) {
            if (scale != 1)
                snprintf(msg, cap, "invalid argument: output frame %d is %d x %d, file %d is %d x %d at scale 1/%d in orientation %d (%d x %d stored)", i, out[i].width,
                         out[i].height, i, c.out_w, c.out_h, scale, c.orientation, h.width, h.height);
            else if (c.orientation == 1) snprintf(msg, cap, "invalid argument: output frame %d is %d x %d, file %d is %d x %d", i, out[i].width, out[i].height, i, h.width, h.height);
            else
                snprintf(msg, cap, "invalid argument: output frame %d is %d x %d, file %d is %d x %d in orientation %d (%d x %d stored)", i, out[i].width, out[i].height, i,
                         c.out_w, c.out_h, c.orientation, h.width, h.height);
            return RFD_ERR_INVALID_ARG;
        }
        if (out[i].stride < (ptrdiff_t)c.out_w * 3) { snprintf(msg, cap, "invalid argument: output frame %d has stride %td < 3 * width", i, out[i].stride); return RFD_ERR_INVALID_ARG; }
        c.rec0 = blocks;
        blocks += (size_t)h.nblocks;
        if (scale != 1) jpeg_idct_sizes(h, scale, c.idct_n);
    }
    return RFD_OK;
}

// ---------------------------------------------------------------- the device entropy stage
struct JpegEntropyFill { size_t scan_used = 0, ivl_used = 0; }; // of the two pools: bytes; u32 words

// Serial: hands a frame its slices when its header allows the interval path and its scan fits what is left of the pools.
inline bool jpeg_entropy_place(const JpegEntLayout &l, JpegEntropyFill &fill, JpegCallFrame &f, size_t len)
{
    size_t want = 0;
    if (!jpeg_device_eligible(nullptr, len, f.hdr, nullptr, nullptr, 0, &want, f.hdr.msg, sizeof f.hdr.msg)) return false; // cap 0: the header's part of the rule only
    const size_t bytes = len - f.hdr.scan;
    if (fill.scan_used + bytes > l.scan_pool || fill.ivl_used + 2 * want > l.ivl_words()) {
        snprintf(f.hdr.msg, sizeof f.hdr.msg, "not eligible for device entropy decoding: %zu scan bytes in %zu intervals do not fit the staging", bytes, want);
        return false;
    }
    f.scan0 = (uint32_t)fill.scan_used; f.ivl0 = (uint32_t)fill.ivl_used; f.nint = (uint32_t)want;
    fill.scan_used += jpeg_align16(bytes);
    fill.ivl_used += 2 * want;
    f.staged = true;
    return true;
}

// Any thread, a placed frame: the pre-scan straight into the frame's interval table, the scan bytes into its slice of the pool.
inline bool jpeg_entropy_stage_frame(const JpegEntLayout &l, void *pin, JpegCallFrame &f, const uint8_t *d, size_t len)
{
    uint32_t *iv = l.intervals(pin) + f.ivl0;
    size_t want = 0;
    if (!jpeg_device_eligible(d, len, f.hdr, iv, iv + f.nint, f.nint, &want, f.hdr.msg, sizeof f.hdr.msg)) { f.staged = false; return false; }
    memcpy(l.scan(pin) + f.scan0, d + f.hdr.scan, (size_t)iv[2 * f.nint - 1] - f.hdr.scan);
    return true;
}

// The descriptors of the staged frames, packed at the front of the table; returns their number and the workgroups in n and groups.
inline JpegEntropyParams jpeg_plan_entropy(const JpegCallFrame *f, int n, const JpegEntLayout &l, void *pin)
{
    JpegEntropyFrame *ef = l.frames(pin);
    JpegEntropyParams p;
    memset(&p, 0, sizeof p);
    for (int i = 0; i < n; ++i) {
        if (!f[i].staged) continue;
        JpegEntropyFrame &e = ef[p.n++];
        memset(&e, 0, sizeof e);
        jpeg_scan_geom(f[i].hdr, e.geom, e.dc, e.ac);
        const uint32_t *iv = l.intervals(pin) + f[i].ivl0;
        e.rec0 = f[i].rec0;
        e.scan0 = f[i].scan0;
        e.file_scan = (uint32_t)f[i].hdr.scan;
        e.scan_bytes = iv[2 * f[i].nint - 1] - e.file_scan;
        e.interval0 = f[i].ivl0;
        e.intervals = (int)f[i].nint;
        e.group0 = p.groups;
        e.frame = i;
        p.groups += jpeg_div_up(e.intervals, kJpegEntropyGroup);
    }
    return p;
}

// ---------------------------------------------------------------- the tables of the inverse-DCT and colour launches
// Where the frames are written: the caller's device pointers and strides, or back to back with tight rows in one device buffer.
struct JpegOutput {
    const rfd_image *frames; // null: packed
    uint8_t *packed;
};

// What the launches and the uploads need to know of the tables.  The two colour lists exist where the batch is scaled or has
// an oriented frame: each lists only the frames that have a workgroup in it.
struct JpegList { int n = 0, tiles = 0; };
struct JpegTables {
    int groups = 0, tiles = 0; // JpegParams: workgroups of the inverse DCT and the colour launch over every frame
    int cgroups = 0;           // workgroups of the reduced inverse DCT of a scaled batch
    JpegList upright, oriented;
    size_t blocks = 0;         // records of the batch
    size_t lists_off = 0, lists_bytes = 0; // the one copy that carries the lists (and the scaled table); 0 bytes: none
};

// workgroups of an upright colour launch over w x h pixels: one thread per 4 pixels of a row, 256 threads
inline int jpeg_row_tiles(int w, int h) { return (int)(((size_t)jpeg_div_up(w, 4) * h + 255) / 256); }

// One list entry and its tiles: frame i joins the list of its orientation, tiled over the w x h it is WRITTEN in -- in rows where
// upright, in squares of kJpegOrientTile where oriented.
inline JpegOrientedFrame jpeg_list_entry(JpegList &l, int i, int orientation, int w, int h)
{
    JpegOrientedFrame e;
    e.frame = i;
    e.orientation = orientation;
    e.tile0 = l.tiles;
    e.tiles_x = orientation == 1 ? 0 : jpeg_oriented_tiles_x(w);
    l.tiles += orientation == 1 ? jpeg_row_tiles(w, h) : e.tiles_x * jpeg_oriented_tiles_x(h);
    ++l.n;
    return e;
}

// Writes into the staging at `pin`: JpegFrame [n]; for an unscaled batch with an oriented frame the upright JpegFrame list and the
// JpegOrientedFrame list; for a scaled batch JpegScaledFrame [n] and its two JpegOrientedFrame lists.
inline JpegTables jpeg_plan_tables(const JpegCallFrame *frames, int n, int scale, bool any_oriented, const JpegOutput &out, const JpegStageLayout &l, void *pin)
{
    JpegTables t;
    JpegFrame *fr = l.frames(pin), *ufr = l.upright(pin);
    JpegOrientedFrame *ofr = l.oriented(pin), *sup = l.scaled_upright(pin), *sor = l.scaled_oriented(pin);
    JpegScaledFrame *sfr = l.scaled(pin);
    size_t out_at = 0;
    for (int i = 0; i < n; ++i) {
        const JpegCallFrame &c = frames[i];
        const JpegHeader &h = c.hdr;
        JpegFrame &f = fr[i];
        memset(&f, 0, sizeof f);
        if (out.frames) {
            f.out = const_cast<uint8_t *>(out.frames[i].data); // the one entry point that writes a frame (rfd.h)
            f.stride = (long long)out.frames[i].stride;
        } else {
            f.out = out.packed + out_at;
            f.stride = (long long)c.out_w * 3;
            out_at += (size_t)c.out_w * 3 * c.out_h;
        }
        f.rec0 = c.rec0; f.coef0 = c.rec0 * 64; f.plane0 = c.rec0 * 64;
        f.width = h.width; f.height = h.height;
        f.ncomp = h.ncomp; f.hmax = h.hmax; f.vmax = h.vmax;
        f.nblocks = h.nblocks;
        f.group0 = t.groups; f.tile0 = t.tiles;
        t.groups += jpeg_div_up(h.nblocks, kJpegGroupBlocks);
        t.tiles += jpeg_row_tiles(h.width, h.height);
        t.blocks += (size_t)h.nblocks;
        for (int k = 0; k < h.ncomp; ++k) {
            f.bw[k] = h.comp[k].bw; f.bh[k] = h.comp[k].bh; f.blk0[k] = h.comp[k].blk0;
            for (int z = 0; z < 64; ++z) f.quant[k][kJpegNatural[z]] = h.quant[h.comp[k].tq][z];
        }
        if (scale == 1 && !any_oriented) continue; // one colour launch over fr: no list
        const JpegOrientedFrame e = jpeg_list_entry(c.orientation == 1 ? t.upright : t.oriented, i, c.orientation, c.out_w, c.out_h);
        if (scale == 1) {
            if (c.orientation == 1) { JpegFrame &u = ufr[t.upright.n - 1]; u = f; u.tile0 = e.tile0; }
            else ofr[t.oriented.n - 1] = e;
            continue;
        }
        (c.orientation == 1 ? sup[t.upright.n - 1] : sor[t.oriented.n - 1]) = e;
        JpegScaledFrame &sf = sfr[i];
        memset(&sf, 0, sizeof sf);
        size_t at = f.plane0; // n^2 <= 64 bytes per block: the scaled planes fit the frame's share of the pool
        for (int k = 0; k < h.ncomp; ++k) {
            const int nk = c.idct_n[k], blk = h.comp[k].bw * h.comp[k].bh;
            sf.n[k] = nk;
            sf.plane[k] = at;
            sf.pitch[k] = h.comp[k].bw * nk;
            sf.cgroup[k] = t.cgroups;
            t.cgroups += jpeg_div_up(blk, 256 / nk);
            at += (size_t)blk * nk * nk;
        }
        sf.width = jpeg_scaled_dim(h.width, scale); sf.height = jpeg_scaled_dim(h.height, scale);
        sf.hup = h.ncomp == 3 ? h.hmax * (8 / scale) / (h.comp[1].h * sf.n[1]) : 1; // 2 for 4:2:2; the vertical factor is always 1
        sf.replicate = scale == 8;
    }
    if (scale != 1) { t.lists_off = l.scaled_off; t.lists_bytes = l.scaled_bytes(t.oriented.n); }
    else if (any_oriented) { t.lists_off = l.oriented_off; t.lists_bytes = l.oriented_bytes(t.upright.n); }
    return t;
}

} // namespace rfd
