// jpeg_desc.h -- the descriptors the JPEG kernels read (kernels_jpeg.hip, kernels_jpeg_entropy.hip), in plain C++ without a HIP
// header: the launch interfaces of kernels.h and the host-side planning of jpeg_plan.h share them, and the latter is built by the
// host compiler alone (tests/cpp/jpeg_plan_check.cpp).
#pragma once
#include <cstddef>
#include <cstdint>

#include "jpeg_entropy.h"

namespace rfd {

// ---------------------------------------------------------------- JPEG decode (kernels_jpeg.hip)
// One frame of a batch.  The frames of a batch share three pools: block records, coefficients, component planes.
struct JpegFrame {
    uint8_t *out;              // device [height][stride] u8 BGR
    long long stride;          // bytes per output row, >= 3 * width
    unsigned long long rec0;   // the frame's first block record in the record pool
    unsigned long long coef0;  // the frame's first value in the coefficient pool; a record's offset counts from here
    unsigned long long plane0; // the frame's first byte in the plane pool: 64 per block, components in order, each plane row-major
    int width, height;
    int ncomp, hmax, vmax;     // 1 or 3 components; luma sampling 1x1, 2x1 or 2x2 (chroma is 1x1)
    int nblocks;
    int group0;                // the frame's first workgroup (32 blocks each) in the inverse-DCT launch
    int tile0;                 // the frame's first workgroup (256 x 4 pixels each) in the colour launch
    int bw[3], bh[3], blk0[3]; // per component: blocks per row / per column (whole MCUs), first block
    uint16_t quant[3][64];     // per component, in NATURAL order
};
struct JpegParams {
    const JpegFrame *frames; // device [n]
    int n;
    int groups, tiles;       // workgroups of the two launches: the sum over the frames
    const uint32_t *rec;     // offset << 7 | count per block (jpeg_parse.h)
    const int16_t *coef;     // quantised coefficients, zigzag order, `count` per block
    uint8_t *planes;
};
constexpr int kJpegGroupBlocks = 32;  // 8 lanes per block
constexpr int kJpegTilePixels = 1024; // one thread per 4 pixels of a row
// EXIF orientation (rfd.h, "EXIF orientation").  A frame of orientation 2..8 takes jpeg_color_oriented_kernel instead of the colour
// kernel.  Every frame of a launch's table needs at least one workgroup there, so each colour launch has a table of its own: the
// oriented one below, which points into the batch's JpegFrame table, and for the upright frames a second JpegFrame table that
// holds only them.  JpegFrame and JpegParams are what they were, so the two kernels that read them are too.
struct JpegOrientedFrame {
    int frame;       // index in JpegOrientedParams::frames: sizes (STORED width and height), planes, out, stride
    int orientation; // 2..8
    int tile0;       // the frame's first workgroup in the oriented launch
    int tiles_x;     // tiles per row of tiles of the ORIENTED frame
};
struct JpegOrientedParams {
    const JpegFrame *frames;           // device: the whole batch, as the inverse DCT reads it
    const JpegOrientedFrame *oriented; // device [n]
    int n, tiles;
    const uint8_t *planes;
};
constexpr int kJpegOrientTile = 64; // a workgroup's square of OUTPUT pixels; origins are multiples of it
inline int jpeg_oriented_tiles_x(int out_w) { return (out_w + kJpegOrientTile - 1) / kJpegOrientTile; }
// Reduced size (rfd.h, "JPEG decode, reduced size").  What a scaled frame adds to its JpegFrame, which keeps the STORED sizes, the
// block counts, the records and the quantisers: component c is inverse-transformed at n[c] x n[c] samples per block into a plane
// of its own pitch.  JpegFrame and JpegParams are what they were, so the kernels of unscaled batches are too.
struct JpegScaledFrame {
    unsigned long long plane[3]; // per component: the plane's first byte in the plane pool, n[c]^2 bytes per block, row-major
    int n[3];                    // the component's inverse-DCT size: 8, 4, 2 or 1
    int pitch[3];                // bytes per plane row: bw[c] * n[c]
    int cgroup[3];               // the component's first workgroup in the reduced inverse-DCT launch (256 / n[c] blocks each)
    int width, height;           // the SCALED size: ceil(stored / s)
    int hup;                     // the horizontal upsampling left for the chroma planes: 2 for 4:2:2, else 1; never a vertical one
    int replicate;               // s = 8: that upsampling is plain replication
};
struct JpegScaledParams {
    const JpegFrame *frames;           // device: the whole batch; out and stride describe the scaled (and oriented) frame
    const JpegScaledFrame *scaled;     // device: the whole batch, frame by frame
    const JpegOrientedFrame *upright;  // device [n_upright]: frame, tile0 (256 x 4 pixels of the scaled frame per workgroup)
    const JpegOrientedFrame *oriented; // device [n_oriented]: as in JpegOrientedParams, tiles over the scaled oriented size
    int n, groups;                     // frames; workgroups of the reduced inverse DCT
    int n_upright, tiles_upright, n_oriented, tiles_oriented;
    const uint32_t *rec;
    const int16_t *coef;
    uint8_t *planes;
};

// ---------------------------------------------------------------- JPEG entropy decode (kernels_jpeg_entropy.hip)
// Huffman decoding of restart-interval files, one thread per interval (jpeg_entropy.h).  One frame of a batch that takes this
// path; the frames share three pools: scan bytes, interval tables, and the record / coefficient pools of JpegParams.
struct JpegEntropyFrame {
    JpegDevHuff dc[3], ac[3];   // per component; the kernel stages the six as one run of words
    JpegScanGeom geom;
    unsigned long long rec0;    // the frame's first block record; its coefficients start at rec0 * 64 (JpegFrame)
    uint32_t scan0, scan_bytes; // the frame's entropy-coded bytes in the scan pool
    uint32_t file_scan;         // what the interval table's positions count from: the file offset of the first scan byte
    uint32_t interval0;         // the frame's table in the interval pool: begin[intervals] | end[intervals]
    int intervals;
    int group0;                 // the frame's first workgroup
    int frame;                  // index in the batch: its status word
    int pad;
};
static_assert(offsetof(JpegEntropyFrame, ac) == 3 * sizeof(JpegDevHuff), "dc | ac is one run");
struct JpegEntropyParams {
    const JpegEntropyFrame *frames; // device [n]
    int n, groups;
    const uint8_t *scan;
    const uint32_t *intervals;
    uint32_t *rec;                  // written: (block * 64) << 7 | count
    int16_t *coef;                  // written: block b's quantised coefficients, zigzag order, at b * 64
    uint32_t *status;               // per frame of the batch, zeroed by the caller: |= 1 when an interval is refused
};
constexpr int kJpegEntropyGroup = 64; // one wave: 64 intervals of one frame

} // namespace rfd
