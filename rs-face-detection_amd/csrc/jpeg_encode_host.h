// jpeg_encode_host.h -- JpegEncoder: everything a context owns for the JPEG encode (include/rfd.h, "JPEG encode"), and what its
// kernels are told.  What a call decides is planned in jpeg_encode_plan.h; jpeg_encode_host.hip enqueues it; the kernels are
// kernels_jpeg_encode.hip.  Host only.
#pragma once
#include "ctx_access.h" // what the entries need of their context: ctx_stream, ctx_device, ctx_jpeg_encoder
#include "host_resources.h"
#include "jpeg_encode_plan.h"

namespace rfd {

struct EncParams {
    const EncTables *tables; // device
    const EncImage *imgs;    // device, [n], group0 / interval0 ascending
    int n;
    int ncomp, h, v;         // jpeg_encode_sampling of the call
    const int32_t *count;    // device or null: images at and past *count are left alone
    int16_t *coef;           // [blocks of the call][64], zigzag order
    uint32_t *interval_len;  // [intervals of the call]: stuffed bytes of each, without its marker
    uint32_t *interval_off;  // where each begins behind its file's header
    unsigned long long slot_bytes;
    int32_t *size;           // device, [n]
};

// pixels -> quantised coefficients: `groups` workgroups (EncPlan::groups)
int launch_jpeg_encode_blocks(const EncParams &p, int groups, hipStream_t s);
// one workgroup per restart interval.  write = false: interval_len alone; true: the bytes and the marker behind them, into the
// slots of the images whose size is not -1
int launch_jpeg_encode_entropy(const EncParams &p, int intervals, bool write, hipStream_t s);
// one workgroup per image: interval_off, size, and the header of a file that fits
int launch_jpeg_encode_assemble(const EncParams &p, hipStream_t s);

// The part of a context that belongs to the JPEG encode, all allocated by the first call that needs it and grown on demand like
// the decoder's staging: a buffer that grows is freed and allocated anew, which waits for the device, so a warm call allocates
// nothing.  Every buffer is reused by the next call in stream order.
struct JpegEncoder {
    static constexpr int kRing = 4;
    PinnedRing<kRing> ring;  // EncTables | EncImage [max_batch_size]
    DevBuf desc;             // its device twin
    DevBuf coef, intervals;  // EncPlan::coef_bytes, interval_bytes
    DevBuf staging, slots, sizes; // host form and test hooks: the frames with tight rows, the files, their sizes

    // The device form: n >= 1 images planned into desc / plan, enqueued on s.  stages: bit 0 the block kernel, bit 1 the rest.
    int enqueue(hipStream_t s, int max_batch, const rfd_jpeg_encode_config &cfg, const EncTables &tables, const EncImage *desc_host, int n, const EncPlan &plan,
                const int32_t *count_dev, size_t slot_bytes, int32_t *size_dev, int stages);
    // host frames -> the staging, desc_host[i].src / stride redirected there
    int stage_frames(hipStream_t s, const rfd_image *imgs, EncImage *desc_host, int n, const EncPlan &plan);
};

} // namespace rfd
