// jpeg_host.h -- JpegDecoder: everything a context owns for the JPEG decode (include/rfd.h, "JPEG decode") and the host side of a
// decode call.  What a call decides is planned in jpeg_plan.h; jpeg_host.hip enqueues it.  Host only.
#pragma once
#include <vector>

#include "host_resources.h"
#include "jpeg_plan.h"

namespace rfd {

struct JpegCall; // one decode call (jpeg_host.hip)

struct JpegDecoder {
    // All allocated by the first decode call.  pin is the page-locked staging the decode threads write and dev its device twin,
    // both laid out by `stage` (JpegStageLayout): JpegFrame [B] | block records | coefficients | the tables of the colour launches
    // of a batch with an oriented frame | the tables of a scaled batch, B = max_batch_size.  A batch without an oriented frame
    // neither writes nor copies the orientation tables.  pin_done: the copies out of pin that the last call enqueued.
    int decode_threads = 4;
    JpegStageLayout stage;
    Pinned<char> pin;
    Event pin_done;
    DevBuf dev, planes, packed; // packed: the device frames of the host-output form, back to back
    // Entropy decoding on the device (rfd_set_jpeg_entropy), all allocated by the first decode call in that mode.  ent_pin and its
    // device twin ent_dev are laid out by `ent` (JpegEntLayout): JpegEntropyFrame [B] | status u32 [B] | interval tables | scan
    // bytes.  The copies out of ent_pin are covered by pin_done as well; ent_done: the status words of the last entropy launch
    // have arrived.
    int entropy = RFD_JPEG_ENTROPY_HOST;
    JpegEntLayout ent;
    Pinned<char> ent_pin;
    DevBuf ent_dev;
    Event ent_done;
    std::vector<int32_t> paths; // rfd_jpeg_last_paths
    // EXIF orientation (rfd_set_jpeg_orientation) and reduced size (rfd_set_jpeg_scale)
    int orientation = RFD_JPEG_ORIENTATION_IGNORE;
    std::vector<int32_t> orientations; // rfd_jpeg_last_orientations
    int scale = 1;

    // Both forms of the decode of n >= 1 files, n <= cfg.max_batch_size: frames on the device (out_on_device) or on the host.
    // Returns with the stream synchronised unless `async` and out_on_device.  Errors are left in set_error.
    int decode(hipStream_t s, const rfd_config &cfg, const uint8_t *const *bytes, const size_t *len, int n, const rfd_image *out, bool out_on_device, bool async);
    // rfd_debug_jpeg_coefficients_device: one file through the device entropy stage alone
    int debug_coefficients(hipStream_t s, const rfd_config &cfg, const uint8_t *bytes, size_t len, int16_t *out, size_t cap_blocks, size_t *blocks);

private:
    int ensure_staging(const rfd_config &cfg, bool device_entropy);
    int entropy_stage(hipStream_t s, JpegCall &k);
    int entropy_enqueue(hipStream_t s, const JpegCall &k);
    int entropy_collect(JpegCall &k, std::vector<int> &refused);
    bool decode_on_host(JpegCall &k, const std::vector<int> &which);
    int upload(hipStream_t s, const JpegCall &k, const JpegTables &t);
    int launch(hipStream_t s, const JpegCall &k, const JpegTables &t);
};

} // namespace rfd
