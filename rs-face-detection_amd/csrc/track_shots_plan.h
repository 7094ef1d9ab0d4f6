// track_shots_plan.h -- the host decisions of the track shots (include/rfd.h, "track shots"): which bounds a config must keep,
// how large the bank of crops may grow, how many copy items a call can produce at most, how a row of crop bytes is cut into the
// chunks of the copy kernel, which of the copy kernel's three paths a (source, destination, row bytes) takes, and how the stream
// list and the stamps of a call lie in one ring slot.  Plain host code: nothing of the device runtime is included, so
// tests/cpp/track_shots_plan_check.cpp builds it with the host compiler alone.  track_shots_host.hip does what is decided here;
// kernels_track_shots.hip runs it (the chunking and the path choice are constexpr, so the kernel calls the very same functions).
#pragma once
#include "track_plan.h"

namespace rfd {

constexpr int kTrackShotMaxSide = 1024;
constexpr size_t kTrackShotMaxBytes = (size_t)1 << 30; // of the bank: streams * max_tracks * crop_w * crop_h * 3
constexpr int kTrackShotCopyThreads = 256;
constexpr uint32_t kTrackShotChunkBytes = 4096; // of a row per workgroup: 256 threads x 16 bytes, a multiple of 16

// The bounds of rfd_track_shot_config; a refusal names its field in msg.
inline bool track_shot_config_ok(const rfd_track_shot_config &c, char *msg, size_t cap)
{
    auto no = [&](const char *what) { snprintf(msg, cap, "%s", what); return false; };
    if (c.crop_w < 1 || c.crop_w > kTrackShotMaxSide) return no("crop_w outside 1..1024");
    if (c.crop_h < 1 || c.crop_h > kTrackShotMaxSide) return no("crop_h outside 1..1024");
    for (int i = 0; i < 6; ++i)
        if (c.reserved[i] != 0) return no("reserved is not 0");
    return true;
}

// Bytes of one crop, and of the bank of a tracker; the heads beside it are 32 bytes per slot and not counted (rfd.h states the
// bound on streams * max_tracks * crop bytes).  Non-positive arguments give 0.
inline size_t track_shot_row_bytes(int crop_w, int crop_h)
{
    return crop_w > 0 && crop_h > 0 ? (size_t)crop_w * (size_t)crop_h * 3 : 0;
}
inline size_t track_shot_bank_bytes(int streams, int max_tracks, int crop_w, int crop_h)
{
    return streams > 0 && max_tracks > 0 ? (size_t)streams * (size_t)max_tracks * track_shot_row_bytes(crop_w, crop_h) : 0;
}
inline bool track_shot_fits(int streams, int max_tracks, int crop_w, int crop_h)
{
    return track_shot_bank_bytes(streams, max_tracks, crop_w, crop_h) <= kTrackShotMaxBytes;
}

// The most copy items a call can produce, known on the host: a keep call has at most one winner per slot of each of its groups
// and never more than it has observations; a collect call lists at most max_tracks endings per frame and never more than cap.
inline int track_shot_keep_bound(int m, int groups, int max_tracks)
{
    return (int)std::min<long long>(std::max(m, 0), (long long)std::max(groups, 0) * max_tracks);
}
inline int track_shot_collect_bound(int cap, int n, int max_tracks)
{
    return (int)std::min<long long>(std::max(cap, 0), (long long)std::max(n, 0) * max_tracks);
}
// The work list of the state holds the items of either call: segments of max_tracks items, one per group or frame.
inline size_t track_shot_item_capacity(int max_batch, int max_tracks) { return (size_t)max_batch * (size_t)max_tracks; }

// The chunks of a row: chunk c is the bytes [c * 4096, min((c + 1) * 4096, row_bytes)) of it.
constexpr uint32_t track_shot_row_chunks(uint32_t row_bytes) { return (row_bytes + kTrackShotChunkBytes - 1) / kTrackShotChunkBytes; }
constexpr uint32_t track_shot_chunk_begin(uint32_t, uint32_t c) { return c * kTrackShotChunkBytes; }
constexpr uint32_t track_shot_chunk_end(uint32_t row_bytes, uint32_t c)
{
    return (c + 1) * kTrackShotChunkBytes < row_bytes ? (c + 1) * kTrackShotChunkBytes : row_bytes;
}

// The path of one copy item.  Chunks start at multiples of 16 within the row, so the residues of the row addresses are those of
// every chunk.  VEC16: both rows 16-byte aligned -- 16-byte loads and stores, then the bytes of the end.  DWORD: the rows share
// their residue mod 4 -- bytes up to the next multiple of 4, dwords, bytes of the end.  BYTES: everything else.
constexpr int kShotCopyVec16 = 0, kShotCopyDword = 1, kShotCopyBytes = 2;
constexpr int track_shot_copy_path(uint64_t src, uint64_t dst, uint32_t row_bytes)
{
    return row_bytes >= 16 && src % 16 == 0 && dst % 16 == 0 ? kShotCopyVec16
         : row_bytes >= 4 && src % 4 == dst % 4             ? kShotCopyDword
                                                            : kShotCopyBytes;
}
// How a chunk of `len` bytes at address `addr` is split on a path: `head` single bytes, `body` units of `unit` bytes, `tail`
// single bytes; head + body * unit + tail == len, and the body starts at a multiple of `unit`.
struct ShotCopySplit {
    uint32_t head, body, tail, unit;
};
constexpr ShotCopySplit track_shot_copy_split(int path, uint64_t addr, uint32_t len)
{
    if (path == kShotCopyVec16) return ShotCopySplit{0u, len / 16, len % 16, 16u};
    if (path == kShotCopyDword) {
        const uint32_t to = (uint32_t)((4 - addr % 4) % 4), head = to < len ? to : len;
        return ShotCopySplit{head, (len - head) / 4, (len - head) % 4, 4u};
    }
    return ShotCopySplit{len, 0u, 0u, 1u};
}

// One ring slot of a call of n frames: the int32 work list (track_plan's 3 n + 1 ints for keep; for collect the stream list as
// it stands in the first n of them), padded to 8 bytes, then stamp[n] as int64.  The slot travels to the device as it stands.
inline size_t track_shot_ring_stamp_offset(int n) { return (track_plan_ints(n) * sizeof(int32_t) + 7) / 8 * 8; }
inline size_t track_shot_ring_bytes(int n) { return track_shot_ring_stamp_offset(n) + (size_t)n * sizeof(int64_t); }
// Fills a slot's stamps: the caller's, or 0 for NULL.
inline void track_shot_ring_stamps(char *slot, const int64_t *stamp, int n)
{
    int64_t *at = reinterpret_cast<int64_t *>(slot + track_shot_ring_stamp_offset(n));
    for (int i = 0; i < n; ++i) at[i] = stamp ? stamp[i] : 0;
}

} // namespace rfd
