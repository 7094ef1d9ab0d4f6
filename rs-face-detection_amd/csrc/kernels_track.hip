// kernels_track.hip -- the tracker's update (include/rfd.h, "tracker"; gfx950, wave64): an IoU tracker with two score
// thresholds, one workgroup of ONE wave per distinct stream of the call, walking that stream's frames in call order.
//
// Layout.  A stream's max_tracks = 64 K slots (K = 1, 2, 4) live in registers for the whole call: lane l holds slots l, 64 + l,
// ..., so "ascending slot order" is (k, lane) order and a ballot per k lists it.  They are read once and written back once.
// The per-row results of the frame in hand (serial, flags) live in LDS, max_det entries each, because a row's fate is only
// known after the whole frame: births come after ageing and ending, and the due list is in row order over both.
//
// A frame.  Rows are read 64 at a time, one per lane; the sequential part walks the set bits of a ballot, so the row in hand is
// wave-uniform (v_readlane) and every lane tests it against its own slots:
//   association   key = IoU bits (monotone for the positive values that pass iou_min > 0), the lane's best over k with the
//                 lower k on ties, a wave maximum, then one ballot per k in ascending k: the lowest set lane of the first
//                 non-empty ballot is the lowest slot among the equal best;
//   ageing, ending, birth, the `ended` and `due` compaction: ballots and prefix counts below the own lane, as face_list_kernel.
// No atomics, nothing that depends on timing: the same bits on every run.  The IoU restates kernels_post.hip's `suppresses`
// (nms.rs:39-54) operation for operation; this file is compiled with -ffp-contract=off like it.  Latency-bound scalar work.
#include "tracker_host.h"

namespace rfd {

constexpr uint32_t kTrackNew = RFD_TRACK_NEW, kTrackConfirmed = RFD_TRACK_CONFIRMED, kTrackDue = RFD_TRACK_DUE;
constexpr uint32_t kTrackPending = 0x80000000u; // LDS only: an unmatched eligible row with score >= new_score awaits step 5

__device__ __forceinline__ float track_lane_f32(float v, int src) // the value lane `src` (wave-uniform) holds
{
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), src));
}

__device__ __forceinline__ float4 track_lane_box(const float4 v, int src)
{
    return make_float4(track_lane_f32(v.x, src), track_lane_f32(v.y, src), track_lane_f32(v.z, src), track_lane_f32(v.w, src));
}

__device__ __forceinline__ float track_area(const float4 b) { return (b.z - b.x + 1.0f) * (b.w - b.y + 1.0f); }

__device__ __forceinline__ float track_iou(const float4 bi, const float area_i, const float4 bj, const float area_j)
{
    const float xx1 = fmaxf(bi.x, bj.x);
    const float yy1 = fmaxf(bi.y, bj.y);
    const float xx2 = fminf(bi.z, bj.z);
    const float yy2 = fminf(bi.w, bj.w);
    float w = xx2 - xx1 + 1.0f;
    float h = yy2 - yy1 + 1.0f;
    w = fmaxf(0.0f, w);
    h = fmaxf(0.0f, h);
    const float inter = w * h;
    const float uni = area_i + area_j - inter;
    return inter / uni;
}

__device__ __forceinline__ uint32_t track_wave_max(uint32_t v) // all 64 lanes active
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int)v, d);
        v = o > v ? o : v;
    }
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)v);
}

// this lane's row of the 64 from `base`: box, score-derived predicates, quality
struct TrackRow {
    float4 box;
    float q;
    bool elig, newok;
};
__device__ __forceinline__ TrackRow track_row(const TrackParams &p, const float *boxes, const float *qual, int i, int cnt)
{
    TrackRow r;
    r.box = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    r.q = 0.0f;
    r.elig = r.newok = false;
    if (i < cnt) {
        const float *s = boxes + 5 * (size_t)i;
        r.box = make_float4(s[0], s[1], s[2], s[3]);
        const float sc = s[4];
        r.q = qual ? qual[i] : sc;
        r.elig = sc >= p.min_score; // false for a NaN
        r.newok = sc >= p.new_score;
    }
    return r;
}

template <int K> __global__ void __launch_bounds__(64) track_update_kernel(TrackParams p)
{
    extern __shared__ __attribute__((aligned(16))) int track_lds[];
    int *s_track = track_lds;                                                 // [max_det]
    uint32_t *s_flags = reinterpret_cast<uint32_t *>(track_lds + p.max_det);  // [max_det]
    const int lane = threadIdx.x;
    const unsigned long long below = (1ull << lane) - 1ull;
    const int g = blockIdx.x;
    const int32_t *group_stream = p.plan, *group_first = p.plan + p.n, *order = p.plan + 2 * (size_t)p.n + 1;
    const int s = group_stream[g], f0 = group_first[g], f1 = group_first[g + 1];
    TrackSlot *slots = p.slots + (size_t)s * p.max_tracks;

    int serial[K], missed[K], hits[K];
    float shot[K];
    float4 box[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int4 a = reinterpret_cast<const int4 *>(slots + k * 64 + lane)[0];
        box[k] = reinterpret_cast<const float4 *>(slots + k * 64 + lane)[1];
        serial[k] = a.x; missed[k] = a.y; hits[k] = a.z; shot[k] = __int_as_float(a.w);
    }
    int next = p.next_serial[s];

    for (int fi = f0; fi < f1; ++fi) {
        const int b = order[fi];
        const int cnt = min(max(p.count[b], 0), p.max_det);
        const float *boxes = p.boxes + (size_t)b * p.max_det * 5;
        const float *qual = p.quality ? p.quality + (size_t)b * p.max_det : nullptr;
        const size_t row0 = (size_t)b * p.max_det;
        uint32_t matched = 0; // bit k: this lane's slot k was matched in this frame
        int n_matched = 0, n_born = 0, n_ended = 0, n_dropped = 0;

        // ---- 1 eligibility, 2 association ----
        for (int base = 0; base < cnt; base += 64) {
            const int i = base + lane;
            const TrackRow r = track_row(p, boxes, qual, i, cnt);
            unsigned long long em = __ballot(r.elig);
            unsigned long long mm = 0; // rows of this chunk that took a slot
            while (em != 0ull) {       // wave-uniform walk in row order
                const int j = __builtin_ctzll(em);
                em &= em - 1ull;
                const float4 rb = track_lane_box(r.box, j);
                const float rq = track_lane_f32(r.q, j);
                const float ra = track_area(rb);
                uint32_t best = 0;
                int bk = 0;
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    const bool open = serial[k] != 0 && ((matched >> k) & 1u) == 0u;
                    const float iou = track_iou(rb, ra, box[k], track_area(box[k]));
                    const uint32_t bits = (open && iou >= p.iou_min) ? __float_as_uint(iou) : 0u; // a NaN is no candidate
                    if (bits > best) { best = bits; bk = k; }
                }
                const uint32_t m = track_wave_max(best);
                if (m == 0u) continue;
                int wk = -1, wl = 0;
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    const unsigned long long bal = __ballot(best == m && bk == k);
                    if (wk < 0 && bal != 0ull) { wk = k; wl = __builtin_ctzll(bal); }
                }
                mm |= 1ull << j;
                ++n_matched;
                if (lane == wl) {
#pragma unroll
                    for (int k = 0; k < K; ++k)
                        if (k == wk) {
                            box[k] = rb; missed[k] = 0; hits[k] += 1;
                            matched |= 1u << k;
                            uint32_t f = hits[k] >= p.min_hits ? kTrackConfirmed : 0u;
                            if (f != 0u && rq > shot[k] * p.improve) { f |= kTrackDue; shot[k] = rq; }
                            s_track[base + j] = serial[k];
                            s_flags[base + j] = f;
                        }
                }
            }
            if (i < cnt && ((mm >> lane) & 1ull) == 0ull) {
                s_track[i] = 0;
                s_flags[i] = (r.elig && r.newok) ? kTrackPending : 0u;
            }
        }

        // ---- 3 ageing, 4 ending ----
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const bool live = serial[k] != 0;
            if (live && ((matched >> k) & 1u) == 0u) missed[k] += 1;
            const bool end = live && missed[k] > p.max_missed;
            const unsigned long long bal = __ballot(end);
            if (end) {
                if (p.ended) p.ended[(size_t)b * p.max_tracks + n_ended + __popcll(bal & below)] = serial[k];
                serial[k] = 0; missed[k] = 0; hits[k] = 0; shot[k] = 0.0f;
                box[k] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            }
            n_ended += __popcll(bal);
        }
        __syncthreads(); // one wave: orders the LDS stores of step 2 before the reads below

        // ---- 5 birth (with 6, 7 for the born rows) ----
        unsigned long long freeb[K];
#pragma unroll
        for (int k = 0; k < K; ++k) freeb[k] = __ballot(serial[k] == 0);
        for (int base = 0; base < cnt; base += 64) {
            const int i = base + lane;
            unsigned long long pm = __ballot(i < cnt && (s_flags[i] & kTrackPending) != 0u);
            if (pm == 0ull) continue;
            const TrackRow r = track_row(p, boxes, qual, i, cnt);
            while (pm != 0ull) {
                const int j = __builtin_ctzll(pm);
                pm &= pm - 1ull;
                int wk = -1, wl = 0;
#pragma unroll
                for (int k = 0; k < K; ++k)
                    if (wk < 0 && freeb[k] != 0ull) { wk = k; wl = __builtin_ctzll(freeb[k]); }
                if (wk < 0) { // no free slot: dropped
                    ++n_dropped;
                    if (lane == 0) s_flags[base + j] = 0u;
                    continue;
                }
#pragma unroll
                for (int k = 0; k < K; ++k)
                    if (k == wk) freeb[k] &= ~(1ull << wl);
                const float4 rb = track_lane_box(r.box, j);
                const float rq = track_lane_f32(r.q, j);
                if (lane == wl) {
#pragma unroll
                    for (int k = 0; k < K; ++k)
                        if (k == wk) {
                            serial[k] = next; box[k] = rb; missed[k] = 0; hits[k] = 1;
                            shot[k] = -__builtin_inff();
                            uint32_t f = kTrackNew | (1 >= p.min_hits ? kTrackConfirmed : 0u);
                            if ((f & kTrackConfirmed) != 0u && rq > shot[k] * p.improve) { f |= kTrackDue; shot[k] = rq; }
                            s_track[base + j] = next;
                            s_flags[base + j] = f;
                        }
                }
                next = next == 0x7fffffff ? 1 : next + 1;
                ++n_born;
            }
        }
        __syncthreads();

        // ---- the rows' outputs and the due list, in row order ----
        int n_due = 0;
        for (int base = 0; base < cnt; base += 64) {
            const int i = base + lane;
            int t = 0;
            uint32_t f = 0u;
            if (i < cnt) {
                t = s_track[i];
                f = s_flags[i];
                p.track[row0 + i] = t;
                p.flags[row0 + i] = f;
            }
            const bool due = (f & kTrackDue) != 0u;
            const unsigned long long bal = __ballot(due);
            if (due) {
                const size_t at = row0 + n_due + __popcll(bal & below); // <= row0 + i
                if (p.due_boxes) {
                    const float *kps = p.lmk + (row0 + i) * 10;
#pragma unroll
                    for (int c = 0; c < 5; ++c) p.due_boxes[at * 5 + c] = boxes[5 * (size_t)i + c];
#pragma unroll
                    for (int c = 0; c < 10; ++c) p.due_lmk[at * 10 + c] = kps[c];
                }
                if (p.due_track) p.due_track[at] = t;
            }
            n_due += __popcll(bal);
        }
        if (lane == 0) {
            if (p.due_count) p.due_count[b] = n_due;
            if (p.due_total) p.due_total[b] = n_due;
            if (p.stats) {
                p.stats[4 * b + 0] = n_matched; p.stats[4 * b + 1] = n_born;
                p.stats[4 * b + 2] = n_ended; p.stats[4 * b + 3] = n_dropped;
            }
        }
        __syncthreads(); // the next frame reuses the LDS arrays
    }

#pragma unroll
    for (int k = 0; k < K; ++k) {
        reinterpret_cast<int4 *>(slots + k * 64 + lane)[0] = make_int4(serial[k], missed[k], hits[k], __float_as_int(shot[k]));
        reinterpret_cast<float4 *>(slots + k * 64 + lane)[1] = box[k];
    }
    if (lane == 0) p.next_serial[s] = next;
}

int launch_track_update(const TrackParams &p, int groups, hipStream_t s)
{
    const size_t lds = track_update_lds_bytes(p.max_det);
    switch (p.max_tracks) {
    case 64: hipLaunchKernelGGL(track_update_kernel<1>, dim3(groups), dim3(64), lds, s, p); break;
    case 128: hipLaunchKernelGGL(track_update_kernel<2>, dim3(groups), dim3(64), lds, s, p); break;
    case 256: hipLaunchKernelGGL(track_update_kernel<4>, dim3(groups), dim3(64), lds, s, p); break;
    default: set_error("tracker: max_tracks %d has no kernel", p.max_tracks); return RFD_ERR_INVALID_ARG;
    }
    RFD_HIP(hipGetLastError());
    return RFD_OK;
}

} // namespace rfd
