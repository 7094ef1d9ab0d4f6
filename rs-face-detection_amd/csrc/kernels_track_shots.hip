// kernels_track_shots.hip -- the track shots (include/rfd.h, "track shots"; gfx950, wave64): decide which due crop becomes a
// track's stored shot, list the tracks an update ended as records, and move the crop bytes of both.
//
// Decide: one workgroup of ONE wave per distinct stream of the call (track_plan's groups), walking that stream's frames in call
// order and each frame's observations in ascending t, like track_fuse_kernel.  The stream's slot serials and its heads are
// staged in LDS once; an observation's track is found with one ballot per 64 slots; what an observation needs (serial, q, bad
// input) is read 64 observations at a time, one per lane, and handed on by v_readlane, and the statuses go back the same way,
// 64 at a time.  Every decision is wave-uniform and lives in LDS until the end, so the chain per observation holds no global
// load at all.  LDS also keeps, per slot, the last kept observation of this call: at the end every slot that has one becomes
// ONE copy item, so a kept shot that was superseded moves no bytes.  The items of group g are segment g of the state's work
// list (max_tracks items and a count each): no atomics, the same list on every run.
//
// List: ONE workgroup of 8 waves; wave w takes frames w, w + 8, ...  Phase 1 stages the head serials of the frame's stream (and
// the identity heads' serials) in the wave's LDS, reads 64 `ended` entries at a time, finds each among the heads with one
// ballot per 64 heads, and packs the found entries of the frame in `ended` order into the state's scratch.  Wave 0 then turns
// the frames' counts into first[] and total by a wave scan, so the order (frame, ended order) comes out of the prefix sums.
// Phase 2 writes one record per lane and one copy item per record below cap.
//
// Copy: blockIdx.x is the item, blockIdx.y the 4096-byte chunk of its row.  The item is found by walking the segments' counts
// (uniform loads); a workgroup at or past the sum leaves.  The path (16-byte units, dwords, bytes) is chosen per item by
// track_shot_copy_path from the two row addresses -- the host's function, so tests/cpp/track_shots_plan_check.cpp covers what
// runs here -- and never touches a byte outside the row.
#include "tracker_host.h"

namespace rfd {

constexpr int kShotMaxTracks = 256;
constexpr int kListWaves = 8;

__device__ __forceinline__ int tsh_count(const int32_t *total, int m) { return total ? min(max(total[0], 0), m) : m; }

// the lowest index below `count` (a multiple of 64) whose LDS entry equals `ser` (wave-uniform), or -1; 0 names nothing
__device__ __forceinline__ int tsh_find(const int *s_serial, int count, int lane, int ser)
{
    if (ser == 0) return -1;
    for (int k = 0; k < count; k += 64) {
        const unsigned long long bal = __ballot(s_serial[k + lane] == ser);
        if (bal != 0ull) return k + __builtin_ctzll(bal);
    }
    return -1;
}

__device__ __forceinline__ int tsh_lanes_below(unsigned long long bal) // set bits of bal below this lane
{
    return __builtin_amdgcn_mbcnt_hi((unsigned)(bal >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)bal, 0u));
}

__global__ void __launch_bounds__(64) track_shot_decide_kernel(TrackShotDecideParams p)
{
    __shared__ int s_serial[kShotMaxTracks];
    __shared__ int s_head[8 * kShotMaxTracks]; // the stream's heads, word w of slot j at w * 256 + j: no read is wider than 32 bits
    __shared__ int s_win[kShotMaxTracks];      // the last kept observation of this call, -1 for none
    __shared__ int s_dirty[kShotMaxTracks];
    constexpr int K = kShotMaxTracks;
    const int lane = threadIdx.x, g = blockIdx.x;
    const TrackShotCommon &c = p.c;
    const int32_t *group_stream = c.plan, *group_first = c.plan + c.n, *order = c.plan + 2 * (size_t)c.n + 1;
    const int s = group_stream[g], f0 = group_first[g], f1 = group_first[g + 1];
    const int count = tsh_count(p.total, p.m), mt = c.max_tracks;
    const TrackSlot *slots = c.slots + (size_t)s * mt;
    TrackShotHead *heads = c.heads + (size_t)s * mt;
    for (int j = lane; j < mt; j += 64) {
        s_serial[j] = slots[j].serial;
        const int4 h0 = reinterpret_cast<const int4 *>(heads + j)[0];
        const int4 h1 = reinterpret_cast<const int4 *>(heads + j)[1];
        int *w = s_head + j;
        w[0 * K] = h0.x; w[1 * K] = h0.y; w[2 * K] = h0.z; w[3 * K] = h0.w;
        w[4 * K] = h1.x; w[5 * K] = h1.y; w[6 * K] = h1.z; w[7 * K] = h1.w;
        s_win[j] = -1;
        s_dirty[j] = 0;
    }
    __syncthreads();

    for (int fi = f0; fi < f1; ++fi) {
        const int b = order[fi];
        const long long stamp = c.stamp[b];
        const int st_lo = (int)(unsigned)stamp, st_hi = (int)(stamp >> 32);
        const int t0 = max(p.first[b], 0), t1 = min(p.first[b + 1], count);
        for (int base = t0; base < t1; base += 64) { // 64 observations at a time: lane l reads what t = base + l needs
            const int mine = base + lane, cnt = min(64, t1 - base);
            int l_ser = 0, l_bad = 0, l_status = 0;
            float l_q = 0.0f;
            if (mine < t1) {
                const int r = p.row[mine];
                l_ser = (r >= 0 && r < c.max_det) ? p.serial[(size_t)b * c.max_det + r] : 0;
                if (p.q) l_q = p.q[mine];
                l_bad = (p.face_status && p.face_status[mine] < 0) || l_q != l_q;
            }
            for (int k = 0; k < cnt; ++k) { // everything below is wave-uniform: every lane computes the same entry
                int st;
                if (__builtin_amdgcn_readlane(l_bad, k) != 0) {
                    st = RFD_TRACK_SHOT_BAD_INPUT;
                } else {
                    const int ser = __builtin_amdgcn_readlane(l_ser, k);
                    const int slot = tsh_find(s_serial, mt, lane, ser);
                    if (slot < 0) {
                        st = RFD_TRACK_SHOT_NO_TRACK;
                    } else {
                        const float q = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(l_q), k));
                        int *w = s_head + slot;
                        const bool stale = w[0] != ser;
                        const int shots = (stale ? 0 : w[1 * K]) + 1, kept = stale ? 0 : w[2 * K];
                        const float hq = stale ? -__builtin_inff() : __int_as_float(w[3 * K]);
                        const bool take = kept == 0 || p.q == nullptr || q > hq;
                        st = take ? RFD_TRACK_SHOT_KEPT : RFD_TRACK_SHOT_PASSED;
                        __syncthreads(); // one wave: every lane has read the head before lane 0 rewrites it
                        if (lane == 0) {
                            w[0] = ser;
                            w[1 * K] = shots;
                            w[2 * K] = kept + (take ? 1 : 0);
                            if (stale || take) w[3 * K] = take ? __float_as_int(p.q ? q : 0.0f) : __float_as_int(hq);
                            if (stale) { w[4 * K] = st_lo; w[5 * K] = st_hi; w[6 * K] = 0; w[7 * K] = 0; }
                            if (take) { w[6 * K] = st_lo; w[7 * K] = st_hi; s_win[slot] = base + k; }
                            s_dirty[slot] = 1;
                        }
                        __syncthreads(); // and the next observation reads what lane 0 wrote
                    }
                }
                if (lane == k) l_status = st;
            }
            if (mine < t1) p.status[mine] = l_status;
        }
    }
    __syncthreads();
    // the heads that changed go back as two 16-byte halves; the winners become segment g of the work list, in slot order
    ShotCopyItem *items = c.items + (size_t)g * mt;
    int made = 0;
    for (int j0 = 0; j0 < mt; j0 += 64) {
        const int j = j0 + lane;
        if (s_dirty[j]) {
            const int *w = s_head + j;
            reinterpret_cast<int4 *>(heads + j)[0] = make_int4(w[0], w[1 * K], w[2 * K], w[3 * K]);
            reinterpret_cast<int4 *>(heads + j)[1] = make_int4(w[4 * K], w[5 * K], w[6 * K], w[7 * K]);
        }
        const int win = s_win[j];
        const unsigned long long bal = __ballot(win >= 0);
        if (win >= 0) items[made + tsh_lanes_below(bal)] = ShotCopyItem{win, s * mt + j};
        made += __popcll(bal);
    }
    if (lane == 0) c.seg_count[g] = made;
}

// scratch of the list kernel: cnt[n], pre[n + 1], found[n][max_tracks]
__global__ void __launch_bounds__(64 * kListWaves) track_record_list_kernel(TrackRecordListParams p)
{
    __shared__ int s_hser[kListWaves][kShotMaxTracks];
    __shared__ int s_iser[kListWaves][kShotMaxTracks];
    const TrackShotCommon &c = p.c;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n = c.n, mt = c.max_tracks;
    int32_t *cnt = p.scratch, *pre = p.scratch + n, *found = p.scratch + 2 * (size_t)n + 1;

    // phase 1: the found entries of every frame, packed in `ended` order; every wave walks the same number of rounds, so the
    // workgroup's barriers order the restaging of a wave's LDS
    for (int b0 = 0; b0 < n; b0 += kListWaves) {
        const int b = b0 + wave;
        const int s = b < n ? c.plan[b] : 0;
        if (b < n) {
            for (int j = lane; j < mt; j += 64) {
                s_hser[wave][j] = c.heads[(size_t)s * mt + j].serial;
                s_iser[wave][j] = p.id_heads ? p.id_heads[(size_t)s * mt + j].serial : 0;
            }
        }
        __syncthreads();
        if (b < n) {
            const int ne = min(max(p.stats[(size_t)b * 4 + 2], 0), mt);
            int made = 0;
            for (int base = 0; base < ne; base += 64) {
                const int e = base + lane, m = min(64, ne - base);
                const int l_ser = e < ne ? p.ended[(size_t)b * mt + e] : 0;
                int l_hit = -1;
                for (int k = 0; k < m; ++k) { // wave-uniform: one ballot per 64 heads
                    const int ser = __builtin_amdgcn_readlane(l_ser, k);
                    const int j = tsh_find(s_hser[wave], mt, lane, ser);
                    const int i = j >= 0 ? tsh_find(s_iser[wave], mt, lane, ser) : -1;
                    if (lane == k && j >= 0) l_hit = j | ((i + 1) << 16);
                }
                const unsigned long long bal = __ballot(l_hit >= 0);
                if (l_hit >= 0) found[(size_t)b * mt + made + tsh_lanes_below(bal)] = l_hit;
                made += __popcll(bal);
            }
            if (lane == 0) cnt[b] = made;
        }
        __syncthreads();
    }
    __syncthreads();
    // the prefix counts over the frames: wave 0, 64 frames at a time
    if (wave == 0) {
        int run = 0;
        for (int b0 = 0; b0 < n; b0 += 64) {
            const int b = b0 + lane;
            const int mine = b < n ? cnt[b] : 0;
            int inc = mine;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const int up = __shfl_up(inc, off, 64);
                if (lane >= off) inc += up;
            }
            if (b < n) {
                pre[b] = run + inc - mine;
                p.first[b] = run + inc - mine;
            }
            run += __shfl(inc, 63, 64);
        }
        if (lane == 0) {
            pre[n] = run;
            p.first[n] = run;
            p.total[0] = run;
            c.seg_count[0] = min(run, p.cap);
        }
    }
    __syncthreads();
    // phase 2: one record per lane
    for (int b = wave; b < n; b += kListWaves) {
        const int s = c.plan[b], r0 = pre[b], made = pre[b + 1] - r0;
        const long long end_stamp = c.stamp[b];
        for (int i = lane; i < made; i += 64) {
            const int r = r0 + i;
            if (r >= p.cap) break;
            const int hit = found[(size_t)b * mt + i], j = hit & 0xffff, ij = (hit >> 16) - 1;
            const TrackShotHead *head = c.heads + (size_t)s * mt + j;
            const int4 h0 = reinterpret_cast<const int4 *>(head)[0];
            const int4 h1 = reinterpret_cast<const int4 *>(head)[1];
            int4 i0 = make_int4(0, -1, -1, __float_as_int(-__builtin_inff())), i1 = make_int4(0, 0, 0, 0);
            if (ij >= 0) {
                i0 = reinterpret_cast<const int4 *>(p.id_heads + (size_t)s * mt + ij)[0];
                i1 = reinterpret_cast<const int4 *>(p.id_heads + (size_t)s * mt + ij)[1];
            }
            // ten 8-byte stores: a record is 8-byte aligned
            int2 *o = reinterpret_cast<int2 *>(p.rec + r);
            o[0] = make_int2(s, h0.x);       // stream, serial
            o[1] = make_int2(b, h0.y);       // frame, shots
            o[2] = make_int2(h0.z, h0.w);    // kept, q
            o[3] = make_int2(h1.x, h1.y);    // first_stamp
            o[4] = make_int2(h1.z, h1.w);    // best_stamp
            o[5] = make_int2((int)(unsigned)end_stamp, (int)(end_stamp >> 32));
            o[6] = make_int2(i0.y, i0.z);    // identity, row
            o[7] = make_int2(i0.w, i1.x);    // id_score, named
            o[8] = make_int2(i1.y, i1.z);    // id_shots, id_weight
            o[9] = make_int2(0, 0);
            c.items[r] = ShotCopyItem{s * mt + j, r};
        }
    }
}

template <class T> __device__ __forceinline__ void shot_copy_units(const uint8_t *src, uint8_t *dst, uint32_t units, int tid)
{
    for (uint32_t i = tid; i < units; i += kTrackShotCopyThreads) reinterpret_cast<T *>(dst)[i] = reinterpret_cast<const T *>(src)[i];
}

__global__ void __launch_bounds__(kTrackShotCopyThreads) shot_copy_kernel(ShotCopyParams p)
{
    // the item of this workgroup: index blockIdx.x of the segments laid end to end
    int at = blockIdx.x, seg = 0;
    for (; seg < p.segments; ++seg) {
        const int have = p.seg_count[seg];
        if (at < have) break;
        at -= have;
    }
    if (seg == p.segments) return; // at or past the device-side count: the whole workgroup leaves
    const ShotCopyItem item = p.items[(size_t)seg * p.seg_stride + at];
    const uint8_t *src_row = p.src + (size_t)item.src * p.row_bytes;
    uint8_t *dst_row = p.dst + (size_t)item.dst * p.row_bytes;
    const int path = track_shot_copy_path((uint64_t)src_row, (uint64_t)dst_row, p.row_bytes); // wave-uniform per item
    const uint32_t begin = track_shot_chunk_begin(p.row_bytes, blockIdx.y), end = track_shot_chunk_end(p.row_bytes, blockIdx.y);
    const uint8_t *src = src_row + begin;
    uint8_t *dst = dst_row + begin;
    const ShotCopySplit cut = track_shot_copy_split(path, (uint64_t)src, end - begin);
    const int tid = threadIdx.x;
    shot_copy_units<uint8_t>(src, dst, cut.head, tid);
    src += cut.head;
    dst += cut.head;
    if (path == kShotCopyVec16) shot_copy_units<uint4>(src, dst, cut.body, tid);
    else if (path == kShotCopyDword) shot_copy_units<uint32_t>(src, dst, cut.body, tid);
    src += (size_t)cut.body * cut.unit;
    dst += (size_t)cut.body * cut.unit;
    shot_copy_units<uint8_t>(src, dst, cut.tail, tid);
}

int launch_track_shot_decide(const TrackShotDecideParams &p, int groups, hipStream_t s)
{
    hipLaunchKernelGGL(track_shot_decide_kernel, dim3(groups), dim3(64), 0, s, p);
    RFD_HIP(hipGetLastError());
    return RFD_OK;
}

int launch_track_record_list(const TrackRecordListParams &p, hipStream_t s)
{
    hipLaunchKernelGGL(track_record_list_kernel, dim3(1), dim3(64 * kListWaves), 0, s, p);
    RFD_HIP(hipGetLastError());
    return RFD_OK;
}

int launch_shot_copy(const ShotCopyParams &p, int bound, hipStream_t s)
{
    if (bound < 1) return RFD_OK;
    hipLaunchKernelGGL(shot_copy_kernel, dim3(bound, track_shot_row_chunks(p.row_bytes)), dim3(kTrackShotCopyThreads), 0, s, p);
    RFD_HIP(hipGetLastError());
    return RFD_OK;
}

} // namespace rfd
