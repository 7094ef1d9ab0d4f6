// kernels_track_identity.hip -- the track identities (include/rfd.h, "track identities"; gfx950, wave64): fuse the embeddings
// of a track's shots into its template, keep the gallery's answer as the track's name, answer "who" for every detection row.
//
// Fuse and label: one workgroup of ONE wave per distinct stream of the call (track_plan's groups), walking that stream's frames
// in call order and each frame's observations in ascending t, so the observations of a stream are handled one after the other
// and no two waves ever touch the same entry.  The stream's slot serials are staged in LDS once; an observation's track is found
// with one ballot per 64 slots.  What an observation needs besides its embedding (row, serial, weight; status and the top two
// gallery entries in label) is read 64 observations at a time, one per lane, and handed on by v_readlane, and the next
// observation's embedding is read while the one in hand is fused: the chain of dependent loads per observation is the entry's
// head and template alone.  Lane l holds elements l, l + 64, ... of the embedding and of the template in registers (J of
// them, dim <= 64 J).  The head of an entry is written by lane 0 and read by every lane at the next observation, the template
// by the lane that owns the element: the barrier at the end of an observation (one wave: a wait for its stores) orders the
// two.  No atomics, nothing that depends on timing: the same bits on every run.  Every f32 operation is one pinned rounding
// (__fadd_rn ...) in the order the header writes; the normalisation is l2_normalize_kernel's (kernels_pre.hip): the same lane
// sums, the same butterfly, one division per element -- with the square root correctly rounded (tid_sqrt below).
// Latency-bound scalar work like the tracker's: the tracker exists so that due faces are few.
//
// Who: fully parallel, 256 rows per workgroup.  The workgroup stages, for its frame's stream, the serial of every slot whose
// entry is current and named (0 otherwise) with the entry's identity and score in LDS; each thread looks its row's serial up
// there with 32-bit reads.
#include "tracker_host.h"

namespace rfd {

constexpr uint32_t kTrackNamed = RFD_TRACK_NAMED;
constexpr int kTrackIdMaxTracks = 256;

__device__ __forceinline__ float tid_wave_sum(float s) // all 64 lanes active; every lane ends with the same bits
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) s = __fadd_rn(s, __shfl_xor(s, off, 64));
    return s;
}

// The correctly rounded square root: the compiler's expansion around the hardware's approximation.  __fsqrt_rn is NOT this
// on this toolchain (it is the bare hardware instruction, one ulp off for some inputs), and the header promises IEEE bits.
__device__ __forceinline__ float tid_sqrt(float v) { return __builtin_sqrtf(v); }

__device__ __forceinline__ bool tid_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

__device__ __forceinline__ int tid_count(const int32_t *total, int m) { return total ? min(max(total[0], 0), m) : m; }

// the stream's slot serials into LDS, max_tracks of them (a multiple of 64)
__device__ __forceinline__ void tid_stage_serials(const TrackIdCommon &c, int s, int lane, int *s_serial)
{
    const TrackSlot *slots = c.slots + (size_t)s * c.max_tracks;
    for (int j = lane; j < c.max_tracks; j += 64) s_serial[j] = slots[j].serial;
    __syncthreads();
}

// the lowest slot that holds serial `ser` (wave-uniform), or -1; 0 names no track
__device__ __forceinline__ int tid_find(const int *s_serial, int max_tracks, int lane, int ser)
{
    if (ser == 0) return -1;
    for (int k = 0; k < max_tracks; k += 64) {
        const unsigned long long bal = __ballot(s_serial[k + lane] == ser);
        if (bal != 0ull) return k + __builtin_ctzll(bal);
    }
    return -1;
}

// the serial of observation t of frame b (wave-uniform), 0 for a row outside the slab
__device__ __forceinline__ int tid_obs_serial(const int32_t *row, const int32_t *serial, int max_det, int b, int t)
{
    const int r = row[t];
    return (r >= 0 && r < max_det) ? serial[(size_t)b * max_det + r] : 0;
}

// lane l's elements l, l + 64, ... of a row of dim values (0 where it owns none)
template <int J> __device__ __forceinline__ void tid_load_row(const float *x, int dim, int lane, float (&v)[J])
{
#pragma unroll
    for (int j = 0; j < J; ++j) v[j] = lane + 64 * j < dim ? x[lane + 64 * j] : 0.0f;
}

template <int J> __global__ void __launch_bounds__(64) track_fuse_kernel(TrackFuseParams p)
{
    __shared__ int s_serial[kTrackIdMaxTracks];
    const int lane = threadIdx.x, g = blockIdx.x;
    const TrackIdCommon &c = p.c;
    const int32_t *group_stream = c.plan, *group_first = c.plan + c.n, *order = c.plan + 2 * (size_t)c.n + 1;
    const int s = group_stream[g], f0 = group_first[g], f1 = group_first[g + 1];
    const int dim = c.dim, count = tid_count(p.total, p.m);
    tid_stage_serials(c, s, lane, s_serial);

    for (int fi = f0; fi < f1; ++fi) {
        const int b = order[fi];
        const int t0 = max(p.first[b], 0), t1 = min(p.first[b + 1], count);
        for (int base = t0; base < t1; base += 64) { // 64 observations at a time: lane l reads what t = base + l needs
            const int mine = base + lane, cnt = min(64, t1 - base);
            int l_ser = 0;
            float l_w = 1.0f;
            if (mine < t1) {
                l_ser = tid_obs_serial(p.row, p.serial, c.max_det, b, mine);
                if (p.weight) l_w = p.weight[mine];
            }
            float nx[J]; // the embedding of the observation to come, read while the one in hand is fused
            tid_load_row<J>(p.emb + (size_t)base * dim, dim, lane, nx);
            for (int k = 0; k < cnt; ++k) {
                const int t = base + k;
                float *q = p.query + (size_t)t * dim;
                const int ser = __builtin_amdgcn_readlane(l_ser, k);
                const float w = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(l_w), k));
                // a. normalise
                float e[J];
                float ss = 0.0f;
#pragma unroll
                for (int j = 0; j < J; ++j) {
                    e[j] = nx[j];
                    if (lane + 64 * j < dim) ss = __fadd_rn(ss, __fmul_rn(e[j], e[j]));
                }
                if (k + 1 < cnt) tid_load_row<J>(p.emb + (size_t)(t + 1) * dim, dim, lane, nx);
                const float norm = tid_sqrt(tid_wave_sum(ss));
#pragma unroll
                for (int j = 0; j < J; ++j) e[j] = __fdiv_rn(e[j], norm);
                const bool bad = !(norm > 0.0f && tid_finite(norm)) || !(w > 0.0f && tid_finite(w)); // a NaN fails both comparisons
                const int slot = bad ? -1 : tid_find(s_serial, c.max_tracks, lane, ser);
                if (slot < 0) { // b, c: the query is the shot alone
#pragma unroll
                    for (int j = 0; j < J; ++j)
                        if (lane + 64 * j < dim) q[lane + 64 * j] = e[j];
                    if (lane == 0) p.status[t] = bad ? RFD_TRACK_FUSE_BAD_INPUT : RFD_TRACK_FUSE_NO_TRACK;
                    continue;
                }
                // d. fuse
                const size_t at = (size_t)s * c.max_tracks + slot;
                TrackIdHead *head = c.heads + at;
                float *S = c.templates + at * dim;
                const int4 h0 = reinterpret_cast<const int4 *>(head)[0];
                const int4 h1 = reinterpret_cast<const int4 *>(head)[1];
                const bool stale = h0.x != ser;
                float acc[J];
                float s2 = 0.0f;
#pragma unroll
                for (int j = 0; j < J; ++j) {
                    const int i = lane + 64 * j;
                    acc[j] = 0.0f;
                    if (i < dim) {
                        const float old = stale ? 0.0f : S[i];
                        acc[j] = __fadd_rn(old, __fmul_rn(w, e[j]));
                        S[i] = acc[j];
                        s2 = __fadd_rn(s2, __fmul_rn(acc[j], acc[j]));
                    }
                }
                if (lane == 0) {
                    const int shots = (stale ? 0 : h1.y) + 1;
                    const float weight = __fadd_rn(stale ? 0.0f : __int_as_float(h1.z), w);
                    reinterpret_cast<int4 *>(head)[0] =
                        stale ? make_int4(ser, -1, -1, __float_as_int(-__builtin_inff())) : h0;
                    reinterpret_cast<int4 *>(head)[1] = make_int4(stale ? 0 : h1.x, shots, __float_as_int(weight), 0);
                }
                const float n2 = tid_sqrt(tid_wave_sum(s2));
#pragma unroll
                for (int j = 0; j < J; ++j)
                    if (lane + 64 * j < dim) q[lane + 64 * j] = __fdiv_rn(acc[j], n2);
                if (lane == 0) p.status[t] = tid_finite(n2) ? RFD_TRACK_FUSE_OK : RFD_TRACK_FUSE_OVERFLOW;
                __syncthreads(); // one wave: the head and template stores have landed before the next observation reads them
            }
        }
    }
}

__global__ void __launch_bounds__(64) track_label_kernel(TrackLabelParams p)
{
    __shared__ int s_serial[kTrackIdMaxTracks];
    const int lane = threadIdx.x, g = blockIdx.x;
    const TrackIdCommon &c = p.c;
    const int32_t *group_stream = c.plan, *group_first = c.plan + c.n, *order = c.plan + 2 * (size_t)c.n + 1;
    const int s = group_stream[g], f0 = group_first[g], f1 = group_first[g + 1];
    const int count = tid_count(p.total, p.m), k = p.k;
    tid_stage_serials(c, s, lane, s_serial);

    for (int fi = f0; fi < f1; ++fi) {
        const int b = order[fi];
        const int t0 = max(p.first[b], 0), t1 = min(p.first[b + 1], count);
        for (int base = t0; base < t1; base += 64) { // 64 observations at a time: lane l reads what t = base + l needs
            const int mine = base + lane, cnt = min(64, t1 - base);
            int l_status = 1, l_ser = 0, l_top_row = -1, l_top_id = -1, l_run_row = -1;
            float l_top = 0.0f, l_run = 0.0f;
            if (mine < t1) {
                l_status = p.status_in[mine];
                l_ser = tid_obs_serial(p.row, p.serial, c.max_det, b, mine);
                const size_t at = (size_t)mine * k;
                l_top = p.scores[at];
                l_top_row = p.rows[at];
                if (p.ids) l_top_id = p.ids[at];
                if (k >= 2) {
                    l_run = p.scores[at + 1];
                    l_run_row = p.rows[at + 1];
                }
            }
            for (int j = 0; j < cnt; ++j) { // everything below is wave-uniform: every lane computes the same entry
                if (__builtin_amdgcn_readlane(l_status, j) != 0) continue;
                const int ser = __builtin_amdgcn_readlane(l_ser, j);
                const int slot = tid_find(s_serial, c.max_tracks, lane, ser);
                if (slot < 0) continue;
                TrackIdHead *head = c.heads + (size_t)s * c.max_tracks + slot;
                const int4 h0 = reinterpret_cast<const int4 *>(head)[0];
                const int named = head->named;
                if (h0.x != ser) continue; // stale: this track was never fused
                const float top = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(l_top), j));
                const float run = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(l_run), j));
                const int top_row = __builtin_amdgcn_readlane(l_top_row, j), top_id = __builtin_amdgcn_readlane(l_top_id, j);
                const bool top_ok = !(top_row == -1 || top != top);
                const bool run_ok = k >= 2 && !(__builtin_amdgcn_readlane(l_run_row, j) == -1 || run != run);
                bool keep = false;
                if (named != 0) {
                    const bool same = h0.y >= 0 ? top_id == h0.y : top_row == h0.z;
                    keep = top_ok && same && top >= p.release;
                }
                const bool take = keep || (top_ok && top >= p.accept && (!run_ok || __fsub_rn(top, run) >= p.margin));
                if (lane == 0) {
                    // a kept name holds its identity; its row and score are refreshed
                    const int4 now = take ? make_int4(ser, keep ? h0.y : top_id, top_row, __float_as_int(top))
                                          : make_int4(ser, -1, -1, __float_as_int(-__builtin_inff()));
                    reinterpret_cast<int4 *>(head)[0] = now;
                    head->named = take ? 1 : 0;
                }
                __syncthreads(); // one wave: the head's stores have landed before the next observation reads it
            }
        }
    }
}

__global__ void __launch_bounds__(256) track_who_kernel(TrackWhoParams p)
{
    __shared__ int s_key[kTrackIdMaxTracks];
    __shared__ int s_ident[kTrackIdMaxTracks];
    __shared__ float s_score[kTrackIdMaxTracks];
    const TrackIdCommon &c = p.c;
    const int b = blockIdx.y, tid = threadIdx.x;
    const int cnt = min(max(p.count[b], 0), c.max_det);
    if ((int)blockIdx.x * 256 >= cnt) return; // the whole workgroup leaves together
    const int s = c.plan[b];
    if (tid < c.max_tracks) {
        const size_t at = (size_t)s * c.max_tracks + tid;
        const int live = c.slots[at].serial;
        const int4 h0 = reinterpret_cast<const int4 *>(c.heads + at)[0];
        const bool ok = live != 0 && h0.x == live && c.heads[at].named != 0;
        s_key[tid] = ok ? live : 0;
        s_ident[tid] = h0.y;
        s_score[tid] = __int_as_float(h0.w);
    }
    __syncthreads();
    const int i = blockIdx.x * 256 + tid;
    if (i >= cnt) return;
    const size_t at = (size_t)b * c.max_det + i;
    const int tr = p.track[at];
    int found = -1;
    if (tr != 0) {
#pragma unroll 1
        for (int j = 0; j < c.max_tracks; ++j)
            if (s_key[j] == tr) { found = j; break; } // the lowest slot
    }
    const uint32_t f = p.flags_in ? p.flags_in[at] : 0u;
    p.who[at] = f | (found >= 0 ? kTrackNamed : 0u);
    if (p.identity) p.identity[at] = found >= 0 ? s_ident[found] : -1;
    if (p.id_score) p.id_score[at] = found >= 0 ? s_score[found] : -__builtin_inff();
}

int launch_track_fuse(const TrackFuseParams &p, int groups, hipStream_t s)
{
    switch (track_identity_lane_elems(p.c.dim)) {
    case 1: hipLaunchKernelGGL(track_fuse_kernel<1>, dim3(groups), dim3(64), 0, s, p); break;
    case 2: hipLaunchKernelGGL(track_fuse_kernel<2>, dim3(groups), dim3(64), 0, s, p); break;
    case 4: hipLaunchKernelGGL(track_fuse_kernel<4>, dim3(groups), dim3(64), 0, s, p); break;
    case 8: hipLaunchKernelGGL(track_fuse_kernel<8>, dim3(groups), dim3(64), 0, s, p); break;
    case 16: hipLaunchKernelGGL(track_fuse_kernel<16>, dim3(groups), dim3(64), 0, s, p); break;
    default: set_error("track identities: dim %d has no kernel", p.c.dim); return RFD_ERR_INVALID_ARG;
    }
    RFD_HIP(hipGetLastError());
    return RFD_OK;
}

int launch_track_label(const TrackLabelParams &p, int groups, hipStream_t s)
{
    hipLaunchKernelGGL(track_label_kernel, dim3(groups), dim3(64), 0, s, p);
    RFD_HIP(hipGetLastError());
    return RFD_OK;
}

int launch_track_who(const TrackWhoParams &p, hipStream_t s)
{
    hipLaunchKernelGGL(track_who_kernel, dim3((p.c.max_det + 255) / 256, p.c.n), dim3(256), 0, s, p);
    RFD_HIP(hipGetLastError());
    return RFD_OK;
}

} // namespace rfd
