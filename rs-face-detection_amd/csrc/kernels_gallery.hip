// kernels_gallery.hip -- the on-device face gallery (include/rfd.h, "gallery"): enrol L2-normalised embeddings as bf16, score a
// batch of queries against every enrolled row on the matrix cores, keep the k best rows per query.
//
// Storage (gallery_offset, kernels.h): MFMA-fragment-major.  Rows in blocks of 16; inside a block, for each 32-wide K step, the 64
// lanes' 16-byte B operands of v_mfma_f32_16x16x32_bf16 lie contiguously (lane l: row l & 15, elements 8 * (l >> 4) .. + 7), so a
// wave reads one (block, K step) with ONE coalesced 1 KiB global_load_dwordx4 and the gallery never passes through LDS.
//
// Search: one pass over the gallery for up to 32 queries.  The queries are rounded to bf16 once per workgroup and kept in LDS as A
// fragments (two 8-byte halves per lane, so every LDS read is 64 bits and conflict-free).  Each wave walks row blocks at a grid
// stride with kGalleryPrefetch K steps (1 KiB each) of loads in flight; per block it issues dim / 32 MFMAs per M-tile into one
// accumulator, K ascending -- a (query, row) score therefore has the same bits wherever the row and the query sit.  C mapping:
// lane & 15 = gallery row of the block, 4 * (lane >> 4) + reg = query of the M-tile.
// Selection: every wave keeps, per query, a list of its k best (score, row) keys in LDS, sorted by (score descending, row
// ascending); the list's last key is the filter, one compare rejects nearly every score, and what passes is inserted by the whole
// wave (one lane per list entry).  No wave touches another wave's list, so the scan needs no barrier, no atomic and no wait.  At
// the end one barrier, the four lists of a query are merged, and the workgroup writes k keys per query to the workspace
// [groups][n][k]; gallery_merge_kernel reduces the groups' lists per query with the same two routines.  The order is total (rows
// are unique), so the result does not depend on which wave or workgroup scored a row.
//
// Identity search (rfd.h, "identities"): rows carry an int32 identity in HBM (-1: a row of its own); the IDENT instantiations of the
// scan and gallery_merge_identities_kernel keep the k best IDENTITIES, each under its best row's key, with the same lists plus one
// identity word per key in LDS, so a list entry's identity never has to be fetched again and a sentinel never indexes the array.
// The scan reads the identities of a block's 16 rows (64 bytes) only if a key of the block passes a list's filter.
// Why the two-level reduction stays exact: an identity of the global top k has its best key in the rows of some wave.  In that
// wave's list it is among the k best distinct identities -- were it not, k other identities of that wave alone would hold keys
// better than its best key, and the same k identities would beat it globally.  A later row of the identity in that wave cannot
// push it out either: it only replaces the identity's key by a better one.  The same holds one level up for a workgroup's merged
// list among the workgroups, so every level may drop all but its k best distinct identities.
//
// Filtered search (rfd.h, "tags"): rows carry a uint32 tag in HBM, and every query of a pass its own (mask, value); row r counts
// for query q iff (tag[r] & mask[q]) == value[q].  The TAGGED instantiations of the scan keep the pass's pairs in LDS next to the
// A fragments and read a block's 16 tags where they read its identities, in a block with a key that passes a list's filter; the
// eligibility is one more term of the predicate a key is offered under.  The merges are unchanged: they see eligible keys only,
// and the argument above holds per query with "live and eligible for the query" in place of "live", because the set of rows
// that count for a query is fixed for the whole pass and every level reduces keys of that one set.
#include "conv_device.h"

namespace rfd {

namespace {

constexpr int kGalleryWaves = 4;     // waves per workgroup (search and merge)
constexpr int kGalleryPrefetch = 8;  // K steps of gallery loads a wave keeps in flight: 8 KiB per wave, 64 KiB per CU at two workgroups

__device__ __forceinline__ uint2 gallery_sentinel() { return make_uint2(0xff800000u, 0xffffffffu); } // score -inf, row -1

// the total order of the results: score descending, then row ascending.  False whenever a score is NaN.
__device__ __forceinline__ bool key_better(float s, int r, float s2, int r2) { return s > s2 || (s == s2 && r < r2); }

// Inserts the wave-uniform key (cs, crow) into the sorted list of k <= 64 keys; the whole wave calls it, lane i owns entry i.
// LDS operations of one wave execute in order, so every lane's reads are done before any lane's write.
__device__ __forceinline__ void list_insert(uint2 *list, int k, float cs, int crow, int lane)
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    const bool in = lane < k;
    uint2 e = gallery_sentinel(), ep = e;
    if (in) {
        e = list[lane];
        if (lane > 0) ep = list[lane - 1];
    }
    const bool ahead = in && key_better(__uint_as_float(e.x), (int)e.y, cs, crow);
    const int pos = __popcll(__ballot(ahead)); // the list is sorted: the keys ahead of the new one are its first `pos`
    if (in && lane >= pos) list[lane] = lane == pos ? make_uint2(__float_as_uint(cs), (uint32_t)crow) : ep;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
}

// Offers every lane's key (s, row) to list `li` of the wave's lists (k keys each); `valid` masks lanes without a key.  The last key
// of a list is its filter; a key that passes is inserted by the whole wave, lowest lane first.  Called with all 64 lanes.
__device__ __forceinline__ void list_offer(uint2 *lists, int li, int k, float s, int row, bool valid, int lane)
{
    bool pass = false;
    if (valid) {
        const uint2 t = lists[li * k + k - 1];
        pass = key_better(s, row, __uint_as_float(t.x), (int)t.y);
    }
    unsigned long long m = __ballot(pass);
    while (m) {
        const int l = __ffsll(m) - 1;
        m &= m - 1;
        list_insert(lists + __builtin_amdgcn_readlane(li, l) * k, k, __int_as_float(__builtin_amdgcn_readlane(__float_as_int(s), l)),
                    __builtin_amdgcn_readlane(row, l), lane);
    }
}

// k best keys of the kGalleryWaves sorted lists at lists + w * wave_pitch, in order, handed to out(j, key); one thread.
template <class Out>
__device__ __forceinline__ void merge_wave_lists(const uint2 *lists, int wave_pitch, int k, Out out)
{
    int h0 = 0, h1 = 0, h2 = 0, h3 = 0;
    for (int j = 0; j < k; ++j) {
        // a list has k keys and j < k heads have been taken in all, so every head index is < k
        const uint2 e0 = lists[h0], e1 = lists[wave_pitch + h1], e2 = lists[2 * wave_pitch + h2], e3 = lists[3 * wave_pitch + h3];
        uint2 b = e0;
        int bi = 0;
        if (key_better(__uint_as_float(e1.x), (int)e1.y, __uint_as_float(b.x), (int)b.y)) { b = e1; bi = 1; }
        if (key_better(__uint_as_float(e2.x), (int)e2.y, __uint_as_float(b.x), (int)b.y)) { b = e2; bi = 2; }
        if (key_better(__uint_as_float(e3.x), (int)e3.y, __uint_as_float(b.x), (int)b.y)) { b = e3; bi = 3; }
        out(j, b);
        h0 += bi == 0; h1 += bi == 1; h2 += bi == 2; h3 += bi == 3;
    }
}

template <class T, class... Rest>
__device__ __forceinline__ T pack_first(T first, Rest...) { return first; }
template <class T>
__device__ __forceinline__ T pack_last(T last) { return last; }
template <class T, class... Rest>
__device__ __forceinline__ auto pack_last(T, Rest... rest) { return pack_last(rest...); }
template <int I, class T, class... Rest>
__device__ __forceinline__ auto pack_at(T first, Rest... rest)
{
    if constexpr (I == 0) return first;
    else return pack_at<I - 1>(rest...);
}

// ---- the identity forms of the three routines above.  A list holds no identity >= 0 twice; lid[i] is the identity of list[i]
//      (-1 for an unlabelled row and for the sentinel, which never equals a candidate's identity >= 0). ----

// list_insert with the candidate's identity c.  An entry of identity c >= 0 ahead of the new key rejects it; one behind it, at p,
// is the entry the new key replaces: it goes in at pos <= p and only [pos, p] shifts.  Without such an entry p is the last index
// and this is list_insert.  At most one lane can hold c (the invariant), and the invariant holds afterwards: c is in the list once.
__device__ __forceinline__ void list_insert_ident(uint2 *list, int32_t *lid, int k, float cs, int crow, int c, int lane)
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    const bool in = lane < k;
    uint2 e = gallery_sentinel(), ep = e;
    int id = -1, idp = -1;
    if (in) {
        e = list[lane];
        id = lid[lane];
        if (lane > 0) { ep = list[lane - 1]; idp = lid[lane - 1]; }
    }
    const bool ahead = in && key_better(__uint_as_float(e.x), (int)e.y, cs, crow);
    const int pos = __popcll(__ballot(ahead));
    const unsigned long long same = __ballot(in && c >= 0 && id == c);
    const int p = same ? __ffsll(same) - 1 : k - 1; // p < pos: the listed key of c is the better one (or the list is full of better keys)
    if (in && lane >= pos && lane <= p) {
        list[lane] = lane == pos ? make_uint2(__float_as_uint(cs), (uint32_t)crow) : ep;
        lid[lane] = lane == pos ? c : idp;
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
}

// list_offer for identities; c is the identity of the lane's row (read by the caller; unused where !valid).  The last key is
// still a correct filter: a key worse than the last key of a full list either repeats a listed identity, whose listed key is
// then the better one, or loses to k distinct identities; a list that is not full ends in the sentinel, which every key of a
// valid lane beats.
__device__ __forceinline__ void list_offer_ident(uint2 *lists, int32_t *lids, int li, int k, float s, int row, int c, bool valid, int lane)
{
    bool pass = false;
    if (valid) {
        const uint2 t = lists[li * k + k - 1];
        pass = key_better(s, row, __uint_as_float(t.x), (int)t.y);
    }
    unsigned long long m = __ballot(pass);
    while (m) {
        const int l = __ffsll(m) - 1;
        m &= m - 1;
        const int at = __builtin_amdgcn_readlane(li, l) * k;
        list_insert_ident(lists + at, lids + at, k, __int_as_float(__builtin_amdgcn_readlane(__float_as_int(s), l)), __builtin_amdgcn_readlane(row, l),
                          __builtin_amdgcn_readlane(c, l), lane);
    }
}

// merge_wave_lists for identities: the k best keys of distinct identities, handed to out(j, key, identity); one thread.  A head
// whose identity was already emitted is skipped.  Head indices: every key taken from a list is either emitted or skipped because
// its identity is in the output, and a list holds k distinct identities (unlabelled keys and sentinels are never skipped), so a
// list is exhausted only once k keys are out: every head index is < k while fewer than k keys are emitted.  The emitted
// identities stay in registers (k <= 32).
template <class Out>
__device__ __forceinline__ void merge_wave_lists_ident(const uint2 *lists, const int32_t *lids, int wave_pitch, int k, Out out)
{
    static_assert(RFD_GALLERY_MAX_K == 32, "the emitted identities are kept in 32 registers");
    int seen[32];
#pragma unroll
    for (int t = 0; t < 32; ++t) seen[t] = -1;
    int h0 = 0, h1 = 0, h2 = 0, h3 = 0;
    for (int j = 0; j < k;) {
        const uint2 e0 = lists[h0], e1 = lists[wave_pitch + h1], e2 = lists[2 * wave_pitch + h2], e3 = lists[3 * wave_pitch + h3];
        uint2 b = e0;
        int bi = 0;
        if (key_better(__uint_as_float(e1.x), (int)e1.y, __uint_as_float(b.x), (int)b.y)) { b = e1; bi = 1; }
        if (key_better(__uint_as_float(e2.x), (int)e2.y, __uint_as_float(b.x), (int)b.y)) { b = e2; bi = 2; }
        if (key_better(__uint_as_float(e3.x), (int)e3.y, __uint_as_float(b.x), (int)b.y)) { b = e3; bi = 3; }
        const int id = lids[bi * wave_pitch + (bi == 0 ? h0 : bi == 1 ? h1 : bi == 2 ? h2 : h3)];
        h0 += bi == 0; h1 += bi == 1; h2 += bi == 2; h3 += bi == 3;
        bool emitted = false;
#pragma unroll
        for (int t = 0; t < 32; ++t) emitted |= seen[t] == id;
        if (id >= 0 && emitted) continue;
#pragma unroll
        for (int t = 0; t < 32; ++t) seen[t] = t == j ? id : seen[t];
        out(j, b, id);
        ++j;
    }
}

} // namespace

// ---- add: f32 -> bf16 (RNE), scattered into the fragment-major layout.  One thread per 16-byte operand. ----
__global__ void __launch_bounds__(256) gallery_add_kernel(const float *__restrict__ emb, int n, int dim, int row0, bf16_t *__restrict__ store)
{
    const int per_row = dim >> 3;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)n * per_row) return;
    const int r = (int)(i / per_row), d = (int)(i - (size_t)r * per_row) * 8;
    const float4 a = *reinterpret_cast<const float4 *>(emb + (size_t)r * dim + d), b = *reinterpret_cast<const float4 *>(emb + (size_t)r * dim + d + 4);
    const uint2 lo = pack_bf16x4(a.x, a.y, a.z, a.w), hi = pack_bf16x4(b.x, b.y, b.z, b.w);
    *reinterpret_cast<uint4 *>(store + gallery_offset(dim, row0 + r, d)) = make_uint4(lo.x, lo.y, hi.x, hi.y);
}

int launch_gallery_add(const float *emb, int n, int dim, int row0, bf16_t *store, hipStream_t s)
{
    const size_t items = (size_t)n * (dim >> 3);
    hipLaunchKernelGGL(gallery_add_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, s, emb, n, dim, row0, store);
    RFD_HIP(hipGetLastError());
    return RFD_OK;
}

// ---- get: the stored bf16 values of rows [row0, row0 + n) as f32 [n][dim] ----
__global__ void __launch_bounds__(256) gallery_get_kernel(const bf16_t *__restrict__ store, int row0, int n, int dim, float *__restrict__ out)
{
    const int per_row = dim >> 3;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)n * per_row) return;
    const int r = (int)(i / per_row), d = (int)(i - (size_t)r * per_row) * 8;
    const uint4 v = *reinterpret_cast<const uint4 *>(store + gallery_offset(dim, row0 + r, d));
    float4 *o = reinterpret_cast<float4 *>(out + (size_t)r * dim + d);
    o[0] = make_float4(bf16_bits_to_f32(v.x & 0xffffu), bf16_bits_to_f32(v.x >> 16), bf16_bits_to_f32(v.y & 0xffffu), bf16_bits_to_f32(v.y >> 16));
    o[1] = make_float4(bf16_bits_to_f32(v.z & 0xffffu), bf16_bits_to_f32(v.z >> 16), bf16_bits_to_f32(v.w & 0xffffu), bf16_bits_to_f32(v.w >> 16));
}

int launch_gallery_get(const bf16_t *store, int row0, int n, int dim, float *out, hipStream_t s)
{
    const size_t items = (size_t)n * (dim >> 3);
    hipLaunchKernelGGL(gallery_get_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, s, store, row0, n, dim, out);
    RFD_HIP(hipGetLastError());
    return RFD_OK;
}

// ---- search: n <= 16 * NMT queries against rows [0, rows); writes ws[blockIdx.x][n][k] ----
// MASKED: rows whose bit in `live` (one 16-bit word per row block; an even number of words is allocated) is clear are scored and
// then never offered to a list.  Every K step loads the aligned 32 bits that hold its block's word right behind its operand,
// kGalleryPrefetch steps ahead, into a register that travels with the operand; the step reads it back into a scalar register
// before it issues the next loads, and a block's last step takes the row's bit from it.  Forms that made the compiler wait for
// every load in flight (vmcnt(0)) inside the loop, which this one does not: loading with the last K step alone (the word becomes
// a value merged from two paths, and all words are copied at every step); loading 16 bits (the words are zero-extended, or packed
// in pairs, at the loop's back edge); using the word after the next loads were issued (old and new value live side by side and
// are copied at the back edge).  The words' address is the last member of the pack `Live` of a MASKED instantiation; without
// MASKED and IDENT the pack is empty, so that instantiation has the arguments and the code of the scan as it was.
// IDENT: the identity scan.  The pack then begins with the identity array (one int32 per row), the lists carry an identity word
// per key behind them in LDS, and the selection goes through the identity forms of the list routines; the MFMA loop, the
// prefetch and the `any` pre-check are the same code.  Without IDENT nothing of this is instantiated.
// TAGGED: the filtered scan.  Behind the identity array (if any) the pack then holds the tag array (one uint32 per row, whole
// blocks of 16) and the pass's masks and values (device, [n] each).  The pairs lie in LDS behind the A fragments, one uint2 per
// query, and are read there as 64-bit broadcasts (the 16 lanes of a group hold the same four queries): held in registers they
// would take 8 * NMT VGPRs that the NMT = 2 instantiations do not have.  The tags of a block are read like its identities, by
// scalar loads inside the `any` branch.  A second ballot, over "eligible and passes its list's filter", then skips the offers
// of a block with nothing eligible in it: a small tenant's lists stay at the sentinel, so every block passes the first one.
// The MFMA loop, the prefetch and the live words are the same code.  Without TAGGED nothing of this is instantiated.
template <int NMT, bool MASKED, bool IDENT, bool TAGGED, class... Live>
__global__ void __launch_bounds__(kGalleryWaves * 64) gallery_search_kernel(const bf16_t *__restrict__ store, int rows, int ksteps,
                                                                             const float *__restrict__ queries, int n, int k,
                                                                             uint2 *__restrict__ ws, Live... live)
{
    static_assert(sizeof...(Live) == (IDENT ? 1 : 0) + (TAGGED ? 3 : 0) + (MASKED ? 1 : 0),
                  "an identity scan takes the identities, a filtered scan the tags, masks and values behind them, a masked scan the live words last");
    extern __shared__ __attribute__((aligned(16))) unsigned char gallery_smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6); // scalar: the walk below is wave-uniform
    const int dim = ksteps * 32, quads = dim >> 2;
    uint2 *afrag = reinterpret_cast<uint2 *>(gallery_smem);  // [NMT][ksteps][2 halves][64 lanes] x 4 bf16
    [[maybe_unused]] uint2 *filt = afrag + NMT * ksteps * 128; // TAGGED: [NMT * 16 queries] (mask, value)
    uint2 *lists = afrag + NMT * ksteps * 128 + (TAGGED ? NMT * 16 : 0); // [waves][NMT * 16 queries][k]
    uint2 *mine = lists + wave * (NMT * 16 * k);
    [[maybe_unused]] int32_t *lids = nullptr, *mine_ids = nullptr;  // IDENT: [waves][NMT * 16 queries][k] identities of the keys
    [[maybe_unused]] const int32_t *ids = nullptr;
    if constexpr (IDENT) {
        lids = reinterpret_cast<int32_t *>(lists + kGalleryWaves * NMT * 16 * k);
        mine_ids = lids + wave * (NMT * 16 * k);
        ids = pack_first(live...);
    }
    [[maybe_unused]] const uint32_t *tags = nullptr;
    if constexpr (TAGGED) {
        constexpr int at = IDENT ? 1 : 0;
        tags = pack_at<at>(live...);
        const uint32_t *fmask = pack_at<at + 1>(live...), *fvalue = pack_at<at + 2>(live...);
        // a query beyond n is never offered; its pair (0, 1) matches no tag
        if (tid < NMT * 16) filt[tid] = tid < n ? make_uint2(fmask[tid], fvalue[tid]) : make_uint2(0u, 1u);
    }

    // queries -> bf16 A fragments: lane (q & 15) + 16 * ((d & 31) >> 3) of K step d >> 5 holds elements d & ~7 .. + 7 of query q
    for (int i = tid; i < NMT * 16 * quads; i += kGalleryWaves * 64) {
        const int q = i / quads, d = (i - q * quads) * 4;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (q < n) v = *reinterpret_cast<const float4 *>(queries + (size_t)q * dim + d);
        afrag[(((q >> 4) * ksteps + (d >> 5)) * 2 + ((d & 7) >> 2)) * 64 + (q & 15) + 16 * ((d & 31) >> 3)] = pack_bf16x4(v.x, v.y, v.z, v.w);
    }
    for (int i = lane; i < NMT * 16 * k; i += 64) mine[i] = gallery_sentinel();
    if constexpr (IDENT)
        for (int i = lane; i < NMT * 16 * k; i += 64) mine_ids[i] = -1;
    __syncthreads();

    const int nblocks = (rows + 15) >> 4;
    const int stride = gridDim.x * kGalleryWaves;
    int blk = blockIdx.x * kGalleryWaves + wave, ks = 0; // the step the MFMAs are at
    if (blk < nblocks) {                                 // wave-uniform
        int pblk = blk, pks = 0;                         // the step the loads are at
        const uint4 *src = reinterpret_cast<const uint4 *>(store) + lane;
        uint4 buf[kGalleryPrefetch];
        // MASKED: a zero the compiler takes for a per-lane value.  With it in the address the words are fetched by vector loads,
        // which return in order behind the operand loads and are waited for by count (vmcnt) at their use; the scalar load that a
        // wave-uniform address gets instead is waited for by the lgkmcnt(0) in front of the very next LDS read.
        int lane_zero = 0;
        if constexpr (MASKED) asm("v_mov_b32 %0, 0" : "=v"(lane_zero));
        uint32_t lw[kGalleryPrefetch] = {}; // MASKED: lw[i] = the live words of the block whose K step is in buf[i] and of its neighbour
        // Loads beyond the wave's last block re-read its last in-range block (never out of bounds); their MFMAs run and are dropped.
        auto issue = [&](uint4 &dst, uint32_t &words) {
            const int b = pblk < nblocks ? pblk : nblocks - 1;
            dst = src[((size_t)b * ksteps + pks) * 64];
            if constexpr (MASKED) words = reinterpret_cast<const uint32_t *>(pack_last(live...))[(b >> 1) + lane_zero];
            if (++pks == ksteps) { pks = 0; pblk += stride; }
        };
#pragma unroll
        for (int i = 0; i < kGalleryPrefetch; ++i) {
            issue(buf[i], lw[i]);
            __builtin_amdgcn_sched_barrier(0); // keep the issue order: the loop waits for buf[0] with the other loads still in flight
        }
        f32x4 acc[NMT];
#pragma unroll
        for (int mt = 0; mt < NMT; ++mt) acc[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
        while (blk < nblocks) {
#pragma unroll
            for (int i = 0; i < kGalleryPrefetch; ++i) {
                const bf16x8 b = __builtin_bit_cast(bf16x8, buf[i]);
                // before issue() loads lw[i] anew; their load was issued right behind buf[i]'s, which the MFMAs below wait for
                uint32_t words = 0;
                if constexpr (MASKED) words = __builtin_amdgcn_readfirstlane(lw[i]);
#pragma unroll
                for (int mt = 0; mt < NMT; ++mt) {
                    const uint2 lo = afrag[((mt * ksteps + ks) * 2 + 0) * 64 + lane], hi = afrag[((mt * ksteps + ks) * 2 + 1) * 64 + lane];
                    acc[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, make_uint4(lo.x, lo.y, hi.x, hi.y)), b, acc[mt], 0, 0, 0);
                }
                issue(buf[i], lw[i]);
                if (++ks == ksteps) {
                    if (blk < nblocks) {
                        const int row = blk * 16 + (lane & 15);
                        bool row_ok = row < rows;
                        if constexpr (MASKED) row_ok = row_ok && ((words >> (16 * (blk & 1) + (lane & 15))) & 1u);
                        // the common case, no score of the block passes its list's filter, costs the compares and one branch
                        bool any = false;
#pragma unroll
                        for (int mt = 0; mt < NMT; ++mt)
#pragma unroll
                            for (int r = 0; r < 4; ++r) {
                                const int q = mt * 16 + 4 * (lane >> 4) + r;
                                if (row_ok && q < n) {
                                    const uint2 t = mine[q * k + k - 1];
                                    any |= key_better(acc[mt][r], row, __uint_as_float(t.x), (int)t.y);
                                }
                            }
                        if (__ballot(any)) {
                            // IDENT: the identities of the block's 16 rows, read once for all its offers and only here, in a
                            // block with a key that passes a filter: one wait per such block.
                            // The address is wave-uniform, so these are scalar loads (the array has 16 words per block, also
                            // for a partial last block): they are waited for by lgkmcnt like the LDS reads around them.  A
                            // per-lane ids[row] is a vector load in a branch, behind which the compiler no longer counts the
                            // operand loads in flight and waits for all of them (vmcnt(0)) at every K step of the loop.
                            [[maybe_unused]] int cid = -1;
                            if constexpr (IDENT) {
                                const int32_t *block_ids = ids + (size_t)__builtin_amdgcn_readfirstlane(blk) * 16;
#pragma unroll
                                for (int i = 0; i < 16; ++i) {
                                    const int v = block_ids[i];
                                    cid = (lane & 15) == i ? v : cid;
                                }
                            }
                            // TAGGED: the tags of the block's 16 rows, read like the identities and with them (one wait for
                            // both); bit 4 mt + r of `elig` = the lane's row is live and eligible for its query of (mt, r).
                            [[maybe_unused]] uint32_t elig = 0;
                            [[maybe_unused]] bool offer = true;
                            if constexpr (TAGGED) {
                                const uint32_t *block_tags = tags + (size_t)__builtin_amdgcn_readfirstlane(blk) * 16;
                                uint32_t tag = 0;
#pragma unroll
                                for (int i = 0; i < 16; ++i) {
                                    const uint32_t v = block_tags[i];
                                    tag = (lane & 15) == i ? v : tag;
                                }
                                bool any_eligible = false;
#pragma unroll
                                for (int mt = 0; mt < NMT; ++mt)
#pragma unroll
                                    for (int r = 0; r < 4; ++r) {
                                        const int q = mt * 16 + 4 * (lane >> 4) + r;
                                        const uint2 f = filt[q];
                                        if (row_ok && q < n && (tag & f.x) == f.y) {
                                            elig |= 1u << (4 * mt + r);
                                            const uint2 t = mine[q * k + k - 1];
                                            any_eligible |= key_better(acc[mt][r], row, __uint_as_float(t.x), (int)t.y);
                                        }
                                    }
                                offer = __ballot(any_eligible) != 0; // wave-uniform
                            }
                            if (offer) {
#pragma unroll
                                for (int mt = 0; mt < NMT; ++mt)
#pragma unroll
                                    for (int r = 0; r < 4; ++r) {
                                        const int q = mt * 16 + 4 * (lane >> 4) + r;
                                        bool valid = row_ok && q < n;
                                        if constexpr (TAGGED) valid = (elig >> (4 * mt + r)) & 1u;
                                        if constexpr (IDENT) list_offer_ident(mine, mine_ids, q, k, acc[mt][r], row, cid, valid, lane);
                                        else list_offer(mine, q, k, acc[mt][r], row, valid, lane);
                                    }
                            }
                        }
                    }
#pragma unroll
                    for (int mt = 0; mt < NMT; ++mt) acc[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
                    ks = 0;
                    blk += stride;
                }
            }
        }
    }
    __syncthreads();
    if (tid < n) {
        uint2 *dst = ws + ((size_t)blockIdx.x * n + tid) * k;
        // IDENT: the workspace keeps keys alone; the merge kernel reads the identities of the few keys it is handed once more
        if constexpr (IDENT) merge_wave_lists_ident(lists + tid * k, lids + tid * k, NMT * 16 * k, k, [&](int j, uint2 key, int) { dst[j] = key; });
        else merge_wave_lists(lists + tid * k, NMT * 16 * k, k, [&](int j, uint2 key) { dst[j] = key; });
    }
}

// ---- merge: one workgroup per query reduces the groups' lists ws[groups][n][k] to scores / rows [n][k] ----
__global__ void __launch_bounds__(kGalleryWaves * 64) gallery_merge_kernel(const uint2 *__restrict__ ws, int groups, int n, int k,
                                                                            float *__restrict__ scores, int32_t *__restrict__ out_rows)
{
    __shared__ uint2 lists[kGalleryWaves * 32];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), q = blockIdx.x;
    uint2 *mine = lists + wave * k;
    if (lane < k) mine[lane] = gallery_sentinel();
    const int total = groups * k;
    for (int base = wave * 64; base < total; base += kGalleryWaves * 64) { // wave-uniform bounds: list_offer runs with all lanes
        const int idx = base + lane;
        uint2 c = gallery_sentinel();
        if (idx < total) {
            const int g = idx / k, j = idx - g * k;
            c = ws[((size_t)g * n + q) * k + j];
        }
        list_offer(mine, 0, k, __uint_as_float(c.x), (int)c.y, (int)c.y >= 0, lane);
    }
    __syncthreads();
    if (tid == 0)
        merge_wave_lists(lists, k, k, [&](int j, uint2 key) {
            scores[(size_t)q * k + j] = __uint_as_float(key.x);
            out_rows[(size_t)q * k + j] = (int32_t)key.y;
        });
}

int gallery_search_groups(int rows, int groups_max)
{
    // at least two row blocks per wave before another workgroup (and its conversion of the queries) is worth starting
    const int nblocks = (rows + 15) / 16;
    return std::max(1, std::min(groups_max, ceil_div(nblocks, kGalleryWaves * 2)));
}

using GalleryLiveWords = const uint16_t *__restrict__;
using GalleryIdentities = const int32_t *__restrict__;
using GalleryTags = const uint32_t *__restrict__; // the tag array, and the masks and the values of a pass

// One pass of the scan as both searches enqueue it: what is common to them, stated once.
struct GalleryScan {
    const bf16_t *store;
    const uint16_t *live; // null: the scan without the mask
    const int32_t *ids;   // null: the plain scan; else the identity scan, whose lists carry an identity word per key
    int rows, dim;
    const float *queries;
    int n, k;
    uint2 *ws;
    int groups_max;
    // null: no filter; else the filtered scan: one uint32 per row, and the pass's masks and values (device, [n] each)
    const uint32_t *tags = nullptr, *fmask = nullptr, *fvalue = nullptr;
};

// The one launch of the scan.  The kernel's pack `Live` is named in full (deduction would drop the pointers' __restrict__, and
// with it the instantiation).
template <int NMT, bool MASKED, bool IDENT, bool TAGGED>
static int launch_gallery_scan(const GalleryScan &a, int groups, size_t lds, hipStream_t s)
{
    constexpr int kLdsFilters = TAGGED ? kGalleryMaxQueries * (int)sizeof(uint2) : 0; // the filtered scan's (mask, value) pairs
    constexpr int kLdsMaxPlain = 2 * 16 * 1024 * 2 + kGalleryWaves * 32 * RFD_GALLERY_MAX_K * 8; // dim 1024, 32 queries, k 32: 96 KiB
    // dim 1024, 32 queries, k 32: 96 KiB of fragments and keys, 16 KiB of identities: 112 of the CU's 160 KiB
    constexpr int kLdsMaxIdent = 2 * 16 * 1024 * 2 + kGalleryWaves * 32 * RFD_GALLERY_MAX_K * (8 + 4);
    static DynLdsOnce once;
    auto launch = [&](auto *kernel, auto... live) -> int {
        RFD_TRY(once.ensure((const void *)kernel, (IDENT ? kLdsMaxIdent : kLdsMaxPlain) + kLdsFilters));
        hipLaunchKernelGGL(kernel, dim3(groups), dim3(kGalleryWaves * 64), lds, s, a.store, a.rows, a.dim / 32, a.queries, a.n, a.k, a.ws, live...);
        RFD_HIP(hipGetLastError());
        return RFD_OK;
    };
    if constexpr (TAGGED) {
        if constexpr (IDENT && MASKED)
            return launch(gallery_search_kernel<NMT, true, true, true, GalleryIdentities, GalleryTags, GalleryTags, GalleryTags, GalleryLiveWords>, a.ids, a.tags,
                          a.fmask, a.fvalue, a.live);
        else if constexpr (IDENT)
            return launch(gallery_search_kernel<NMT, false, true, true, GalleryIdentities, GalleryTags, GalleryTags, GalleryTags>, a.ids, a.tags, a.fmask, a.fvalue);
        else if constexpr (MASKED)
            return launch(gallery_search_kernel<NMT, true, false, true, GalleryTags, GalleryTags, GalleryTags, GalleryLiveWords>, a.tags, a.fmask, a.fvalue, a.live);
        else return launch(gallery_search_kernel<NMT, false, false, true, GalleryTags, GalleryTags, GalleryTags>, a.tags, a.fmask, a.fvalue);
    } else if constexpr (IDENT && MASKED) return launch(gallery_search_kernel<NMT, true, true, false, GalleryIdentities, GalleryLiveWords>, a.ids, a.live);
    else if constexpr (IDENT) return launch(gallery_search_kernel<NMT, false, true, false, GalleryIdentities>, a.ids);
    else if constexpr (MASKED) return launch(gallery_search_kernel<NMT, true, false, false, GalleryLiveWords>, a.live);
    else return launch(gallery_search_kernel<NMT, false, false, false>);
}

// the instantiation for a pass: one or two M-tiles, with or without the mask
template <bool IDENT, bool TAGGED>
static int launch_gallery_scan_for(const GalleryScan &a, int nmt, int groups, size_t lds, hipStream_t s)
{
    auto *scan = a.live ? (nmt == 2 ? launch_gallery_scan<2, true, IDENT, TAGGED> : launch_gallery_scan<1, true, IDENT, TAGGED>)
                        : (nmt == 2 ? launch_gallery_scan<2, false, IDENT, TAGGED> : launch_gallery_scan<1, false, IDENT, TAGGED>);
    return scan(a, groups, lds, s);
}

// checks the pass, enqueues its scan and returns the workgroups whose lists the merge reduces
static int launch_gallery_scan_pass(const char *who, const GalleryScan &a, hipStream_t s, int *groups)
{
    if (a.n < 1 || a.n > kGalleryMaxQueries || a.k < 1 || a.k > RFD_GALLERY_MAX_K || a.dim % 32 != 0 || a.rows < 0 || a.groups_max < 1) {
        set_error("%s: n %d, k %d, dim %d, rows %d out of range", who, a.n, a.k, a.dim, a.rows);
        return RFD_ERR_INVALID_ARG;
    }
    *groups = gallery_search_groups(a.rows, a.groups_max);
    const int nmt = a.n > 16 ? 2 : 1;
    const size_t keys = (size_t)kGalleryWaves * nmt * 16 * a.k, lds = (size_t)nmt * 16 * a.dim * sizeof(bf16_t) + keys * sizeof(uint2);
    if (a.tags) { // the pairs of the M-tiles' queries lie between the fragments and the keys
        if (!a.fmask || !a.fvalue) { set_error("%s: a filtered pass without its masks or values", who); return RFD_ERR_INVALID_ARG; }
        const size_t flds = lds + (size_t)nmt * 16 * sizeof(uint2);
        if (!a.ids) return launch_gallery_scan_for<false, true>(a, nmt, *groups, flds, s);
        return launch_gallery_scan_for<true, true>(a, nmt, *groups, flds + keys * sizeof(int32_t), s);
    }
    if (!a.ids) return launch_gallery_scan_for<false, false>(a, nmt, *groups, lds, s);
    return launch_gallery_scan_for<true, false>(a, nmt, *groups, lds + keys * sizeof(int32_t), s); // an identity word per key
}

int launch_gallery_search(const bf16_t *store, const uint16_t *live, int rows, int dim, const float *queries, int n, int k, uint2 *ws, int groups_max,
                          float *scores, int32_t *out_rows, hipStream_t s)
{
    int groups = 0;
    RFD_TRY(launch_gallery_scan_pass("launch_gallery_search", {store, live, nullptr, rows, dim, queries, n, k, ws, groups_max}, s, &groups));
    hipLaunchKernelGGL(gallery_merge_kernel, dim3(n), dim3(kGalleryWaves * 64), 0, s, ws, groups, n, k, scores, out_rows);
    RFD_HIP(hipGetLastError());
    return RFD_OK;
}

// ---- identity merge: gallery_merge_kernel with the identity forms of the two routines; writes the k best identities' keys and
//      identities, and the empty entry where !(score >= min_score) (a suffix: the keys are in descending order).  ids: the
//      identity array, read for the keys of the workspace (rows >= 0 only), or null: all unlabelled. ----
__global__ void __launch_bounds__(kGalleryWaves * 64) gallery_merge_identities_kernel(const uint2 *__restrict__ ws, int groups, int n, int k,
                                                                                       const int32_t *__restrict__ ids, float min_score,
                                                                                       float *__restrict__ scores, int32_t *__restrict__ out_rows,
                                                                                       int32_t *__restrict__ out_ids)
{
    __shared__ uint2 lists[kGalleryWaves * 32];
    __shared__ int32_t lids[kGalleryWaves * 32];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), q = blockIdx.x;
    uint2 *mine = lists + wave * k;
    int32_t *mine_ids = lids + wave * k;
    if (lane < k) {
        mine[lane] = gallery_sentinel();
        mine_ids[lane] = -1;
    }
    const int total = groups * k;
    for (int base = wave * 64; base < total; base += kGalleryWaves * 64) { // wave-uniform bounds: list_offer_ident runs with all lanes
        const int idx = base + lane;
        uint2 c = gallery_sentinel();
        if (idx < total) {
            const int g = idx / k, j = idx - g * k;
            c = ws[((size_t)g * n + q) * k + j];
        }
        const bool valid = (int)c.y >= 0; // a sentinel's row never indexes the identity array
        int cid = -1;
        if (valid && ids) cid = ids[c.y];
        list_offer_ident(mine, mine_ids, 0, k, __uint_as_float(c.x), (int)c.y, cid, valid, lane);
    }
    __syncthreads();
    if (tid == 0)
        merge_wave_lists_ident(lists, lids, k, k, [&](int j, uint2 key, int id) {
            const float sc = __uint_as_float(key.x);
            const bool keep = sc >= min_score; // false for the sentinel unless min_score is -inf, and then the sentinel is what is written
            scores[(size_t)q * k + j] = keep ? sc : __uint_as_float(gallery_sentinel().x);
            out_rows[(size_t)q * k + j] = keep ? (int32_t)key.y : -1;
            out_ids[(size_t)q * k + j] = keep ? id : -1;
        });
}

int launch_gallery_search_identities(const bf16_t *store, const uint16_t *live, const int32_t *ids, int rows, int dim, const float *queries, int n, int k,
                                     float min_score, uint2 *ws, int groups_max, float *scores, int32_t *out_rows, int32_t *out_ids, hipStream_t s)
{
    // ids null: no identity was ever set, every row is its own identity, and the plain scan selects exactly that
    int groups = 0;
    RFD_TRY(launch_gallery_scan_pass("launch_gallery_search_identities", {store, live, ids, rows, dim, queries, n, k, ws, groups_max}, s, &groups));
    hipLaunchKernelGGL(gallery_merge_identities_kernel, dim3(n), dim3(kGalleryWaves * 64), 0, s, ws, groups, n, k, ids, min_score, scores, out_rows, out_ids);
    RFD_HIP(hipGetLastError());
    return RFD_OK;
}

// The filtered form (rfd.h, "tags"): launch_gallery_search_identities on the rows r with (tags[r] & fmask[q]) == fvalue[q] for
// query q.  The merge is the identity merge: the workspace holds eligible keys only.
int launch_gallery_search_filtered(const bf16_t *store, const uint16_t *live, const int32_t *ids, const uint32_t *tags, const uint32_t *fmask,
                                   const uint32_t *fvalue, int rows, int dim, const float *queries, int n, int k, float min_score, uint2 *ws, int groups_max,
                                   float *scores, int32_t *out_rows, int32_t *out_ids, hipStream_t s)
{
    if (!tags) { set_error("launch_gallery_search_filtered: the tag array is null"); return RFD_ERR_INVALID_ARG; }
    int groups = 0;
    RFD_TRY(launch_gallery_scan_pass("launch_gallery_search_filtered", {store, live, ids, rows, dim, queries, n, k, ws, groups_max, tags, fmask, fvalue}, s, &groups));
    hipLaunchKernelGGL(gallery_merge_identities_kernel, dim3(n), dim3(kGalleryWaves * 64), 0, s, ws, groups, n, k, ids, min_score, scores, out_rows, out_ids);
    RFD_HIP(hipGetLastError());
    return RFD_OK;
}

// ---- identities of rows: ids[rows[i]] = vals[i], or -1 where vals is null (remove).  rows: a device list of distinct rows, so
//      every word has one writer. ----
__global__ void __launch_bounds__(256) gallery_set_identities_kernel(int32_t *__restrict__ ids, const int32_t *__restrict__ rows,
                                                                     const int32_t *__restrict__ vals, int n)
{
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    if (i < n) ids[rows[i]] = vals ? vals[i] : -1;
}

int launch_gallery_set_identities(int32_t *ids, const int32_t *rows, const int32_t *vals, int n, hipStream_t s)
{
    hipLaunchKernelGGL(gallery_set_identities_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, ids, rows, vals, n);
    RFD_HIP(hipGetLastError());
    return RFD_OK;
}

// ---- tags of rows: tags[rows[i]] = vals[i], or 0 where vals is null (remove, whose list may name a row twice: every writer
//      of a word then writes 0).  rows: a device list of rows, distinct where vals is given. ----
__global__ void __launch_bounds__(256) gallery_set_tags_kernel(uint32_t *__restrict__ tags, const int32_t *__restrict__ rows,
                                                               const uint32_t *__restrict__ vals, int n)
{
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    if (i < n) tags[rows[i]] = vals ? vals[i] : 0u;
}

int launch_gallery_set_tags(uint32_t *tags, const int32_t *rows, const uint32_t *vals, int n, hipStream_t s)
{
    hipLaunchKernelGGL(gallery_set_tags_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, tags, rows, vals, n);
    RFD_HIP(hipGetLastError());
    return RFD_OK;
}

// ---- remove / replace: rows[i] of the store takes bf16(emb[i]) (RNE), or zeros where emb is null.  One thread per 16-byte
//      operand; the first `nwords` threads also store the new live words of the blocks the call touches (blk ascending and
//      distinct, so every word has one writer).  rows / blk / word: device copies of the host's lists. ----
__global__ void __launch_bounds__(256) gallery_put_kernel(const float *__restrict__ emb, const int32_t *__restrict__ rows, int n, int dim,
                                                          bf16_t *__restrict__ store, const int32_t *__restrict__ blk,
                                                          const int32_t *__restrict__ word, int nwords, uint16_t *__restrict__ live)
{
    const int per_row = dim >> 3;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < (size_t)nwords) live[blk[i]] = (uint16_t)word[i];
    if (i >= (size_t)n * per_row) return;
    const int r = (int)(i / per_row), d = (int)(i - (size_t)r * per_row) * 8;
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (emb) {
        const float4 a = *reinterpret_cast<const float4 *>(emb + (size_t)r * dim + d), b = *reinterpret_cast<const float4 *>(emb + (size_t)r * dim + d + 4);
        const uint2 lo = pack_bf16x4(a.x, a.y, a.z, a.w), hi = pack_bf16x4(b.x, b.y, b.z, b.w);
        v = make_uint4(lo.x, lo.y, hi.x, hi.y);
    }
    *reinterpret_cast<uint4 *>(store + gallery_offset(dim, rows[r], d)) = v;
}

int launch_gallery_put(const float *emb, const int32_t *rows, int n, int dim, bf16_t *store, const int32_t *blk, const int32_t *word, int nwords,
                       uint16_t *live, hipStream_t s)
{
    const size_t items = (size_t)n * (dim >> 3); // nwords <= n <= items
    hipLaunchKernelGGL(gallery_put_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, s, emb, rows, n, dim, store, blk, word, nwords, live);
    RFD_HIP(hipGetLastError());
    return RFD_OK;
}

// ---- live words of rows [row0, row1), row0 < row1: their bits are set, the other bits of the two end blocks stay.  One thread per
//      block, so every word has one writer. ----
__global__ void __launch_bounds__(256) gallery_live_range_kernel(uint16_t *__restrict__ live, int row0, int row1)
{
    const int b0 = row0 >> 4, b = b0 + (int)(blockIdx.x * 256 + threadIdx.x);
    if (b > ((row1 - 1) >> 4)) return;
    const int lo = std::max(row0 - b * 16, 0), hi = std::min(row1 - b * 16, 16); // bits [lo, hi) of word b
    const uint32_t mask = (0xffffu >> (16 - hi)) & (0xffffu << lo) & 0xffffu;
    live[b] = (uint16_t)(mask == 0xffffu ? mask : (live[b] | mask));
}

int launch_gallery_live_range(uint16_t *live, int row0, int row1, hipStream_t s)
{
    const int nb = ((row1 - 1) >> 4) - (row0 >> 4) + 1;
    hipLaunchKernelGGL(gallery_live_range_kernel, dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, s, live, row0, row1);
    RFD_HIP(hipGetLastError());
    return RFD_OK;
}

// ---- file forms: bf16 values in row-major order <-> the fragment-major store, no conversion.  One thread per 16-byte operand. ----
__global__ void __launch_bounds__(256) gallery_import_kernel(const bf16_t *__restrict__ src, int n, int dim, int row0, bf16_t *__restrict__ store)
{
    const int per_row = dim >> 3;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)n * per_row) return;
    const int r = (int)(i / per_row), d = (int)(i - (size_t)r * per_row) * 8;
    *reinterpret_cast<uint4 *>(store + gallery_offset(dim, row0 + r, d)) = *reinterpret_cast<const uint4 *>(src + (size_t)r * dim + d);
}

__global__ void __launch_bounds__(256) gallery_export_kernel(const bf16_t *__restrict__ store, int row0, int n, int dim, bf16_t *__restrict__ out)
{
    const int per_row = dim >> 3;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)n * per_row) return;
    const int r = (int)(i / per_row), d = (int)(i - (size_t)r * per_row) * 8;
    *reinterpret_cast<uint4 *>(out + (size_t)r * dim + d) = *reinterpret_cast<const uint4 *>(store + gallery_offset(dim, row0 + r, d));
}

int launch_gallery_import(const bf16_t *src, int n, int dim, int row0, bf16_t *store, hipStream_t s)
{
    const size_t items = (size_t)n * (dim >> 3);
    hipLaunchKernelGGL(gallery_import_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, s, src, n, dim, row0, store);
    RFD_HIP(hipGetLastError());
    return RFD_OK;
}

int launch_gallery_export(const bf16_t *store, int row0, int n, int dim, bf16_t *out, hipStream_t s)
{
    const size_t items = (size_t)n * (dim >> 3);
    hipLaunchKernelGGL(gallery_export_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, s, store, row0, n, dim, out);
    RFD_HIP(hipGetLastError());
    return RFD_OK;
}

} // namespace rfd
