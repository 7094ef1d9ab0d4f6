// kernels_gallery_nearest.hip -- the gallery's self-join (include/rfd.h, "nearest"): for every row a of a range, the best other
// row b under the gallery's total order (score descending, row ascending).  The decomposition is planned on the host
// (gallery_nearest_plan.h); this file holds the scan, the merge and their launch.
//
// Scan: a workgroup owns one A tile (tile_rows rows of the range) and one B split (every splits-th group of four row blocks).
// The stored (block, K step) is the B operand of v_mfma_f32_16x16x32_bf16, and the A operand has the same lane-to-element map (lane l: row
// l & 15, elements 8 * (l >> 4) .. + 7), so an A fragment is the 16 bytes gallery_offset() names for the lane's row -- read per
// lane, which also serves tiles that do not start at a block.  Every wave walks its block of the split's groups as the search
// walks its own: one coalesced 1 KiB load per K step straight from HBM, kPrefetch* of them in flight, dim / 32 MFMAs per
// (M-tile, block) into one accumulator from +0, K ascending.  score(a, b) therefore has the bits rfd_gallery_search returns for
// row b and the query rfd_gallery_get_rows(a) -- the same products in the same chain -- and score(b, a) has them too.
// Where the A tile lives is the form (chosen per dim and call in the plan):
//   KS == 0, any dim: A fragments in LDS, two 8-byte halves per lane as in the search, re-read for every MFMA.
//   KS > 0, dim == 32 * KS: A fragments in registers (4 KS per M-tile), the K loop unrolled at compile time, one wave per SIMD.
// Selection, in registers: C lane mapping lane & 15 = B row of the block, 4 * (lane >> 4) + reg = A row of the M-tile.  A lane
// keeps one best key per (M-tile, reg); its B rows ascend while it walks, so "strictly greater" keeps the lower row among equal
// scores and never takes a NaN or -inf.  Scores are computed regardless; an ineligible key is simply never taken.  At the end
// the 16 lanes of a group are reduced by shuffles, the four waves through LDS, both under the total order, and the workgroup
// writes one key per A row to ws[split][n].  No atomics; every word has one writer.
// Eligibility of b for a: b is live, b != a, a is live, mode (not the same identity >= 0) and the tag rule.  The live word, the
// 16 identities and the 16 tags of a block are read per block through wave-uniform addresses (scalar loads, which do not
// count against the operand loads in flight); the A rows' identity, tag and liveness once per tile.
// Merge: up to a wave per A row reduces the splits' keys, applies min_score, looks the winner's identity up and writes the three
// outputs, or the empty entry.
#include "conv_device.h"
#include "gallery_nearest_plan.h"

namespace rfd {

namespace {

constexpr int kPrefetchLds = 8;        // K steps of B loads a wave of the LDS form keeps in flight, as the search does
constexpr int kPrefetchRegisters = 16; // ... and of the register form, which runs one wave per SIMD: a whole block of dim 512

__device__ __forceinline__ bool nearest_better(float s, int r, float s2, int r2) { return s > s2 || (s == s2 && r < r2); }

struct NearestArgs {
    int rows, ksteps, row0, n;
    int mode; // RFD_GALLERY_NEAREST_*
    uint32_t tag_mask;
    int tiles, splits, blocks;
};

} // namespace

template <int NMT, int KS, int kPrefetch>
__global__ void __launch_bounds__(kNearestWaves * 64) gallery_nearest_kernel(const bf16_t *__restrict__ store, const uint32_t *__restrict__ live,
                                                                             const int32_t *__restrict__ ids, const uint32_t *__restrict__ tags,
                                                                             const NearestArgs p, uint2 *__restrict__ ws)
{
    // live: pairs of 16-bit live words, or null: every row below `rows` is live.  ids, tags: one word per row in whole blocks of
    // 16, or null: every row is unlabelled / every tag is 0.  ws: [splits][n] keys.
    extern __shared__ __attribute__((aligned(16))) unsigned char nearest_smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ksteps = KS > 0 ? KS : p.ksteps, dim = ksteps * 32;
    const int tile = (int)(blockIdx.x % (unsigned)p.tiles), split = (int)(blockIdx.x / (unsigned)p.tiles);
    const int a0 = p.row0 + tile * (NMT * 16), a_end = p.row0 + p.n; // the tile's first A row; the call's last + 1 (a0 < a_end)
    uint2 *red = reinterpret_cast<uint2 *>(nearest_smem);            // [waves][NMT * 16] keys
    [[maybe_unused]] uint2 *afrag = red + kNearestWaves * NMT * 16;  // KS == 0: [NMT][ksteps][2 halves][64 lanes] x 4 bf16
    const uint4 *store4 = reinterpret_cast<const uint4 *>(store);

    // ---- the A tile.  A row beyond the call re-reads the call's last row (in bounds) and is never written. ----
    [[maybe_unused]] uint4 areg[NMT][KS > 0 ? KS : 1];
    if constexpr (KS > 0) {
#pragma unroll
        for (int mt = 0; mt < NMT; ++mt) {
            const int a = min(a0 + mt * 16 + (lane & 15), a_end - 1);
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) areg[mt][ks] = store4[gallery_offset(dim, a, ks * 32 + 8 * (lane >> 4)) >> 3];
        }
    } else {
        for (int i = tid; i < NMT * ksteps * 64; i += kNearestWaves * 64) {
            const int l = i & 63, ks = (i >> 6) % ksteps, mt = (i >> 6) / ksteps;
            const int a = min(a0 + mt * 16 + (l & 15), a_end - 1);
            const uint4 v = store4[gallery_offset(dim, a, ks * 32 + 8 * (l >> 4)) >> 3];
            afrag[((mt * ksteps + ks) * 2 + 0) * 64 + l] = make_uint2(v.x, v.y);
            afrag[((mt * ksteps + ks) * 2 + 1) * 64 + l] = make_uint2(v.z, v.w);
        }
        __syncthreads();
    }
    // per (M-tile, reg), the A row 16 mt + 4 (lane >> 4) + r of the tile: its identity and tag, and in bit 4 mt + r of a_ok whether
    // it is in the call and live
    [[maybe_unused]] int a_id[NMT][4];
    [[maybe_unused]] uint32_t a_tag[NMT][4];
    uint32_t a_ok = 0u;
    const bool by_identity = p.mode == RFD_GALLERY_NEAREST_OTHER_IDENTITY && ids != nullptr; // wave-uniform
    const bool by_tag = p.tag_mask != 0u && tags != nullptr;                                  // wave-uniform
    const int a_lane = a0 + 4 * (lane >> 4); // the lane's A row of (mt, r) is a_lane + 16 mt + r
#pragma unroll
    for (int mt = 0; mt < NMT; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int a = a_lane + mt * 16 + r, ac = min(a, a_end - 1);
            uint32_t word = 0xffffffffu;
            if (live) word = live[ac >> 5];
            a_ok |= (a < a_end ? (word >> (ac & 31)) & 1u : 0u) << (4 * mt + r);
            a_id[mt][r] = by_identity ? ids[ac] : -1;
            a_tag[mt][r] = by_tag ? (tags[ac] & p.tag_mask) : 0u;
        }
    float best_s[NMT][4];
    int best_r[NMT][4];
#pragma unroll
    for (int mt = 0; mt < NMT; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) { best_s[mt][r] = -INFINITY; best_r[mt][r] = -1; }

    // ---- the walk: the split's groups of four blocks, split, split + splits, ...; the wave takes its block of each ----
    const int b_end = p.blocks, stride = p.splits * kNearestWaves;
    int blk = split * kNearestWaves + wave;
    if (blk < b_end) { // wave-uniform
        int pblk = blk, pks = 0; // the step the loads are at
        const uint4 *src = store4 + lane;
        uint4 buf[kPrefetch];
        // loads beyond the wave's last block re-read its last block (never out of bounds); their MFMAs run and are dropped
        const int last = blk + ((b_end - 1 - blk) / stride) * stride;
        auto issue = [&](uint4 &dst) {
            const int b = pblk < b_end ? pblk : last;
            dst = src[((size_t)b * ksteps + pks) * 64];
            if (++pks == ksteps) { pks = 0; pblk += stride; }
        };
#pragma unroll
        for (int i = 0; i < kPrefetch; ++i) {
            issue(buf[i]);
            __builtin_amdgcn_sched_barrier(0); // keep the issue order: the loop waits for buf[0] with the other loads still in flight
        }
        f32x4 acc[NMT];
#pragma unroll
        for (int mt = 0; mt < NMT; ++mt) acc[mt] = f32x4{0.f, 0.f, 0.f, 0.f};

        // the selection of a finished block: a compare and two selects per score, behind the eligibility of the pair
        auto select = [&](int b) {
            const int ub = __builtin_amdgcn_readfirstlane(b);
            const int row = ub * 16 + (lane & 15);
            const int rel = row - a_lane; // mt * 16 + r where the lane's B row is its A row of (mt, r)
            bool b_ok = row < p.rows;
            if (live) b_ok = b_ok && ((live[ub >> 1] >> (16 * (ub & 1) + (lane & 15))) & 1u);
            [[maybe_unused]] int b_id = -1;
            [[maybe_unused]] uint32_t b_tag = 0u;
            if (by_identity) {
                const int32_t *block_ids = ids + (size_t)ub * 16;
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int v = block_ids[i];
                    b_id = (lane & 15) == i ? v : b_id;
                }
            }
            if (by_tag) {
                const uint32_t *block_tags = tags + (size_t)ub * 16;
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const uint32_t v = block_tags[i];
                    b_tag = (lane & 15) == i ? v : b_tag;
                }
                b_tag &= p.tag_mask;
            }
#pragma unroll
            for (int mt = 0; mt < NMT; ++mt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    bool ok = b_ok && ((a_ok >> (4 * mt + r)) & 1u) && rel != mt * 16 + r && a_tag[mt][r] == b_tag;
                    ok = ok && !(a_id[mt][r] >= 0 && a_id[mt][r] == b_id);
                    const bool take = ok && acc[mt][r] > best_s[mt][r];
                    best_s[mt][r] = take ? acc[mt][r] : best_s[mt][r];
                    best_r[mt][r] = take ? row : best_r[mt][r];
                }
#pragma unroll
            for (int mt = 0; mt < NMT; ++mt) acc[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
        };

        if constexpr (KS > 0) {
            static_assert(KS % kPrefetch == 0, "the ring of loads keeps its place from block to block");
            for (; blk < b_end; blk += stride) {
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) {
                    const bf16x8 b = __builtin_bit_cast(bf16x8, buf[ks % kPrefetch]);
#pragma unroll
                    for (int mt = 0; mt < NMT; ++mt)
                        acc[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, areg[mt][ks]), b, acc[mt], 0, 0, 0);
                    issue(buf[ks % kPrefetch]);
                    __builtin_amdgcn_sched_barrier(0); // the load stays behind its step's MFMAs, kPrefetch steps ahead of its use
                }
                select(blk);
            }
        } else {
            int ks = 0; // the step the MFMAs are at
            while (blk < b_end) {
#pragma unroll
                for (int i = 0; i < kPrefetch; ++i) {
                    const bf16x8 b = __builtin_bit_cast(bf16x8, buf[i]);
#pragma unroll
                    for (int mt = 0; mt < NMT; ++mt) {
                        const uint2 lo = afrag[((mt * ksteps + ks) * 2 + 0) * 64 + lane], hi = afrag[((mt * ksteps + ks) * 2 + 1) * 64 + lane];
                        acc[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, make_uint4(lo.x, lo.y, hi.x, hi.y)), b, acc[mt], 0, 0, 0);
                    }
                    issue(buf[i]);
                    if (++ks == ksteps) {
                        if (blk < b_end) select(blk); // past the last block the ring's remaining steps are dropped
                        ks = 0;
                        blk += stride;
                    }
                }
            }
        }
    }

    // ---- reduce: the 16 lanes of a group, then the four waves, under the total order ----
#pragma unroll
    for (int mt = 0; mt < NMT; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float s = best_s[mt][r];
            int row = best_r[mt][r];
#pragma unroll
            for (int d = 1; d < 16; d <<= 1) {
                const float s2 = __shfl_xor(s, d);
                const int r2 = __shfl_xor(row, d);
                // a lane without a key holds (-inf, -1), which no key of a lane loses to: a taken score is > -inf
                const bool other = r2 >= 0 && (row < 0 || nearest_better(s2, r2, s, row));
                s = other ? s2 : s;
                row = other ? r2 : row;
            }
            if ((lane & 15) == 0) red[wave * (NMT * 16) + mt * 16 + 4 * (lane >> 4) + r] = make_uint2(__float_as_uint(s), (uint32_t)row);
        }
    __syncthreads();
    if (tid < NMT * 16 && a0 + tid < a_end) {
        uint2 b = red[tid];
#pragma unroll
        for (int w = 1; w < kNearestWaves; ++w) {
            const uint2 c = red[w * (NMT * 16) + tid];
            if ((int)c.y >= 0 && ((int)b.y < 0 || nearest_better(__uint_as_float(c.x), (int)c.y, __uint_as_float(b.x), (int)b.y))) b = c;
        }
        ws[(size_t)split * p.n + (a0 - p.row0) + tid] = b;
    }
}

// ---- merge: ws[splits][n] -> the three outputs.  `lanes` (a power of two <= 64) consecutive lanes own one A row: each reduces
//      every lanes-th split's key, then the lanes are reduced by shuffles under the total order, and the first writes.  One
//      thread per row where the row has one key; a wave per row where the gallery was cut into many splits -- a single thread
//      walking 1 024 keys one load at a time took 0.5 ms, longer than the scan they came from. ----
__global__ void __launch_bounds__(256) gallery_nearest_merge_kernel(const uint2 *__restrict__ ws, int splits, int n, int lanes, const int32_t *__restrict__ ids,
                                                                    float min_score, float *__restrict__ scores, int32_t *__restrict__ out_rows,
                                                                    int32_t *__restrict__ out_ids)
{
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t i = t / (unsigned)lanes;
    const int sub = (int)(t % (unsigned)lanes);
    uint2 b = make_uint2(0xff800000u, 0xffffffffu); // (-inf, -1): no key
    if (i < (size_t)n)
        for (int s = sub; s < splits; s += lanes) {
            const uint2 c = ws[(size_t)s * n + i];
            if ((int)c.y >= 0 && ((int)b.y < 0 || nearest_better(__uint_as_float(c.x), (int)c.y, __uint_as_float(b.x), (int)b.y))) b = c;
        }
    for (int d = 1; d < lanes; d <<= 1) { // the lanes of a row are an aligned group of one wave: 256 and 64 are multiples of `lanes`
        const uint2 c = make_uint2(__shfl_xor(b.x, d), __shfl_xor(b.y, d));
        if ((int)c.y >= 0 && ((int)b.y < 0 || nearest_better(__uint_as_float(c.x), (int)c.y, __uint_as_float(b.x), (int)b.y))) b = c;
    }
    if (i >= (size_t)n || sub != 0) return;
    const float sc = __uint_as_float(b.x);
    const bool keep = (int)b.y >= 0 && sc >= min_score; // a sentinel's row never indexes the identity array
    scores[i] = keep ? sc : -INFINITY;
    out_rows[i] = keep ? (int32_t)b.y : -1;
    if (out_ids) out_ids[i] = keep && ids ? ids[b.y] : -1;
}

int launch_gallery_nearest(const bf16_t *store, const uint16_t *live, const int32_t *ids, const uint32_t *tags, int rows, int dim, int row0, int n, int mode,
                           float min_score, uint32_t tag_mask, const GalleryNearestPlan &plan, uint2 *ws, float *scores, int32_t *out_rows, int32_t *out_ids,
                           hipStream_t s)
{
    if (n < 1 || plan.grid < 1 || plan.grid > 0x7fffffffll || dim < 32 || dim > 1024 || dim % 32 != 0 || !store || !ws || !scores || !out_rows) {
        set_error("launch_gallery_nearest: n %d, dim %d, grid %lld out of range or a null buffer", n, dim, (long long)plan.grid);
        return RFD_ERR_INVALID_ARG;
    }
    const NearestArgs a = {rows, dim / 32, row0, n, mode, tag_mask, plan.tiles, plan.splits, plan.blocks};
    const uint32_t *live2 = reinterpret_cast<const uint32_t *>(live); // an even number of words is allocated
    if (plan.form == kNearestFormRegisters) {
        if (dim != 512 || plan.tile_rows != 64) { set_error("launch_gallery_nearest: the register form is dim 512, 64 rows"); return RFD_ERR_INVALID_ARG; }
        hipLaunchKernelGGL((gallery_nearest_kernel<4, 16, kPrefetchRegisters>), dim3((unsigned)plan.grid), dim3(kNearestWaves * 64), kNearestWaves * 64 * sizeof(uint2), s, store, live2, ids, tags, a, ws);
    } else {
        if (plan.tile_rows != 32) { set_error("launch_gallery_nearest: the LDS form has 32 rows per tile"); return RFD_ERR_INVALID_ARG; }
        const size_t lds = kNearestWaves * 32 * sizeof(uint2) + (size_t)2 * 16 * dim * sizeof(bf16_t); // keys, then the A fragments: at most 65 KiB
        static DynLdsOnce once;
        RFD_TRY(once.ensure((const void *)gallery_nearest_kernel<2, 0, kPrefetchLds>, kNearestWaves * 32 * (int)sizeof(uint2) + 2 * 16 * 1024 * (int)sizeof(bf16_t)));
        hipLaunchKernelGGL((gallery_nearest_kernel<2, 0, kPrefetchLds>), dim3((unsigned)plan.grid), dim3(kNearestWaves * 64), lds, s, store, live2, ids, tags, a, ws);
    }
    RFD_HIP(hipGetLastError());
    int lanes = 1; // of the merge per A row: the power of two that covers the splits, at most a wave
    while (lanes < plan.splits && lanes < 64) lanes *= 2;
    const size_t merge_blocks = ((size_t)n * lanes + 255) / 256;
    hipLaunchKernelGGL(gallery_nearest_merge_kernel, dim3((unsigned)merge_blocks), dim3(256), 0, s, ws, plan.splits, n, lanes, ids, min_score, scores, out_rows, out_ids);
    RFD_HIP(hipGetLastError());
    return RFD_OK;
}

} // namespace rfd
