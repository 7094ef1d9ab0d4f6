// kernels_redact.hip -- the redaction of detection rows in BGR frames (include/rfd.h, "redaction"; gfx950, wave64): one launch,
// tile-driven.  Workgroup (t, b) of four waves owns tile t of frame b: a square of whole frame-anchored cells, rd_tile_side(cell)
// <= 64 pixels a side (redact_plan.h), cut by the frame's right and bottom edge.  No workgroup reads or writes a byte of a pixel
// outside its tile, so in place no workgroup can read what another one has already painted, and a cell mean -- taken over the
// whole cell, which lies in one tile -- is always a mean of SOURCE pixels.
//
// Pixels of a thread: the tile's rows are 16 groups of four pixels = 12 bytes; thread t takes group t & 15 of the rows t >> 4,
// + 16, + 32, + 48, so a wave instruction covers four rows of 192 contiguous bytes.  Its 16 pixels' cover is a 16-bit mask.
//
// 1. Rows.  In chunks of 256, thread t evaluates row base + t of the frame (selection, rd_region); the rows whose region meets
//    the tile are compacted into LDS by a ballot per wave and the waves' counts, so max_det rows never have to fit at once; then
//    every thread tests its pixels against the chunk's list (RECT: the ranges; ELLIPSE: rd_ellipse_covers, one right-hand side
//    per row of the tile); a thread passes over a region that misses its four columns, and over every region once its pixels are
//    all covered.  The selected, non-skipped rows are counted on the way; workgroup 0 of a frame stores applied[b].
// 2. In place, the workgroup leaves when no pixel of its tile is covered.
// 3. A full group is read as three unaligned dwords (one global_load_dwordx3, any byte alignment), a group cut by the frame or
//    the tile by bytes.  PIXELATE: every thread adds its pixels into the tile's cell sums in LDS (ds_add_u32, integer: any order
//    gives the same bits), one add per channel and run of pixels in a cell; behind a barrier one thread per cell turns the sums
//    into the packed mean; behind the next barrier -- every source byte the workgroup needs has been read -- the stores begin.
// 4. Stores.  A pixel is three bytes at any byte offset, so a dword next to a pixel that is not written holds bytes this workgroup
//    does not own.  A store therefore holds bytes of written pixels only: a group whose four pixels are all written goes out as
//    three unaligned dwords (its 12 bytes exactly), every other written pixel as three byte stores.  In place the written
//    pixels are the covered ones; out of place they are all pixels of the tile, the uncovered ones with their source value.
// No global atomics, no scratch; the same bits on every run.
#include "redact_host.h"

namespace rfd {

constexpr int kRdThreads = 256, kRdWaves = kRdThreads / 64, kRdChunk = kRdThreads;

typedef uint32_t rd_u32_unaligned __attribute__((aligned(1)));

// pixel j (0 .. 3) of a group's 12 bytes in three dwords, as B | G << 8 | R << 16
__device__ __forceinline__ uint32_t rd_get(const uint32_t d[3], int j)
{
    switch (j) {
    case 0: return d[0] & 0xffffffu;
    case 1: return (d[0] >> 24) | ((d[1] & 0xffffu) << 8);
    case 2: return (d[1] >> 16) | ((d[2] & 0xffu) << 16);
    default: return d[2] >> 8;
    }
}

__device__ __forceinline__ void rd_put(uint32_t d[3], int j, uint32_t c)
{
    switch (j) {
    case 0: d[0] = (d[0] & 0xff000000u) | c; break;
    case 1: d[0] = (d[0] & 0x00ffffffu) | (c << 24); d[1] = (d[1] & 0xffff0000u) | (c >> 8); break;
    case 2: d[1] = (d[1] & 0x0000ffffu) | (c << 16); d[2] = (d[2] & 0xffffff00u) | (c >> 16); break;
    default: d[2] = (d[2] & 0x000000ffu) | (c << 8); break;
    }
}

// The first npx (1 .. 4) pixels of the group at s: four as three unaligned dwords, fewer by bytes, zero-filled.
__device__ __forceinline__ void rd_load(const uint8_t *s, int npx, uint32_t d[3])
{
    if (npx == 4) {
        const rd_u32_unaligned *q = reinterpret_cast<const rd_u32_unaligned *>(s);
        d[0] = q[0]; d[1] = q[1]; d[2] = q[2];
    } else {
        d[1] = d[2] = 0u;
        d[0] = (uint32_t)s[0] | ((uint32_t)s[1] << 8) | ((uint32_t)s[2] << 16);
        if (npx > 1) { d[0] |= (uint32_t)s[3] << 24; d[1] = (uint32_t)s[4] | ((uint32_t)s[5] << 8); }
        if (npx > 2) { d[1] |= ((uint32_t)s[6] << 16) | ((uint32_t)s[7] << 24); d[2] = (uint32_t)s[8]; }
    }
}

__global__ void __launch_bounds__(kRdThreads) redact_kernel(RdParams p)
{
    __shared__ uint32_t s_ex[kRdChunk], s_ey[kRdChunk]; // the chunk's regions that meet the tile: X0 | X1 << 16, Y0 | Y1 << 16
    __shared__ int s_hits[kRdWaves], s_applied[kRdWaves];
    __shared__ int s_sum[kRdMaxTileCells * 3];
    __shared__ uint32_t s_mean[kRdMaxTileCells];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.y;
    const RdImage im = p.imgs[b];
    const int T = p.tile, cell = p.cell;
    const int tiles_x = rd_tiles(im.w, T);
    if ((int)blockIdx.x >= tiles_x * rd_tiles(im.h, T)) return; // a smaller frame of the call: uniform over the workgroup
    const int tyi = (int)blockIdx.x / tiles_x, txi = (int)blockIdx.x - tyi * tiles_x;
    const int tx0 = txi * T, ty0 = tyi * T;
    const int tw = min(T, im.w - tx0), th = min(T, im.h - ty0); // the tile inside the frame: 1 .. T
    const int tx1 = tx0 + tw - 1, ty1 = ty0 + th - 1;

    // this thread's pixels: group gx of rows ry + 16 k; bit 4 k + j of a mask is pixel j of row k
    const int lx0 = 4 * (tid & 15), ry = tid >> 4;
    const int npx = min(max(tw - lx0, 0), 4);
    uint32_t vmask = 0; // the pixels that exist
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (ry + 16 * k < th) vmask |= ((1u << npx) - 1u) << (4 * k);

    // ---- 1. the rows of the frame ----
    const int cnt = min(max(p.count[b], 0), p.max_det);
    uint32_t mask = 0; // the pixels covered
    int applied = 0;   // this wave's selected, non-skipped rows
    for (int base = 0; base < cnt; base += kRdChunk) { // uniform over the workgroup
        const int i = base + tid;
        bool valid = false, hit = false;
        RdRegion g = {0, 0, -1, -1, true};
        if (i < cnt) {
            const size_t row = (size_t)b * p.max_det + i;
            if (!p.sel || (p.sel[row] & p.sel_mask) == p.sel_value) {
                const float *bx = p.boxes + row * 5;
                g = rd_region(bx[0], bx[1], bx[2], bx[3], p.margin_x, p.margin_top, p.margin_bottom, im.w, im.h);
                valid = !g.skipped;
                hit = valid && g.x0 <= tx1 && g.x1 >= tx0 && g.y0 <= ty1 && g.y1 >= ty0;
            }
        }
        applied += __popcll(__ballot(valid));
        const unsigned long long hits = __ballot(hit);
        if (lane == 0) s_hits[wave] = __popcll(hits);
        __syncthreads();
        // the four waves' counts, by every lane with all lanes active (lane l reads entry l & 3): a wide LDS read is what
        // tests/test_build_cpu.py forbids under a predicate
        const int mine = s_hits[lane & (kRdWaves - 1)];
        int at = 0, total = 0;
#pragma unroll
        for (int k = 0; k < kRdWaves; ++k) {
            const int c = __shfl(mine, k);
            if (k < wave) at += c;
            total += c;
        }
        if (hit) {
            at += __popcll(hits & ((1ull << lane) - 1ull));
            s_ex[at] = (uint32_t)g.x0 | ((uint32_t)g.x1 << 16); // 0 <= x0 <= x1 < 32768
            s_ey[at] = (uint32_t)g.y0 | ((uint32_t)g.y1 << 16);
        }
        __syncthreads();
        for (int e = 0; e < total; ++e) {
            const uint32_t ex = s_ex[e], ey = s_ey[e];
            const int X0 = (int)(ex & 0xffffu), X1 = (int)(ex >> 16), Y0 = (int)(ey & 0xffffu), Y1 = (int)(ey >> 16);
            // nothing left to cover, or the region misses this thread's four columns: a wave whose lanes all say so skips the region
            if ((mask & vmask) == vmask || X1 < tx0 + lx0 || X0 > tx0 + lx0 + 3) continue;
            const int w = X1 - X0 + 1, h = Y1 - Y0 + 1;
            const uint64_t h2 = rd_sq(h);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int y = ty0 + ry + 16 * k;
                if (y < Y0 || y > Y1) continue;
                uint32_t bits = 0;
                if (p.shape == RFD_REDACT_RECT) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int x = tx0 + lx0 + j;
                        bits |= (x >= X0 && x <= X1 ? 1u : 0u) << j;
                    }
                } else {
                    const uint64_t rhs = rd_ellipse_rhs(2 * (y - Y0) + 1 - h, w, h);
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int x = tx0 + lx0 + j;
                        bits |= (x >= X0 && x <= X1 && rd_sq(2 * (x - X0) + 1 - w) * h2 <= rhs ? 1u : 0u) << j;
                    }
                }
                mask |= bits << (4 * k);
            }
        }
        // the next chunk's stores into s_hits come behind this chunk's second barrier, its stores into the list behind its own
        // first barrier, which every thread reaches only after the loop above
    }
    mask &= vmask;
    if (lane == 0) s_applied[wave] = applied;
    const int any = __syncthreads_or(mask != 0);
    applied = s_applied[lane & (kRdWaves - 1)]; // likewise
    applied += __shfl_xor(applied, 1);
    applied += __shfl_xor(applied, 2);
    if (blockIdx.x == 0 && tid == 0 && p.applied) p.applied[b] = applied;

    // ---- 2. nothing to do here ----
    if (!any && p.in_place) return;

    // ---- 3. the source pixels, the cell means ----
    const bool pixelate = any && p.mode == RFD_REDACT_PIXELATE;
    const bool need_src = !p.in_place || pixelate;
    const int ncx = T / cell; // cells per tile side
    const int cx0 = lx0 / cell, rem0 = lx0 - cx0 * cell;
    uint32_t px[4][3];
#pragma unroll
    for (int k = 0; k < 4; ++k) px[k][0] = px[k][1] = px[k][2] = 0u;
    if (pixelate) {
        for (int c = tid; c < ncx * ncx * 3; c += kRdThreads) s_sum[c] = 0;
        __syncthreads();
    }
    if (need_src) {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if ((vmask >> (4 * k)) & 15u)
                rd_load(im.src + (long long)(ty0 + ry + 16 * k) * im.sstride + (long long)(tx0 + lx0) * 3, npx, px[k]);
    }
    if (pixelate) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (!((vmask >> (4 * k)) & 15u)) continue;
            int *cs = s_sum + ((ry + 16 * k) / cell) * ncx * 3;
            int cx = cx0, rem = rem0, sb = 0, sg = 0, sr = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (j >= npx) break;
                const uint32_t c = rd_get(px[k], j);
                sb += (int)(c & 0xffu); sg += (int)((c >> 8) & 0xffu); sr += (int)(c >> 16);
                ++rem;
                if (rem == cell || j == npx - 1) { // the run of this cell ends
                    atomicAdd(&cs[cx * 3 + 0], sb); atomicAdd(&cs[cx * 3 + 1], sg); atomicAdd(&cs[cx * 3 + 2], sr);
                    sb = sg = sr = 0;
                    if (rem == cell) { ++cx; rem = 0; }
                }
            }
        }
        __syncthreads();
        for (int c = tid; c < ncx * ncx; c += kRdThreads) {
            const int cyi = c / ncx, cxi = c - cyi * ncx;
            const int cw = min(cell, tw - cxi * cell), ch = min(cell, th - cyi * cell); // the cell inside the frame
            if (cw > 0 && ch > 0) {
                const uint32_t n = (uint32_t)(cw * ch); // 1 .. 4096; a sum is at most 255 * 4096
                const uint32_t mb = ((uint32_t)s_sum[c * 3 + 0] + n / 2u) / n, mg = ((uint32_t)s_sum[c * 3 + 1] + n / 2u) / n,
                               mr = ((uint32_t)s_sum[c * 3 + 2] + n / 2u) / n;
                s_mean[c] = mb | (mg << 8) | (mr << 16);
            }
        }
    }
    __syncthreads(); // every load of the workgroup has been used (or, without cell sums, belongs to the thread that stores it)

    // ---- 4. the stores ----
    const uint32_t wmask = p.in_place ? mask : vmask;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t wbits = (wmask >> (4 * k)) & 15u, cbits = (mask >> (4 * k)) & 15u;
        if (!wbits) continue;
        const uint32_t *means = s_mean + ((ry + 16 * k) / cell) * ncx;
        uint32_t out[3] = {px[k][0], px[k][1], px[k][2]};
        int cx = cx0, rem = rem0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if ((cbits >> j) & 1u) rd_put(out, j, pixelate ? means[cx] : p.fill);
            if (++rem == cell) { ++cx; rem = 0; }
        }
        uint8_t *d = im.dst + (long long)(ty0 + ry + 16 * k) * im.dstride + (long long)(tx0 + lx0) * 3;
        if (wbits == 15u) {
            rd_u32_unaligned *q = reinterpret_cast<rd_u32_unaligned *>(d);
            q[0] = out[0]; q[1] = out[1]; q[2] = out[2];
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if ((wbits >> j) & 1u) {
                    const uint32_t c = rd_get(out, j);
                    d[3 * j + 0] = (uint8_t)c; d[3 * j + 1] = (uint8_t)(c >> 8); d[3 * j + 2] = (uint8_t)(c >> 16);
                }
            }
        }
    }
}

int launch_redact(const RdParams &p, RdGrid grid, hipStream_t s)
{
    hipLaunchKernelGGL(redact_kernel, dim3(grid.x, grid.y), dim3(kRdThreads), 0, s, p);
    RFD_HIP(hipGetLastError());
    return RFD_OK;
}

} // namespace rfd
