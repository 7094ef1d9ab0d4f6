// kernels_annotate.hip -- box outlines, landmark marks and text labels drawn into BGR frames (include/rfd.h, "annotation"; gfx950,
// wave64): one launch, tile-driven, with the tile ownership of kernels_redact.hip.  Workgroup (t, b) of four waves owns tile t of
// frame b, 64 x 64 pixels cut by the frame's right and bottom edge, and reads or writes no byte of a pixel outside it, so in place
// no workgroup can read what another one has painted (alpha < 256 blends with SOURCE pixels only).
//
// Pixels of a thread: as in the redaction, thread t takes the group of four pixels t & 15 of the tile's rows t >> 4, + 16, + 32,
// + 48.  What its 16 pixels have won is a 4-bit code each in one 64-bit word: 0 nothing yet, 1 .. 4 style 0 .. 3, 5 the text colour.
//
// 1. Rows.  In ascending chunks of 256, thread t evaluates row base + t of the frame: its style, its box (an_box), its string
//    (an_text, formatted here once, not per pixel), its mark centres, all clamped (an_clamp), and its extent (an_extent).  The rows
//    whose extent meets the tile are compacted IN ORDER into LDS by a ballot per wave and the waves' counts.  Then every thread
//    walks the chunk's list and asks an_layer for each of its pixels that no earlier row has taken: chunks ascend and the list
//    keeps the order, so a pixel's first cover is its winner (the lowest row index), and within a row an_layer gives the highest
//    layer.  A thread passes over a row whose extent misses its four columns, and over every row once its pixels are all decided.
// 2. In place, the workgroup leaves when no pixel of its tile is covered, before it reads a pixel.
// 3. Loads and stores as in the redaction: a group whose four pixels are all written is read and written as three unaligned dwords
//    (its 12 bytes exactly), every other pixel by bytes.  In place the written pixels are the covered ones, and the source is read
//    only for a blend; out of place all pixels of the tile are written, the uncovered ones with their source value.  A thread
//    reads and writes its own pixels only, so no barrier stands between its loads and its stores.
// The font is __constant__ memory.  No global atomics, no scratch; the same bits on every run.
#include "annotate_host.h"

namespace rfd {

constexpr int kAnThreads = 256, kAnWaves = kAnThreads / 64, kAnChunk = kAnThreads;

__constant__ AnFont d_an_font = AN_FONT_INIT;

typedef uint32_t an_u32_unaligned __attribute__((aligned(1)));

// pixel j (0 .. 3) of a group's 12 bytes in three dwords, as B | G << 8 | R << 16
__device__ __forceinline__ uint32_t an_get(const uint32_t d[3], int j)
{
    switch (j) {
    case 0: return d[0] & 0xffffffu;
    case 1: return (d[0] >> 24) | ((d[1] & 0xffffu) << 8);
    case 2: return (d[1] >> 16) | ((d[2] & 0xffu) << 16);
    default: return d[2] >> 8;
    }
}

__device__ __forceinline__ void an_set(uint32_t d[3], int j, uint32_t c)
{
    switch (j) {
    case 0: d[0] = (d[0] & 0xff000000u) | c; break;
    case 1: d[0] = (d[0] & 0x00ffffffu) | (c << 24); d[1] = (d[1] & 0xffff0000u) | (c >> 8); break;
    case 2: d[1] = (d[1] & 0x0000ffffu) | (c << 16); d[2] = (d[2] & 0xffffff00u) | (c >> 16); break;
    default: d[2] = (d[2] & 0x000000ffu) | (c << 8); break;
    }
}

// The first npx (1 .. 4) pixels of the group at s: four as three unaligned dwords, fewer by bytes, zero-filled.
__device__ __forceinline__ void an_load(const uint8_t *s, int npx, uint32_t d[3])
{
    if (npx == 4) {
        const an_u32_unaligned *q = reinterpret_cast<const an_u32_unaligned *>(s);
        d[0] = q[0]; d[1] = q[1]; d[2] = q[2];
    } else {
        d[1] = d[2] = 0u;
        d[0] = (uint32_t)s[0] | ((uint32_t)s[1] << 8) | ((uint32_t)s[2] << 16);
        if (npx > 1) { d[0] |= (uint32_t)s[3] << 24; d[1] = (uint32_t)s[4] | ((uint32_t)s[5] << 8); }
        if (npx > 2) { d[1] |= ((uint32_t)s[6] << 16) | ((uint32_t)s[7] << 24); d[2] = (uint32_t)s[8]; }
    }
}

__global__ void __launch_bounds__(kAnThreads) annotate_kernel(AnParams p)
{
    // the chunk's rows whose extent meets the tile, in row order: the extent inside the frame as X0 | X1 << 16, Y0 | Y1 << 16; the
    // clamped box; the clamped mark centres; the glyph string; len | style << 8
    __shared__ uint32_t s_ex[kAnChunk], s_ey[kAnChunk];
    __shared__ int32_t s_box[4][kAnChunk], s_mx[5][kAnChunk], s_my[5][kAnChunk];
    __shared__ uint32_t s_glo[kAnChunk], s_ghi[kAnChunk], s_meta[kAnChunk];
    __shared__ int s_hits[kAnWaves], s_applied[kAnWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.y;
    const RdImage im = p.imgs[b];
    const int T = kAnTile;
    const int tiles_x = rd_tiles(im.w, T);
    if ((int)blockIdx.x >= tiles_x * rd_tiles(im.h, T)) return; // a smaller frame of the call: uniform over the workgroup
    const int tyi = (int)blockIdx.x / tiles_x, txi = (int)blockIdx.x - tyi * tiles_x;
    const int tx0 = txi * T, ty0 = tyi * T;
    const int tw = min(T, im.w - tx0), th = min(T, im.h - ty0); // the tile inside the frame: 1 .. T
    const int tx1 = tx0 + tw - 1, ty1 = ty0 + th - 1;

    // this thread's pixels: group lx0 / 4 of rows ry + 16 k; bit 4 k + j of a mask is pixel j of row k
    const int lx0 = 4 * (tid & 15), ry = tid >> 4;
    const int npx = min(max(tw - lx0, 0), 4);
    uint32_t vmask = 0; // the pixels that exist
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (ry + 16 * k < th) vmask |= ((1u << npx) - 1u) << (4 * k);

    // ---- 1. the rows of the frame ----
    const int cnt = min(max(p.count[b], 0), p.max_det);
    const int t = p.thickness, rad = p.mark_radius, sc = p.text_scale;
    uint32_t mask = 0; // the pixels covered
    uint64_t win = 0;  // their codes
    int applied = 0;   // this wave's drawn, non-skipped rows
    for (int base = 0; base < cnt; base += kAnChunk) { // uniform over the workgroup
        const int i = base + tid;
        bool valid = false, hit = false;
        int style = -1;
        AnRow r;
        AnExtent e = {0, 0, -1, -1};
        if (i < cnt) {
            const size_t row = (size_t)b * p.max_det + i;
            const uint32_t word = p.sel ? p.sel[row] : 0u;
            style = an_style(word, p.n_styles, p.mask, p.want);
            if (style >= 0) {
                const float *bx = p.boxes + row * 5;
                const AnBox g = an_box(bx[0], bx[1], bx[2], bx[3], p.margin_x, p.margin_top, p.margin_bottom);
                valid = !g.skipped;
                if (valid) {
                    an_row_box(r, g);
#pragma unroll
                    for (int m = 0; m < 5; ++m) {
                        float lx = 0.0f, ly = 0.0f;
                        if (rad > 0) { lx = p.landmarks[row * 10 + 2 * m]; ly = p.landmarks[row * 10 + 2 * m + 1]; }
                        an_row_mark(r, m, lx, ly, rad);
                    }
                    const int32_t label = p.label_source == RFD_ANNOTATE_ARRAY ? p.label[row] : 0;
                    const float value = p.value_source == RFD_ANNOTATE_ARRAY ? p.value[row] : bx[4];
                    r.text = an_text(p.label_source, label, p.value_source, value);
                    e = an_extent(r, t, rad, sc);
                    hit = e.x0 <= tx1 && e.x1 >= tx0 && e.y0 <= ty1 && e.y1 >= ty0;
                }
            }
        }
        applied += __popcll(__ballot(valid));
        const unsigned long long hits = __ballot(hit);
        if (lane == 0) s_hits[wave] = __popcll(hits);
        __syncthreads();
        // the four waves' counts, by every lane with all lanes active (lane l reads entry l & 3), as in the redaction
        const int mine = s_hits[lane & (kAnWaves - 1)];
        int at = 0, total = 0;
#pragma unroll
        for (int k = 0; k < kAnWaves; ++k) {
            const int c = __shfl(mine, k);
            if (k < wave) at += c;
            total += c;
        }
        if (hit) {
            at += __popcll(hits & ((1ull << lane) - 1ull));
            s_ex[at] = (uint32_t)max(e.x0, 0) | ((uint32_t)min(e.x1, im.w - 1) << 16); // 0 <= X0 <= X1 < 32768: the extent meets the tile
            s_ey[at] = (uint32_t)max(e.y0, 0) | ((uint32_t)min(e.y1, im.h - 1) << 16);
            s_box[0][at] = r.xa; s_box[1][at] = r.ya; s_box[2][at] = r.xb; s_box[3][at] = r.yb;
#pragma unroll
            for (int m = 0; m < 5; ++m) { s_mx[m][at] = r.mx[m]; s_my[m][at] = r.my[m]; }
            s_glo[at] = (uint32_t)r.text.glyphs;
            s_ghi[at] = (uint32_t)(r.text.glyphs >> 32);
            s_meta[at] = (uint32_t)r.text.len | ((uint32_t)style << 8);
        }
        __syncthreads();
        for (int q = 0; q < total; ++q) {
            const uint32_t ex = s_ex[q], ey = s_ey[q];
            const int X0 = (int)(ex & 0xffffu), X1 = (int)(ex >> 16), Y0 = (int)(ey & 0xffffu), Y1 = (int)(ey >> 16);
            // nothing left to decide, or the extent misses this thread's four columns: a wave whose lanes all say so skips the row
            if ((mask & vmask) == vmask || X1 < tx0 + lx0 || X0 > tx0 + lx0 + 3) continue;
            AnRow w;
            w.xa = s_box[0][q]; w.ya = s_box[1][q]; w.xb = s_box[2][q]; w.yb = s_box[3][q];
#pragma unroll
            for (int m = 0; m < 5; ++m) { w.mx[m] = s_mx[m][q]; w.my[m] = s_my[m][q]; }
            const uint32_t meta = s_meta[q];
            w.text.glyphs = (uint64_t)s_glo[q] | ((uint64_t)s_ghi[q] << 32);
            w.text.len = (int32_t)(meta & 0xffu);
            const uint64_t row_code = (uint64_t)(meta >> 8) + 1u;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int y = ty0 + ry + 16 * k;
                if (y < Y0 || y > Y1) continue;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int bit = 4 * k + j;
                    if (!((vmask & ~mask) >> bit & 1u)) continue;
                    const int layer = an_layer(w, t, rad, sc, d_an_font, tx0 + lx0 + j, y);
                    if (layer) {
                        mask |= 1u << bit;
                        win |= (layer == 4 ? (uint64_t)5 : row_code) << (4 * bit);
                    }
                }
            }
        }
        // the next chunk's stores into s_hits come behind this chunk's second barrier, its stores into the list behind its own
        // first barrier, which every thread reaches only after the loop above
    }
    if (lane == 0) s_applied[wave] = applied;
    const int any = __syncthreads_or(mask != 0);
    applied = s_applied[lane & (kAnWaves - 1)];
    applied += __shfl_xor(applied, 1);
    applied += __shfl_xor(applied, 2);
    if (blockIdx.x == 0 && tid == 0 && p.applied) p.applied[b] = applied;

    // ---- 2. nothing to do here ----
    if (!any && p.in_place) return;

    // ---- 3. the source pixels, the colours, the stores ----
    const uint32_t alpha = (uint32_t)p.alpha;
    const bool need_src = !p.in_place || alpha != 256u;
    const uint32_t wmask = p.in_place ? mask : vmask;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t wbits = (wmask >> (4 * k)) & 15u, cbits = (mask >> (4 * k)) & 15u;
        if (!wbits) continue;
        const long long line = ty0 + ry + 16 * k, col = (long long)(tx0 + lx0) * 3;
        uint32_t out[3] = {0u, 0u, 0u};
        if (need_src) an_load(im.src + line * im.sstride + col, npx, out);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (!((cbits >> j) & 1u)) continue;
            const uint32_t code = (uint32_t)(win >> (4 * (4 * k + j))) & 15u;
            const uint32_t c = code == 5u ? p.text_colour : code == 1u ? p.colour[0] : code == 2u ? p.colour[1] : code == 3u ? p.colour[2] : p.colour[3];
            const uint32_t s = an_get(out, j);
            an_set(out, j, an_blend(c & 0xffu, s & 0xffu, alpha) | (an_blend((c >> 8) & 0xffu, (s >> 8) & 0xffu, alpha) << 8) |
                               (an_blend(c >> 16, s >> 16, alpha) << 16));
        }
        uint8_t *d = im.dst + line * im.dstride + col;
        if (wbits == 15u) {
            an_u32_unaligned *o = reinterpret_cast<an_u32_unaligned *>(d);
            o[0] = out[0]; o[1] = out[1]; o[2] = out[2];
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if ((wbits >> j) & 1u) {
                    const uint32_t c = an_get(out, j);
                    d[3 * j + 0] = (uint8_t)c; d[3 * j + 1] = (uint8_t)(c >> 8); d[3 * j + 2] = (uint8_t)(c >> 16);
                }
            }
        }
    }
}

int launch_annotate(const AnParams &p, RdGrid grid, hipStream_t s)
{
    hipLaunchKernelGGL(annotate_kernel, dim3(grid.x, grid.y), dim3(kAnThreads), 0, s, p);
    RFD_HIP(hipGetLastError());
    return RFD_OK;
}

} // namespace rfd
