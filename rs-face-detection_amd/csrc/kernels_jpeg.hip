// kernels_jpeg.hip -- the parallel half of the baseline JPEG decoder (rfd.h, "JPEG decode"), gfx950.
//
// Two launches per batch, whatever the number, sizes and samplings of its frames, and a third where a frame is stored through
// an EXIF orientation: every workgroup finds its frame in the descriptor table (JpegFrame, kernels.h) by its own index, as the
// liveness crops do.
//   jpeg_idct_kernel   8 lanes per 8x8 block, 32 blocks per workgroup.  Lane j gathers column j of the block from the block's
//                      truncated zigzag run (positions past the run are zero), dequantises, runs the column pass of
//                      jidctint.c, hands the result over through LDS, runs the row pass on row j and stores its 8 samples as
//                      one 8-byte word.  A wave's eight blocks are neighbours in a plane, so it writes 8 rows of 64 bytes.
//   jpeg_color_kernel  one thread per 4 pixels of an output row: h2v1 / h2v2 fancy upsampling (jdsample.c) of the two chroma
//                      planes, jdcolor.c's fixed-point YCbCr -> RGB, three 4-byte stores of B,G,R bytes (single bytes where the
//                      row is not 4-byte aligned or the image ends inside the quad).
//   jpeg_color_oriented_kernel  frames of orientation 2..8 (rfd.h, "EXIF orientation"): the same pixels, computed along stored
//                      rows into an LDS tile and stored along output rows; described at the kernel.
//   jpeg_idct_reduced_kernel, jpeg_color_scaled_kernel, jpeg_color_scaled_oriented_kernel  the three launches of a batch decoded
//                      at 1/2, 1/4 or 1/8 size (rfd.h, "JPEG decode, reduced size"); described at the kernels.
// All arithmetic is 32-bit integer.  The IDCT computes in unsigned words, so that coefficients no 8-bit image produces wrap
// instead of overflowing a signed type; nothing indexes memory with a data-dependent value except the zigzag run, whose
// length is masked to 64 and whose extent the host sized.
#include "kernels.h"

namespace rfd {

namespace {

// zigzag position of natural (row-major) index n
__device__ const unsigned char kZigzagOf[64] = {0,  1,  5,  6,  14, 15, 27, 28, 2,  4,  7,  13, 16, 26, 29, 42, 3,  8,  12, 17, 25, 30,
                                                41, 43, 9,  11, 18, 24, 31, 40, 44, 53, 10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38,
                                                46, 51, 55, 60, 21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63};

typedef unsigned int U;

__device__ inline int descale(U v, int n) { return (int)(v + (1u << (n - 1))) >> n; }

// jidctint.c jpeg_idct_islow, one dimension: x = frequencies 0..7 -> o = the eight sums scaled by 2^13, before the descale
__device__ __forceinline__ void idct_1d(const U (&x)[8], U (&o)[8])
{
    U z2 = x[2], z3 = x[6];
    U z1 = (z2 + z3) * 4433u;                 // FIX(0.541196100)
    U tmp2 = z1 - z3 * 15137u;                // FIX(1.847759065)
    U tmp3 = z1 + z2 * 6270u;                 // FIX(0.765366865)
    U tmp0 = (x[0] + x[4]) << 13, tmp1 = (x[0] - x[4]) << 13;
    const U tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    tmp0 = x[7]; tmp1 = x[5]; tmp2 = x[3]; tmp3 = x[1];
    z1 = tmp0 + tmp3; z2 = tmp1 + tmp2; z3 = tmp0 + tmp2;
    U z4 = tmp1 + tmp3;
    const U z5 = (z3 + z4) * 9633u;           // FIX(1.175875602)
    tmp0 *= 2446u;                            // FIX(0.298631336)
    tmp1 *= 16819u;                           // FIX(2.053119869)
    tmp2 *= 25172u;                           // FIX(3.072711026)
    tmp3 *= 12299u;                           // FIX(1.501321110)
    z1 = 0u - z1 * 7373u;                     // FIX(0.899976223)
    z2 = 0u - z2 * 20995u;                    // FIX(2.562915447)
    z3 = z5 - z3 * 16069u;                    // FIX(1.961570560)
    z4 = z5 - z4 * 3196u;                     // FIX(0.390180644)
    tmp0 += z1 + z3; tmp1 += z2 + z4; tmp2 += z2 + z3; tmp3 += z1 + z4;
    o[0] = tmp10 + tmp3; o[7] = tmp10 - tmp3;
    o[1] = tmp11 + tmp2; o[6] = tmp11 - tmp2;
    o[2] = tmp12 + tmp1; o[5] = tmp12 - tmp1;
    o[3] = tmp13 + tmp0; o[4] = tmp13 - tmp0;
}

// the frame whose first workgroup is the last one <= g (first[] ascends strictly: every frame has at least one workgroup)
template <int JpegFrame::*First> __device__ inline const JpegFrame &frame_of(const JpegParams &p, int g)
{
    int lo = 0, hi = p.n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (p.frames[mid].*First <= g) lo = mid; else hi = mid - 1;
    }
    return p.frames[lo];
}

constexpr int kWsBlock = 72, kWsRow = 9; // LDS pitch of a block and of a row in it, in words: both passes touch 32 distinct banks

__global__ __launch_bounds__(256) void jpeg_idct_kernel(JpegParams p)
{
    __shared__ U ws[kJpegGroupBlocks * kWsBlock];
    const int g = blockIdx.x;
    const JpegFrame &f = frame_of<&JpegFrame::group0>(p, g);
    const int lb = threadIdx.x >> 3, j = threadIdx.x & 7;
    const int blk = (g - f.group0) * kJpegGroupBlocks + lb;
    const bool valid = blk < f.nblocks;
    const int c = (f.ncomp == 3 && blk >= f.blk0[1]) ? (blk >= f.blk0[2] ? 2 : 1) : 0;
    U x[8], o[8];
    {
        uint32_t rec = valid ? p.rec[f.rec0 + (unsigned)blk] : 0u;
        const int count = min((int)(rec & 127u), 64);
        const int16_t *run = p.coef + f.coef0 + (rec >> 7);
        const uint16_t *q = f.quant[c];
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const int nat = r * 8 + j, z = kZigzagOf[nat];
            x[r] = z < count ? (U)((int)run[z] * (int)q[nat]) : 0u;
        }
    }
    idct_1d(x, o); // column j
    U *w = ws + lb * kWsBlock;
#pragma unroll
    for (int r = 0; r < 8; ++r) w[r * kWsRow + j] = (U)descale(o[r], 13 - 2);
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 8; ++k) x[k] = w[j * kWsRow + k];
    idct_1d(x, o); // row j
    if (!valid) return;
    uint32_t lo = 0, hi = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        lo |= (uint32_t)min(max(descale(o[k], 13 + 2 + 3) + 128, 0), 255) << (8 * k);
        hi |= (uint32_t)min(max(descale(o[k + 4], 13 + 2 + 3) + 128, 0), 255) << (8 * k);
    }
    const int b = blk - f.blk0[c], by = b / f.bw[c], bx = b - by * f.bw[c];
    uint8_t *plane = p.planes + f.plane0 + (size_t)f.blk0[c] * 64;
    *reinterpret_cast<uint2 *>(plane + ((size_t)by * 8 + j) * ((size_t)f.bw[c] * 8) + (size_t)bx * 8) = make_uint2(lo, hi);
}

__device__ inline int clamp255(int v) { return min(max(v, 0), 255); }

struct Quad { int a, b, c, d; };

// the four upsampled samples of one chroma plane under pixels x0 .. x0 + 3 of row y (pw: the plane's row pitch).  replicate: a
// horizontal factor of 2 is plain replication whatever the row's length (a decode at 1/8: jdsample.c has no fancy filter there)
__device__ __forceinline__ Quad chroma_quad(const uint8_t *pl, int pw, int hmax, int vmax, int dw, int dh, int x0, int y, bool replicate = false)
{
    if (hmax == 1) { // 4:4:4
        const uint8_t *r = pl + (size_t)y * pw + x0;
        return Quad{r[0], r[1], r[2], r[3]};
    }
    const int i0 = x0 >> 1, rn = vmax == 2 ? y >> 1 : y;
    const uint8_t *near = pl + (size_t)rn * pw;
    if (replicate || dw <= 2) { // libjpeg filters only planes of more than two samples per row; these are replicated
        const int a = near[min(i0, dw - 1)], b = near[min(i0 + 1, dw - 1)];
        return Quad{a, a, b, b};
    }
    // samples i0 - 1 .. i0 + 2, clamped into the row: a clamped one is only read where the edge rule ignores it
    const int k0 = max(i0 - 1, 0), k1 = i0, k2 = min(i0 + 1, dw - 1), k3 = min(i0 + 2, dw - 1);
    if (vmax == 1) { // h2v1_fancy_upsample
        const int s0 = near[k0], s1 = near[k1], s2 = near[k2], s3 = near[k3];
        return Quad{i0 == 0 ? s1 : (3 * s1 + s0 + 1) >> 2, i0 == dw - 1 ? s1 : (3 * s1 + s2 + 2) >> 2, (3 * s2 + s1 + 1) >> 2,
                    i0 + 1 >= dw - 1 ? s2 : (3 * s2 + s3 + 2) >> 2};
    }
    // h2v2_fancy_upsample: column sums of the nearer row (3/4) and the farther one (1/4), which at the edges is the row itself
    const uint8_t *far = pl + (size_t)((y & 1) ? min(rn + 1, dh - 1) : max(rn - 1, 0)) * pw;
    const int s0 = 3 * near[k0] + far[k0], s1 = 3 * near[k1] + far[k1], s2 = 3 * near[k2] + far[k2], s3 = 3 * near[k3] + far[k3];
    return Quad{i0 == 0 ? (4 * s1 + 8) >> 4 : (3 * s1 + s0 + 8) >> 4, i0 == dw - 1 ? (4 * s1 + 7) >> 4 : (3 * s1 + s2 + 7) >> 4, (3 * s2 + s1 + 8) >> 4,
                i0 + 1 >= dw - 1 ? (4 * s2 + 7) >> 4 : (3 * s2 + s3 + 7) >> 4};
}

__device__ __forceinline__ uint32_t bgr_of(int Y, int cb, int cr) // jdcolor.c build_ycc_rgb_table, written out -> B | G << 8 | R << 16
{
    const int u = cb - 128, v = cr - 128;
    return (uint32_t)clamp255(Y + ((116130 * u + 32768) >> 16)) | (uint32_t)clamp255(Y + ((-22554 * u - 46802 * v + 32768) >> 16)) << 8 |
           (uint32_t)clamp255(Y + ((91881 * v + 32768) >> 16)) << 16;
}

__global__ __launch_bounds__(256) void jpeg_color_kernel(JpegParams p)
{
    const int t = blockIdx.x;
    const JpegFrame &f = frame_of<&JpegFrame::tile0>(p, t);
    const int W = f.width, H = f.height, qw = (W + 3) >> 2;
    const int q = (t - f.tile0) * 256 + (int)threadIdx.x;
    const int y = q / qw, x0 = (q - y * qw) * 4;
    if (y >= H) return;
    const uint8_t *base = p.planes + f.plane0;
    const uint8_t *yr = base + (size_t)y * (f.bw[0] * 8) + x0; // x0 + 3 stays inside the row: the plane is padded to whole blocks
    const int Y0 = yr[0], Y1 = yr[1], Y2 = yr[2], Y3 = yr[3];
    uint32_t p0, p1, p2, p3; // B | G << 8 | R << 16 per pixel
    if (f.ncomp == 1) {
        p0 = (uint32_t)Y0 * 0x010101u; p1 = (uint32_t)Y1 * 0x010101u; p2 = (uint32_t)Y2 * 0x010101u; p3 = (uint32_t)Y3 * 0x010101u;
    } else {
        const int hmax = f.hmax, vmax = f.vmax, dw = (W + hmax - 1) / hmax, dh = (H + vmax - 1) / vmax, pwc = f.bw[1] * 8;
        const Quad cb = chroma_quad(base + (size_t)f.blk0[1] * 64, pwc, hmax, vmax, dw, dh, x0, y);
        const Quad cr = chroma_quad(base + (size_t)f.blk0[2] * 64, pwc, hmax, vmax, dw, dh, x0, y);
        p0 = bgr_of(Y0, cb.a, cr.a); p1 = bgr_of(Y1, cb.b, cr.b); p2 = bgr_of(Y2, cb.c, cr.c); p3 = bgr_of(Y3, cb.d, cr.d);
    }
    uint8_t *dst = f.out + (long long)y * f.stride + (long long)x0 * 3;
    if (x0 + 3 < W && (reinterpret_cast<uintptr_t>(dst) & 3) == 0) {
        uint32_t *d4 = reinterpret_cast<uint32_t *>(dst); // B0 G0 R0 B1 | G1 R1 B2 G2 | R2 B3 G3 R3
        d4[0] = p0 | p1 << 24;
        d4[1] = p1 >> 8 | p2 << 16;
        d4[2] = p2 >> 16 | p3 << 8;
    } else {
        const uint32_t px[4] = {p0, p1, p2, p3};
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (x0 + i < W) { dst[3 * i] = (uint8_t)px[i]; dst[3 * i + 1] = (uint8_t)(px[i] >> 8); dst[3 * i + 2] = (uint8_t)(px[i] >> 16); }
    }
}

// EXIF orientation 2..8: the pixels of jpeg_color_kernel, stored through the index map of rfd.h ("EXIF orientation").  A workgroup
// owns a kJpegOrientTile square of the OUTPUT frame, whose origin is a multiple of the tile and so of 4.  The square is the image
// of a rectangle of the stored frame (mirrored and, for 5..8, transposed); that rectangle may start at any x, and chroma_quad wants
// a multiple of 4, so the workgroup computes the quads that enclose it: up to 17 per row, 16 where the stored width is a multiple
// of 4.  It walks them along STORED rows, so the plane reads are row-contiguous as in jpeg_color_kernel, and parks each pixel as
// one B | G << 8 | R << 16 word in LDS.  After the barrier it walks OUTPUT rows: a thread gathers four neighbouring output pixels
// and stores them by jpeg_color_kernel's rule.  A wave stores 4 rows of 192 contiguous bytes.
// LDS pitch 69 words.  The gather is 32-bit reads, which bank by (word mod 32) within each half of a wave.  A half covers 8 quads
// x 4 output rows.  Transposed (5..8), pixel i of quad q in row r reads word +-(4 q + i) * 69 +- r + c: 4 * 69 q = 20 q (mod 32)
// runs over the eight multiples of 4 and r fills the residues, 32 distinct banks.  Not transposed, it reads word +-69 r +- (4 q +
// i) + c = +-5 r +- 4 q (mod 32), distinct again.  The writes of the first phase (16 quads x 2 rows per half, words 69 ry + 4 q + i)
// are 2-way: q and q + 8 share a bank.
constexpr int kOrientPitch = kJpegOrientTile + 5;

__global__ __launch_bounds__(256) void jpeg_color_oriented_kernel(JpegOrientedParams p)
{
    constexpr int T = kJpegOrientTile;
    __shared__ uint32_t px[T * kOrientPitch];
    const int t = blockIdx.x;
    int lo = 0, hi = p.n - 1; // the frame whose first tile is the last one <= t: tile0 ascends strictly
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (p.oriented[mid].tile0 <= t) lo = mid; else hi = mid - 1;
    }
    const JpegOrientedFrame &of = p.oriented[lo];
    const JpegFrame &f = p.frames[of.frame];
    const int W = f.width, H = f.height, o = of.orientation; // W, H: the STORED size
    const bool transposed = o >= 5, flipx = o == 2 || o == 3 || o == 7 || o == 8, flipy = o == 3 || o == 4 || o == 6 || o == 7;
    const int Wo = transposed ? H : W, Ho = transposed ? W : H;
    const int tl = t - of.tile0, ty = tl / of.tiles_x, tx = tl - ty * of.tiles_x;
    const int X0 = tx * T, Y0 = ty * T, X1 = min(X0 + T, Wo) - 1, Y1 = min(Y0 + T, Ho) - 1; // the tile's output pixels, inclusive
    // the stored rectangle [sx0, sx1] x [sy0, sy1] they come from
    const int a0 = transposed ? Y0 : X0, a1 = transposed ? Y1 : X1, b0 = transposed ? X0 : Y0, b1 = transposed ? X1 : Y1;
    const int sx0 = flipx ? W - 1 - a1 : a0, sx1 = flipx ? W - 1 - a0 : a1, sy0 = flipy ? H - 1 - b1 : b0, sy1 = flipy ? H - 1 - b0 : b1;
    const int sxa = sx0 & ~3, nq = ((sx1 - sxa) >> 2) + 1, rows = sy1 - sy0 + 1; // nq <= 17: word 4 * 16 + 3 < kOrientPitch; rows <= T
    const uint8_t *base = p.planes + f.plane0;
    const int hmax = f.hmax, vmax = f.vmax, dw = (W + hmax - 1) / hmax, dh = (H + vmax - 1) / vmax, pwc = f.bw[1] * 8;
    for (int k = (int)threadIdx.x; k < nq * rows; k += 256) {
        const int ry = k / nq, y = sy0 + ry, x0 = sxa + (k - ry * nq) * 4; // x0 <= sx1 < W
        const uint8_t *yr = base + (size_t)y * (f.bw[0] * 8) + x0;        // x0 + 3 stays inside the row: the plane is padded to whole blocks
        const int Y0s = yr[0], Y1s = yr[1], Y2s = yr[2], Y3s = yr[3];
        uint32_t *w = px + ry * kOrientPitch + (x0 - sxa);
        if (f.ncomp == 1) {
            w[0] = (uint32_t)Y0s * 0x010101u; w[1] = (uint32_t)Y1s * 0x010101u; w[2] = (uint32_t)Y2s * 0x010101u; w[3] = (uint32_t)Y3s * 0x010101u;
        } else {
            const Quad cb = chroma_quad(base + (size_t)f.blk0[1] * 64, pwc, hmax, vmax, dw, dh, x0, y);
            const Quad cr = chroma_quad(base + (size_t)f.blk0[2] * 64, pwc, hmax, vmax, dw, dh, x0, y);
            w[0] = bgr_of(Y0s, cb.a, cr.a); w[1] = bgr_of(Y1s, cb.b, cr.b); w[2] = bgr_of(Y2s, cb.c, cr.c); w[3] = bgr_of(Y3s, cb.d, cr.d);
        }
    }
    __syncthreads();
    // one output pixel to the right is this many words further in LDS
    const int step = transposed ? (flipy ? -kOrientPitch : kOrientPitch) : (flipx ? -1 : 1);
    for (int k = (int)threadIdx.x; k < T * T / 4; k += 256) {
        const int xo = X0 + 4 * ((k & 7) | (k >> 2 & 8)), yo = Y0 + ((k >> 3 & 3) | (k >> 6) << 2); // a half wave: 8 quads x 4 rows
        if (xo > X1 || yo > Y1) continue;
        const int a = transposed ? yo : xo, b = transposed ? xo : yo;
        const int at = ((flipy ? H - 1 - b : b) - sy0) * kOrientPitch + (flipx ? W - 1 - a : a) - sxa;
        uint32_t v[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = xo + i <= X1 ? px[at + i * step] : 0u; // X1 <= Wo - 1: a pixel beyond the row has no word
        uint8_t *dst = f.out + (long long)yo * f.stride + (long long)xo * 3;
        if (xo + 3 < Wo && (reinterpret_cast<uintptr_t>(dst) & 3) == 0) {
            uint32_t *d4 = reinterpret_cast<uint32_t *>(dst); // B0 G0 R0 B1 | G1 R1 B2 G2 | R2 B3 G3 R3
            d4[0] = v[0] | v[1] << 24;
            d4[1] = v[1] >> 8 | v[2] << 16;
            d4[2] = v[2] >> 16 | v[3] << 8;
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (xo + i < Wo) { dst[3 * i] = (uint8_t)v[i]; dst[3 * i + 1] = (uint8_t)(v[i] >> 8); dst[3 * i + 2] = (uint8_t)(v[i] >> 16); }
        }
    }
}

// ---- reduced size (rfd.h, "JPEG decode, reduced size"): jidctred.c's 4 x 4, 2 x 2 and 1 x 1 inverse DCTs, and the 8 x 8 one for
// the chroma of a 4:2:0 file at 1/2, in ONE launch.  A workgroup belongs to one component of one frame (JpegScaledFrame::cgroup),
// so the size n is uniform in it, and covers 256 / n consecutive blocks of the component's plane, 64 / n per wave.
//   n = 8   jpeg_idct_kernel's form: 8 lanes per block, lane j column j, then row j, one 8-byte store.
//   n = 4   a wave owns 16 blocks.  Column pass: 16 blocks x the 7 columns that are read (0 1 2 3 5 6 7) = 112 tasks over the 64
//           lanes, block fastest; a task gathers the 7 frequencies that are read from its block's run and leaves 4 words.  Row
//           pass: lane = block + 16 * row; it reads its row's 7 words and stores 4 samples as one word.  Neighbouring lanes hold
//           neighbouring blocks of a block row, so the wave stores 4 rows of 64 contiguous bytes.
//   n = 2   a wave owns 32 blocks: 32 x 5 columns (0 1 3 5 7) = 160 tasks, 2 words each; lane = block + 32 * row, 5 words in, one
//           2-byte store; 2 rows of 64 contiguous bytes per wave.
//   n = 1   one lane per block, no LDS: descale(dc, 3); a wave stores 64 contiguous bytes.
// Only the frequencies in the read set are gathered and multiplied.  LDS holds [block][row][column index] words; all accesses are
// 32-bit, which bank by (word mod 32) within each half of a wave.
//   n = 4   block pitch 34, row pitch 7.  A half of the column pass is 16 blocks x 2 column indices: word 34 b + ci = 2 b + ci (mod
//           32), 32 distinct banks.  A half of the row pass is 16 blocks x 2 rows r, r + 1: word 34 b + 7 r + k = 2 b + 7 r + k, and
//           7 r, 7 r + 7 differ in parity: 32 distinct banks for every k.
//   n = 2   block pitch 11, row pitch 5.  A half of either pass is 32 blocks at one column index / one row: word 11 b + const, and 11
//           is odd: 32 distinct banks.
constexpr int kRed4Block = 34, kRed4Row = 7, kRed2Block = 11, kRed2Row = 5;
static_assert(64 * kRed4Block <= kJpegGroupBlocks * kWsBlock && 128 * kRed2Block <= kJpegGroupBlocks * kWsBlock, "the three layouts share one array");

// the frequency x[r] of column `col` of a block: zero past the block's run
#define RFD_JPEG_GATHER(r) \
    { const int nat = (r) * 8 + col, z = kZigzagOf[nat]; x##r = z < count ? (U)((int)run[z] * (int)q[nat]) : 0u; }

__global__ __launch_bounds__(256) void jpeg_idct_reduced_kernel(JpegScaledParams p)
{
    __shared__ U ws[kJpegGroupBlocks * kWsBlock];
    const int g = blockIdx.x;
    int lo = 0, hi = p.n - 1; // the frame whose first workgroup is the last one <= g: cgroup[0] ascends strictly
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (p.scaled[mid].cgroup[0] <= g) lo = mid; else hi = mid - 1;
    }
    const JpegFrame &f = p.frames[lo];
    const JpegScaledFrame &sf = p.scaled[lo];
    const int c = (f.ncomp == 3 && g >= sf.cgroup[1]) ? (g >= sf.cgroup[2] ? 2 : 1) : 0;
    const int n = sf.n[c], bw = f.bw[c], nb = bw * f.bh[c], pitch = sf.pitch[c];
    const uint32_t *rec = p.rec + f.rec0 + (unsigned)f.blk0[c];
    const int16_t *coef = p.coef + f.coef0;
    const uint16_t *q = f.quant[c];
    uint8_t *plane = p.planes + sf.plane[c];
    const int t = (int)threadIdx.x, wave = t >> 6, lane = t & 63;
    if (n == 8) { // jpeg_idct_kernel's body over this kernel's descriptors, copied so that that kernel's code stays what it was: keep in step with it
        const int lb = t >> 3, j = t & 7, b = (g - sf.cgroup[c]) * 32 + lb;
        const bool valid = b < nb;
        U x[8], o[8];
        {
            const uint32_t r = valid ? rec[b] : 0u;
            const int count = min((int)(r & 127u), 64);
            const int16_t *run = coef + (r >> 7);
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int nat = k * 8 + j, z = kZigzagOf[nat];
                x[k] = z < count ? (U)((int)run[z] * (int)q[nat]) : 0u;
            }
        }
        idct_1d(x, o); // column j
        U *w = ws + lb * kWsBlock;
#pragma unroll
        for (int k = 0; k < 8; ++k) w[k * kWsRow + j] = (U)descale(o[k], 13 - 2);
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 8; ++k) x[k] = w[j * kWsRow + k];
        idct_1d(x, o); // row j
        if (!valid) return;
        uint32_t lo4 = 0, hi4 = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            lo4 |= (uint32_t)min(max(descale(o[k], 13 + 2 + 3) + 128, 0), 255) << (8 * k);
            hi4 |= (uint32_t)min(max(descale(o[k + 4], 13 + 2 + 3) + 128, 0), 255) << (8 * k);
        }
        const int by = b / bw, bx = b - by * bw;
        *reinterpret_cast<uint2 *>(plane + ((size_t)by * 8 + j) * (size_t)pitch + (size_t)bx * 8) = make_uint2(lo4, hi4);
    } else if (n == 4) {
        const int wb0 = (g - sf.cgroup[c]) * 64 + wave * 16; // the wave's first block
        for (int k = lane; k < 16 * 7; k += 64) {
            const int lb = k & 15, ci = k >> 4, col = ci + (ci >> 2), b = wb0 + lb;
            const uint32_t r = b < nb ? rec[b] : 0u;
            const int count = min((int)(r & 127u), 64);
            const int16_t *run = coef + (r >> 7);
            U x0, x1, x2, x3, x5, x6, x7;
            RFD_JPEG_GATHER(0) RFD_JPEG_GATHER(1) RFD_JPEG_GATHER(2) RFD_JPEG_GATHER(3) RFD_JPEG_GATHER(5) RFD_JPEG_GATHER(6) RFD_JPEG_GATHER(7)
            const U t0 = x0 << 14, t2 = x2 * 15137u - x6 * 6270u, t10 = t0 + t2, t12 = t0 - t2;
            const U a = x5 * 11893u + x1 * 8697u - x7 * 1730u - x3 * 17799u, d = x3 * 7373u + x1 * 20995u - x7 * 4176u - x5 * 4926u;
            U *w = ws + (wave * 16 + lb) * kRed4Block + ci;
            w[0] = (U)descale(t10 + d, 12); w[kRed4Row] = (U)descale(t12 + a, 12);
            w[2 * kRed4Row] = (U)descale(t12 - a, 12); w[3 * kRed4Row] = (U)descale(t10 - d, 12);
        }
        __syncthreads();
        const int lb = lane & 15, row = lane >> 4, b = wb0 + lb;
        if (b >= nb) return;
        const U *w = ws + (wave * 16 + lb) * kRed4Block + row * kRed4Row; // columns 0 1 2 3 5 6 7
        const U x0 = w[0], x1 = w[1], x2 = w[2], x3 = w[3], x5 = w[4], x6 = w[5], x7 = w[6];
        const U t0 = x0 << 14, t2 = x2 * 15137u - x6 * 6270u, t10 = t0 + t2, t12 = t0 - t2;
        const U a = x5 * 11893u + x1 * 8697u - x7 * 1730u - x3 * 17799u, d = x3 * 7373u + x1 * 20995u - x7 * 4176u - x5 * 4926u;
        const uint32_t v = (uint32_t)clamp255(descale(t10 + d, 19) + 128) | (uint32_t)clamp255(descale(t12 + a, 19) + 128) << 8 |
                           (uint32_t)clamp255(descale(t12 - a, 19) + 128) << 16 | (uint32_t)clamp255(descale(t10 - d, 19) + 128) << 24;
        const int by = b / bw, bx = b - by * bw;
        *reinterpret_cast<uint32_t *>(plane + ((size_t)by * 4 + row) * (size_t)pitch + (size_t)bx * 4) = v;
    } else if (n == 2) {
        const int wb0 = (g - sf.cgroup[c]) * 128 + wave * 32;
        for (int k = lane; k < 32 * 5; k += 64) {
            const int lb = k & 31, ci = k >> 5, col = ci ? 2 * ci - 1 : 0, b = wb0 + lb;
            const uint32_t r = b < nb ? rec[b] : 0u;
            const int count = min((int)(r & 127u), 64);
            const int16_t *run = coef + (r >> 7);
            U x0, x1, x3, x5, x7;
            RFD_JPEG_GATHER(0) RFD_JPEG_GATHER(1) RFD_JPEG_GATHER(3) RFD_JPEG_GATHER(5) RFD_JPEG_GATHER(7)
            const U t10 = x0 << 15, t0 = x5 * 6967u + x1 * 29692u - x7 * 5906u - x3 * 10426u;
            U *w = ws + (wave * 32 + lb) * kRed2Block + ci;
            w[0] = (U)descale(t10 + t0, 13); w[kRed2Row] = (U)descale(t10 - t0, 13);
        }
        __syncthreads();
        const int lb = lane & 31, row = lane >> 5, b = wb0 + lb;
        if (b >= nb) return;
        const U *w = ws + (wave * 32 + lb) * kRed2Block + row * kRed2Row; // columns 0 1 3 5 7
        const U t10 = w[0] << 15, t0 = w[3] * 6967u + w[1] * 29692u - w[4] * 5906u - w[2] * 10426u;
        const uint32_t v = (uint32_t)clamp255(descale(t10 + t0, 20) + 128) | (uint32_t)clamp255(descale(t10 - t0, 20) + 128) << 8;
        const int by = b / bw, bx = b - by * bw;
        *reinterpret_cast<uint16_t *>(plane + ((size_t)by * 2 + row) * (size_t)pitch + (size_t)bx * 2) = (uint16_t)v;
    } else {
        const int b = (g - sf.cgroup[c]) * 256 + t;
        if (b >= nb) return;
        const uint32_t r = rec[b];
        const U dc = (r & 127u) ? (U)((int)coef[r >> 7] * (int)q[0]) : 0u;
        const int by = b / bw, bx = b - by * bw;
        plane[(size_t)by * (size_t)pitch + (size_t)bx] = (uint8_t)clamp255(descale(dc, 3) + 128);
    }
}
#undef RFD_JPEG_GATHER

// Where the colour kernels of a scaled frame read: a plane pitch and offset per component (JpegScaledFrame) instead of the 8 x 8
// blocks of JpegFrame.  The planes of a scaled frame fill at most half of the 64 bytes per block that the pool gives the frame, so
// the up to 3 bytes a quad reads beyond the last row of a plane whose pitch is no multiple of 4 stay in the frame's own share.
struct ScaledSrc {
    const uint8_t *y, *cb, *cr;
    int py, pc, ncomp, hup, dw, dh;
    bool replicate;
};
__device__ __forceinline__ ScaledSrc scaled_src(const JpegScaledParams &p, const JpegFrame &f, const JpegScaledFrame &sf)
{
    return ScaledSrc{p.planes + sf.plane[0], p.planes + sf.plane[1], p.planes + sf.plane[2], sf.pitch[0], sf.pitch[1], f.ncomp, sf.hup,
                     (sf.width + sf.hup - 1) / sf.hup, sf.height, sf.replicate != 0};
}
// pixels x0 .. x0 + 3 of row y of the scaled frame, as B | G << 8 | R << 16: jpeg_color_kernel's arithmetic
__device__ __forceinline__ void scaled_quad(const ScaledSrc &s, int x0, int y, uint32_t &p0, uint32_t &p1, uint32_t &p2, uint32_t &p3)
{
    const uint8_t *yr = s.y + (size_t)y * s.py + x0;
    const int Y0 = yr[0], Y1 = yr[1], Y2 = yr[2], Y3 = yr[3];
    if (s.ncomp == 1) {
        p0 = (uint32_t)Y0 * 0x010101u; p1 = (uint32_t)Y1 * 0x010101u; p2 = (uint32_t)Y2 * 0x010101u; p3 = (uint32_t)Y3 * 0x010101u;
    } else {
        const Quad cb = chroma_quad(s.cb, s.pc, s.hup, 1, s.dw, s.dh, x0, y, s.replicate);
        const Quad cr = chroma_quad(s.cr, s.pc, s.hup, 1, s.dw, s.dh, x0, y, s.replicate);
        p0 = bgr_of(Y0, cb.a, cr.a); p1 = bgr_of(Y1, cb.b, cr.b); p2 = bgr_of(Y2, cb.c, cr.c); p3 = bgr_of(Y3, cb.d, cr.d);
    }
}
// four pixels of an output row at dst, W - x0 of them inside the row: jpeg_color_kernel's store rule
__device__ __forceinline__ void store_quad(uint8_t *dst, int inside, uint32_t p0, uint32_t p1, uint32_t p2, uint32_t p3)
{
    if (inside >= 4 && (reinterpret_cast<uintptr_t>(dst) & 3) == 0) {
        uint32_t *d4 = reinterpret_cast<uint32_t *>(dst); // B0 G0 R0 B1 | G1 R1 B2 G2 | R2 B3 G3 R3
        d4[0] = p0 | p1 << 24;
        d4[1] = p1 >> 8 | p2 << 16;
        d4[2] = p2 >> 16 | p3 << 8;
    } else {
        const uint32_t px[4] = {p0, p1, p2, p3};
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (i < inside) { dst[3 * i] = (uint8_t)px[i]; dst[3 * i + 1] = (uint8_t)(px[i] >> 8); dst[3 * i + 2] = (uint8_t)(px[i] >> 16); }
    }
}
// the entry of a tile table whose first tile is the last one <= t (tile0 ascends strictly)
__device__ inline const JpegOrientedFrame &tile_entry(const JpegOrientedFrame *e, int n, int t)
{
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (e[mid].tile0 <= t) lo = mid; else hi = mid - 1;
    }
    return e[lo];
}

// jpeg_color_kernel over the upright frames of a scaled batch: one thread per 4 pixels of a row of the SCALED frame
__global__ __launch_bounds__(256) void jpeg_color_scaled_kernel(JpegScaledParams p)
{
    const int t = blockIdx.x;
    const JpegOrientedFrame &e = tile_entry(p.upright, p.n_upright, t);
    const JpegFrame &f = p.frames[e.frame];
    const JpegScaledFrame &sf = p.scaled[e.frame];
    const int W = sf.width, H = sf.height, qw = (W + 3) >> 2;
    const int q = (t - e.tile0) * 256 + (int)threadIdx.x;
    const int y = q / qw, x0 = (q - y * qw) * 4;
    if (y >= H) return;
    uint32_t p0, p1, p2, p3;
    scaled_quad(scaled_src(p, f, sf), x0, y, p0, p1, p2, p3);
    store_quad(f.out + (long long)y * f.stride + (long long)x0 * 3, W - x0, p0, p1, p2, p3);
}

// jpeg_color_oriented_kernel over the oriented frames of a scaled batch: the stored image is scaled, then the index map is applied
// to the scaled image, so W and H below are the SCALED stored size and the tiles count over the scaled oriented size.  The output
// tile, the LDS tile, its pitch and with them the bank argument are that kernel's.  The tile walk is a copy of that kernel's, made so
// that its code stays what it was (one __forceinline__ walk for both changes that kernel's registers and instruction count): keep the
// two in step.
__global__ __launch_bounds__(256) void jpeg_color_scaled_oriented_kernel(JpegScaledParams p)
{
    constexpr int T = kJpegOrientTile;
    __shared__ uint32_t px[T * kOrientPitch];
    const int t = blockIdx.x;
    const JpegOrientedFrame &of = tile_entry(p.oriented, p.n_oriented, t);
    const JpegFrame &f = p.frames[of.frame];
    const JpegScaledFrame &sf = p.scaled[of.frame];
    const int W = sf.width, H = sf.height, o = of.orientation;
    const bool transposed = o >= 5, flipx = o == 2 || o == 3 || o == 7 || o == 8, flipy = o == 3 || o == 4 || o == 6 || o == 7;
    const int Wo = transposed ? H : W, Ho = transposed ? W : H;
    const int tl = t - of.tile0, ty = tl / of.tiles_x, tx = tl - ty * of.tiles_x;
    const int X0 = tx * T, Y0 = ty * T, X1 = min(X0 + T, Wo) - 1, Y1 = min(Y0 + T, Ho) - 1; // the tile's output pixels, inclusive
    const int a0 = transposed ? Y0 : X0, a1 = transposed ? Y1 : X1, b0 = transposed ? X0 : Y0, b1 = transposed ? X1 : Y1;
    const int sx0 = flipx ? W - 1 - a1 : a0, sx1 = flipx ? W - 1 - a0 : a1, sy0 = flipy ? H - 1 - b1 : b0, sy1 = flipy ? H - 1 - b0 : b1;
    const int sxa = sx0 & ~3, nq = ((sx1 - sxa) >> 2) + 1, rows = sy1 - sy0 + 1; // nq <= 17: word 4 * 16 + 3 < kOrientPitch; rows <= T
    const ScaledSrc src = scaled_src(p, f, sf);
    for (int k = (int)threadIdx.x; k < nq * rows; k += 256) {
        const int ry = k / nq, x0 = sxa + (k - ry * nq) * 4; // x0 <= sx1 < W
        uint32_t *w = px + ry * kOrientPitch + (x0 - sxa);
        scaled_quad(src, x0, sy0 + ry, w[0], w[1], w[2], w[3]);
    }
    __syncthreads();
    const int step = transposed ? (flipy ? -kOrientPitch : kOrientPitch) : (flipx ? -1 : 1); // one output pixel to the right, in LDS words
    for (int k = (int)threadIdx.x; k < T * T / 4; k += 256) {
        const int xo = X0 + 4 * ((k & 7) | (k >> 2 & 8)), yo = Y0 + ((k >> 3 & 3) | (k >> 6) << 2); // a half wave: 8 quads x 4 rows
        if (xo > X1 || yo > Y1) continue;
        const int a = transposed ? yo : xo, b = transposed ? xo : yo;
        const int at = ((flipy ? H - 1 - b : b) - sy0) * kOrientPitch + (flipx ? W - 1 - a : a) - sxa;
        uint32_t v[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = xo + i <= X1 ? px[at + i * step] : 0u; // X1 <= Wo - 1: a pixel beyond the row has no word
        store_quad(f.out + (long long)yo * f.stride + (long long)xo * 3, Wo - xo, v[0], v[1], v[2], v[3]);
    }
}

} // namespace

int launch_jpeg_decode_scaled(const JpegScaledParams &p, hipStream_t s)
{
    if (p.n < 1) return RFD_OK;
    hipLaunchKernelGGL(jpeg_idct_reduced_kernel, dim3((unsigned)p.groups), dim3(256), 0, s, p);
    RFD_HIP(hipGetLastError());
    if (p.n_upright > 0) {
        hipLaunchKernelGGL(jpeg_color_scaled_kernel, dim3((unsigned)p.tiles_upright), dim3(256), 0, s, p);
        RFD_HIP(hipGetLastError());
    }
    if (p.n_oriented > 0) {
        hipLaunchKernelGGL(jpeg_color_scaled_oriented_kernel, dim3((unsigned)p.tiles_oriented), dim3(256), 0, s, p);
        RFD_HIP(hipGetLastError());
    }
    return RFD_OK;
}

int launch_jpeg_decode_oriented(const JpegParams &p, const JpegParams &upright, const JpegOrientedParams &o, hipStream_t s)
{
    if (p.n < 1) return RFD_OK;
    hipLaunchKernelGGL(jpeg_idct_kernel, dim3((unsigned)p.groups), dim3(256), 0, s, p);
    RFD_HIP(hipGetLastError());
    if (upright.n > 0) {
        hipLaunchKernelGGL(jpeg_color_kernel, dim3((unsigned)upright.tiles), dim3(256), 0, s, upright);
        RFD_HIP(hipGetLastError());
    }
    if (o.n > 0) {
        hipLaunchKernelGGL(jpeg_color_oriented_kernel, dim3((unsigned)o.tiles), dim3(256), 0, s, o);
        RFD_HIP(hipGetLastError());
    }
    return RFD_OK;
}

int launch_jpeg_decode(const JpegParams &p, hipStream_t s)
{
    if (p.n < 1) return RFD_OK;
    hipLaunchKernelGGL(jpeg_idct_kernel, dim3((unsigned)p.groups), dim3(256), 0, s, p);
    RFD_HIP(hipGetLastError());
    hipLaunchKernelGGL(jpeg_color_kernel, dim3((unsigned)p.tiles), dim3(256), 0, s, p);
    RFD_HIP(hipGetLastError());
    return RFD_OK;
}

} // namespace rfd
