// kernels_jpeg_encode.hip -- BGR frames to baseline JPEG files (include/rfd.h, "JPEG encode").  Four launches per call, whatever
// the number and sizes of its images; every workgroup has kEncGroup = 256 threads.
//
//   jpeg_encode_blocks_kernel      pixels -> quantised coefficients.  8 threads per 8 x 8 block, 32 blocks per workgroup: thread r
//                                  reads row r of the block's pixels (colour, edge replication, downsampling), runs the row pass
//                                  of jfdctint.c and leaves it in LDS; then, as column r, the column pass and the quantisation,
//                                  into LDS in zigzag order; the block leaves as 128 contiguous bytes.  A dummy block does the work
//                                  of the block whose DC it repeats and drops the AC.  A component reads the pixels it needs:
//                                  4:2:0 frames are read three times (L2 serves the second and third).
//   jpeg_encode_entropy_kernel     one workgroup per restart interval, run twice.  The workgroup walks its blocks in chunks of
//                                  kEncChunk, one block per thread: the bit length of every block (DC difference against the block
//                                  before it of the same component, read straight from the coefficients; AC symbols), a workgroup
//                                  prefix sum of the lengths, then every thread packs its block into the chunk's bit buffer in LDS
//                                  (LDS `or`; only the first and last word of a block are shared with a neighbour).  The whole
//                                  bytes of the buffer leave 256 at a time, a second prefix sum counting the FF bytes that take a
//                                  stuffed 00 behind them; the bits of a last partial byte open the next chunk.  <false> only adds
//                                  up the interval's length; <true>, behind the assembly kernel, writes the bytes where they belong
//                                  in the slot, and RSTn or EOI behind them.
//   jpeg_encode_assemble_kernel    one workgroup per image: exclusive scan of the interval lengths (64-bit), the capacity check,
//                                  size, and the header of a file that fits.
//
// No global atomics, no scratch; every value is written with vector stores.  Memory safety does not depend on the data: the bit
// buffer holds kEncChunk blocks at kEncMaxBlockBits, which no block can exceed (coefficients are clamped to what the tables can
// code), and a slot is written only when the scan has shown that the whole file fits.
#include "jpeg_encode_host.h"

namespace rfd {

namespace {

#define RFD_GLOBAL __attribute__((address_space(1)))
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
template <class T> __device__ __forceinline__ const RFD_GLOBAL T *global_in(const void *p) { return (const RFD_GLOBAL T *)p; }
template <class T> __device__ __forceinline__ RFD_GLOBAL T *global_out(void *p) { return (RFD_GLOBAL T *)p; }

// zigzag position of natural index n (the inverse of kEncNatural)
__device__ const uint8_t kZigzagOf[64] = {0,  1,  5,  6,  14, 15, 27, 28, 2,  4,  7,  13, 16, 26, 29, 42, 3,  8,  12, 17, 25, 30, 41, 43, 9,  11, 18, 24, 31, 40, 44, 53,
                                          10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38, 46, 51, 55, 60, 21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63};

// the image whose first workgroup (of the block kernel) or first interval is the last one <= g: both ascend strictly
template <bool kByGroup> __device__ inline int image_of(const EncParams &p, int g)
{
    int lo = 0, hi = p.n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        const int first = kByGroup ? p.imgs[mid].group0 : p.imgs[mid].interval0;
        if (first <= g) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// Exclusive prefix sum of v over the 256 threads of the workgroup; *total: the sum.  tmp: kScanTmp elements of LDS; the waves'
// sums lie two elements apart, so that their reads cannot merge into a 128-bit LDS read, which this library does not issue where
// EXEC may be partial.  Two barriers, the first of which also ends whatever the workgroup did with LDS before.
constexpr int kScanTmp = 2 * kEncGroup / 64;
template <class T> __device__ __forceinline__ T group_scan(T v, T *tmp, T *total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    T inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const T t = __shfl_up(inc, o, 64);
        if (lane >= o) inc += t;
    }
    __syncthreads();
    if (lane == 63) tmp[2 * wave] = inc;
    __syncthreads();
    T base = 0, sum = 0;
#pragma unroll
    for (int w = 0; w < kEncGroup / 64; ++w) {
        const T t = tmp[2 * w];
        if (w < wave) base += t;
        sum += t;
    }
    *total = sum;
    return base + inc - v;
}

// ---- pixels -> coefficients ----

// N neighbouring pixels of a row from column x0 on, as B | G << 8 | R << 16.  Dwords where the run lies inside the row and begins
// at a 4-aligned address, else single bytes with the columns at and past W reading pixel W - 1; both give the same values.
template <int N> __device__ __forceinline__ void load_run(const uint8_t *row, int x0, int W, uint32_t (&px)[N])
{
    const uint8_t *s = row + 3LL * x0;
    if (x0 + N <= W && (reinterpret_cast<uintptr_t>(s) & 3) == 0) {
        const RFD_GLOBAL uint32_t *w = global_in<uint32_t>(s);
        uint32_t d[3 * N / 4];
#pragma unroll
        for (int k = 0; k < 3 * N / 4; ++k) d[k] = w[k];
#pragma unroll
        for (int i = 0; i < N; ++i) {
            const int k = (3 * i) >> 2, sh = ((3 * i) & 3) * 8;
            uint32_t v = d[k] >> sh;
            if (sh > 8) v |= d[k + 1] << (32 - sh); // 3 i + 2 < 3 N: d[k + 1] exists
            px[i] = v & 0xFFFFFFu;
        }
    } else {
#pragma unroll
        for (int i = 0; i < N; ++i) {
            const RFD_GLOBAL uint8_t *b = global_in<uint8_t>(row + 3LL * min(x0 + i, W - 1));
            px[i] = (uint32_t)b[0] | (uint32_t)b[1] << 8 | (uint32_t)b[2] << 16;
        }
    }
}

// jccolor.c: one of Y, Cb, Cr of a pixel.  24-bit products: every coefficient is below 2^16, every sum below 2^25.
struct Colour {
    int r, g, b, add;
};
__device__ __forceinline__ Colour colour_of(int c)
{
    if (c == 0) return Colour{19595, 38470, 7471, 32768};
    if (c == 1) return Colour{-11059, -21709, 32768, (128 << 16) + 32767};
    return Colour{32768, -27439, -5329, (128 << 16) + 32767};
}
__device__ __forceinline__ int sample_of(const Colour &k, uint32_t px)
{
    return (__mul24(k.r, (int)(px >> 16)) + __mul24(k.g, (int)((px >> 8) & 255u)) + __mul24(k.b, (int)(px & 255u)) + k.add) >> 16;
}

__device__ __forceinline__ int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// jfdctint.c, one pass over eight values: the row pass (kFirst) scales up by 2 bits, the column pass takes them off again
template <bool kFirst> __device__ __forceinline__ void fdct_pass(int (&d)[8])
{
    constexpr int n = kFirst ? 13 - 2 : 13 + 2;
    const int tmp0 = d[0] + d[7], tmp7 = d[0] - d[7], tmp1 = d[1] + d[6], tmp6 = d[1] - d[6];
    const int tmp2 = d[2] + d[5], tmp5 = d[2] - d[5], tmp3 = d[3] + d[4], tmp4 = d[3] - d[4];
    const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    d[0] = kFirst ? (tmp10 + tmp11) << 2 : descale(tmp10 + tmp11, 2);
    d[4] = kFirst ? (tmp10 - tmp11) << 2 : descale(tmp10 - tmp11, 2);
    int z1 = (tmp12 + tmp13) * 4433;
    d[2] = descale(z1 + tmp13 * 6270, n);
    d[6] = descale(z1 - tmp12 * 15137, n);
    z1 = tmp4 + tmp7;
    int z2 = tmp5 + tmp6, z3 = tmp4 + tmp6, z4 = tmp5 + tmp7;
    const int z5 = (z3 + z4) * 9633;
    const int t4 = tmp4 * 2446, t5 = tmp5 * 16819, t6 = tmp6 * 25172, t7 = tmp7 * 12299;
    z1 *= -7373; z2 *= -20995;
    z3 = z3 * -16069 + z5; z4 = z4 * -3196 + z5;
    d[7] = descale(t4 + z1 + z3, n);
    d[5] = descale(t5 + z2 + z4, n);
    d[3] = descale(t6 + z2 + z3, n);
    d[1] = descale(t7 + z1 + z4, n);
}

} // namespace

__global__ __launch_bounds__(kEncGroup) void jpeg_encode_blocks_kernel(EncParams p)
{
    __shared__ int ws[kEncBlocksPerGroup][64];       // the row pass
    __shared__ uint32_t zz[kEncBlocksPerGroup][32];  // the quantised block in zigzag order, two i16 per word
    const int g = blockIdx.x;
    const int img = image_of<true>(p, g);
    if (p.count != nullptr && img >= *p.count) return; // the whole workgroup: a workgroup never spans two images
    const EncImage *d = &p.imgs[img];
    const int lb = threadIdx.x >> 3, r = threadIdx.x & 7;
    const int blocks = d->blocks;
    const int b_mine = (g - d->group0) * kEncBlocksPerGroup + lb;
    const bool live = b_mine < blocks;
    const int b = live ? b_mine : blocks - 1; // the threads past the image's last block keep the barriers company
    const int c = p.ncomp == 3 ? (b >= d->comp0[2] ? 2 : b >= d->comp0[1] ? 1 : 0) : 0;
    const int rel = b - d->comp0[c], bw = d->bw[c], wb = d->wb[c], hb = d->hb[c];
    const int by = rel / bw, bx = rel - by * bw;
    const int h = c == 0 ? p.h : 1;
    const int fx = c == 0 ? 1 : p.h, fy = c == 0 ? 1 : p.v; // input samples per sample of this component
    // the block whose samples this one transforms: itself, or for a dummy block the one whose DC it repeats
    const bool dummy = bx >= wb || by >= hb;
    int sx = bx, sy = by;
    if (by >= hb) { sy = hb - 1; sx = min(bx / h * h + h - 1, wb - 1); }
    else if (bx >= wb) sx = wb - 1;
    const int W = d->width, H = d->height;
    const int y = min(sy * 8 + r, d->ch[c] - 1);   // downsampled rows repeat the component's last one
    const uint8_t *row0 = d->src + (long long)min(y * fy, H - 1) * d->stride;
    const Colour k = colour_of(c);
    int s[8];
    if (fx == 1) { // fy == 1 as well: there is no 1 x 2 sampling
        uint32_t px[8];
        load_run<8>(row0, sx * 8, W, px);
#pragma unroll
        for (int i = 0; i < 8; ++i) s[i] = sample_of(k, px[i]);
    } else {
        uint32_t px[16];
        load_run<16>(row0, sx * 16, W, px);
#pragma unroll
        for (int i = 0; i < 8; ++i) s[i] = sample_of(k, px[2 * i]) + sample_of(k, px[2 * i + 1]);
        if (fy == 2) { // the input's rows are extended to a whole row group only: row 2 y + 1 exists or repeats row H - 1
            const uint8_t *row1 = d->src + (long long)min(y * 2 + 1, H - 1) * d->stride;
            load_run<16>(row1, sx * 16, W, px);
#pragma unroll
            for (int i = 0; i < 8; ++i) s[i] = (s[i] + sample_of(k, px[2 * i]) + sample_of(k, px[2 * i + 1]) + 1 + (i & 1)) >> 2;
        } else {
#pragma unroll
            for (int i = 0; i < 8; ++i) s[i] = (s[i] + (i & 1)) >> 1;
        }
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) s[i] -= 128;
    fdct_pass<true>(s);
#pragma unroll
    for (int i = 0; i < 8; ++i) ws[lb][r * 8 + i] = s[i];
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 8; ++i) s[i] = ws[lb][i * 8 + r]; // column r
    fdct_pass<false>(s);
    const int t = c == 0 ? 0 : 1;
    const RFD_GLOBAL uint32_t *recip = global_in<uint32_t>(p.tables->recip[t]), *half = global_in<uint32_t>(p.tables->half[t]);
    int16_t *zz16 = reinterpret_cast<int16_t *>(&zz[lb][0]);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int n = i * 8 + r;
        const int v = s[i];
        // (|v| + d / 2) / d as a multiplication (jpeg_encode_recip); |v| < 2^15.  An AC value the tables cannot code (above 1023:
        // no 8-bit image gives one) is clamped, so that no block exceeds kEncMaxBlockBits.
        int q = (int)__umulhi((uint32_t)abs(v) + half[n], recip[n]);
        q = min(q, n == 0 ? 1024 : 1023);
        q = v < 0 ? -q : q;
        if (dummy && n != 0) q = 0;
        zz16[kZigzagOf[n]] = (int16_t)q;
    }
    __syncthreads();
    // words r, r + 8, r + 16, r + 24 of the block: 32 contiguous bytes per 8 lanes and store
    uint32_t out[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) out[j] = zz[lb][j * 8 + r];
    if (live) {
        RFD_GLOBAL uint32_t *dst = global_out<uint32_t>(p.coef + ((size_t)d->block0 + (size_t)b) * 64);
#pragma unroll
        for (int j = 0; j < 4; ++j) dst[j * 8 + r] = out[j];
    }
}

// ---- entropy coding ----

namespace {

// one chunk at its worst case, the carried byte in front, and a word of slack for the carry's read
constexpr int kEncBufWords = (kEncChunk * kEncMaxBlockBits / 8 + 1 + 3) / 4 + 2;

// A thread's window on the chunk's bit buffer: bits go in most significant first; whole words leave with an LDS `or`.
struct BitSink {
    uint32_t *buf;
    unsigned long long acc; // the pending bits, left-aligned
    int word, fill;         // the word acc's top belongs to, and the bits of acc in use (below 32 between puts)
    __device__ __forceinline__ void open(uint32_t *b, uint32_t bit) { buf = b; acc = 0; word = (int)(bit >> 5); fill = (int)(bit & 31u); }
    __device__ __forceinline__ void put(uint32_t value, int len) // len <= 26
    {
        acc |= (unsigned long long)value << (64 - fill - len);
        fill += len;
        if (fill >= 32) {
            atomicOr(&buf[word], (uint32_t)(acc >> 32));
            acc <<= 32; ++word; fill -= 32;
        }
    }
    __device__ __forceinline__ void close()
    {
        if (fill > 0) atomicOr(&buf[word], (uint32_t)(acc >> 32));
    }
};

__device__ __forceinline__ int size_of(int v) { return 32 - __clz(abs(v)); }               // 0 for 0
__device__ __forceinline__ uint32_t magnitude_of(int v, int size) { return (uint32_t)(v - (v < 0 ? 1 : 0)) & ((1u << size) - 1u); }

// The AC symbols of a block (zz: its 64 coefficients in zigzag order, global memory): their bits, and with kPack the bits
// themselves into the sink.  ac: the table's code << 8 | length by symbol, in LDS.
template <bool kPack> __device__ __forceinline__ uint32_t walk_ac(const int16_t *zz, const uint32_t *ac, BitSink &sink)
{
    uint32_t bits = 0;
    int run = 0;
    const uint32_t zrl = ac[0xF0], eob = ac[0x00];
    for (int g8 = 0; g8 < 8; ++g8) {
        const u32x4 q = *global_in<u32x4>(zz + g8 * 8);
        const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            if (j == 0 && g8 == 0) continue; // DC
            const int v = (int)(int16_t)(w[j >> 1] >> (16 * (j & 1)));
            if (v == 0) { ++run; continue; }
            const int size = size_of(v);
            const uint32_t e = ac[((run & 15) << 4) | (size & 15)];
            if (kPack) {
                for (int z = run >> 4; z > 0; --z) sink.put(zrl >> 8, (int)(zrl & 255u));
                sink.put(e >> 8, (int)(e & 255u));
                sink.put(magnitude_of(v, size), size);
            } else {
                bits += (uint32_t)(run >> 4) * (zrl & 255u) + (e & 255u) + (uint32_t)size;
            }
            run = 0;
        }
    }
    if (run > 0) {
        if (kPack) sink.put(eob >> 8, (int)(eob & 255u)); else bits += eob & 255u;
    }
    return bits;
}

// block k of MCU `mcu` in the scan's order -> its index among the image's blocks, and its component
__device__ __forceinline__ int scan_block(const EncParams &p, const EncImage *d, int mcu, int k, int *comp)
{
    const int hv = p.h * p.v;
    const int my = mcu / d->mcux, mx = mcu - my * d->mcux;
    if (k < hv) {
        *comp = 0;
        const int j = k / p.h, i = k - j * p.h;
        return (my * p.v + j) * d->bw[0] + mx * p.h + i;
    }
    *comp = 1 + k - hv;
    return d->comp0[*comp] + mcu; // one block per MCU: my * mcux + mx
}

} // namespace

template <bool kWrite> __global__ __launch_bounds__(kEncGroup) void jpeg_encode_entropy_kernel(EncParams p)
{
    __shared__ uint32_t buf[kEncBufWords];
    __shared__ uint32_t ac_tab[2][256];
    __shared__ uint32_t dc_tab[2][12];
    __shared__ uint32_t tmp[kScanTmp];
    const int g = blockIdx.x, tid = threadIdx.x;
    const int img = image_of<false>(p, g);
    if (p.count != nullptr && img >= *p.count) return;
    if (kWrite && p.size[img] < 0) return; // the file does not fit: its slot stays as it is
    const EncImage *d = &p.imgs[img];
    for (int k = tid; k < 512; k += kEncGroup) ac_tab[k >> 8][k & 255] = p.tables->ac[k >> 8][k & 255];
    if (tid < 24) dc_tab[tid / 12][tid % 12] = p.tables->dc[tid / 12][tid % 12];
    __syncthreads();
    const int j = g - d->interval0;
    const int mcu0 = j * d->interval, mcu1 = min(mcu0 + d->interval, d->mcus);
    const int per_mcu = p.ncomp == 3 ? p.h * p.v + 2 : 1;
    const int nblk = (mcu1 - mcu0) * per_mcu; // <= 65535 * 6
    const int16_t *coef = p.coef + (size_t)d->block0 * 64;
    uint8_t *dst = kWrite ? d->out + p.tables->header_len + p.interval_off[g] : nullptr;
    uint32_t carry_bits = 0, carry_byte = 0, outpos = 0;
    for (int s0 = 0; s0 < nblk; s0 += kEncChunk) {
        const int s = s0 + tid;
        const bool valid = s < nblk;
        // this thread's block, its DC difference and its length
        int comp = 0, blk = 0, diff = 0, dsize = 0;
        uint32_t nbits = 0;
        BitSink sink{};
        if (valid) {
            const int mcu = mcu0 + s / per_mcu, k = s - (mcu - mcu0) * per_mcu;
            blk = scan_block(p, d, mcu, k, &comp);
            // the block before it of the same component: the MCU's previous luma block, else the previous MCU's last luma block
            // or its block of the same chroma component; none at the interval's start
            int pred = 0, pc;
            if (comp == 0 && k > 0) pred = coef[(size_t)scan_block(p, d, mcu, k - 1, &pc) * 64];
            else if (mcu > mcu0) pred = coef[(size_t)scan_block(p, d, mcu - 1, comp == 0 ? p.h * p.v - 1 : k, &pc) * 64];
            diff = (int)coef[(size_t)blk * 64] - pred;
            dsize = min(size_of(diff), 11); // |diff| <= 2047 for DC within -1024 .. 1023
            nbits = (dc_tab[comp ? 1 : 0][dsize] & 255u) + (uint32_t)dsize + walk_ac<false>(coef + (size_t)blk * 64, ac_tab[comp ? 1 : 0], sink);
        }
        uint32_t chunk_bits;
        const uint32_t at = group_scan<uint32_t>(nbits, tmp, &chunk_bits);
        // the buffer: the carried bits in front, zeros behind; one word more than the bits need, for the carry's read
        uint32_t total_bits = carry_bits + chunk_bits;
        const int words = (int)((total_bits + 31u) >> 5) + 1;
        for (int k = tid; k < words; k += kEncGroup) buf[k] = k == 0 ? carry_byte << 24 : 0u;
        __syncthreads();
        if (valid) {
            sink.open(buf, carry_bits + at);
            const uint32_t e = dc_tab[comp ? 1 : 0][dsize];
            sink.put(e >> 8, (int)(e & 255u));
            if (dsize > 0) sink.put(magnitude_of(diff, dsize), dsize);
            walk_ac<true>(coef + (size_t)blk * 64, ac_tab[comp ? 1 : 0], sink);
            sink.close();
        }
        if (s0 + kEncChunk >= nblk) { // the interval's last chunk: 1-bits up to the byte
            const uint32_t pad = (0u - total_bits) & 7u;
            if (tid == 0 && pad) atomicOr(&buf[total_bits >> 5], ((1u << pad) - 1u) << (32u - (total_bits & 31u) - pad));
            total_bits += pad;
        }
        __syncthreads();
        const uint32_t nbytes = total_bits >> 3;
        carry_bits = total_bits & 7u;
        carry_byte = (buf[nbytes >> 2] >> (24u - 8u * (nbytes & 3u))) & 255u; // the bits past carry_bits are zero
        for (uint32_t base = 0; base < nbytes; base += kEncGroup) {
            const uint32_t bi = base + (uint32_t)tid;
            const bool in = bi < nbytes;
            const uint32_t byte = in ? (buf[bi >> 2] >> (24u - 8u * (bi & 3u))) & 255u : 0u;
            const uint32_t ff = in && byte == 255u ? 1u : 0u;
            uint32_t ffs;
            const uint32_t before = group_scan<uint32_t>(ff, tmp, &ffs);
            if (kWrite && in) {
                RFD_GLOBAL uint8_t *o = global_out<uint8_t>(dst + outpos + (uint32_t)tid + before);
                o[0] = (uint8_t)byte;
                if (ff) o[1] = 0;
            }
            outpos += min(nbytes - base, (uint32_t)kEncGroup) + ffs;
        }
        // the next chunk clears the buffer behind its first scan's barrier
    }
    if (tid == 0) {
        if (kWrite) {
            RFD_GLOBAL uint8_t *o = global_out<uint8_t>(dst + outpos);
            o[0] = 0xFF;
            o[1] = (uint8_t)(j + 1 < d->intervals ? 0xD0 + (j & 7) : 0xD9);
        } else {
            p.interval_len[g] = outpos;
        }
    }
}

__global__ __launch_bounds__(kEncGroup) void jpeg_encode_assemble_kernel(EncParams p)
{
    __shared__ unsigned long long tmp[kScanTmp];
    const int img = blockIdx.x, tid = threadIdx.x;
    if (p.count != nullptr && img >= *p.count) {
        if (tid == 0) p.size[img] = 0;
        return;
    }
    const EncImage *d = &p.imgs[img];
    const EncTables *t = p.tables;
    unsigned long long running = 0;
    for (int base = 0; base < d->intervals; base += kEncGroup) {
        const int k = base + tid;
        const unsigned long long len = k < d->intervals ? (unsigned long long)p.interval_len[d->interval0 + k] + 2ull : 0ull; // and RSTn or EOI
        unsigned long long sum;
        const unsigned long long at = running + group_scan<unsigned long long>(len, tmp, &sum);
        if (k < d->intervals) p.interval_off[d->interval0 + k] = (uint32_t)min(at, 0xFFFFFFFFull); // used only where the file fits: below 2^31
        running += sum;
    }
    const unsigned long long total = (unsigned long long)t->header_len + running;
    const bool fits = total <= p.slot_bytes && total <= 0x7FFFFFFFull;
    if (tid == 0) p.size[img] = fits ? (int32_t)total : -1;
    if (!fits) return;
    const int size_at = t->size_at, dri_at = t->dri_at;
    for (int k = tid; k < t->header_len; k += kEncGroup) {
        uint32_t byte = t->header[k];
        if (k >= size_at && k < size_at + 4) {
            const uint32_t v = k < size_at + 2 ? (uint32_t)d->height : (uint32_t)d->width;
            byte = (k - size_at) & 1 ? v & 255u : v >> 8;
        }
        if (dri_at > 0 && k >= dri_at && k < dri_at + 2) byte = k == dri_at ? (uint32_t)d->dri >> 8 : (uint32_t)d->dri & 255u;
        global_out<uint8_t>(d->out)[k] = (uint8_t)byte;
    }
}

int launch_jpeg_encode_blocks(const EncParams &p, int groups, hipStream_t s)
{
    if (p.n <= 0 || groups <= 0) return RFD_OK;
    hipLaunchKernelGGL(jpeg_encode_blocks_kernel, dim3((unsigned)groups), dim3(kEncGroup), 0, s, p);
    RFD_HIP(hipGetLastError());
    return RFD_OK;
}

int launch_jpeg_encode_entropy(const EncParams &p, int intervals, bool write, hipStream_t s)
{
    if (p.n <= 0 || intervals <= 0) return RFD_OK;
    if (write) hipLaunchKernelGGL(jpeg_encode_entropy_kernel<true>, dim3((unsigned)intervals), dim3(kEncGroup), 0, s, p);
    else hipLaunchKernelGGL(jpeg_encode_entropy_kernel<false>, dim3((unsigned)intervals), dim3(kEncGroup), 0, s, p);
    RFD_HIP(hipGetLastError());
    return RFD_OK;
}

int launch_jpeg_encode_assemble(const EncParams &p, hipStream_t s)
{
    if (p.n <= 0) return RFD_OK;
    hipLaunchKernelGGL(jpeg_encode_assemble_kernel, dim3((unsigned)p.n), dim3(kEncGroup), 0, s, p);
    RFD_HIP(hipGetLastError());
    return RFD_OK;
}

} // namespace rfd
