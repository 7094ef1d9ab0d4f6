// kernels_frame.hip -- frames in camera and decoder formats to packed BGR (include/rfd.h, "frames in camera and decoder formats").
//
//   frame_convert_kernel  one launch per batch.  A thread takes one work item of frame_plan.h: 4 neighbouring pixels of a row, or
//                         of the two rows that share a chroma row in NV12 / NV21 / I420, so a chroma pair is read once.  The
//                         frame of a workgroup is found by binary search over the first workgroups (the rule of frame_of in
//                         kernels_jpeg.hip); a workgroup never spans two frames, so the format switch is uniform.
//
// Consecutive lanes read consecutive dwords of a plane row and store consecutive 12-byte runs of the output row.
// A read is one dword where its 4 bytes lie inside the row and its address is 4-aligned (16 bytes for 4 BGRA / RGBA pixels at a
// 16-aligned address), else single bytes; a store is three dwords where 4 pixels lie inside the row and the address is
// 4-aligned, else single bytes.  Which path runs depends on addresses only and both give the same bytes.  No byte outside
// [0, row_bytes) of a plane row is read, no byte at or past 3 * width of an output row is written.  Offsets are 64-bit: a
// row index times a stride exceeds 2^31 for large frames.  No LDS, no atomics, no scratch.
#include "frame_host.h"

namespace rfd {

namespace {

// Planes and frames are global memory, but their addresses come out of a descriptor, where the compiler cannot see it and would
// emit flat_* accesses; these casts make them global_load / global_store.
#define RFD_GLOBAL __attribute__((address_space(1)))
typedef uint32_t u32x4 __attribute__((ext_vector_type(4))); // a plain vector: HIP's uint4 is a class and cannot be read through the cast
template <class T> __device__ __forceinline__ const RFD_GLOBAL T *global_in(const uint8_t *p) { return (const RFD_GLOBAL T *)p; }
template <class T> __device__ __forceinline__ RFD_GLOBAL T *global_out(uint8_t *p) { return (RFD_GLOBAL T *)p; }

// the frame whose first workgroup is the last one <= g (group0 ascends strictly: every frame has at least one workgroup)
__device__ inline const FrameDesc &frame_of(const FrameParams &p, int g)
{
    int lo = 0, hi = p.n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (p.frames[mid].group0 <= g) lo = mid; else hi = mid - 1;
    }
    return p.frames[lo];
}

// bytes src[0 .. 3] as one little-endian word; `inside` of them lie inside the row, the others read as 0
__device__ __forceinline__ uint32_t load_quad(const uint8_t *src, long long inside)
{
    if (inside >= 4 && (reinterpret_cast<uintptr_t>(src) & 3) == 0) return *global_in<uint32_t>(src);
    const RFD_GLOBAL uint8_t *b = global_in<uint8_t>(src);
    uint32_t v = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (i < inside) v |= (uint32_t)b[i] << (8 * i);
    return v;
}

// bytes src[0 .. 1], as above
__device__ __forceinline__ uint32_t load_pair(const uint8_t *src, long long inside)
{
    if (inside >= 2 && (reinterpret_cast<uintptr_t>(src) & 1) == 0) return *global_in<uint16_t>(src);
    const RFD_GLOBAL uint8_t *b = global_in<uint8_t>(src);
    return (inside >= 1 ? (uint32_t)b[0] : 0u) | (inside >= 2 ? (uint32_t)b[1] << 8 : 0u);
}

// four pixels (B | G << 8 | R << 16 each) of an output row at dst, `inside` of them inside the row: the store rule of store_quad
// in kernels_jpeg.hip
__device__ __forceinline__ void store_quad(uint8_t *dst, int inside, uint32_t p0, uint32_t p1, uint32_t p2, uint32_t p3)
{
    if (inside >= 4 && (reinterpret_cast<uintptr_t>(dst) & 3) == 0) {
        RFD_GLOBAL uint32_t *d4 = global_out<uint32_t>(dst); // B0 G0 R0 B1 | G1 R1 B2 G2 | R2 B3 G3 R3
        d4[0] = p0 | p1 << 24;
        d4[1] = p1 >> 8 | p2 << 16;
        d4[2] = p2 >> 16 | p3 << 8;
    } else {
        const uint32_t px[4] = {p0, p1, p2, p3};
        RFD_GLOBAL uint8_t *d1 = global_out<uint8_t>(dst);
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (i < inside) { d1[3 * i] = (uint8_t)px[i]; d1[3 * i + 1] = (uint8_t)(px[i] >> 8); d1[3 * i + 2] = (uint8_t)(px[i] >> 16); }
    }
}

__device__ __forceinline__ uint32_t byte_of(uint32_t w, int i) { return (w >> (8 * i)) & 255u; }
__device__ __forceinline__ uint32_t swap_rb(uint32_t p) { return (p & 0xFF00u) | ((p >> 16) & 255u) | ((p & 255u) << 16); }
__device__ __forceinline__ uint32_t clamp255(int v) { return (uint32_t)min(max(v, 0), 255); }

// The products are 24-bit ones (v_mul_i32_i24 / v_mad_i32_i24, full rate, where a 32-bit v_mul_lo_u32 is quarter rate): every
// coefficient is below 2^23 in magnitude, every other factor below 2^9, every product and sum inside int32 (rfd.h), so the low
// 32 bits __mul24 gives are exact.  (Measured: 5 % at most; DESIGN.md, "Frames", on what the kernel costs.)
//
// The chroma part of rfd.h's sums for one (U, V), shared by the 2 or 4 luma samples it serves.  The rounding term rides in it,
// and so does -CY * y0: CY * max(Y - y0, 0) = CY * max(Y, y0) - CY * y0, which leaves one max per luma sample.
struct Chroma {
    int r, g, b;
};
__device__ __forceinline__ Chroma chroma_of(const FrameCoef &c, uint32_t U, uint32_t V)
{
    const int u = (int)U - 128, v = (int)V - 128, k = 524288 - __mul24(c.cy, c.y0);
    return Chroma{__mul24(c.cvr, v) + k, __mul24(c.cug, u) + __mul24(c.cvg, v) + k, __mul24(c.cub, u) + k};
}
__device__ __forceinline__ uint32_t bgr_of(const FrameCoef &c, uint32_t Y, const Chroma &k)
{
    const int y = max((int)Y, c.y0); // y0 = 0 in the full ranges
    return clamp255((__mul24(c.cy, y) + k.b) >> 20) | clamp255((__mul24(c.cy, y) + k.g) >> 20) << 8 | clamp255((__mul24(c.cy, y) + k.r) >> 20) << 16;
}
// pixels x0 .. x0 + 3 of one luma row (yw: its 4 bytes) under the chroma pairs a (x0, x0 + 1) and b (x0 + 2, x0 + 3)
__device__ __forceinline__ void store_luma_row(uint8_t *dst, int inside, const FrameCoef &c, uint32_t yw, const Chroma &a, const Chroma &b)
{
    store_quad(dst, inside, bgr_of(c, byte_of(yw, 0), a), bgr_of(c, byte_of(yw, 1), a), bgr_of(c, byte_of(yw, 2), b), bgr_of(c, byte_of(yw, 3), b));
}

} // namespace

__global__ __launch_bounds__(256) void frame_convert_kernel(FrameParams p)
{
    const int g = blockIdx.x;
    const FrameDesc f = frame_of(p, g); // a copy: no store of this thread can then be taken for a write to the descriptor
    const int W = f.width, quads = f.quads;
    const int q = (g - f.group0) * kFrameGroup + (int)threadIdx.x;
    const int r = q / quads, x0 = (q - r * quads) * 4;
    if (r >= f.item_rows) return;
    const int inside = W - x0; // pixels of this quad inside the row, >= 1
    const int format = f.format;
    if (format >= RFD_PIXEL_NV12 && format <= RFD_PIXEL_I420) {
        const int y0 = 2 * r, cw = (W + 1) >> 1;
        uint32_t u0, v0, u1, v1; // the chroma pairs under x0, x0 + 1 and x0 + 2, x0 + 3
        if (format == RFD_PIXEL_I420) {
            const int i0 = x0 >> 1;
            const uint32_t uu = load_pair(f.plane[1] + (long long)r * f.stride[1] + i0, cw - i0);
            const uint32_t vv = load_pair(f.plane[2] + (long long)r * f.stride[2] + i0, cw - i0);
            u0 = uu & 255u; u1 = uu >> 8; v0 = vv & 255u; v1 = vv >> 8;
        } else { // U V U V (NV12) or V U V U (NV21): the pair under pixel x lies at byte x & ~1 of the row
            const uint32_t w = load_quad(f.plane[1] + (long long)r * f.stride[1] + x0, 2LL * cw - x0);
            const int first = format == RFD_PIXEL_NV12 ? 0 : 1;
            u0 = byte_of(w, first); v0 = byte_of(w, 1 - first); u1 = byte_of(w, 2 + first); v1 = byte_of(w, 3 - first);
        }
        const Chroma a = chroma_of(f.coef, u0, v0), b = chroma_of(f.coef, u1, v1);
        const uint8_t *yr = f.plane[0] + (long long)y0 * f.stride[0] + x0;
        uint8_t *dst = f.out + (long long)y0 * f.out_stride + (long long)x0 * 3;
        store_luma_row(dst, inside, f.coef, load_quad(yr, inside), a, b);
        if (y0 + 1 < f.height) store_luma_row(dst + f.out_stride, inside, f.coef, load_quad(yr + f.stride[0], inside), a, b);
        return;
    }
    const long long row = (long long)r;
    uint8_t *dst = f.out + row * f.out_stride + (long long)x0 * 3;
    uint32_t p0, p1, p2, p3;
    if (format == RFD_PIXEL_YUYV || format == RFD_PIXEL_UYVY) { // Y0 U Y1 V | U Y0 V Y1: 4 bytes per pixel pair
        const uint8_t *src = f.plane[0] + row * f.stride[0] + 2LL * x0;
        const long long left = 4LL * ((W + 1) >> 1) - 2LL * x0;
        const uint32_t w0 = load_quad(src, left), w1 = load_quad(src + 4, left - 4);
        const int yb = format == RFD_PIXEL_YUYV ? 0 : 1, ub = 1 - yb;
        const Chroma a = chroma_of(f.coef, byte_of(w0, ub), byte_of(w0, ub + 2)), b = chroma_of(f.coef, byte_of(w1, ub), byte_of(w1, ub + 2));
        p0 = bgr_of(f.coef, byte_of(w0, yb), a); p1 = bgr_of(f.coef, byte_of(w0, yb + 2), a);
        p2 = bgr_of(f.coef, byte_of(w1, yb), b); p3 = bgr_of(f.coef, byte_of(w1, yb + 2), b);
    } else if (format == RFD_PIXEL_GRAY) {
        const uint32_t w = load_quad(f.plane[0] + row * f.stride[0] + x0, inside);
        p0 = byte_of(w, 0) * 0x010101u; p1 = byte_of(w, 1) * 0x010101u; p2 = byte_of(w, 2) * 0x010101u; p3 = byte_of(w, 3) * 0x010101u;
    } else if (format == RFD_PIXEL_BGRA || format == RFD_PIXEL_RGBA) { // the fourth byte is dropped
        const uint8_t *src = f.plane[0] + row * f.stride[0] + 4LL * x0;
        if (inside >= 4 && (reinterpret_cast<uintptr_t>(src) & 15) == 0) {
            const u32x4 w = *global_in<u32x4>(src);
            p0 = w.x; p1 = w.y; p2 = w.z; p3 = w.w;
        } else {
            const long long left = 4LL * inside;
            p0 = load_quad(src, left); p1 = load_quad(src + 4, left - 4); p2 = load_quad(src + 8, left - 8); p3 = load_quad(src + 12, left - 12);
        }
        p0 &= 0xFFFFFFu; p1 &= 0xFFFFFFu; p2 &= 0xFFFFFFu; p3 &= 0xFFFFFFu;
        if (format == RFD_PIXEL_RGBA) { p0 = swap_rb(p0); p1 = swap_rb(p1); p2 = swap_rb(p2); p3 = swap_rb(p3); }
    } else { // BGR, RGB: 12 bytes, the layout of store_quad read back
        const uint8_t *src = f.plane[0] + row * f.stride[0] + 3LL * x0;
        const long long left = 3LL * inside;
        const uint32_t w0 = load_quad(src, left), w1 = load_quad(src + 4, left - 4), w2 = load_quad(src + 8, left - 8);
        p0 = w0 & 0xFFFFFFu; p1 = w0 >> 24 | (w1 & 0xFFFFu) << 8; p2 = w1 >> 16 | (w2 & 255u) << 16; p3 = w2 >> 8;
        if (format == RFD_PIXEL_RGB) { p0 = swap_rb(p0); p1 = swap_rb(p1); p2 = swap_rb(p2); p3 = swap_rb(p3); }
    }
    store_quad(dst, inside, p0, p1, p2, p3);
}

int launch_frame_convert(const FrameParams &p, hipStream_t s)
{
    if (p.n <= 0 || p.groups <= 0) return RFD_OK;
    hipLaunchKernelGGL(frame_convert_kernel, dim3((unsigned)p.groups), dim3(kFrameGroup), 0, s, p);
    RFD_HIP(hipGetLastError());
    return RFD_OK;
}

} // namespace rfd
