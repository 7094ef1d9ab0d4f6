// kernels_pre.hip -- letterbox resize + tensorise on the GPU (gfx950).
//
// Replaces RetinaFaceDetection::_preprocess (reference face_detection.rs:131-198: cv::resize
// INTER_LINEAR on CV_8UC3, paste at the top-left of a zero canvas) and the tensorise loop
// (face_detection.rs:220-232: HWC BGR u8 -> planar RGB f32, raw 0..255).  One pass: each thread
// produces one canvas pixel and writes it in up to three layouts.  HBM-bound byte work:
// reads ~4 source pixels, writes 8 B (NHWC4 bf16) per pixel.
//
// The bilinear arithmetic restates OpenCV's 8-bit fixed-point path (resize.cpp: 11-bit
// coefficients, int horizontal pass, (((b0*(S0>>4))>>16)+((b1*(S1>>4))>>16)+2)>>2 vertical pass,
// and the INTER_AREA 2x2 mean when both scale factors are exactly 2).  Integer-exact.
#include "kernels.h"

namespace rfd {

__device__ __forceinline__ int coef11(float v)
{
    // cv::saturate_cast<short>(v): round half to even, saturate
    int r = __float2int_rn(v);
    return max(-32768, min(32767, r));
}

// one destination pixel of cv::resize(INTER_LINEAR) on CV_8UC3 (see the header): v = B,G,R
__device__ __forceinline__ void resize_linear_px(const uint8_t *src, long long stride, int h, int w, double scale_x,
                                                 double scale_y, int area_fast, int x, int y, int v[3])
{
    if (area_fast) {
        const uint8_t *s0 = src + (long long)(2 * y) * stride + 2 * x * 3;
        const uint8_t *s1 = s0 + stride;
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = (s0[c] + s0[c + 3] + s1[c] + s1[c + 3] + 2) >> 2;
        return;
    }
    float fx = (float)(((double)x + 0.5) * scale_x - 0.5);
    int sx = (int)floorf(fx);
    fx -= (float)sx;
    if (sx < 0) { fx = 0.0f; sx = 0; }
    if (sx >= w - 1) { fx = 0.0f; sx = w - 1; }
    const int a0 = coef11((1.0f - fx) * 2048.0f), a1 = coef11(fx * 2048.0f);
    const int sx1 = min(sx + 1, w - 1);

    float fy = (float)(((double)y + 0.5) * scale_y - 0.5);
    const int sy = (int)floorf(fy);
    fy -= (float)sy;
    const int b0 = coef11((1.0f - fy) * 2048.0f), b1 = coef11(fy * 2048.0f);
    const int sy0 = min(max(sy, 0), h - 1), sy1 = min(max(sy + 1, 0), h - 1);
    const uint8_t *S0 = src + (long long)sy0 * stride;
    const uint8_t *S1 = src + (long long)sy1 * stride;
    // The two taps of a row are the 6 consecutive bytes sx*3 .. sx*3+5 (sx1 = sx + 1): one unaligned 8-byte load per row instead
    // of six byte loads (round 3: the byte loads, not the arithmetic, held this kernel at 1.9 TB/s).  The wide load may touch
    // the 2 bytes behind the second tap, so it is used only where those still lie inside the frame's own extent; the last pixels
    // of the last row (and the clamped right edge, sx1 == sx) take the byte path.  Same integers either way.
    typedef uint64_t u64_unaligned __attribute__((aligned(1)));
    int t0[6], t1[6];
    // (the frame's real extent is (h-1) * stride + w * 3 bytes -- a caller's buffer with padded rows need not own the padding
    //  behind its LAST row (an OpenCV ROI, an exactly-sized allocation); round-3 advisor finding)
    const long long o0 = (long long)sy0 * stride + sx * 3, o1 = (long long)sy1 * stride + sx * 3, lim = (long long)(h - 1) * stride + (long long)w * 3 - 8;
    if (sx1 == sx + 1 && o0 <= lim && o1 <= lim) {
        const uint64_t q0 = *reinterpret_cast<const u64_unaligned *>(src + o0), q1 = *reinterpret_cast<const u64_unaligned *>(src + o1);
#pragma unroll
        for (int k = 0; k < 6; ++k) { t0[k] = (int)((q0 >> (8 * k)) & 0xff); t1[k] = (int)((q1 >> (8 * k)) & 0xff); }
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) { t0[c] = S0[sx * 3 + c]; t0[3 + c] = S0[sx1 * 3 + c]; t1[c] = S1[sx * 3 + c]; t1[3 + c] = S1[sx1 * 3 + c]; }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int r0 = t0[c] * a0 + t0[3 + c] * a1;
        const int r1 = t1[c] * a0 + t1[3 + c] * a1;
        v[c] = (((b0 * (r0 >> 4)) >> 16) + ((b1 * (r1 >> 4)) >> 16) + 2) >> 2;
        v[c] = min(255, max(0, v[c]));
    }
}

__global__ void __launch_bounds__(256) preprocess_kernel(PreParams p)
{
    const int b = blockIdx.z;
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= p.net_w || y >= p.net_h) return;
    const PreImage im = p.imgs[b];

    int v[3] = {0, 0, 0}; // B,G,R of the canvas pixel; outside the pasted region the canvas is 0
    if (x < im.new_w && y < im.new_h) resize_linear_px(im.src, im.stride, im.h, im.w, im.scale_x, im.scale_y, im.area_fast, x, y, v);
    const size_t pix = ((size_t)b * p.net_h + y) * p.net_w + x;
    if (p.out_nhwc4) {
        // u8 -> bf16 is exact (8 significant bits); channel order R,G,B,0 (face_detection.rs:226 [2-i])
        const uint32_t r = __float_as_uint((float)v[2]) >> 16, g = __float_as_uint((float)v[1]) >> 16;
        const uint32_t bl = __float_as_uint((float)v[0]) >> 16;
        uint2 o;
        o.x = r | (g << 16);
        o.y = bl;
        *reinterpret_cast<uint2 *>(p.out_nhwc4 + pix * 4) = o;
    }
    if (p.out_det_img) {
        uint8_t *d = p.out_det_img + pix * 3;
        d[0] = (uint8_t)v[0]; d[1] = (uint8_t)v[1]; d[2] = (uint8_t)v[2];
    }
    if (p.out_tensor) {
        const size_t plane = (size_t)p.net_h * p.net_w;
        float *t = p.out_tensor + (size_t)b * 3 * plane + (size_t)y * p.net_w + x;
        // (p / pixel_scale - mean) / std with scale 1, mean 0, std 1 (face_detection.rs:105-107, 227)
        t[0] = ((float)v[2] / 1.0f - 0.0f) / 1.0f;
        t[plane] = ((float)v[1] / 1.0f - 0.0f) / 1.0f;
        t[2 * plane] = ((float)v[0] / 1.0f - 0.0f) / 1.0f;
    }
}

int launch_preprocess(const PreParams &p, int n, hipStream_t s)
{
    dim3 grid(ceil_div(p.net_w, 64), ceil_div(p.net_h, 4), n);
    hipLaunchKernelGGL(preprocess_kernel, grid, dim3(256), 0, s, p);
    RFD_HIP(hipGetLastError());
    return RFD_OK;
}

__device__ __forceinline__ uint32_t f32_to_bf16_bits(float f)
{
    uint32_t u = __float_as_uint(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (u >> 16) | 0x40u;
    u += 0x7fffu + ((u >> 16) & 1u);
    return u >> 16;
}

__global__ void __launch_bounds__(256) tensor_to_nhwc4_kernel(const float *__restrict__ t,
                                                              bf16_t *__restrict__ out, size_t plane,
                                                              size_t total)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; // pixel index over n*H*W
    if (i >= total) return;
    const size_t b = i / plane, q = i - b * plane;
    const float *s = t + b * 3 * plane + q;
    uint2 o;
    o.x = f32_to_bf16_bits(s[0]) | (f32_to_bf16_bits(s[plane]) << 16);
    o.y = f32_to_bf16_bits(s[2 * plane]);
    *reinterpret_cast<uint2 *>(out + i * 4) = o;
}

int launch_tensor_to_nhwc4(const float *tensor, bf16_t *out, int n, int H, int W, hipStream_t s)
{
    const size_t plane = (size_t)H * W, total = plane * n;
    hipLaunchKernelGGL(tensor_to_nhwc4_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s,
                       tensor, out, plane, total);
    RFD_HIP(hipGetLastError());
    return RFD_OK;
}

// ------------------------------------------------------------------------------------------------
// FaceAlignment::call (face_alignment.rs:27-141).  Set-up: one thread per face estimates the 4-DOF similarity from
// the five key points to the template as cv::estimateAffinePartial2D(LMEDS, 3.0, 2000, 0.99, 10) does (:48-60; restated
// from OpenCV 4.x calib3d ptsetreg.cpp as in oracle/rfd_oracle.c, where every step is cited): 13 two-point samples from a
// cv::RNG re-seeded on every call (so the SAME index pairs for every face), the exact similarity through each pair in f64,
// f32 squared errors, least median, inliers within 2.5 * 1.4826 * (1 + 5 / 3) * sqrt(median), then the least-squares
// similarity over the inliers (the fixed point of the reference's 10 Levenberg-Marquardt iterations on this linear problem;
// documented divergence ~1e-12).  Rounds 1-3 used the all-points closed form: no outlier rejection.  The matrix is then
// inverted as cv::warpAffine does; no model (coincident points) takes the reference's crop + resize branch (:62-110,
// quirks kept).
// Warp: one thread per output pixel, cv::warpAffine's fixed-point coordinates (10 -> 5 fractional bits) and 15-bit
// bilinear weights, out-of-image taps = 0.  Integer-exact against the oracle.
// ------------------------------------------------------------------------------------------------
constexpr int kLmedsIters = 13; // RANSACUpdateNumIters(0.99, 0.45, 2, 2000) = round(log(0.01) / log(1 - 0.55^2)); tests/test_oracle_cpu.py

__device__ __forceinline__ unsigned cv_rng_next(unsigned long long &state) // cv::RNG: multiply-with-carry
{
    state = (unsigned long long)(unsigned)state * 4164903690u + (unsigned)(state >> 32);
    return (unsigned)state;
}

__device__ void similarity_2pt(const float *src, const float *dst, int i0, int i1, double M[6])
{
    const double x1 = src[2 * i0], y1 = src[2 * i0 + 1], x2 = src[2 * i1], y2 = src[2 * i1 + 1];
    const double X1 = dst[2 * i0], Y1 = dst[2 * i0 + 1], X2 = dst[2 * i1], Y2 = dst[2 * i1 + 1];
    const double d = 1. / ((x1 - x2) * (x1 - x2) + (y1 - y2) * (y1 - y2));
    const double S0 = d * ((X1 - X2) * (x1 - x2) + (Y1 - Y2) * (y1 - y2));
    const double S1 = d * ((Y1 - Y2) * (x1 - x2) - (X1 - X2) * (y1 - y2));
    const double S2 = d * ((Y1 - Y2) * (x1 * y2 - x2 * y1) - (X1 * y2 - X2 * y1) * (y1 - y2) - (X1 * x2 - X2 * x1) * (x1 - x2));
    const double S3 = d * (-(X1 - X2) * (x1 * y2 - x2 * y1) - (Y1 * x2 - Y2 * x1) * (x1 - x2) - (Y1 * y2 - Y2 * y1) * (y1 - y2));
    M[0] = S0; M[1] = -S1; M[2] = S2; M[3] = S1; M[4] = S0; M[5] = S3;
}

__device__ __forceinline__ void similarity_errors5(const float *src, const float *dst, const double M[6], float err[5])
{
    const float F0 = (float)M[0], F1 = (float)M[1], F2 = (float)M[2], F3 = (float)M[3], F4 = (float)M[4], F5 = (float)M[5];
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        const float fx = src[2 * i], fy = src[2 * i + 1];
        const float a = F0 * fx + F1 * fy + F2 - dst[2 * i];
        const float b = F3 * fx + F4 * fy + F5 - dst[2 * i + 1];
        err[i] = a * a + b * b;
    }
}

// The key LMedS orders an error by: its bit pattern as an int, the largest int for a NaN of either sign.  As an int a NaN whose
// sign bit is set would rank below every number, and which sign an invalid operation gives its NaN is the platform's choice
// (DESIGN.md section 2), so EVERY NaN ranks above every number.  As lmeds_error_key in oracle/rfd_oracle.c.
__device__ __forceinline__ int lmeds_error_key(float e) { return e != e ? 0x7fffffff : __float_as_int(e); }

// returns false: no model (the reference's empty matrix).  Every array is indexed at compile time (no scratch: tests/test_build_cpu.py).
__device__ bool estimate_similarity_lmeds5(const float *src, const float *dst, double M[6])
{
    unsigned long long rng = 0xffffffffffffffffull; // RNG rng((uint64)-1)
    double best[6] = {0, 0, 0, 0, 0, 0}, min_median = 1.7976931348623157e308;
    float err[5];
    for (int it = 0; it < kLmedsIters; ++it) {
        const int i0 = (int)(cv_rng_next(rng) % 5u);
        int i1;
        do i1 = (int)(cv_rng_next(rng) % 5u); while (i1 == i0);
        double Ms[6];
        similarity_2pt(src, dst, i0, i1, Ms);
        similarity_errors5(src, dst, Ms, err);
        // element 2 of the errors ordered by their keys (std::nth_element on errf.ptr<int>())
        int e0 = lmeds_error_key(err[0]), e1 = lmeds_error_key(err[1]), e2 = lmeds_error_key(err[2]), e3 = lmeds_error_key(err[3]), e4 = lmeds_error_key(err[4]);
#define RFD_CS(a, b) { const int lo_ = min(a, b), hi_ = max(a, b); a = lo_; b = hi_; }
        RFD_CS(e0, e1) RFD_CS(e3, e4) RFD_CS(e2, e4) RFD_CS(e2, e3) RFD_CS(e1, e4) RFD_CS(e0, e3) RFD_CS(e0, e2) RFD_CS(e1, e3) RFD_CS(e1, e2)
#undef RFD_CS
        const double median = (double)__int_as_float(e2);
        if (median < min_median) {
            min_median = median;
#pragma unroll
            for (int k = 0; k < 6; ++k) best[k] = Ms[k];
        }
    }
    if (!(min_median < 1.7976931348623157e308)) return false;
    double sigma = 2.5 * 1.4826 * (1 + 5. / 3) * sqrt(min_median);
    if (!(sigma > 0.001)) sigma = 0.001;
    const float t = (float)(sigma * sigma);
    similarity_errors5(src, dst, best, err);
    int cnt = 0;
    bool use[5];
#pragma unroll
    for (int i = 0; i < 5; ++i) { use[i] = err[i] <= t; cnt += use[i]; }
    if (cnt < 2) return false;
#pragma unroll
    for (int k = 0; k < 6; ++k) M[k] = best[k];
    // least squares over the inliers
    double msx = 0, msy = 0, mdx = 0, mdy = 0;
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        if (!use[i]) continue;
        msx += (double)src[2 * i]; msy += (double)src[2 * i + 1];
        mdx += (double)dst[2 * i]; mdy += (double)dst[2 * i + 1];
    }
    msx /= cnt; msy /= cnt; mdx /= cnt; mdy /= cnt;
    double sxx = 0, sa = 0, sb = 0;
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        if (!use[i]) continue;
        const double xs = (double)src[2 * i] - msx, ys = (double)src[2 * i + 1] - msy;
        const double xd = (double)dst[2 * i] - mdx, yd = (double)dst[2 * i + 1] - mdy;
        sxx += xs * xs + ys * ys;
        sa += xs * xd + ys * yd;
        sb += xs * yd - ys * xd;
    }
    if (sxx > 0.0) {
        const double a = sa / sxx, bb = sb / sxx;
        M[0] = a; M[1] = -bb; M[2] = mdx - (a * msx - bb * msy);
        M[3] = bb; M[4] = a; M[5] = mdy - (bb * msx + a * msy);
    }
    return true;
}

__device__ __forceinline__ int cv_round_sat(double v)
{
    if (v >= 2147483647.0) return 2147483647;
    if (v <= -2147483648.0) return (-2147483647 - 1);
    return __double2int_rn(v);
}

// A face of a launch is done always (total null: the one-face entries) or, in a packed face list, while it lies below
// min(*total, cap): the count is read from HBM, the host never sees it.
__device__ __forceinline__ bool face_in_list(const int *total, int cap, int b) { return !total || b < min(*total, cap); }

__global__ void align_setup_kernel(AlignParams p)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= p.n || !face_in_list(p.total, p.cap, b)) return;
    AlignFace f;
    memset(&f, 0, sizeof f);
    const int found = p.found ? p.found[b] : 3;
    const PreImage im = p.imgs[p.frame ? p.frame[b] : b];
    if (!(found & 1)) {
        f.mode = -2;
    } else if (!(found & 2)) {
        f.mode = -1; // landmarks = None: estimate_affine_partial_2d rejects the empty point set (:48)
    } else {
        const float *src = p.kps + (size_t)b * 10;
        double M[6];
        if (estimate_similarity_lmeds5(src, p.std_lmk, M)) {
            double D = M[0] * M[4] - M[1] * M[3];
            D = D != 0 ? 1. / D : 0;
            const double A11 = M[4] * D, A22 = M[0] * D;
            M[0] = A11; M[1] *= -D; M[3] *= -D; M[4] = A22;
            const double b1 = -M[0] * M[2] - M[1] * M[5], b2 = -M[3] * M[2] - M[4] * M[5];
            M[2] = b1; M[5] = b2;
            for (int i = 0; i < 6; ++i) f.M[i] = M[i];
            f.mode = 0;
        } else { // empty transformation (:62): crop around the box and resize
            const float *det = p.box + (size_t)b * 5;
            const float margin = 44.0f;
            const float bb0 = fmaxf(det[0] - margin / 2.0f, 0.0f), bb1 = fmaxf(det[1] - margin / 2.0f, 0.0f);
            const float bb2 = fmaxf(det[2] + margin / 2.0f, (float)im.w); // `max`, as written (:77)
            const float bb3 = fmaxf(det[1] + margin / 2.0f, (float)im.h); // det[1], as written (:78)
            f.x0 = (int)bb0; f.y0 = (int)bb1;
            f.rw = (int)bb2 - f.x0; f.rh = (int)bb3 - f.y0;
            if (f.rw <= 0 || f.rh <= 0 || f.x0 + f.rw > im.w || f.y0 + f.rh > im.h) {
                f.mode = -3;
            } else {
                f.mode = 1;
                f.scale_x = 1.0 / ((double)p.out_w / f.rw);
                f.scale_y = 1.0 / ((double)p.out_h / f.rh);
                const int ix = cv_round_sat(f.scale_x), iy = cv_round_sat(f.scale_y);
                f.area_fast = fabs(f.scale_x - ix) < 2.220446049250313e-16 && fabs(f.scale_y - iy) < 2.220446049250313e-16 &&
                              ix == 2 && iy == 2;
            }
        }
    }
    p.faces[b] = f;
    p.status[b] = f.mode;
}

// one pixel of the aligned crop of a face with mode >= 0: v = B,G,R.  The arithmetic of both warp kernels.
__device__ __forceinline__ void align_warp_px(const AlignFace &f, const PreImage &im, int x, int y, int v[3])
{
    if (f.mode == 1) {
        resize_linear_px(im.src + (long long)f.y0 * im.stride + f.x0 * 3, im.stride, f.rh, f.rw, f.scale_x, f.scale_y,
                         f.area_fast, x, y, v);
    } else {
        constexpr int AB_BITS = 10, AB_SCALE = 1 << AB_BITS, INTER_BITS = 5, TAB = 1 << INTER_BITS;
        constexpr int round_delta = AB_SCALE / TAB / 2;
        const int X0 = cv_round_sat((f.M[1] * y + f.M[2]) * AB_SCALE) + round_delta;
        const int Y0 = cv_round_sat((f.M[4] * y + f.M[5]) * AB_SCALE) + round_delta;
        const int adelta = cv_round_sat(f.M[0] * x * AB_SCALE), bdelta = cv_round_sat(f.M[3] * x * AB_SCALE);
        const int X = (X0 + adelta) >> (AB_BITS - INTER_BITS), Y = (Y0 + bdelta) >> (AB_BITS - INTER_BITS);
        const int sx = max(-32768, min(32767, X >> INTER_BITS)), sy = max(-32768, min(32767, Y >> INTER_BITS));
        const int fx = X & (TAB - 1), fy = Y & (TAB - 1);
        int wt[4] = {(TAB - fy) * (TAB - fx) * 32, (TAB - fy) * fx * 32, fy * (TAB - fx) * 32, fy * fx * 32};
        if (fx == 0 && fy == 0) { wt[0] = 32767; wt[3] = 1; }
        int acc[3] = {0, 0, 0};
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int px = sx + (t & 1), py = sy + (t >> 1);
            if (px >= 0 && px < im.w && py >= 0 && py < im.h) {
                const uint8_t *s = im.src + (long long)py * im.stride + px * 3;
                acc[0] += s[0] * wt[t]; acc[1] += s[1] * wt[t]; acc[2] += s[2] * wt[t];
            }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = (acc[c] + (1 << 14)) >> 15;
    }
}

__global__ void __launch_bounds__(256) align_warp_kernel(AlignParams p)
{
    const int b = p.face0 + blockIdx.y;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= p.out_w * p.out_h || !face_in_list(p.total, p.cap, b)) return;
    const int y = i / p.out_w, x = i - y * p.out_w;
    const AlignFace &f = p.faces[b];
    uint8_t *d = p.out + ((size_t)b * p.out_h * p.out_w + i) * 3;
    if (f.mode < 0) { d[0] = d[1] = d[2] = 0; return; }
    const PreImage im = p.imgs[p.frame ? p.frame[b] : b];
    int v[3];
    align_warp_px(f, im, x, y, v);
    d[0] = (uint8_t)v[0]; d[1] = (uint8_t)v[1]; d[2] = (uint8_t)v[2];
}

constexpr int kMaxGridY = 65535; // faces per launch of the kernels that take the face from blockIdx.y

int launch_face_align_setup(const AlignParams &p, hipStream_t s)
{
    hipLaunchKernelGGL(align_setup_kernel, dim3(ceil_div(p.n, 64)), dim3(64), 0, s, p);
    RFD_HIP(hipGetLastError());
    return RFD_OK;
}

int launch_face_align(const AlignParams &p, hipStream_t s)
{
    RFD_TRY(launch_face_align_setup(p, s));
    AlignParams q = p;
    for (q.face0 = 0; q.face0 < p.n; q.face0 += kMaxGridY) {
        hipLaunchKernelGGL(align_warp_kernel, dim3(ceil_div(p.out_w * p.out_h, 256), min(p.n - q.face0, kMaxGridY)), dim3(256), 0, s, q);
        RFD_HIP(hipGetLastError());
    }
    return RFD_OK;
}

// ------------------------------------------------------------------------------------------------
// The model inputs of the two stages after alignment (face_quality.rs:43-44,56-101, face_extraction.rs:38-77): resize to the
// model's image_size, BGR -> RGB, (p - mean) * scale, NHWC -> NCHW.  Byte work + two f32 roundings per value, pinned with
// __fsub_rn / __fmul_rn so that no contraction can merge them.  Plane stores: lane i writes float i of a row-major plane.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ void face_tensor_store(const FaceTensorCfg &c, int b, int i, const int v[3], bool zero)
{
    const size_t plane = (size_t)c.out_w * c.out_h;
    float *t = c.out + (size_t)b * 3 * plane + i;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) // output channel R,G,B = crop channel 2,1,0
        t[ch * plane] = zero ? 0.0f : __fmul_rn(__fsub_rn((float)v[2 - ch], c.mean[ch]), c.scale[ch]);
}

// align_warp_kernel + the planes of every config of the crop's own size, from the registers that hold the pixel
__global__ void __launch_bounds__(256) align_warp_tensor_kernel(AlignParams p, FaceTensorParams t)
{
    const int b = p.face0 + blockIdx.y;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= p.out_w * p.out_h || !face_in_list(p.total, p.cap, b)) return;
    const int y = i / p.out_w, x = i - y * p.out_w;
    const AlignFace &f = p.faces[b];
    const bool zero = f.mode < 0;
    int v[3] = {0, 0, 0};
    if (!zero) {
        const PreImage im = p.imgs[p.frame ? p.frame[b] : b];
        align_warp_px(f, im, x, y, v);
    }
    if (p.out) {
        uint8_t *d = p.out + ((size_t)b * p.out_h * p.out_w + i) * 3;
        d[0] = (uint8_t)v[0]; d[1] = (uint8_t)v[1]; d[2] = (uint8_t)v[2];
    }
#pragma unroll
    for (int j = 0; j < kMaxFaceTensors; ++j)
        if (j < t.k) face_tensor_store(t.cfg[j], b, i, v, zero);
}

int launch_face_align_tensors(const AlignParams &a, const FaceTensorParams &t, hipStream_t s)
{
    RFD_TRY(launch_face_align_setup(a, s));
    if (a.total && !a.out && !t.k) return RFD_OK; // a face list alone: the status is all that was asked for
    AlignParams q = a;
    for (q.face0 = 0; q.face0 < a.n; q.face0 += kMaxGridY) {
        hipLaunchKernelGGL(align_warp_tensor_kernel, dim3(ceil_div(a.out_w * a.out_h, 256), min(a.n - q.face0, kMaxGridY)), dim3(256), 0, s, q, t);
        RFD_HIP(hipGetLastError());
    }
    return RFD_OK;
}

// crops in HBM -> the planes of config blockIdx.z of face blockIdx.y: resize (or copy), swap, normalise
__global__ void __launch_bounds__(256) face_tensor_kernel(FaceTensorParams p)
{
    const FaceTensorCfg &c = p.cfg[blockIdx.z];
    const int b = p.face0 + blockIdx.y;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= c.out_w * c.out_h || !face_in_list(p.total, p.cap, b)) return;
    const bool zero = p.status && p.status[b] < 0;
    int v[3] = {0, 0, 0};
    if (!zero) {
        const long long stride = (long long)p.crop_w * 3;
        const uint8_t *src = p.crops + (size_t)b * p.crop_h * stride;
        if (c.same) {
            const uint8_t *s = src + (size_t)i * 3;
            v[0] = s[0]; v[1] = s[1]; v[2] = s[2];
        } else {
            const int y = i / c.out_w, x = i - y * c.out_w;
            resize_linear_px(src, stride, p.crop_h, p.crop_w, c.scale_x, c.scale_y, c.area_fast, x, y, v);
        }
    }
    face_tensor_store(c, b, i, v, zero);
}

int launch_face_tensors(const FaceTensorParams &p, hipStream_t s)
{
    if (p.k < 1) return RFD_OK;
    int px = 0;
    for (int j = 0; j < p.k; ++j) px = max(px, p.cfg[j].out_w * p.cfg[j].out_h);
    FaceTensorParams q = p;
    for (q.face0 = 0; q.face0 < p.n; q.face0 += kMaxGridY) {
        hipLaunchKernelGGL(face_tensor_kernel, dim3(ceil_div(px, 256), min(p.n - q.face0, kMaxGridY), p.k), dim3(256), 0, s, q);
        RFD_HIP(hipGetLastError());
    }
    return RFD_OK;
}

// quality decision rule, face_quality.rs:159-168.  `max_by(|a, b| a.partial_cmp(b).unwrap())` keeps the LAST of equal maxima
// and panics on a NaN: such a row is marked klass = -1 / score = NaN here (the host entry turns it into an error).
__global__ void __launch_bounds__(64) quality_decide_kernel(const float *__restrict__ logits, int n, int classes, float threshold,
                                                           float *__restrict__ score, int *__restrict__ klass)
{
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= n) return;
    const float *l = logits + (size_t)b * classes;
    int best = 0;
    float m = l[0];
    bool nan = m != m;
    for (int i = 1; i < classes; ++i) {
        const float x = l[i];
        nan |= x != x;
        if (x >= m) { m = x; best = i; }
    }
    if (best == 1 && m < threshold) { best = 0; m = l[0]; } // :163-166
    score[b] = nan ? __int_as_float(0x7fc00000) : m;
    klass[b] = nan ? -1 : best;
}

int launch_quality_decide(const float *logits, int n, int classes, float threshold, float *score, int *klass, hipStream_t s)
{
    hipLaunchKernelGGL(quality_decide_kernel, dim3(ceil_div(n, 64)), dim3(64), 0, s, logits, n, classes, threshold, score, klass);
    RFD_HIP(hipGetLastError());
    return RFD_OK;
}

// normalize_outputs, utils.rs:148-154: array / array.norm_l2().  One wave64 per row: lane l sums the squares of elements l,
// l + 64, ... in ascending order, the 64 partial sums meet in a fixed xor butterfly (every lane ends with the same bits: IEEE
// addition commutes), then one correctly rounded square root and one correctly rounded division per element.  The square
// root is the compiler's expansion around the hardware's approximation (__builtin_sqrtf): __fsqrt_rn is the bare hardware
// instruction on this toolchain, one ulp off for some inputs (a subnormal sum of squares among them).
__global__ void __launch_bounds__(256) l2_normalize_kernel(const float *emb, int n, int dim, float *out) // out may be emb
{
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= n) return; // whole waves leave together: every shuffle below runs with all 64 lanes
    const float *x = emb + (size_t)row * dim;
    float s = 0.0f;
    for (int i = lane; i < dim; i += 64) s = __fadd_rn(s, __fmul_rn(x[i], x[i]));
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) s = __fadd_rn(s, __shfl_xor(s, off, 64));
    const float norm = __builtin_sqrtf(s);
    float *o = out + (size_t)row * dim;
    for (int i = lane; i < dim; i += 64) o[i] = __fdiv_rn(x[i], norm);
}

int launch_l2_normalize(const float *emb, int n, int dim, float *out, hipStream_t s)
{
    hipLaunchKernelGGL(l2_normalize_kernel, dim3(ceil_div(n, 4)), dim3(256), 0, s, emb, n, dim, out);
    RFD_HIP(hipGetLastError());
    return RFD_OK;
}

// ------------------------------------------------------------------------------------------------
// FaceAntiSpoofing (face_antispoofing.rs): the inputs of the k miniFAS models of a face, from the source frame and the
// selected box, and the rule on their outputs.
// Geometry: one thread per (face, model) restates _get_scale_image :245-295 and _get_new_box :342-385.  Every f32 operation
// is a single pinned rounding (__fsub_rn ...) in the reference's order, because each result is truncated to an integer pixel
// coordinate: a contraction or a reassociation could move a crop by a pixel.  Rust's `as i32` truncates toward zero,
// saturates and maps NaN to 0; its i32 `+` / `-` wrap (a release build).  Mat::roi (:324) accepts a rectangle iff
// 0 <= x, 0 <= w, x + w <= cols (same in y); cv::resize (:332) rejects an empty one: either makes the reference return Err
// for the whole face, so the k validity bits of a face are reduced to one status.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ int rust_f32_as_i32(float f)
{
    if (f != f) return 0;
    if (f >= 2147483648.0f) return 2147483647;
    if (f <= -2147483648.0f) return -2147483647 - 1;
    return (int)f;
}

__device__ __forceinline__ float rust_f32_min(float a, float b) // f32::min: a NaN operand yields the other one
{
    if (a != a) return b;
    if (b != b) return a;
    return a < b ? a : b;
}

__device__ __forceinline__ int wrap_span(int hi, int lo) // hi - lo + 1 in wrapping i32 arithmetic
{
    return (int)((unsigned)hi - (unsigned)lo + 1u);
}

constexpr int kLiveGeoFaces = 64 / kMaxFaceTensors; // faces per workgroup of the geometry kernel

__global__ void __launch_bounds__(64) liveness_geometry_kernel(LiveParams p)
{
    __shared__ int bad[kLiveGeoFaces];
    const int fl = threadIdx.x / kMaxFaceTensors, j = threadIdx.x % kMaxFaceTensors;
    const int b = blockIdx.x * kLiveGeoFaces + fl;
    if (threadIdx.x < kLiveGeoFaces) bad[threadIdx.x] = 0;
    __syncthreads();
    const bool active = b < p.n && j < p.k;
    const bool found = active && (p.found[b] & 1);
    LiveRoi g;
    memset(&g, 0, sizeof g);
    float weight = 0.0f;
    int ltx = 0, lty = 0, rbx = 0, rby = 0;
    if (found) {
        const float *det = p.box + (size_t)b * 5;
        const LiveImage im = p.imgs[b];
        const float scale_ori = p.cfg[j].scale;
        // _get_scale_image :249-262
        const float xmin = det[0], ymin = det[1], xmax = det[2], ymax = det[3];
        const float det_height = __fsub_rn(ymax, ymin);
        const float c_x = __fdiv_rn(__fadd_rn(xmin, xmax), 2.0f);
        const float half = __fmul_rn(0.47f, det_height);
        const int left = rust_f32_as_i32(__fsub_rn(c_x, half)), right = rust_f32_as_i32(__fadd_rn(c_x, half));
        const int bx = left, by = rust_f32_as_i32(ymin);
        const int bw = wrap_span(right, left), bh = rust_f32_as_i32(__fadd_rn(__fsub_rn(ymax, ymin), 1.0f));
        // _get_new_box :347-384
        const float w1 = __fsub_rn((float)im.w, 1.0f), h1 = __fsub_rn((float)im.h, 1.0f);
        const float scale = rust_f32_min(__fdiv_rn(h1, (float)bh), rust_f32_min(__fdiv_rn(w1, (float)bw), scale_ori));
        const float new_w = __fmul_rn((float)bw, scale), new_h = __fmul_rn((float)bh, scale);
        const float cx = __fadd_rn(__fdiv_rn((float)bw, 2.0f), (float)bx), cy = __fadd_rn(__fdiv_rn((float)bh, 2.0f), (float)by);
        float fx0 = __fsub_rn(cx, __fdiv_rn(new_w, 2.0f)), fy0 = __fsub_rn(cy, __fdiv_rn(new_h, 2.0f));
        float fx1 = __fadd_rn(cx, __fdiv_rn(new_w, 2.0f)), fy1 = __fadd_rn(cy, __fdiv_rn(new_h, 2.0f));
        if (fx0 < 0.0f) { fx1 = __fsub_rn(fx1, fx0); fx0 = 0.0f; }
        if (fy0 < 0.0f) { fy1 = __fsub_rn(fy1, fy0); fy0 = 0.0f; }
        if (fx1 > w1) { fx0 = __fsub_rn(fx0, __fadd_rn(__fsub_rn(fx1, (float)im.w), 1.0f)); fx1 = w1; }
        if (fy1 > h1) { fy0 = __fsub_rn(fy0, __fadd_rn(__fsub_rn(fy1, (float)im.h), 1.0f)); fy1 = h1; }
        ltx = rust_f32_as_i32(fx0); lty = rust_f32_as_i32(fy0); rbx = rust_f32_as_i32(fx1); rby = rust_f32_as_i32(fy1);
        weight = __fdiv_rn(scale, scale_ori);
        // Mat::roi(Rect(ltx, lty, rbx - ltx + 1, rby - lty + 1)) :323-324, then cv::resize :332
        g.x0 = ltx; g.y0 = lty; g.rw = wrap_span(rbx, ltx); g.rh = wrap_span(rby, lty);
        const bool valid = g.x0 >= 0 && g.y0 >= 0 && g.rw > 0 && g.rh > 0 && (long long)g.x0 + g.rw <= im.w &&
                           (long long)g.y0 + g.rh <= im.h;
        if (valid) { // cv::resize's scale bookkeeping for this ROI (as align_setup_kernel's fallback branch)
            g.scale_x = 1.0 / ((double)p.cfg[j].out_w / g.rw);
            g.scale_y = 1.0 / ((double)p.cfg[j].out_h / g.rh);
            const int ix = cv_round_sat(g.scale_x), iy = cv_round_sat(g.scale_y);
            g.area_fast = fabs(g.scale_x - ix) < 2.220446049250313e-16 && fabs(g.scale_y - iy) < 2.220446049250313e-16 &&
                          ix == 2 && iy == 2;
        } else {
            bad[fl] = 1; // every writer stores the same value
        }
    }
    __syncthreads();
    if (!active) return;
    const int st = !found ? -2 : (bad[fl] ? -3 : 0);
    g.ok = st == 0;
    const size_t o = (size_t)b * p.k + j;
    p.geo[o] = g;
    p.weights[o] = st == 0 ? weight : 0.0f;
    if (p.rois) { int *r = p.rois + o * 4; r[0] = ltx; r[1] = lty; r[2] = rbx; r[3] = rby; }
    if (j == 0) p.status[b] = st;
}

// Crop, resize, tensorise: workgroup blockIdx.x of face blockIdx.y is one 256-pixel tile of the flat tile table -- the tiles
// of model 0, then of model 1, ... (cfg[j].tile0) -- so that outputs of different sizes share one launch and no workgroup is
// idle.  The ROI is resized as a frame of its own: resize_linear_px gets the ROI's first pixel, the frame's stride and the
// ROI's height and width, so its wide-load guard ends at the ROI's last pixel, inside the frame.  _preprocess :188-213:
// cvt_color(RGB2BGR) and the store to channel 2 - i cancel, plane c = byte channel c of the frame, raw 0..255.
__global__ void __launch_bounds__(256) liveness_tensor_kernel(LiveParams p)
{
    const int t = blockIdx.x, b = blockIdx.y;
    int j = 0;
#pragma unroll
    for (int q = 1; q < kMaxFaceTensors; ++q)
        if (q < p.k && t >= p.cfg[q].tile0) j = q;
    const LiveCfg &c = p.cfg[j];
    const int i = (t - c.tile0) * 256 + threadIdx.x;
    if (i >= c.out_w * c.out_h) return;
    const LiveRoi &g = p.geo[(size_t)b * p.k + j];
    int v[3] = {0, 0, 0};
    if (g.ok) {
        const LiveImage im = p.imgs[b];
        const int y = i / c.out_w, x = i - y * c.out_w;
        resize_linear_px(im.src + (long long)g.y0 * im.stride + (long long)g.x0 * 3, im.stride, g.rh, g.rw, g.scale_x, g.scale_y,
                         g.area_fast, x, y, v);
    }
    const size_t plane = (size_t)c.out_w * c.out_h;
    float *o = c.out + (size_t)b * 3 * plane + i;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) o[ch * plane] = (float)v[ch]; // a face with a negative status: 0.0f
}

int launch_liveness_tensors(const LiveParams &p, hipStream_t s)
{
    static_assert(64 % kMaxFaceTensors == 0, "a face's models share a wave of the geometry kernel");
    hipLaunchKernelGGL(liveness_geometry_kernel, dim3(ceil_div(p.n, kLiveGeoFaces)), dim3(64), 0, s, p);
    RFD_HIP(hipGetLastError());
    hipLaunchKernelGGL(liveness_tensor_kernel, dim3(p.tiles, p.n), dim3(256), 0, s, p);
    RFD_HIP(hipGetLastError());
    return RFD_OK;
}

// _postprocess :228-238 for one face per thread: live_score = live_score + column(1) * w and total_weight += w in model
// order, one division, score > threshold.  Everything is read before anything is written (score may be weights when k = 1).
__global__ void __launch_bounds__(64) liveness_decide_kernel(LiveLogits l, int kc, int k, int j0, int n, int classes,
                                                            const float *weights, float threshold, float *acc, float *score,
                                                            int *live)
{
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= n) return;
    float s = 0.0f, w = 0.0f;
    if (j0 > 0) { s = acc[2 * b]; w = acc[2 * b + 1]; }
#pragma unroll
    for (int q = 0; q < kLiveDecideChunk; ++q)
        if (q < kc) {
            const float wq = weights[(size_t)b * k + j0 + q];
            s = __fadd_rn(s, __fmul_rn(l.p[q][(size_t)b * classes + 1], wq));
            w = __fadd_rn(w, wq);
        }
    if (j0 + kc < k) { acc[2 * b] = s; acc[2 * b + 1] = w; return; }
    const float r = __fdiv_rn(s, w);
    score[b] = r;
    live[b] = r > threshold ? 1 : 0;
}

int launch_liveness_decide(const LiveLogits &l, int kc, int k, int j0, int n, int classes, const float *weights, float threshold,
                           float *acc, float *score, int *live, hipStream_t s)
{
    hipLaunchKernelGGL(liveness_decide_kernel, dim3(ceil_div(n, 64)), dim3(64), 0, s, l, kc, k, j0, n, classes, weights, threshold,
                       acc, score, live);
    RFD_HIP(hipGetLastError());
    return RFD_OK;
}

} // namespace rfd
