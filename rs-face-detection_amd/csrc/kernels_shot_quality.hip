// kernels_shot_quality.hip -- the shot quality of every detection row (include/rfd.h, "shot quality"; gfx950, wave64): one
// launch, kSqGroupsPerFrame workgroups of sixteen waves per frame, each walking rows j, j + 8, ... of its frame up to the count it
// reads on the device.  A workgroup has one (frame, row) in hand at a time.
//
// Pixel pass.  The region of the row (shot_quality_plan.h) is read once.  A lane takes four consecutive pixels = 12 bytes of a
// source row, the lanes of a wave consecutive groups, so a wave instruction covers 768 contiguous bytes; the 12 bytes start at
// any alignment (3-byte pixels, any stride, any data pointer) and are read as three unaligned dwords, which gfx950 serves as
// one global_load_dwordx3; the last w % 4 pixels of a row take byte loads, so nothing outside the region is touched.  A region
// narrower than 129 pixels gives a wave several source rows at once (L = 8, 16 or 32 lanes per row), so a 40-pixel face still
// fills 40 of 64 lanes.  The sixteen waves interleave the region's rows, and a lane issues the loads of up to four of its groups
// before it uses the first, so a wide region has tens of KiB in flight.
//
// Cell sums.  A lane maps its first pixel to a cell column with one 32-bit division (sq_cell, the inverse of the edges) and
// steps the remainder by 32 per pixel; it sums the pixels of a cell in a register and adds each run into the 32 x 32 int32
// array in LDS with ds_add_u32 (no return value).  Integer sums: any order gives the same bits.  A lane issues one add per
// cell it touches (at most four, one from 128 pixels of width on); lanes of one instruction that hit the same cell are
// serialised by the LDS, which is the price of this form on wide regions ("shot quality").
//
// After the pass: thread t turns cell t into its 8.4 fixed-point mean in place, then the 900 interior Laplacians;
// A1, A2 (64-bit), the sum of the means and the count of dark or bright cells are reduced by wave shuffles and sixteen-entry LDS
// arrays; thread 0 does the landmark terms and the final f32 / f64 steps, every one a pinned rounding (__fsub_rn ...), and
// stores the row.  No global atomics, no scratch; rows at or past the count are never written.
#include "shot_quality_host.h"

namespace rfd {

constexpr int kSqThreads = 1024, kSqWaves = kSqThreads / 64, kSqCells = kSqGrid * kSqGrid;

__device__ __forceinline__ int sq_grey(uint32_t b, uint32_t g, uint32_t r) { return (int)((b * 1868u + g * 9617u + r * 4899u + 8192u) >> 14); }

__device__ __forceinline__ int sq_wave_sum(int v) // all 64 lanes active
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

__device__ __forceinline__ long long sq_wave_sum64(long long v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const int lo = __shfl_xor((int)(uint32_t)(unsigned long long)v, d), hi = __shfl_xor((int)((unsigned long long)v >> 32), d);
        v += (long long)(((unsigned long long)(uint32_t)hi << 32) | (uint32_t)lo);
    }
    return v;
}

__device__ __forceinline__ float sq_min1(float a) { return a < 1.0f ? a : 1.0f; }
__device__ __forceinline__ float sq_quiet(float a) { return a != a ? __uint_as_float(0x7FC00000u) : a; } // one NaN, whatever made it

// The 12 bytes of group c (pixels 4 c .. 4 c + 3 of a region row that starts at src) as three dwords; the row's tail of 1 .. 3
// pixels by bytes, zero-filled.
__device__ __forceinline__ void sq_load(const uint8_t *src, int c, int w, uint32_t d[3])
{
    const int npx = min(4, w - 4 * c);
    const uint8_t *s = src + (long long)c * 12;
    if (npx == 4) {
        typedef uint32_t u32_unaligned __attribute__((aligned(1)));
        const u32_unaligned *q = reinterpret_cast<const u32_unaligned *>(s);
        d[0] = q[0]; d[1] = q[1]; d[2] = q[2];
    } else {
        d[1] = d[2] = 0u;
        d[0] = (uint32_t)s[0] | ((uint32_t)s[1] << 8) | ((uint32_t)s[2] << 16);
        if (npx > 1) { d[0] |= (uint32_t)s[3] << 24; d[1] = (uint32_t)s[4] | ((uint32_t)s[5] << 8); }
        if (npx > 2) { d[1] |= ((uint32_t)s[6] << 16) | ((uint32_t)s[7] << 24); d[2] = (uint32_t)s[8]; }
    }
}

// The pixels of group c into the cells of their row: the cell column of pixel 4 c by one division (sq_cell's), then the
// remainder stepped by 32 per pixel -- w >= 32, so at most one cell further each; one LDS add per run of pixels in a cell.
__device__ __forceinline__ void sq_add(int *cells, int c, int w, const uint32_t d[3])
{
    const int xr = 4 * c, npx = min(4, w - xr);
    const int grey[4] = {sq_grey(d[0] & 0xffu, (d[0] >> 8) & 0xffu, (d[0] >> 16) & 0xffu), sq_grey(d[0] >> 24, d[1] & 0xffu, (d[1] >> 8) & 0xffu),
                         sq_grey((d[1] >> 16) & 0xffu, d[1] >> 24, d[2] & 0xffu), sq_grey((d[2] >> 8) & 0xffu, (d[2] >> 16) & 0xffu, d[2] >> 24)};
    const uint32_t num = 32u * (uint32_t)(xr + 1) - 1u;
    uint32_t col = num / (uint32_t)w, rem = num - col * (uint32_t)w;
    int acc = grey[0];
#pragma unroll
    for (int k = 1; k < 4; ++k) {
        if (k < npx) {
            rem += 32u;
            if (rem >= (uint32_t)w) {
                rem -= (uint32_t)w;
                atomicAdd(&cells[col], acc);
                ++col;
                acc = 0;
            }
            acc += grey[k];
        }
    }
    atomicAdd(&cells[col], acc);
}

__global__ void __launch_bounds__(kSqThreads) shot_quality_kernel(SqParams p)
{
    __shared__ int s_cell[kSqCells];
    __shared__ int s_a1[kSqWaves], s_sum[kSqWaves], s_out[kSqWaves];
    __shared__ long long s_a2[kSqWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.y;
    const int cnt = min(max(p.count[b], 0), p.max_det);
    const SqImage im = p.imgs[b];

    for (int i = blockIdx.x; i < cnt; i += gridDim.x) { // uniform over the workgroup
        const size_t row = (size_t)b * p.max_det + i;
        const float *bx = p.boxes + row * 5;
        const SqRegion g = sq_region(bx[0], bx[1], bx[2], bx[3], im.w, im.h);
        int a1 = 0, msum = 0, nout = 0;
        long long a2 = 0;
        if (g.measured) {
            const int w = (int)g.w, h = (int)g.h; // 32 .. kSqMaxSide, inside the frame
            for (int c = tid; c < kSqCells; c += kSqThreads) s_cell[c] = 0;
            __syncthreads();

            // ---- pixel pass ----
            const int chunks = (w + 3) >> 2; // groups of four pixels per source row
            int lshift = 6;                  // L = 1 << lshift lanes per source row
            if (chunks <= 32) { lshift = 3; while ((1 << lshift) < chunks) ++lshift; }
            const int L = 1 << lshift, R = 64 >> lshift; // R source rows per wave pass
            const int sub = lane >> lshift, cl = lane & (L - 1);
            for (int y0 = wave * R; y0 < h; y0 += kSqWaves * R) {
                const int yr = y0 + sub;
                if (yr >= h) continue;
                int *cells = s_cell + sq_cell(yr, h) * kSqGrid;
                const uint8_t *src = im.src + (long long)(g.y0 + yr) * im.stride + (long long)g.x0 * 3;
                // four groups of a lane per trip, their loads issued before the first is used (up to 48 KiB of a region in flight
                // over the sixteen waves).  Measured: no faster than four waves with one load each, so the pass is not bound by
                // load latency ("shot quality", Cost)
                for (int c0 = cl; c0 < chunks; c0 += 4 * L) {
                    uint32_t d[4][3];
#pragma unroll
                    for (int u = 0; u < 4; ++u)
                        if (c0 + u * L < chunks) sq_load(src, c0 + u * L, w, d[u]);
#pragma unroll
                    for (int u = 0; u < 4; ++u)
                        if (c0 + u * L < chunks) sq_add(cells, c0 + u * L, w, d[u]);
                }
            }
            __syncthreads();

            // ---- cell means in place, 8.4 fixed point: a thread reads and writes its own cells only ----
            for (int c = tid; c < kSqCells; c += kSqThreads) {
                const int r = c >> 5, k = c & 31;
                const uint32_t n = (uint32_t)(sq_edge(k + 1, w) - sq_edge(k, w)) * (uint32_t)(sq_edge(r + 1, h) - sq_edge(r, h)); // 1 .. 2^20
                const int m = (int)((16u * (uint32_t)s_cell[c] + n / 2u) / n); // 16 * 255 * 2^20 + 2^19 < 2^32
                s_cell[c] = m;
                msum += m;
                nout += (m <= p.lo16 || m >= p.hi16) ? 1 : 0;
            }
            __syncthreads();

            // ---- the Laplacian over the 30 x 30 interior ----
            for (int e = tid; e < 900; e += kSqThreads) {
                const int r = 1 + e / 30, k = 1 + e % 30;
                const int *m = s_cell + r * kSqGrid + k;
                const int lap = 4 * m[0] - m[-kSqGrid] - m[kSqGrid] - m[-1] - m[1];
                a1 += lap;
                a2 += (long long)lap * lap;
            }
            a1 = sq_wave_sum(a1);
            a2 = sq_wave_sum64(a2);
            msum = sq_wave_sum(msum);
            nout = sq_wave_sum(nout);
            if (lane == 0) { s_a1[wave] = a1; s_a2[wave] = a2; s_sum[wave] = msum; s_out[wave] = nout; }
            __syncthreads();
            // the sixteen waves' sums, by every lane with all lanes active (lane l reads entry l & 15, four shuffle steps): a wide
            // LDS read under thread 0's predicate is what tests/test_build_cpu.py forbids
            a1 = s_a1[lane & (kSqWaves - 1)]; a2 = s_a2[lane & (kSqWaves - 1)]; msum = s_sum[lane & (kSqWaves - 1)]; nout = s_out[lane & (kSqWaves - 1)];
#pragma unroll
            for (int d = 1; d < kSqWaves; d <<= 1) {
                a1 += __shfl_xor(a1, d);
                msum += __shfl_xor(msum, d);
                nout += __shfl_xor(nout, d);
                const int lo = __shfl_xor((int)(uint32_t)(unsigned long long)a2, d), hi = __shfl_xor((int)((unsigned long long)a2 >> 32), d);
                a2 += (long long)(((unsigned long long)(uint32_t)hi << 32) | (uint32_t)lo);
            }
        }

        if (tid == 0) {
            float sharp = 0.0f, mean = 0.0f, expo = 0.0f;
            if (g.measured) {
                const int t1 = a1, ts = msum, to = nout;
                const long long t2 = a2;
                const long long V = 900ll * t2 - (long long)t1 * t1;
                sharp = (float)__ddiv_rn((double)V, 207360000.0);
                mean = (float)__ddiv_rn((double)ts, 16384.0);
                expo = __fsub_rn(1.0f, __fdiv_rn((float)to, 1024.0f));
            }
            // the landmark terms
            const float *l = p.lmk + row * 10;
            const float lx = l[0], ly = l[1], rx = l[2], ry = l[3], nx = l[4], ny = l[5], mly = l[7], mry = l[9];
            const float d = __fsub_rn(rx, lx);
            const float ey = __fmul_rn(__fadd_rn(ly, ry), 0.5f), my = __fmul_rn(__fadd_rn(mly, mry), 0.5f);
            const float v = __fsub_rn(my, ey);
            float yaw = 0.0f, roll = 0.0f, pitch = 0.0f, pose = 0.0f;
            if (d > 0.0f && v > 0.0f) {
                yaw = __fdiv_rn(fabsf(__fsub_rn(__fsub_rn(nx, lx), __fsub_rn(rx, nx))), d);
                roll = __fdiv_rn(fabsf(__fsub_rn(ry, ly)), d);
                pitch = fabsf(__fsub_rn(__fdiv_rn(__fsub_rn(ny, ey), v), p.pitch0));
                const float t = __fadd_rn(__fadd_rn(__fmul_rn(yaw, p.w_yaw), __fmul_rn(roll, p.w_roll)), __fmul_rn(pitch, p.w_pitch));
                pose = t < 1.0f ? __fsub_rn(1.0f, t) : 0.0f;
            }
            const float size = (float)(g.w < g.h ? g.w : g.h);
            float q = 0.0f;
            if (g.measured) {
                const float a = p.times_score ? __fmul_rn(bx[4], pose) : pose;
                q = __fmul_rn(__fmul_rn(__fmul_rn(a, sq_min1(__fdiv_rn(sharp, p.sharp_ref))), sq_min1(__fdiv_rn(size, p.size_ref))), expo);
            }
            p.quality[row] = sq_quiet(q);
            if (p.parts) {
                float4 *o = reinterpret_cast<float4 *>(p.parts + row * RFD_SHOT_QUALITY_PARTS);
                o[0] = make_float4(sharp, mean, expo, sq_quiet(yaw));
                o[1] = make_float4(sq_quiet(roll), sq_quiet(pitch), pose, size);
            }
            if (p.status) p.status[row] = g.measured ? 0 : 1;
        }
        // the next row's stores into s_cell and the sixteen-entry arrays come behind its own barriers, which every thread reaches
        // only after it has read the arrays above
    }
}

int launch_shot_quality(const SqParams &p, hipStream_t s)
{
    hipLaunchKernelGGL(shot_quality_kernel, dim3(kSqGroupsPerFrame, p.n), dim3(kSqThreads), 0, s, p);
    RFD_HIP(hipGetLastError());
    return RFD_OK;
}

} // namespace rfd
