// kernels_splitk.hip -- the latency schedule's convolution: the generic implicit-GEMM tile of kernels_conv.hip with the K range
// cut into S segments that run as S workgroups (rfd_config.schedule = RFD_SCHEDULE_LATENCY, passes of <= RFD_LATENCY_MAX_BATCH images).
//
// Why: at 1-2 images the 20 x 20 / 40 x 40 half of the network gives the throughput kernels 4-50 tiles for 256 CUs, each walking
// a K of 1024-4608 alone (stage-4 conv2: 16 tiles, 72 K steps, 41-47 us).  Here the grid is tiles x S:
//   - workgroup (tile, s) accumulates K steps [s * nk / S, (s + 1) * nk / S) in f32 registers -- same staging as conv_igemm_kernel
//     (LDS-DMA, XOR swizzle, 3-slot activation ring, one drain + one barrier per step, v_mfma_f32_16x16x32_bf16) -- and stores the
//     partial tile to its own f32 workspace slab [tile][s] with plain 16-byte vector stores;
//   - every wave drains its stores, the workgroup meets at a barrier, one lane makes the slabs visible device-wide (agent-scope release:
//     write-back of this XCD's L2) and draws ONE ticket from the tile's arrival counter;
//   - the workgroup that draws ticket S - 1 is the combiner: agent-scope acquire, then it reads all S slabs FROM THE WORKSPACE in
//     segment order 0 .. S - 1 (its own included: the order of the f32 additions never depends on who arrived last), runs the
//     ordinary epilogue (conv_device.h) and stores the counter back to 0, so the next launch -- a hipGraph replay included -- finds
//     it clean;
//   - every other workgroup exits behind its ticket.  Nobody waits for anybody: no spin, no grid barrier, no cooperative launch.
// A drawn ticket >= S (a counter left dirty by a faulted launch on a reused context) sets the context's give-up word -- the one
// check_nms_flag turns into RFD_ERR_HIP -- and the workgroup returns without touching a slab it does not own.
//
// S and the segment boundaries are a function of the LAYER (number of K steps) alone, the decision to split one of the layer and
// the pixels of ONE image: a frame's results are the same bits for every batch size of a latency pass and every position in it.
// K order inside a segment: (ky, kx, chunk), the order of the weight rows, for every layer (the chunk-major order of the
// throughput schedule's 3x3 kernels is not reproduced: the two schedules do not promise each other's bits).
// Hazard rules: no scratch, every vmcnt wait a full drain, lgkmcnt(0) in front of every barrier that frees
// a DMA slot, no 128-bit LDS read under partial EXEC (the fragment reads sit in the uniform K loop), one tile per workgroup
// (40 KiB of LDS: up to four workgroups share a CU).
#include "conv_device.h"

namespace rfd {

// Selection (conv_splitk_plan, conv_splitk_wants): conv_select.hip.
template <int BM, int BN, int WAVES_M, int WAVES_N>
__global__ void __launch_bounds__(WAVES_M *WAVES_N * 64) conv_splitk_kernel(const ConvParams p, const int S)
{
    constexpr int NSX = 3;
    constexpr int NT = WAVES_M * WAVES_N * 64, NW = WAVES_M * WAVES_N;
    constexpr int WM = BM / WAVES_M, WN = BN / WAVES_N;
    constexpr int TM = WM / 16, TN = WN / 16;
    constexpr int XP = BM / 8 / NW, WP = (BN / 8 + NW - 1) / NW;
    static_assert((BM / 8) % NW == 0, "X tile pieces must divide over the waves");
    static_assert(WN % 32 == 0 && WM % 16 == 0, "the epilogue stores 8-channel groups of 16-pixel row tiles");

    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    bf16_t *Xs = reinterpret_cast<bf16_t *>(smem);  // [NSX][BM*64]
    bf16_t *Ws = Xs + NSX * BM * 64;                // [2][BN*64]

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave % WAVES_M, wn = wave / WAVES_M;
    const int HoWo = p.Ho * p.Wo;
    const int M = p.B * HoWo;
    const int K1 = p.KH * p.KW * p.Cin;
    const int K = K1 + p.Cin2;
    const int nk1 = K1 >> 6, nk = K >> 6;
    const int tiles_n = p.Cout / BN;
    // block -> (m tile, segment, n tile), n tile fastest: neighbours in an XCD's chunk share the activation segment
    const int lid = xcd_remap(blockIdx.x, gridDim.x);
    const int tn_ = lid % tiles_n, seg = (lid / tiles_n) % S, tm_ = lid / (tiles_n * S);
    const int tile = tm_ * tiles_n + tn_;
    const int m0 = tm_ * BM, n0 = tn_ * BN;
    const int kt0 = seg * nk / S, kt1 = (seg + 1) * nk / S; // whole K steps; a function of (nk, S) alone

    const int lr = lane >> 3, chunk = (lane & 7) ^ lr;
    const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<bf16_t *>(p.x), 0, (uint32_t)((size_t)p.B * p.H * p.W * p.ldx * 2), 0x00020000);
    const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<bf16_t *>(p.w), 0, (uint32_t)((size_t)p.Cout * K * 2), 0x00020000);
    const __amdgpu_buffer_rsrc_t rx2 = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<bf16_t *>(p.Cin2 ? p.x2 : p.x), 0,
        (uint32_t)(p.Cin2 ? (size_t)p.B * p.H2 * p.W2 * p.Cin2 * 2 : 0), 0x00020000);
    uint32_t xoff[XP], xoff2[XP];
    int hi0[XP], wi0[XP];
#pragma unroll
    for (int q = 0; q < XP; ++q) {
        const int m = m0 + (wave + NW * q) * 8 + lr;
        xoff2[q] = kOob;
        if (m < M) {
            const int b = m / HoWo, rem = m - b * HoWo;
            const int ho = rem / p.Wo, wo = rem - ho * p.Wo;
            hi0[q] = ho * p.stride - p.pad;
            wi0[q] = wo * p.stride - p.pad;
            xoff[q] = (uint32_t)(((((long long)b * p.H + hi0[q]) * p.W + wi0[q]) * p.ldx + p.x_coff + chunk * 8) * 2);
            if (p.Cin2)
                xoff2[q] = (uint32_t)(((((long long)b * p.H2 + ho * p.stride2) * p.W2 + wo * p.stride2) * p.Cin2 + chunk * 8) * 2);
        } else {
            hi0[q] = -(1 << 28); // fails every bounds check -> zero rows
            wi0[q] = 0;
            xoff[q] = 0;
        }
    }
    uint32_t woff[WP];
#pragma unroll
    for (int q = 0; q < WP; ++q) {
        const int piece = wave + NW * q;
        // LDS row rho = i*16 + fq*4 + r (the MFMA A-operand row) holds output channel (i>>1)*32 + fq*8 + (i&1)*4 + r of the
        // wave's WN-wide slice (as conv_igemm_kernel: a lane's 2 x 4 accumulator registers are 8 consecutive channels)
        const int rho = (piece < BN / 8 ? piece * 8 + lr : 0);
        const int rw_ = rho % WN, i_ = rw_ >> 4, fq_ = (rw_ >> 2) & 3, r_ = rw_ & 3;
        const int chn = (rho - rw_) + (i_ >> 1) * 32 + fq_ * 8 + (i_ & 1) * 4 + r_;
        woff[q] = (uint32_t)(((size_t)(n0 + chn) * K + chunk * 8) * 2);
    }

    // positions of the NEXT tiles to stage, starting at this segment's first K step: K order (ky, kx, chunk)
    const int kc_n = p.Cin >> 6;
    int kt_x = kt0, kt_w = kt0;
    int kc = 0, kx = 0, ky = 0;
    if (kt0 < nk1) {
        const int tap = kt0 / kc_n;
        kc = kt0 - tap * kc_n;
        ky = tap / p.KW;
        kx = tap - ky * p.KW;
    }
    auto stage_x = [&](int slot) {
        if (kt_x < nk1) {
            const uint32_t tap = (uint32_t)((ky * p.W + kx) * p.ldx * 2); // scalar
#pragma unroll
            for (int q = 0; q < XP; ++q) {
                const bool ok = (unsigned)(hi0[q] + ky) < (unsigned)p.H && (unsigned)(wi0[q] + kx) < (unsigned)p.W;
                blds16(rx, ok ? xoff[q] + tap : kOob, (uint32_t)(kc << 7), Xs + slot * BM * 64 + (wave + NW * q) * 512);
            }
        } else {
#pragma unroll
            for (int q = 0; q < XP; ++q)
                blds16(rx2, xoff2[q], (uint32_t)((kt_x - nk1) << 7), Xs + slot * BM * 64 + (wave + NW * q) * 512);
        }
        ++kt_x;
        if (++kc == kc_n) {
            kc = 0;
            if (++kx == p.KW) { kx = 0; ++ky; }
        }
    };
    auto stage_w = [&](int slot) {
        const uint32_t col = (uint32_t)(kt_w << 7);
#pragma unroll
        for (int q = 0; q < WP; ++q) {
            const int piece = wave + NW * q;
            if (piece < BN / 8) blds16(rw, woff[q], col, Ws + slot * BN * 64 + piece * 512);
        }
        ++kt_w;
    };

    f32x4 acc[TN][TM];
#pragma unroll
    for (int i = 0; i < TN; ++i)
#pragma unroll
        for (int j = 0; j < TM; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int frow = lane & 15, fq = lane >> 4;

    // optional input affine (+ReLU): per-channel scale/shift staged once in LDS behind the operand slots
    float *Sc = reinterpret_cast<float *>(Ws + 2 * BN * 64);
    if (p.in_scale) {
        for (int c = tid; c < K1; c += NT) {
            Sc[c] = p.in_scale[c];
            Sc[K1 + c] = p.in_shift[c];
        }
        __syncthreads();
    }
    // prologue, in queue order: X0, W0, X1
    stage_x(0);
    stage_w(0);
    if (kt0 + 1 < kt1) stage_x(1);

    int xslot = 0, wslot = 0, xstage = NSX - 1, wstage = 1;
    for (int kt = kt0; kt < kt1; ++kt) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // full drain: lands X(kt), W(kt) and X(kt+1)
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); /* no LDS read in flight at a barrier that frees a ring slot for DMA (tools/isa_check.py) */
        if (kt + 1 < kt1) {
            stage_w(wstage);
            wstage ^= 1;
        }
        if (kt + NSX - 1 < kt1) {
            stage_x(xstage);
            xstage = xstage + 1 == NSX ? 0 : xstage + 1;
        }
        const int slot = xslot;
        xslot = xslot + 1 == NSX ? 0 : xslot + 1;
        const bf16_t *xs = Xs + slot * BM * 64 + (wm * WM) * 64;
        const bf16_t *ws = Ws + wslot * BN * 64 + (wn * WN) * 64;
        wslot ^= 1;
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            bf16x8 af[TN], bfr[TM];
            const int ch = kk * 4 + fq;
#pragma unroll
            for (int i = 0; i < TN; ++i) {
                const int r = i * 16 + frow;
                af[i] = *reinterpret_cast<const bf16x8 *>(ws + r * 64 + ((ch ^ (r & 7)) << 3));
            }
#pragma unroll
            for (int j = 0; j < TM; ++j) {
                const int r = j * 16 + frow;
                bfr[j] = *reinterpret_cast<const bf16x8 *>(xs + r * 64 + ((ch ^ (r & 7)) << 3));
            }
            if (p.in_scale) {
                // this lane's 8 operand elements are input channels kt*64 + kk*32 + fq*8 .. +7 of one pixel
                const float *sc = Sc + kt * 64 + kk * 32 + fq * 8;
                const float4 s0 = *reinterpret_cast<const float4 *>(sc), s1 = *reinterpret_cast<const float4 *>(sc + 4);
                const float4 t0 = *reinterpret_cast<const float4 *>(sc + K1), t1 = *reinterpret_cast<const float4 *>(sc + K1 + 4);
                const float ss[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w};
                const float tt[8] = {t0.x, t0.y, t0.z, t0.w, t1.x, t1.y, t1.z, t1.w};
#pragma unroll
                for (int j = 0; j < TM; ++j) {
                    bf16x8 v = bfr[j];
#pragma unroll
                    for (int e = 0; e < 8; ++e) v[e] = (__bf16)fmaxf(__builtin_fmaf((float)v[e], ss[e], tt[e]), 0.f); // one fused multiply-add, as in every kernel that applies the input affine
                    bfr[j] = v;
                }
            }
#pragma unroll
            for (int i = 0; i < TN; ++i)
#pragma unroll
                for (int j = 0; j < TM; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
        }
    }

    // ---- partial tile -> workspace slab [tile][seg]: register r of thread t at float4 index r * NT + t (lane-linear 16-byte stores) ----
    constexpr int SLAB4 = BM * BN / 4; // float4 per slab
    float4 *slab = reinterpret_cast<float4 *>(p.sk_ws) + ((size_t)tile * S + seg) * SLAB4;
#pragma unroll
    for (int i = 0; i < TN; ++i)
#pragma unroll
        for (int j = 0; j < TM; ++j)
            slab[(i * TM + j) * NT + tid] = make_float4(acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // every wave: its slab stores have left the CU ...
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    // ... then ONE lane publishes them device-wide and draws the ticket (the last K step's LDS reads are done: smem is free)
    int *tick = reinterpret_cast<int *>(smem);
    if (tid == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // the write-back has completed before the ticket is drawn
        const unsigned t = __hip_atomic_fetch_add(p.sk_cnt + tile, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (t >= (unsigned)S) { // a counter left dirty (context reused after a faulted launch): report, never index out of range
            if (p.fail) __hip_atomic_store(p.fail, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        } else if (t == (unsigned)S - 1) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        *tick = (int)t;
    }
    __syncthreads();
    if (*tick != S - 1) return; // not the last arrival (or a dirty counter): done

    // ---- combiner: the S slabs in segment order, then the ordinary epilogue ----
    constexpr int TH = TN / 2;
    uint4 resv[TM][TH];
    conv_prefetch_residual<TM, TH, WM, WN>(p, resv, m0, n0, wm, wn, frow, fq, M, HoWo);
    const float4 *sl = reinterpret_cast<const float4 *>(p.sk_ws) + (size_t)tile * S * SLAB4;
#pragma unroll
    for (int i = 0; i < TN; ++i)
#pragma unroll
        for (int j = 0; j < TM; ++j) {
            const float4 v = sl[(i * TM + j) * NT + tid];
            acc[i][j] = f32x4{v.x, v.y, v.z, v.w};
        }
    for (int s = 1; s < S; ++s) {
        sl += SLAB4;
#pragma unroll
        for (int i = 0; i < TN; ++i)
#pragma unroll
            for (int j = 0; j < TM; ++j) {
                const float4 v = sl[(i * TM + j) * NT + tid];
                acc[i][j][0] += v.x; acc[i][j][1] += v.y; acc[i][j][2] += v.z; acc[i][j][3] += v.w;
            }
    }
    if (tid == 0) __hip_atomic_store(p.sk_cnt + tile, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); // clean for the next launch
    conv_epilogue<TM, TN, WM, WN>(p, acc, resv, m0, n0, wm, wn, frow, fq, M);
}

template <int BM, int BN, int WAVES_M, int WAVES_N> static int launch_splitk_cfg(const ConvParams &p, const SplitKPlan &pl, hipStream_t s)
{
    const size_t lds = (size_t)(3 * BM + 2 * BN) * 64 * sizeof(bf16_t) + (p.in_scale ? (size_t)2 * p.KH * p.KW * p.Cin * sizeof(float) : 0);
    auto kern = conv_splitk_kernel<BM, BN, WAVES_M, WAVES_N>;
    static DynLdsOnce once;
    RFD_TRY(once.ensure(reinterpret_cast<const void *>(kern), (int)((size_t)(3 * BM + 2 * BN) * 64 * sizeof(bf16_t) + 16384)));
    hipLaunchKernelGGL(kern, dim3(pl.tiles * pl.S), dim3(WAVES_M * WAVES_N * 64), lds, s, p, pl.S);
    RFD_HIP(hipGetLastError());
    return RFD_OK;
}

int launch_conv_splitk(const ConvParams &p, hipStream_t s)
{
    SplitKPlan pl;
    if (!conv_splitk_wants(p, &pl)) { set_error("split-K conv: the layer does not qualify"); return RFD_ERR_INVALID_ARG; }
    if (p.in_scale && (p.KH != 1 || p.KW != 1 || p.pad != 0 || p.Cin > 2048)) {
        set_error("split-K conv: the input affine is only defined for un-padded 1x1 convs with Cin <= 2048");
        return RFD_ERR_INVALID_ARG;
    }
    // the workspace and the counters are sized at context creation from the same plan: a mismatch is a bug, never an out-of-range write
    if (!p.sk_ws || !p.sk_cnt || pl.ws_bytes > p.sk_ws_bytes || pl.tiles > p.sk_cnt_n) {
        set_error("split-K conv: workspace of %zu bytes / %d counters, the layer needs %zu / %d", p.sk_ws_bytes, p.sk_cnt_n, pl.ws_bytes, pl.tiles);
        return RFD_ERR_CAPACITY;
    }
    return launch_splitk_cfg<64, 64, 2, 2>(p, pl, s);
}

} // namespace rfd
