// conv_select.hip -- which kernel runs a layer: pure host functions of the layer description (ConvParams / B2BParams), the forced
// tile and, for the stem, the CU count.  No HIP call, no allocation, no string formatting: the launchers (kernels_conv.hip,
// kernels_ring.hip, kernels_splitk.hip) execute the choice, rfd_debug_op_kernels and rfd_debug_op_kernels_static print it, and
// tests/test_kernel_choice_cpu.py replays the pinned table tests/golden/kernel_choice.json against it on any machine.
#include "kernels.h"

namespace rfd {

const char *conv_kernel_name(ConvKernel k)
{
    switch (k) {
#define RFD_NAME(id, name) case id: return name;
        RFD_CONV_KERNELS(RFD_NAME)
#undef RFD_NAME
    default: return "(no kernel)";
    }
}

// ---- which forced tiles admit which kernel family (TILE_HEURISTIC admits all of them by their size rules) ----
static bool tile_bars_b2b_s1_persistent(int t) { return t == TILE_128 || t == TILE_256x128 || t == TILE_GENERIC; }
static bool tile_admits_pw_stream(int t, int Cin)
{
    return t == TILE_HEURISTIC || t == TILE_PERSISTENT || t == TILE_PW_STREAM || (t == TILE_PW_STREAM_K128 && Cin == 128) ||
           (t == TILE_PW_STREAM_K256 && Cin == 256);
}
static bool tile_admits_pw_wide(int t) { return t == TILE_HEURISTIC || t == TILE_PERSISTENT || t == TILE_PW_WIDE; }
static bool tile_admits_pw_gemm(int t) { return t == TILE_HEURISTIC || t == TILE_PERSISTENT || t == TILE_PW_GEMM; }
static bool tile_admits_c64(int t) { return t == TILE_HEURISTIC || t == TILE_PERSISTENT || t == TILE_C64; }
static bool tile_admits_halo(int t) { return t == TILE_HEURISTIC || t == TILE_PERSISTENT || t == TILE_HALO_SMALL || t == TILE_HALO_LARGE; }
static bool tile_forces_pair(int t) { return t == TILE_PERSISTENT || t == TILE_PAIR; }

// ---- latency schedule: pure functions of the layer shape and the pixels of one image ----
// Split when the throughput schedule's 128 x 128 tiling of ONE image would give at most kSplitKMaxTiles128 workgroups (an eighth
// of the 256 CUs) and K has at least kSplitKMinSteps steps of 64.  Both limits come from the per-op table at one image
// (profiles/latency_schedule_per_op_b1.txt): with 4 <= nk < 16 (heads, stage-4 conv3, the 64 -> 64 SSH
// context convs) or 50-64 tiles (the 80 x 80 level, stage 2, stage-4 conv3 and the first stage-4 conv1) the slab round trip costs
// more than the idle CUs give back -- those layers measured slower split and keep their throughput kernels.
constexpr int kSplitKMaxTiles128 = 32;
constexpr int kSplitKMinSteps = 16;

int conv_splitk_segments(int nk)
{
    if (nk < kSplitKMinSteps) return 1;
    return std::min(nk / 8, kSplitKMaxSegments); // segments of 8+ K steps: 2 .. 8
}

bool conv_splitk_plan(int K, int Cout, int HoWo, int B, SplitKPlan *pl)
{
    if (K % 64 != 0 || Cout % 64 != 0 || HoWo < 1 || B < 1) return false; // 64 x 64 tiles
    const int nk = K / 64;
    const long long tiles128 = (long long)ceil_div(HoWo, 128) * ceil_div(Cout, 128);
    if (nk < kSplitKMinSteps || tiles128 > kSplitKMaxTiles128) return false;
    pl->S = conv_splitk_segments(nk);
    pl->bm = 64;
    pl->bn = 64;
    pl->tiles = ceil_div(B * HoWo, pl->bm) * (Cout / pl->bn);
    pl->ws_bytes = (size_t)pl->tiles * pl->S * pl->bm * pl->bn * sizeof(float);
    return true;
}

bool conv_splitk_wants(const ConvParams &p, SplitKPlan *pl)
{
    if (!p.latency || p.force_tile != TILE_HEURISTIC || p.co_running || p.w1) return false;
    if (p.Cin % 64 != 0 || p.Cin2 % 64 != 0) return false;
    return conv_splitk_plan(p.KH * p.KW * p.Cin + p.Cin2, p.Cout, p.Ho * p.Wo, p.B, pl);
}

// shapes the ring kernel accepts
bool conv_ring_supports(const ConvParams &p, bool *kx3)
{
    if (p.Cout % 128 != 0 || p.Cin % 64 != 0 || p.Cin2 % 64 != 0 || p.w1) return false;
    const bool k3 = p.KH == 3 && p.KW == 3 && p.stride == 1 && p.pad == 1 && p.Cin2 == 0 && !p.in_scale && p.Ho == p.H && p.Wo == p.W &&
                    p.W >= 3; // choose_one's kx_ok: these layers accumulate chunk-major in every kernel that runs them
    if (kx3) *kx3 = k3;
    if (p.in_scale && (p.Cin2 || (size_t)2 * p.KH * p.KW * p.Cin * sizeof(float) > 16 * 1024)) return false;
    return true;
}

// ---- the stem ----
ConvKernel choose_stem(int B, int H, int W, bool conv1_offered, int force_tile, int cus)
{
    const int ntiles = B * ceil_div(H / 4, kStemPH) * ceil_div(W / 4, kStemPW);
    // persistent form from 4 tiles per workgroup slot (2 workgroups per CU by LDS): weights stay in registers, the next patch is
    // prefetched
    if (ntiles < 4 * 2 * cus) return K_STEM;
    // with the first unit's conv1 on the pooled tile when the caller offers it (Network does when the next op of the range is that
    // conv); a forced tile keeps the two ops apart, so that the conv runs the kernel the tile asks for
    return conv1_offered && force_tile == TILE_HEURISTIC ? K_STEM_PERSISTENT_CONV1 : K_STEM_PERSISTENT;
}

// ---- stage 1's back-to-back pairs ----
void choose_b2b_s1(const B2BParams &p, bool w1_behind_w3, ConvStep *st)
{
    const int M = p.B * p.H * p.W;
    const int ntiles = ceil_div(M, 128);
    // Round 4: the weight-resident barrier-free pair kernel (pw_pair_kernel<.., NCR = 2, HALF1>, the form that runs the stage
    // 1 -> 2 boundary) takes stage 1's pairs too: W3 [256][64 or 128] + W1 [64][256] stay in LDS, every wave is an independent
    // pipeline over its 16 pixels.  TILE_PAIR forces it, TILE_PERSISTENT keeps the older persistent kernels below.
    const bool pair_ok = w1_behind_w3 && (p.Cin2 == 0 ? p.res != nullptr : (!p.res && p.bias3b)) && (size_t)M * 256 * 2 < 0xfffffff0ull;
    if (pair_ok && (p.force_tile == TILE_PAIR || (p.force_tile == TILE_HEURISTIC && ntiles >= 512))) {
        ConvParams &c = st->p;
        memset(&c, 0, sizeof c);
        c.x = p.x; c.w = p.w3; c.bias = p.bias3; c.x2 = p.x2; c.bias2 = p.bias3b; c.res = p.res;
        c.scale2 = p.scale; c.shift2 = p.shift; c.y = p.raw; c.w1 = p.w1; c.bias1 = p.bias1; c.t1 = p.t1; c.n1 = 64;
        c.B = p.B; c.H = c.Ho = c.H2 = p.H; c.W = c.Wo = c.W2 = p.W; c.Cin = p.Cin; c.Cin2 = p.Cin2; c.stride2 = 1; c.Cout = 256;
        c.KH = c.KW = 1; c.stride = 1; c.ldx = p.Cin; c.ldy = 256; c.y_split = c.n_valid = 1 << 30; c.co_running = 1;
        st->kernel = p.Cin2 ? K_PW_PAIR_1_1_RAW_1_2_HALF : K_PW_PAIR_1_1_RAW_0_2_HALF;
        return;
    }
    const bool persistent_ok = !tile_bars_b2b_s1_persistent(p.force_tile);
    // K1 = 64 and at least two tiles per CU: the persistent form (TILE_PERSISTENT forces it whatever the size)
    if (p.Cin2 == 0 && persistent_ok && (ntiles >= 512 || p.force_tile == TILE_PERSISTENT)) { st->kernel = K_B2B_S1_PERSISTENT; return; }
    // K1 = 128 (fused shortcut, no residual): persistent 64-pixel tiles, both filter banks resident
    if (p.Cin2 == 64 && !p.res && persistent_ok && (M >= 64 * 1024 || p.force_tile == TILE_PERSISTENT)) { st->kernel = K_B2B_S1_PERSISTENT_K128; return; }
    st->kernel = K_B2B_S1;
}

// ---- convolutions ----
// chunk-major K order is set for halo-shape layers only (choose_one), and those reach the generic kernel on the tiles that have
// a chunk-major instantiation alone
static int pick_igemm(ConvStep *st, ConvKernel k, ConvKernel k_chunk_major, int BM, int BN)
{
    st->kernel = st->p.k_chunk_major ? k_chunk_major : k;
    if (st->kernel != K_NONE) return RFD_OK;
    set_error("conv: the %d x %d tile has no chunk-major form", BM, BN);
    return RFD_ERR_INVALID_ARG;
}
static int pick(ConvStep *st, ConvKernel k)
{
    st->kernel = k;
    return RFD_OK;
}

// one convolution (no pair): validation, then the rules in the order of their precedence
static int choose_one(const ConvParams &p, ConvStep *st)
{
    if (p.Cin % 64 != 0 || p.Cin2 % 64 != 0 || p.Cout % 32 != 0) {
        set_error("conv: Cin=%d must be a multiple of 64 and Cout=%d of 32", p.Cin, p.Cout);
        return RFD_ERR_INVALID_ARG;
    }
    if (p.in_scale && (p.KH != 1 || p.KW != 1 || p.pad != 0 || p.Cin > 2048)) {
        set_error("conv: the input affine is only defined for un-padded 1x1 convs with Cin <= 2048");
        return RFD_ERR_INVALID_ARG;
    }
    if ((size_t)p.B * p.H * p.W * p.ldx * 2 >= 0xfffffff0ull || (size_t)p.B * p.H2 * p.W2 * p.Cin2 * 2 >= 0xfffffff0ull) {
        set_error("conv: an input tensor of %zu bytes exceeds the 4 GiB buffer-addressing limit; lower max_batch_size",
                  (size_t)p.B * p.H * p.W * p.Cin * 2);
        return RFD_ERR_CAPACITY;
    }
    st->p = p;
    const int tile = p.force_tile;
    {   // latency schedule (rfd_config.schedule; a forced tile wins): the K range as segments over several workgroups
        SplitKPlan skp;
        if (conv_splitk_wants(p, &skp)) return pick(st, K_SPLITK_64_64_2_2);
    }
    const int M = p.B * p.Ho * p.Wo;
    // layer shapes conv3x3_halo_kernel accepts (any size, any forced tile): all their kernels accumulate chunk-major
    const bool halo_shape = p.KH == 3 && p.KW == 3 && p.stride == 1 && p.pad == 1 && p.Cin2 == 0 && !p.in_scale && !p.res && !p.y2 &&
                            !p.yf && p.y && p.Ho == p.H && p.Wo == p.W && p.n_valid >= p.Cout && p.Cin % 128 == 0 &&
                            (p.Cout % 128 == 0 || p.Cout == 192) && p.Cout <= 512 && (p.y_split >= p.Cout || p.y_split % 8 == 0) &&
                            (p.W % 16 == 0 || p.W == 40);
    if (halo_shape) st->p.k_chunk_major = 1;
    // TILE_128_EIGHT_WAVES: the generic 128 x 128 tile with EIGHT waves (32 x 64 wave tiles, two waves per SIMD from one workgroup):
    // for the small-M layers whose grid gives a CU a single workgroup (A/B; bit-identical, same K order)
    if (tile == TILE_128_EIGHT_WAVES && p.Cout % 128 == 0 && !p.in_scale) return pick_igemm(st, K_IGEMM_128_128_4_2_3, K_IGEMM_128_128_4_2_3_CM, 128, 128);
    // TILE_KX_FOUR_WAVES: the merged-kx 3x3 kernel in its older four-wave form (64 x 64 wave tiles)
    if (tile == TILE_KX_FOUR_WAVES && p.KH == 3 && p.KW == 3 && p.stride == 1 && p.pad == 1 && p.Cin2 == 0 && !p.in_scale && p.Ho == p.H && p.Wo == p.W &&
        p.W >= 3 && p.Cout % 128 == 0)
        return pick(st, K_CONV3X3_KX_128_2_2);
    // wave-specialised loader / consumer ring (kernels_ring.hip): TILE_RING = wherever the shape allows (tests, A/B)
    bool kx3 = false;
    if (tile == TILE_RING && conv_ring_supports(p, &kx3)) return pick(st, kx3 ? K_RING_KX3 : K_RING);
    {   // The ring runs the small-M, long-K layers it measured faster on, in its generic form: stage-4 conv1 (2048 -> 512: 27.3 vs
        // 28.8 us per 16 images in isolation) and the stride-2 conv2 of stage 4's first unit (48.6 vs 52.7 us); end to end +1.1 %
        // in two alternating A/B pairs on one box (7 798 / 7 734 vs 7 716 / 7 650 img/s; profiles/r04_ab_ring_env.jsonl).  Every
        // other layer stays with the kernels above (the ring is slower there: DESIGN_AB_RECORD.md round 4).  Bit-identical either
        // way (tests/test_ring_gpu.py).  RFD_CONV_RING=0 switches it off.
        static const bool ring_on = [] { const char *e = getenv("RFD_CONV_RING"); return !e || atoi(e) >= 1; }();
        if (ring_on && tile == TILE_HEURISTIC && conv_ring_supports(p, &kx3) && !kx3 && p.B * p.Ho * p.Wo <= 128 * 64 &&
            p.KH * p.KW * p.Cin + p.Cin2 >= 2048 && p.Cout == 512)
            return pick(st, K_RING);
    }
    // short-K, wide-N pointwise layers with a residual: persistent X-stationary streaming kernel
    // (one output: the raw sum or, at the end of a stage, the activated one; K = 64 only the latter -- the forms instantiated)
    const bool pw_ok = p.KH == 1 && p.KW == 1 && p.stride == 1 && p.pad == 0 && p.Cin2 == 0 && !p.in_scale && !p.yf && p.res &&
                       !(p.y && p.y2) && !(p.y && p.Cin == 64) &&
                       !p.res_up2 && !p.res_post && p.ldx == p.Cin && p.x_coff == 0 && p.Cout % 128 == 0 && p.Cout >= 4 * p.Cin &&
                       p.y_coff == 0 && p.y_split >= p.Cout && p.n_valid >= p.Cout && (!p.y || p.ldy == p.Cout) &&
                       (p.Cin == 64 || p.Cin == 128 || p.Cin == 256) && tile_admits_pw_stream(tile, p.Cin);
    // a persistent workgroup walks all N / 128 chunks of its tiles one after the other: below ~half a GPU of tiles (small
    // batches; B = 1: 13 tiles at 40 x 40) the generic kernel's tiles_m x N / 128 independent workgroups are faster
    if (pw_ok && (p.y || p.y2) && ((p.Cout >> 7) & 1) == 0 && p.Cout <= 1024 && (M >= 128 * 128 || tile == TILE_PERSISTENT)) {
        if (p.Cin == 64) return pick(st, K_PW_STREAM_1_Y2);
        if (p.Cin == 128) return pick(st, p.y ? K_PW_STREAM_2_Y : K_PW_STREAM_2_Y2);
        return pick(st, p.y ? K_PW_STREAM_4_Y : K_PW_STREAM_4_Y2);
    }
    // wide pointwise GEMMs that pw_stream does not take (conv3 + fused shortcut of the down-sampling units, stage-4 conv3, and
    // N >= 512 conv1s, where the 256 x 256 tile measured faster than pw_gemm's 256 x 128: 32.8 vs 39.3 us for 1024 -> 512 at
    // 40 x 40 x 16): persistent 256 x 256 tiles (a forced tile that admits it: whatever the size)
    const bool pww_ok = p.KH == 1 && p.KW == 1 && p.stride == 1 && p.pad == 0 && !p.in_scale && !p.yf && (p.y || p.y2) &&
                        (!p.res || (!p.res_up2 && !p.res_post)) && p.Cin2 % 64 == 0 && p.Cin + p.Cin2 >= 384 && p.Cout % 256 == 0 &&
                        p.Cout >= 512 && p.Cout <= 2048 && p.y_split >= p.Cout && p.n_valid >= p.Cout && M % 8 == 0 &&
                        tile_admits_pw_wide(tile);
    if (pww_ok && (tile != TILE_HEURISTIC || ceil_div(M, 256) * (p.Cout / 256) >= 150)) return pick(st, K_PW_WIDE);
    // long-K pointwise layers without a residual (conv1 of the units): persistent activation-streaming kernel
    // (a forced tile that admits it: whatever the size)
    const bool pwg_ok = p.KH == 1 && p.KW == 1 && p.stride == 1 && p.pad == 0 && p.Cin2 == 0 && !p.y2 && !p.yf && p.Ho == p.H && p.Wo == p.W &&
                        p.y && p.Cin % 128 == 0 && p.Cin >= 256 && p.Cin <= 2048 && p.Cout % 128 == 0 && p.Cout <= 1024 && p.y_split >= p.Cout &&
                        p.n_valid >= p.Cout && M % 8 == 0 && tile_admits_pw_gemm(tile);
    // (with a residual -- the FPN laterals -- only from 400 items: 52 vs 57 us for 512 -> 256 at 80 x 80 x 16, but 27 vs 25 us for the
    //  200 items of 1024 -> 256 at 40 x 40)
    if (pwg_ok && (tile != TILE_HEURISTIC || ceil_div(M, 256) * (p.Cout / 128) >= (p.res ? 400 : 150))) {
        // 128-pixel x 256-channel items where they cover all channels of an N = 256 layer and still fill the GPU (TILE_PW_GEMM: never)
        const bool wide = p.Cout == 256 && ceil_div(p.B * p.H * p.W, 128) >= 150 && tile != TILE_PW_GEMM;
        if (p.in_scale) return pick(st, wide ? K_PW_GEMM_AFF_WIDE : K_PW_GEMM_AFF);
        return pick(st, wide ? K_PW_GEMM_WIDE : K_PW_GEMM);
    }
    // 64 -> 64 3x3: filter bank resident in LDS, halo tile staged once for all nine taps
    const bool c64_ok = p.KH == 3 && p.KW == 3 && p.stride == 1 && p.pad == 1 && p.Cin == 64 && p.Cout == 64 && p.Cin2 == 0 && !p.in_scale &&
                        !p.res && !p.y2 && !p.yf && p.y && p.Ho == p.H && p.Wo == p.W && p.y_split >= 64 && p.n_valid >= 64 &&
                        tile_admits_c64(tile);
    if (c64_ok && (M >= 96 * 256 || tile == TILE_PERSISTENT)) return pick(st, K_CONV3X3_C64); // >= 96 tiles of 16 x 16 pixels
    // Cin >= 128 3x3: persistent halo-tile kernel; work items of 128 / 192 / 256 output channels (TN = 4 / 6 / 8).  Every 3x3
    // kernel accumulates in the same order, so the choice changes no bit of the result.
    // TILE_HALO_SMALL: smallest item, TILE_HALO_LARGE: largest item, whatever the size
    if (halo_shape && tile_admits_halo(tile)) {
        const int tiles = p.W == 40 ? p.B * ceil_div(p.H, 6) : p.B * (p.W / 16) * ceil_div(p.H, 16);
        const bool forced = tile != TILE_HEURISTIC;
        if (p.Cout == 192) {
            if (forced || tiles >= 100) return pick(st, p.W == 40 ? K_HALO_40_6_6 : K_HALO_16_16_6);
        } else {
            // (the 256-channel item is not instantiated for the 40-wide row tile: its per-pixel address registers next to 128
            //  accumulators spill to scratch, and scratch reloads share the DMA counters; 128-channel items measured 5 % slower
            //  there at B = 32 and are what the size rule picks at B = 16 anyway)
            const int items8 = p.Cout % 256 == 0 && p.W != 40 ? tiles * (p.Cout / 256) : 0, items4 = tiles * (p.Cout / 128);
            // 256-channel items read the halo half as often, 128-channel items fill the last round of workgroups better:
            // 256 unless its share of busy CU-rounds is clearly lower (B = 32, 80 x 80: 800 items = 3.1 rounds vs 1600 = 6.25)
            auto fill = [](int n) { return (double)n / (ceil_div(n, 256) * 256); };
            const bool use8 = tile == TILE_HALO_LARGE ? items8 > 0 : (tile == TILE_HALO_SMALL ? false : items8 >= 200 && fill(items8) >= fill(items4) - 0.05);
            if (use8) return pick(st, K_HALO_16_16_8);
            if (forced || items4 >= 200) return pick(st, p.W == 40 ? K_HALO_40_6_4 : K_HALO_16_16_4);
        }
    }
    const bool kx_ok = p.KH == 3 && p.KW == 3 && p.stride == 1 && p.pad == 1 && p.Cin2 == 0 && !p.in_scale && p.Ho == p.H &&
                       p.Wo == p.W && p.W >= 3 && tile != TILE_128 && tile != TILE_256x128;
    // Eight waves (32 x 64 wave tiles) since round 4: the layers that come here have small grids (stage-4 conv2: 200 tiles on 256
    // CUs), so a CU mostly holds ONE workgroup, and with four waves that is one wave per SIMD -- nothing covers its barrier, drain
    // and fragment-read latencies (1 725 cycles per 32-MFMA step).  Two waves per SIMD from the same workgroup: 53.8 -> 46.1 us
    // (stage-4 conv2, 16 images), 73 -> 65 us at 32 images where two four-wave workgroups already shared a CU, 30.5 -> 27.4 us
    // (SSH 80 x 80 context conv); same K order, bit-identical (TILE_KX_FOUR_WAVES: the four-wave form).
    if (kx_ok && p.Cout % 128 == 0) return pick(st, K_CONV3X3_KX_128_4_2);
    // (with BN = 64 the merged-kx kernel measured 7 % slower than the generic 128x64 tile at 3 workgroups / CU)
    // Per-layer tile choice for a chain that has the GPU to itself (unsplit passes, B < 16; tools/tile_sweep.py): the
    // 128x64 tile (3 workgroups per CU, twice the grid) wins by 5-28 % where the 128x128 grid cannot give every CU a
    // workgroup, and by 5-11 % on the 1x1 layers whose FLOPs per byte of activation traffic are far below the machine
    // balance (more loads in flight per CU).  With a second chain co-running (batch split) the other chain already
    // fills those gaps and the same choice measured 2.5 % SLOWER end to end, so it is not applied there.
    const long long n128 = (long long)ceil_div(M, 128) * (p.Cout / 128);
    const double act_bytes = 2.0 * ((double)(p.KH * p.KW * p.Cin + p.Cin2) / (p.stride * p.stride) +
                                    (double)p.Cout * (1 + (p.res ? 1 : 0) + (p.y && p.y2 ? 1 : 0)));
    const double flop_per_byte = 2.0 * (p.KH * p.KW * p.Cin + p.Cin2) * p.Cout / act_bytes;
    const bool prefer_small = tile == TILE_HEURISTIC && !p.co_running && (n128 <= 256 || (p.KH == 1 && flop_per_byte < 110.0));
    if (p.Cout % 128 == 0 && tile != TILE_NO_128 && !prefer_small) {
        // The 8-wave 256x128 tile with a 3-slot ring (1 workgroup per CU) measured 5-13 % SLOWER than two
        // co-resident 128x128 workgroups on every layer of this network (profiles/): opt-in only.
        if (tile == TILE_256x128) return pick_igemm(st, K_IGEMM_256_128_4_2_3, K_IGEMM_256_128_4_2_3_CM, 256, 128);
        // the 80 KiB ring leaves no room for the input-affine table next to a second workgroup
        if (tile == TILE_128 || p.in_scale) return pick_igemm(st, K_IGEMM_128_128_2_2_2, K_IGEMM_128_128_2_2_2_CM, 128, 128);
        // eight waves on the 128 x 128 tile (round 4; as in the merged-kx kernel above): 46.5 vs 49.5 us and 39.2 vs 41.0 us on the
        // stride-2 3x3 layers, 24.8 vs 26.2 us on the 1024 -> 256 lateral; the K = 2048 lateral ties (26.5 vs 26.0) and keeps four
        if (!(p.KH == 1 && p.Cin + p.Cin2 >= 2048)) return pick_igemm(st, K_IGEMM_128_128_4_2_3, K_IGEMM_128_128_4_2_3_CM, 128, 128);
        return pick_igemm(st, K_IGEMM_128_128_2_2_3, K_NONE, 128, 128);
    }
    // fused SSH pair (conv1 + ctx1 along N): eight waves (32 x 96 wave tiles) since round 4 -- these layers have at most 50 tiles
    // below the halo kernel's threshold, one workgroup per CU, and the four-wave form needs 284 registers (one wave per SIMD)
    if (p.Cout % 192 == 0 && p.Cout % 128 != 0)
        return (tile == TILE_128 || tile == TILE_KX_FOUR_WAVES) ? pick_igemm(st, K_IGEMM_128_192_2_2_2, K_IGEMM_128_192_2_2_2_CM, 128, 192)
                                                                : pick_igemm(st, K_IGEMM_128_192_4_2_2, K_IGEMM_128_192_4_2_2_CM, 128, 192);
    // 128x64: the 2-slot ring keeps 3 workgroups per CU, which measured faster than a deeper ring at 2
    if (p.Cout % 64 == 0) {
        if (tile == TILE_256x64) return pick_igemm(st, K_IGEMM_256_64_4_1_2, K_NONE, 256, 64); // 64x64 wave tiles, 2 workgroups / CU
        return pick_igemm(st, K_IGEMM_128_64_4_1_2, K_NONE, 128, 64);
    }
    return pick_igemm(st, K_IGEMM_128_32_4_1_2, K_NONE, 128, 32);
}

int choose_conv(const ConvParams &p, bool w1_behind_w, ConvPlan *plan)
{
    plan->steps = 0;
    // every kernel addresses its tensors through 32-bit buffer descriptors and offsets: inputs, outputs (M x Cout, M x ldy) and,
    // for a back-to-back pair, conv1's output (M x n1) must each stay below 4 GiB -- checked before ANY path is chosen
    // (round-3 advisor finding: the pair branch used to return before the guard; B >= 328 at the stage 1 -> 2 boundary wrapped)
    {
        const size_t Mo = (size_t)p.B * p.Ho * p.Wo, lim = 0xfffffff0ull;
        const size_t in1 = (size_t)p.B * p.H * p.W * (p.ldx ? p.ldx : p.Cin) * 2, in2 = (size_t)p.B * p.H2 * p.W2 * p.Cin2 * 2;
        const size_t out = Mo * (size_t)std::max(p.Cout, p.ldy) * (p.yf ? 4 : 2), out1 = p.w1 ? Mo * (size_t)p.n1 * 2 : 0;
        if (in1 >= lim || in2 >= lim || out >= lim || out1 >= lim) {
            set_error("conv: a tensor of %zu bytes exceeds the 4 GiB buffer-addressing limit; lower max_batch_size",
                      std::max(std::max(in1, in2), std::max(out, out1)));
            return RFD_ERR_CAPACITY;
        }
    }
    if (!p.w1) {
        plan->steps = 1;
        return choose_one(p, &plan->step[0]);
    }
    // conv3 of a dim-match unit + the next unit's conv1 (OP_B2B beyond stage 1).  One persistent kernel where pw_stream
    // itself would run (the tiles that keep the generic kernels and small batches: two launches; bit-identical either way).
    const int M1 = p.B * p.Ho * p.Wo;
    // two shapes: (i) a middle unit of stage 2: 128 -> 512, raw sum out, conv1 512 -> 128 on relu(BN(raw));
    //             (ii) the last unit of stage 1: 64 -> 256, activated output only, conv1 256 -> 128 of stage 2's first unit on it
    const bool act_out = !p.y && p.y2;
    const bool s3 = !act_out && p.Cin == 256 && p.Cout == 1024 && p.y && !p.y2 && p.ldy == p.Cout; // stage 3's middle units: pw_pair_kernel only
    const bool b23 = act_out && p.Cin == 128 && p.Cout == 512 && p.n1 == 256;                     // stage 2 -> 3 boundary: pw_pair_kernel only
    const bool shape = s3 || b23 || (act_out ? (p.Cin == 64 && p.Cout == 256 && p.n1 == 128) : (p.Cin == 128 && p.Cout == 512 && p.n1 == 128 && p.y && !p.y2 && p.ldy == p.Cout));
    // the first unit of stage 2: conv3 128 -> 512 with the 1x1 stride-2 shortcut 256 -> 512 as second K segment, no residual
    const bool u1 = !act_out && p.Cin == 128 && p.Cin2 == 256 && p.stride2 == 2 && p.Cout == 512 && p.n1 == 128 && !p.res && p.y && !p.y2 && p.ldy == p.Cout && p.bias2;
    const bool fuse = p.KH == 1 && p.KW == 1 && p.stride == 1 && p.pad == 0 && (u1 || (shape && p.Cin2 == 0 && p.res)) && !p.in_scale &&
                      !p.res_up2 && !p.res_post && !p.relu && !p.yf && p.ldx == p.Cin && p.x_coff == 0 &&
                      p.y_coff == 0 && p.y_split >= p.Cout && p.n_valid >= p.Cout &&
                      (tile_forces_pair(p.force_tile) || (p.force_tile == TILE_HEURISTIC && M1 >= 128 * 128));
    // the pair as its two convolutions, as the small-batch rule above already runs it
    ConvParams a = p;
    a.w1 = nullptr; a.bias1 = nullptr; a.t1 = nullptr;
    ConvParams q;
    memset(&q, 0, sizeof q);
    q.x = act_out ? p.y2 : p.y; q.w = p.w1; q.bias = p.bias1; q.zero = p.zero;
    if (!act_out) { q.in_scale = p.scale2; q.in_shift = p.shift2; }
    q.y = p.t1;
    q.B = p.B; q.H = q.Ho = p.Ho; q.W = q.Wo = p.Wo; q.Cin = p.Cout; q.Cout = p.n1;
    q.KH = q.KW = 1; q.stride = 1; q.pad = 0;
    q.ldx = p.Cout; q.ldy = p.n1; q.y_split = 1 << 30; q.n_valid = 1 << 30; q.relu = 1;
    q.force_tile = p.force_tile == TILE_PAIR ? TILE_HEURISTIC : p.force_tile; q.co_running = p.co_running;
    if (p.latency) q.fail = p.fail;
    q.latency = p.latency; q.sk_ws = p.sk_ws; q.sk_cnt = p.sk_cnt; q.sk_ws_bytes = p.sk_ws_bytes; q.sk_cnt_n = p.sk_cnt_n; // one after the other on one stream: shared
    // latency schedule: a pair one of whose convolutions is split never runs fused, whatever the batch (the fused kernel sums in
    // the throughput order; a frame's bits must not depend on the size of the latency pass)
    SplitKPlan skp;
    const bool split_pair = conv_splitk_wants(a, &skp) || conv_splitk_wants(q, &skp);
    if (fuse && !split_pair && w1_behind_w) {
        ConvStep *st = &plan->step[0];
        plan->steps = 1;
        st->p = p;
        if (u1) return pick(st, K_PW_PAIR_2_1_RAW_4);
        if (s3) {
            if (p.n1 != 256) { set_error("conv pair: stage-3 form instantiated for n1 = 256, got %d", p.n1); return RFD_ERR_INVALID_ARG; }
            return pick(st, K_PW_PAIR_4_2_RAW);
        }
        if (b23) return pick(st, K_PW_PAIR_2_2_ACT);
        // the stage 1 -> 2 boundary: both filter banks (96 KiB) resident in LDS, barrier-free
        if (act_out) return pick(st, K_PW_PAIR_1_1_ACT_0_2);
        return pick(st, K_PW_B2B_2); // stage 2's middle units
    }
    plan->steps = 2;
    RFD_TRY(choose_one(a, &plan->step[0]));
    return choose_one(q, &plan->step[1]);
}

} // namespace rfd
