// network.hip -- graph construction, workspace planning, weights and execution of the RetinaFace
// network (build-defined: SURVEY.md Appendix B; the reference only knows the Triton model name
// "face_detection_retina", config.rs:25, and the 9-output contract its decode implies).
#include "network.h"

#include <math.h>
#include <algorithm>
#include <utility>

namespace rfd {

// ------------------------------------------------------------------------------------------------
// Graph
// ------------------------------------------------------------------------------------------------
int Graph::add_tensor(int C, int H, int W, int f32)
{
    TensorDesc t;
    t.C_logical = C;
    t.C = (f32 || C == 4 || C % 64 == 0) ? C : (C + 63) / 64 * 64; // bf16 activations: K of every consumer is a multiple of 64
    t.H = H; t.W = W; t.is_f32 = f32; t.buffer = -1; t.first = 1 << 30; t.last = -1;
    tensors.push_back(t);
    return (int)tensors.size() - 1;
}

// extra_k > 0: reserve extra_k more columns per row for a fused shortcut conv; parent >= 0: this layer
// lives in those columns (at col_off) of layer `parent` and allocates nothing.
int Graph::add_layer(const std::string &name, int cin, int cout, int k, int stride, int pad, float gain,
                     int has_affine, int extra_k, int parent, int col_off, int kind, int cout_dev)
{
    Layer L;
    L.name = name; L.cin = cin; L.cout = cout; L.kh = k; L.kw = k; L.stride = stride; L.pad = pad;
    L.gain = gain; L.has_affine = has_affine; L.kind = kind;
    L.cin_d = kind == LK_CONV ? (cin + 63) / 64 * 64 : cin;
    L.cout_d = cout_dev ? cout_dev : cout;
    if (parent >= 0) {
        L.w_off = layers[parent].w_off + col_off;
        L.ldw = layers[parent].ldw;
        L.w_elems = 0;
    } else {
        L.w_off = w_total;
        if (kind == LK_CONV0) { L.ldw = 7 * 32; L.w_elems = (size_t)cout * L.ldw; }
        else if (kind == LK_FIRST3X3) { L.ldw = 36; L.w_elems = (size_t)cout * 36; }        // [cout][3][3][4]
        else if (kind == LK_DEPTHWISE) { L.ldw = L.cout_d; L.w_elems = (size_t)9 * L.cout_d; } // [9][C]
        else { L.ldw = (size_t)k * k * L.cin_d + extra_k; L.w_elems = (size_t)L.cout_d * L.ldw; }
    }
    w_total += (L.w_elems + 63) & ~(size_t)63; // keep every layer 128-byte aligned
    L.b_off = b_total;
    b_total += (size_t)L.cout_d;
    L.a_off = a_total;
    if (has_affine) a_total += (size_t)2 * L.cout_d;
    layers.push_back(L);
    return (int)layers.size() - 1;
}

int Graph::add_conv(int layer, int in, int out, int relu, int res, int out2, int outf)
{
    Op o;
    o.kind = OP_CONV; o.layer = layer; o.in = in; o.out = out; o.out2 = out2; o.outf = outf; o.res = res;
    o.in2 = -1; o.layer2 = -1; o.in_affine = -1;
    o.layer_n2 = -1; o.x_coff = 0; o.y_split = 1 << 30; o.y_split_add = 0; o.n_valid = 1 << 30;
    o.layer_b = -1; o.out_b = -1; o.branch = 0;
    o.relu = relu; o.res_up2 = 0; o.res_post = 0; o.head_softmax = 0; o.y_coff = 0;
    ops.push_back(o);
    return (int)ops.size() - 1;
}

// RetinaFace-R50: pre-activation ResNet-50 (units 3,4,6,3; stride on the 3x3) + 256-ch FPN + SSH
// context modules + 1x1 heads (A = 2), every BN folded into the preceding conv or applied as the
// post-add affine of the previous unit's epilogue.  82 convolutions (the 9 head convs run as three
// fused N = 32 GEMMs).
void Graph::build_r50()
{
    const int H = net_h, W = net_w;
    input = add_tensor(4, H, W);
    const int l0 = add_layer("conv0", 3, 64, 7, 2, 3, 1.0f / 128.0f, 1, 0, -1, 0, LK_CONV0);
    // stem: conv0 + BN + ReLU + max pool + BN1 + ReLU as ONE kernel (the 320x320x64 conv0 activation stays on chip)
    const int t_p = add_tensor(64, H / 4, W / 4);
    {
        Op o{OP_STEM, l0, input, t_p, -1, -1, -1, -1, -1, -1, -1, 0, 1 << 30, 0, 1 << 30, 0, -1, -1, 1, 0, 0, 0, 0};
        ops.push_back(o);
    }
    static const int units[4] = {3, 4, 6, 3};
    static const int mids[4] = {64, 128, 256, 512};
    int x_act = t_p, x_raw = -1, cin = 64, h = H / 4, w = W / 4;
    int prev_l3 = -1; // conv3 layer of the previous unit when its BN+ReLU output was NOT materialised
    int b2b_t1 = -1;  // conv1 output already produced by the previous unit's back-to-back kernel
    int c_out[4] = {-1, -1, -1, -1};
    for (int s = 0; s < 4; ++s) {
        const int mid = mids[s], cout = mid * 4;
        for (int u = 0; u < units[s]; ++u) {
            const int stride = (s > 0 && u == 0) ? 2 : 1;
            const bool dim_match = u > 0;
            const int ho = h / stride, wo = w / stride;
            char nm[64];
            int t1 = b2b_t1; // stage 1: this unit's conv1 already ran inside the previous unit's back-to-back kernel
            b2b_t1 = -1;
            if (t1 < 0) {
                snprintf(nm, sizeof nm, "stage%d_unit%d_conv1", s + 1, u + 1);
                const int l1 = add_layer(nm, cin, mid, 1, 1, 0, 1.0f, 0);
                t1 = add_tensor(mid, h, w);
                // inside a stage the previous unit stores only its raw sum; its BN+ReLU ("act") is applied
                // to this conv's input fragments on the fly instead of round-tripping a second tensor
                const int o1 = add_conv(l1, x_act >= 0 ? x_act : x_raw, t1, 1);
                if (x_act < 0) ops[o1].in_affine = prev_l3;
            }
            snprintf(nm, sizeof nm, "stage%d_unit%d_conv2", s + 1, u + 1);
            const int l2 = add_layer(nm, mid, mid, 3, stride, 1, 1.0f, 0);
            const int t2 = add_tensor(mid, ho, wo);
            add_conv(l2, t1, t2, 1);
            // conv3 (+ identity residual) -- or, in the first unit of a stage, conv3 and the 1x1 shortcut
            // conv fused as ONE GEMM over the concatenated K = [mid | cin]: the shortcut tensor never exists
            snprintf(nm, sizeof nm, "stage%d_unit%d_conv3", s + 1, u + 1);
            const int l3 = add_layer(nm, mid, cout, 1, 1, 0, 1.0f, 1, dim_match ? 0 : cin);
            int ls = -1;
            if (!dim_match) {
                snprintf(nm, sizeof nm, "stage%d_unit%d_sc", s + 1, u + 1);
                ls = add_layer(nm, cin, cout, 1, stride, 0, 1.0f, 0, 0, l3, mid);
            }
            const bool last = u + 1 == units[s];
            // Stages 1-3: only stage outputs materialise BN+ReLU, the units in between hand over the raw sum alone and the next
            // conv1 applies the affine to its operand fragments.  (Round 1 measured that as a loss for stage 3 with the generic
            // kernel; with the HBM-bound streaming kernels of round 2 -- pw_stream without the second output, pw_gemm<true> --
            // it is +1-2 % end to end: 7.24 k vs 7.09-7.19 k img/s on one box.  Stage 4 too: 7.13-7.18 k, so it keeps both.)
            const bool fuse_act = s < 3;
            const int t_raw = last ? -1 : add_tensor(cout, ho, wo);
            const int t_act = (last || !fuse_act) ? add_tensor(cout, ho, wo) : -1;
            const int o3 = add_conv(l3, t2, t_raw, 0, dim_match ? x_raw : -1, t_act);
            if (!dim_match) { ops[o3].in2 = x_act; ops[o3].layer2 = ls; }
            if (s <= 1 && last) {
                // the last unit of stage 1 with stage 2's first conv1 (256 -> 128 at 160 x 160, on the stage output): pw_b2b_kernel;
                // the last unit of stage 2 with stage 3's first conv1 (512 -> 256 at 80 x 80): pw_pair_kernel
                snprintf(nm, sizeof nm, "stage%d_unit%d_conv1", s + 2, 1);
                const int l1n = add_layer(nm, cout, mids[s + 1], 1, 1, 0, 1.0f, 0);
                b2b_t1 = add_tensor(mids[s + 1], ho, wo);
                ops[o3].kind = OP_B2B; ops[o3].layer_b = l1n; ops[o3].out_b = b2b_t1;
            }
            if ((s <= 1 || (s == 2 && dim_match)) && !last) {
                // stage 1: conv3 of this unit and conv1 of the NEXT unit run back to back in one kernel; the
                // activated 256-channel tile stays in LDS (conv_b2b_s1_kernel).  Stages 2 (every unit) and 3 (the dim-match units):
                // the same pairing -- pw_b2b_kernel / pw_pair_kernel, or two launches where it does not pay
                snprintf(nm, sizeof nm, "stage%d_unit%d_conv1", s + 1, u + 2);
                const int l1n = add_layer(nm, cout, mid, 1, 1, 0, 1.0f, 0);
                b2b_t1 = add_tensor(mid, ho, wo);
                ops[o3].kind = OP_B2B; ops[o3].layer_b = l1n; ops[o3].out_b = b2b_t1;
            }
            x_raw = t_raw; x_act = t_act; prev_l3 = l3; cin = cout; h = ho; w = wo;
        }
        c_out[s] = x_act;
    }
    // FPN (c1 = stage2 out @ /8, c2 = stage3 out @ /16, c3 = stage4 out @ /32), each level immediately followed by
    // its SSH context module + fused heads (reference slot order 32,16,8).  The stride-32 and stride-16 chains are
    // side branches: small grids, independent of everything after them -> they overlap the stride-8 work.
    // SSH: one 384-channel buffer O = [b1 0:128 | b2 128:192 | b3 192:256 | tc 256:320 | td 320:384]; sibling convs
    // that share an input run as ONE GEMM along N:  {conv1, ctx1}(f) -> b1 | tc ;  {ctx2, ctx3a}(tc) -> b2 | td ;
    // ctx3b(td) -> b3 ;  heads read the concat O[:, 0:256].  (All five carry the post-concat ReLU.)
    const int c1 = c_out[1], c2 = c_out[2], c3 = c_out[3];
    auto T = [&](int t) -> TensorDesc & { return tensors[t]; };
    auto ssh_and_head = [&](int l, int f, int branch) {
        const int fh = T(f).H, fw = T(f).W, st = kStrides[l];
        const size_t first = ops.size();
        char nm[64];
        const int o = add_tensor(384, fh, fw);
        snprintf(nm, sizeof nm, "ssh%d_conv1", st);
        const int la = add_layer(nm, 256, 128, 3, 1, 1, 1.0f, 0);
        snprintf(nm, sizeof nm, "ssh%d_ctx1", st);
        const int lb = add_layer(nm, 256, 64, 3, 1, 1, 1.0f, 0);
        {
            Op &A = ops[add_conv(la, f, o, 1)];
            A.layer_n2 = lb; A.y_split = 128; A.y_split_add = 128;
        }
        snprintf(nm, sizeof nm, "ssh%d_ctx2", st);
        const int lc = add_layer(nm, 64, 64, 3, 1, 1, 1.0f, 0);
        snprintf(nm, sizeof nm, "ssh%d_ctx3a", st);
        const int ld = add_layer(nm, 64, 64, 3, 1, 1, 1.0f, 0);
        {
            Op &B = ops[add_conv(lc, o, o, 1)];
            B.layer_n2 = ld; B.x_coff = 256; B.y_coff = 128; B.y_split = 64; B.y_split_add = 128;
        }
        snprintf(nm, sizeof nm, "ssh%d_ctx3b", st);
        {
            Op &C = ops[add_conv(add_layer(nm, 64, 64, 3, 1, 1, 1.0f, 0), o, o, 1)];
            C.x_coff = 320; C.y_coff = 192;
        }
        snprintf(nm, sizeof nm, "head%d", st);
        heads[l] = add_tensor(32, fh, fw, 1);
        ops[add_conv(add_layer(nm, 256, 32, 1, 1, 0, 1.0f, 0), o, -1, 0, -1, -1, heads[l])].head_softmax = 1;
        for (size_t i = first; i < ops.size(); ++i) ops[i].branch = branch;
    };
    const int lat3 = add_layer("fpn_lat3", 2048, 256, 1, 1, 0, 1.0f, 0);
    const int p3 = add_tensor(256, T(c3).H, T(c3).W);
    add_conv(lat3, c3, p3, 1);
    ssh_and_head(0, p3, 1);
    const int lat2 = add_layer("fpn_lat2", 1024, 256, 1, 1, 0, 1.0f, 0);
    const int p2pre = add_tensor(256, T(c2).H, T(c2).W);
    {
        const int o = add_conv(lat2, c2, p2pre, 1, p3);
        ops[o].res_up2 = 1; ops[o].res_post = 1;
    }
    const int ag2 = add_layer("fpn_aggr2", 256, 256, 3, 1, 1, 0.8f, 0);
    const int p2 = add_tensor(256, T(c2).H, T(c2).W);
    add_conv(ag2, p2pre, p2, 1);
    ssh_and_head(1, p2, 2);
    const int lat1 = add_layer("fpn_lat1", 512, 256, 1, 1, 0, 1.0f, 0);
    const int p1pre = add_tensor(256, T(c1).H, T(c1).W);
    {
        const int o = add_conv(lat1, c1, p1pre, 1, p2);
        ops[o].res_up2 = 1; ops[o].res_post = 1;
    }
    const int ag1 = add_layer("fpn_aggr1", 256, 256, 3, 1, 1, 0.8f, 0);
    const int p1 = add_tensor(256, T(c1).H, T(c1).W);
    add_conv(ag1, p1pre, p1, 1);
    ssh_and_head(2, p1, 0);
}

// RetinaFace-MobileNet-0.25 (BASELINE.json configs[1]): MobileNetV1 x0.25 backbone (first 3x3/2 conv, 13
// depthwise-separable blocks), 64-channel FPN, SSH (32 | 16 | 16) and the same fused heads / anchor contract.
// Activation tensors are zero-padded to 64 channels on the device so that every pointwise / FPN / SSH / head
// conv runs on the MFMA implicit-GEMM kernel; depthwise 3x3 and the first conv have their own small kernels.
void Graph::build_mnet025()
{
    const int H = net_h, W = net_w;
    input = add_tensor(4, H, W);
    auto T = [&](int t) -> TensorDesc & { return tensors[t]; };
    auto simple_op = [&](int kind, int layer, int in, int out) {
        Op o{kind, layer, in, out, -1, -1, -1, -1, -1, -1, -1, 0, 1 << 30, 0, 1 << 30, 0, -1, -1, 1, 0, 0, 0, 0};
        ops.push_back(o);
    };
    int h = H / 2, w = W / 2;
    int x = add_tensor(8, h, w);
    simple_op(OP_FIRST, add_layer("conv1", 3, 8, 3, 2, 1, 1.0f / 128.0f, 0, 0, -1, 0, LK_FIRST3X3, 8), input, x);
    static const int couts[13] = {16, 32, 32, 64, 64, 128, 128, 128, 128, 128, 128, 256, 256};
    static const int strides[13] = {1, 2, 1, 2, 1, 2, 1, 1, 1, 1, 1, 2, 1};
    int cin = 8, c1 = -1, c2 = -1, c3 = -1;
    for (int i = 0; i < 13; ++i) {
        char nm[64];
        const int ho = h / strides[i], wo = w / strides[i];
        snprintf(nm, sizeof nm, "block%d_dw", i + 1);
        const int tdw = add_tensor(cin, ho, wo);
        simple_op(OP_DW, add_layer(nm, 1, cin, 3, strides[i], 1, 1.0f, 0, 0, -1, 0, LK_DEPTHWISE, T(tdw).C), x, tdw);
        snprintf(nm, sizeof nm, "block%d_pw", i + 1);
        const int tpw = add_tensor(couts[i], ho, wo);
        add_conv(add_layer(nm, cin, couts[i], 1, 1, 0, 1.0f, 0, 0, -1, 0, LK_CONV, T(tpw).C), tdw, tpw, 1);
        x = tpw; cin = couts[i]; h = ho; w = wo;
        if (i == 4) c1 = x;   // 64 ch @ /8
        if (i == 10) c2 = x;  // 128 ch @ /16
        if (i == 12) c3 = x;  // 256 ch @ /32
    }
    // FPN (64 channels), each level immediately followed by its SSH + head chain; the stride-32 / stride-16 chains
    // are side branches (own streams), as in the R50 graph.
    // SSH: O[64] = [conv1 0:32 | ctx2 32:48 | ctx3b 48:64], ctx1: 64 -> 16, ctx3a: 16 -> 16; ReLU after concat
    auto ssh_and_head = [&](int l, int f, int branch) {
        const int fh = T(f).H, fw = T(f).W, st = kStrides[l];
        const size_t first = ops.size();
        char nm[64];
        const int o = add_tensor(64, fh, fw);
        snprintf(nm, sizeof nm, "ssh%d_conv1", st);
        add_conv(add_layer(nm, 64, 32, 3, 1, 1, 1.0f, 0), f, o, 1);
        snprintf(nm, sizeof nm, "ssh%d_ctx1", st);
        const int tc = add_tensor(16, fh, fw);
        add_conv(add_layer(nm, 64, 16, 3, 1, 1, 1.0f, 0, 0, -1, 0, LK_CONV, 64), f, tc, 1);
        snprintf(nm, sizeof nm, "ssh%d_ctx2", st);
        { Op &B = ops[add_conv(add_layer(nm, 16, 16, 3, 1, 1, 1.0f, 0, 0, -1, 0, LK_CONV, 32), tc, o, 1)]; B.y_coff = 32; B.n_valid = 16; }
        snprintf(nm, sizeof nm, "ssh%d_ctx3a", st);
        const int td = add_tensor(16, fh, fw);
        add_conv(add_layer(nm, 16, 16, 3, 1, 1, 1.0f, 0, 0, -1, 0, LK_CONV, 64), tc, td, 1);
        snprintf(nm, sizeof nm, "ssh%d_ctx3b", st);
        { Op &C = ops[add_conv(add_layer(nm, 16, 16, 3, 1, 1, 1.0f, 0, 0, -1, 0, LK_CONV, 32), td, o, 1)]; C.y_coff = 48; C.n_valid = 16; }
        snprintf(nm, sizeof nm, "head%d", st);
        heads[l] = add_tensor(32, fh, fw, 1);
        ops[add_conv(add_layer(nm, 64, 32, 1, 1, 0, 1.0f, 0), o, -1, 0, -1, -1, heads[l])].head_softmax = 1;
        for (size_t i = first; i < ops.size(); ++i) ops[i].branch = branch;
    };
    const int p3 = add_tensor(64, T(c3).H, T(c3).W);
    add_conv(add_layer("fpn_lat3", 256, 64, 1, 1, 0, 1.0f, 0), c3, p3, 1);
    ssh_and_head(0, p3, 1);
    const int p2pre = add_tensor(64, T(c2).H, T(c2).W);
    { const int o = add_conv(add_layer("fpn_lat2", 128, 64, 1, 1, 0, 1.0f, 0), c2, p2pre, 1, p3); ops[o].res_up2 = 1; ops[o].res_post = 1; }
    const int p2 = add_tensor(64, T(c2).H, T(c2).W);
    add_conv(add_layer("fpn_aggr2", 64, 64, 3, 1, 1, 0.8f, 0), p2pre, p2, 1);
    ssh_and_head(1, p2, 2);
    const int p1pre = add_tensor(64, T(c1).H, T(c1).W);
    { const int o = add_conv(add_layer("fpn_lat1", 64, 64, 1, 1, 0, 1.0f, 0), c1, p1pre, 1, p2); ops[o].res_up2 = 1; ops[o].res_post = 1; }
    const int p1 = add_tensor(64, T(c1).H, T(c1).W);
    add_conv(add_layer("fpn_aggr1", 64, 64, 3, 1, 1, 0.8f, 0), p1pre, p1, 1);
    ssh_and_head(2, p1, 0);
}

void Graph::plan()
{
    const int nops = (int)ops.size();
    auto touch = [&](int t, int i, bool write) {
        if (t < 0) return;
        TensorDesc &d = tensors[t];
        if (write) d.first = std::min(d.first, i);
        d.last = std::max(d.last, i);
    };
    tensors[input].first = -1;
    for (int i = 0; i < nops; ++i) {
        const Op &o = ops[i];
        touch(o.in, i, false);
        touch(o.in2, i, false);
        touch(o.res, i, false);
        touch(o.out, i, true);
        touch(o.out2, i, true);
        touch(o.outf, i, true);
        touch(o.out_b, i, true);
    }
    for (int l = 0; l < 3; ++l) tensors[heads[l]].last = nops; // consumed by decode after the net
    // side-branch ops run concurrently with later main-stream ops: everything they read or write keeps its buffer
    // to the end of the pass (no reuse in either direction)
    for (int i = 0; i < nops; ++i) {
        const Op &o = ops[i];
        if (!o.branch) continue;
        const int ts[7] = {o.in, o.in2, o.res, o.out, o.out2, o.outf, o.out_b};
        for (int t : ts)
            if (t >= 0) tensors[t].last = nops;
    }
    buffer_bytes_per_image.clear();
    std::vector<int> free_list;
    auto assign = [&](int t) {
        TensorDesc &d = tensors[t];
        if (d.buffer >= 0) return;
        const size_t need = d.bytes_per_image();
        int best = -1;
        for (size_t k = 0; k < free_list.size(); ++k) {
            const int bi = free_list[k];
            if (buffer_bytes_per_image[bi] >= need &&
                (best < 0 || buffer_bytes_per_image[bi] < buffer_bytes_per_image[free_list[best]]))
                best = (int)k;
        }
        if (best >= 0) {
            d.buffer = free_list[best];
            free_list.erase(free_list.begin() + best);
        } else {
            buffer_bytes_per_image.push_back(need);
            d.buffer = (int)buffer_bytes_per_image.size() - 1;
        }
    };
    // batch-contiguous I/O tensors (written by preprocess / read by decode over the whole batch): exclusive buffers
    auto assign_exclusive = [&](int t) {
        buffer_bytes_per_image.push_back(tensors[t].bytes_per_image());
        tensors[t].buffer = (int)buffer_bytes_per_image.size() - 1;
        tensors[t].last = nops; // never released
    };
    assign_exclusive(input);
    for (int l = 0; l < 3; ++l) assign_exclusive(heads[l]);
    for (int i = 0; i < nops; ++i) {
        for (size_t t = 0; t < tensors.size(); ++t) // release tensors dead before op i
            if (tensors[t].buffer >= 0 && tensors[t].last == i - 1 && tensors[t].last < nops)
                free_list.push_back(tensors[t].buffer);
        const Op &o = ops[i];
        if (o.out >= 0) assign(o.out);
        if (o.out2 >= 0) assign(o.out2);
        if (o.outf >= 0) assign(o.outf);
        if (o.out_b >= 0) assign(o.out_b);
    }
}

int Graph::build(int backbone_, int w, int h)
{
    backbone = backbone_; net_w = w; net_h = h;
    if (w <= 0 || h <= 0 || (w % 32) != 0 || (h % 32) != 0) {
        set_error("image_size (%d,%d) must be positive multiples of 32", w, h);
        return RFD_ERR_INVALID_ARG;
    }
    if (backbone == RFD_BACKBONE_R50) {
        build_r50();
    } else if (backbone == RFD_BACKBONE_MNET025) {
        build_mnet025();
    } else {
        set_error("backbone %d is not implemented in this build", backbone);
        return RFD_ERR_INVALID_ARG;
    }
    plan();
    return RFD_OK;
}

double Graph::layer_macs(int i) const
{
    const Op &o = ops[i];
    const Layer &L = layers[o.layer];
    if (o.kind == OP_STEM) return (double)(net_h / 2) * (net_w / 2) * L.cout * L.kh * L.kw * L.cin;
    if (o.kind == OP_DW) return (double)tensors[o.out].H * tensors[o.out].W * L.cout * 9;
    const int t = o.out >= 0 ? o.out : (o.out2 >= 0 ? o.out2 : o.outf);
    double m = (double)tensors[t].H * tensors[t].W * L.cout * L.kh * L.kw * L.cin;
    if (o.layer2 >= 0) m += (double)tensors[t].H * tensors[t].W * L.cout * layers[o.layer2].cin;
    if (o.layer_n2 >= 0) m += (double)tensors[t].H * tensors[t].W * layers[o.layer_n2].cout * L.kh * L.kw * L.cin;
    if (o.layer_b >= 0) m += (double)tensors[t].H * tensors[t].W * layers[o.layer_b].cout * layers[o.layer_b].cin;
    return m;
}

double Graph::macs_per_image() const
{
    double s = 0;
    for (size_t i = 0; i < ops.size(); ++i) s += layer_macs((int)i);
    return s;
}

// ------------------------------------------------------------------------------------------------
// Network
// ------------------------------------------------------------------------------------------------
// latency schedule: the split-K workspace per stream and the arrival counters per op, from the graph alone; returns the counters of
// all ops together
int Network::plan_splitk()
{
    // the same plan launch_conv_splitk() makes, at the largest latency pass: workspace per stream, counters per op
    const int Bl = std::min(max_batch, (int)RFD_LATENCY_MAX_BATCH);
    sk_cnt_off.assign(g.ops.size(), 0);
    sk_cnt_n.assign(g.ops.size(), 0);
    int cnt_total = 0;
    for (size_t i = 0; i < g.ops.size(); ++i) {
        const Op &o = g.ops[i];
        if (o.kind != OP_CONV && o.kind != OP_B2B) continue;
        const Layer &L = g.layers[o.layer];
        const int tout = o.out >= 0 ? o.out : (o.out2 >= 0 ? o.out2 : o.outf);
        const int HoWo = g.tensors[tout].H * g.tensors[tout].W;
        const int cout = L.cout_d + (o.layer_n2 >= 0 ? g.layers[o.layer_n2].cout_d : 0);
        const int K = L.kh * L.kw * L.cin_d + (o.layer2 >= 0 ? g.layers[o.layer2].cin_d : 0);
        SplitKPlan pl;
        const int br = std::min(std::max(o.branch, 0), 2);
        if (L.cin_d % 64 == 0 && conv_splitk_plan(K, cout, HoWo, Bl, &pl)) {
            sk_ws_bytes[br] = std::max(sk_ws_bytes[br], pl.ws_bytes);
            sk_cnt_n[i] = std::max(sk_cnt_n[i], pl.tiles);
        }
        if (o.kind == OP_B2B && conv_splitk_plan(cout, g.layers[o.layer_b].cout_d, HoWo, Bl, &pl)) { // the pair's conv1: 1x1 on this op's output
            sk_ws_bytes[br] = std::max(sk_ws_bytes[br], pl.ws_bytes);
            sk_cnt_n[i] = std::max(sk_cnt_n[i], pl.tiles);
        }
        sk_cnt_off[i] = cnt_total;
        cnt_total += sk_cnt_n[i];
    }
    return cnt_total;
}

int Network::create(int backbone, int net_w, int net_h, int max_batch_, int precision_, int schedule_)
{
    RFD_TRY(g.build(backbone, net_w, net_h));
    max_batch = max_batch_;
    precision = precision_;
    schedule = schedule_;
    if (schedule == RFD_SCHEDULE_LATENCY) {
        const int cnt_total = plan_splitk();
        for (int b = 0; b < 3; ++b)
            if (sk_ws_bytes[b]) RFD_HIP(hipMalloc((void **)&d_sk_ws[b], sk_ws_bytes[b]));
        RFD_HIP(hipMalloc((void **)&d_sk_cnt, (size_t)std::max(cnt_total, 1) * sizeof(unsigned)));
        RFD_HIP(hipMemset(d_sk_cnt, 0, (size_t)std::max(cnt_total, 1) * sizeof(unsigned))); // (the synchronize below orders it)
    }
    if (precision != 0) {
        for (const Op &o : g.ops)
            if (o.kind == OP_DW || o.kind == OP_FIRST) { set_error("f32 parity mode: this backbone has no f32 kernels (RetinaFace-R50 only)"); return RFD_ERR_INVALID_ARG; }
        use_graph = false;
        RFD_HIP(hipMalloc((void **)&d_w32, g.w_total * sizeof(float)));
        RFD_HIP(hipMemset(d_w32, 0, g.w_total * sizeof(float)));
        d_buffers32.assign(g.buffer_bytes_per_image.size(), nullptr);
        for (size_t i = 0; i < d_buffers32.size(); ++i) {
            RFD_HIP(hipMalloc(&d_buffers32[i], g.buffer_bytes_per_image[i] * 2 * (size_t)max_batch));
            RFD_HIP(hipMemset(d_buffers32[i], 0, g.buffer_bytes_per_image[i] * 2 * (size_t)max_batch));
        }
    }
    RFD_HIP(hipMalloc((void **)&d_w, g.w_total * sizeof(bf16_t)));
    RFD_HIP(hipMalloc((void **)&d_b, (g.b_total + g.a_total) * sizeof(float))); // biases, then affines
    RFD_HIP(hipMemset(d_w, 0, g.w_total * sizeof(bf16_t)));
    RFD_HIP(hipMemset(d_b, 0, (g.b_total + g.a_total) * sizeof(float)));
    for (int i = 0; i < kPool; ++i) RFD_HIP(hipStreamCreateWithFlags(&pool[i], hipStreamNonBlocking));
    assign_streams(2, 5, -1); // provisional (the measured-best order of one configuration); tune_streams() decides
    for (int hh = 0; hh < kMaxParts; ++hh) {
        for (int i = 0; i < 2; ++i) {
            RFD_HIP(hipEventCreateWithFlags(&ev_fork[hh][i], hipEventDisableTiming));
            RFD_HIP(hipEventCreateWithFlags(&ev_join[hh][i], hipEventDisableTiming));
        }
        RFD_HIP(hipEventCreateWithFlags(&ev_part_join[hh], hipEventDisableTiming));
    }
    RFD_HIP(hipEventCreateWithFlags(&ev_part_fork, hipEventDisableTiming));
    RFD_HIP(hipMalloc((void **)&d_zero, 256));
    RFD_HIP(hipMemset(d_zero, 0, 256));
    d_buffers.assign(g.buffer_bytes_per_image.size(), nullptr);
    for (size_t i = 0; i < d_buffers.size(); ++i)
    {
        RFD_HIP(hipMalloc(&d_buffers[i], g.buffer_bytes_per_image[i] * (size_t)max_batch));
        RFD_HIP(hipMemset(d_buffers[i], 0, g.buffer_bytes_per_image[i] * (size_t)max_batch));
    }
    // hipMemset on device memory returns before the fill has run, and it runs on the NULL stream, which the non-blocking streams
    // everything else uses are not ordered with: without this the fill of d_w could land AFTER the first set_layer() copies and
    // zero layer 0's weights (round 3: one fresh context in ~16 returned no detections; tests/test_pipeline_gpu.py caught it).
    RFD_HIP(hipDeviceSynchronize());
    return RFD_OK;
}

void Network::destroy()
{
    if (d_w) (void)hipFree(d_w);
    if (d_b) (void)hipFree(d_b);
    if (d_zero) (void)hipFree(d_zero);
    d_zero = nullptr;
    if (d_w32) (void)hipFree(d_w32);
    d_w32 = nullptr;
    for (int b = 0; b < 3; ++b) {
        if (d_sk_ws[b]) (void)hipFree(d_sk_ws[b]);
        d_sk_ws[b] = nullptr; sk_ws_bytes[b] = 0;
    }
    if (d_sk_cnt) (void)hipFree(d_sk_cnt);
    d_sk_cnt = nullptr;
    if (d_stem32) (void)hipFree(d_stem32);
    d_stem32 = nullptr;
    for (void *p : d_buffers32)
        if (p) (void)hipFree(p);
    d_buffers32.clear();
    for (void *p : d_buffers)
        if (p) (void)hipFree(p);
    for (void *p : d_alt)
        if (p) (void)hipFree(p);
    d_alt.clear();
    for (int hh = 0; hh < kMaxParts; ++hh) {
        for (int i = 0; i < 2; ++i) {
            if (ev_fork[hh][i]) (void)hipEventDestroy(ev_fork[hh][i]);
            if (ev_join[hh][i]) (void)hipEventDestroy(ev_join[hh][i]);
            side[hh][i] = nullptr; ev_fork[hh][i] = ev_join[hh][i] = nullptr;
        }
        if (ev_part_join[hh]) (void)hipEventDestroy(ev_part_join[hh]);
        part_stream[hh] = nullptr; ev_part_join[hh] = nullptr;
    }
    for (int i = 0; i < kPool; ++i) {
        if (pool[i]) (void)hipStreamDestroy(pool[i]);
        pool[i] = nullptr;
    }
    if (ev_part_fork) (void)hipEventDestroy(ev_part_fork);
    ev_part_fork = nullptr;

    for (hipEvent_t e : ev) (void)hipEventDestroy(e);
    for (hipGraphExec_t ge : graph_exec)
        if (ge) (void)hipGraphExecDestroy(ge);
    graph_exec.clear();
    d_w = nullptr; d_b = nullptr; d_buffers.clear(); ev.clear();
}

static inline uint64_t splitmix64(uint64_t x)
{
    x += 0x9e3779b97f4a7c15ull;
    x = (x ^ (x >> 30)) * 0xbf58476d1ce4e5b9ull;
    x = (x ^ (x >> 27)) * 0x94d049bb133111ebull;
    return x ^ (x >> 31);
}
struct Gauss { // counter-based Box-Muller: element i of stream `key`
    uint64_t key;
    void pair(uint64_t i, float &a, float &b) const
    {
        const uint64_t r1 = splitmix64(key + 2 * i), r2 = splitmix64(key + 2 * i + 1);
        const double u1 = ((double)(r1 >> 11) + 1.0) * (1.0 / 9007199254740993.0);
        const double u2 = (double)(r2 >> 11) * (1.0 / 9007199254740992.0);
        const double rr = sqrt(-2.0 * log(u1)), th = 6.283185307179586 * u2;
        a = (float)(rr * cos(th));
        b = (float)(rr * sin(th));
    }
};

// Seeded random weights (there is no model file anywhere in the reference): He-scaled so that
// activations stay O(1) through the 50+ layers in bf16; post-add affines ~ 1/sqrt(1+u).
int Network::init_synthetic(uint64_t seed, hipStream_t s)
{
    int unit_in_stage = 0;
    for (size_t li = 0; li < g.layers.size(); ++li) {
        const Layer &L = g.layers[li];
        const size_t n = (size_t)L.cout * L.kh * L.kw * L.cin;
        std::vector<float> w(n + 1), b(L.cout), sc(L.cout), sh(L.cout);
        const float stdv = sqrtf(2.0f / (float)(L.kh * L.kw * L.cin)) * L.gain; // depthwise: cin = 1 -> fan-in 9
        Gauss gw{splitmix64(seed * 1315423911ull + li * 2654435761ull)};
        for (size_t i = 0; i < n; i += 2) {
            float a, c;
            gw.pair(i / 2, a, c);
            w[i] = a * stdv;
            w[i + 1] = c * stdv;
        }
        Gauss gb{splitmix64(seed * 7919ull + li * 104729ull + 17)};
        const bool head = L.name.compare(0, 4, "head") == 0;
        if (L.name.find("unit1_conv3") != std::string::npos) unit_in_stage = 1;
        else if (L.name.find("_conv3") != std::string::npos) ++unit_in_stage;
        for (int c = 0; c < L.cout; c += 2) {
            float a, d;
            gb.pair(c / 2, a, d);
            b[c] = 0.05f * a;
            if (c + 1 < L.cout) b[c + 1] = 0.05f * d;
            float e, f;
            gb.pair(1000000 + c / 2, e, f);
            const float base = L.name == "conv0" ? 1.0f : 1.0f / sqrtf(1.0f + (float)unit_in_stage);
            sc[c] = base * (1.0f + 0.1f * fmaxf(-2.f, fminf(2.f, e)));
            sh[c] = 0.05f * f;
            if (c + 1 < L.cout) { sc[c + 1] = base * (1.0f - 0.1f * fmaxf(-2.f, fminf(2.f, e))); sh[c + 1] = -0.05f * f; }
        }
        if (head) {
            // channels: 0,1 bg logits, 2,3 fg logits, 4..11 box deltas, 12..31 landmark deltas.
            // fg-bg logit difference ~ N(-2, ~1): a fraction of a percent of anchors pass 0.7.
            const size_t K = (size_t)L.kh * L.kw * L.cin;
            for (int c = 0; c < L.cout; ++c) {
                const float g2 = c < 4 ? 0.6f : (c < 12 ? 0.25f : 0.35f);
                for (size_t k = 0; k < K; ++k) w[c * K + k] *= g2;
                b[c] = c < 2 ? 1.0f : (c < 4 ? -1.0f : 0.0f);
            }
        }
        RFD_TRY(set_layer((int)li, w.data(), b.data(), s));
        if (L.has_affine) RFD_TRY(set_affine((int)li, sc.data(), sh.data(), s));
    }
    RFD_HIP(hipStreamSynchronize(s));
    weights_ready = true;
    return RFD_OK;
}

int Network::set_layer(int idx, const float *w, const float *bias, hipStream_t s)
{
    if (idx < 0 || idx >= (int)g.layers.size()) { set_error("layer index %d out of range", idx); return RFD_ERR_INVALID_ARG; }
    const Layer &L = g.layers[idx];
    const int taps = L.kh * L.kw;
    // logical [cout][kh][kw][cin] f32 -> device bf16, zero padded to the device shape
    size_t rows = L.cout_d, K = 0;
    std::vector<bf16_t> hw;
    if (L.kind == LK_CONV0) { // [64][7][7][3] -> [64][7][8 kx][4 c]
        K = 7 * 32; rows = L.cout;
        hw.assign(rows * K, 0);
        for (int n = 0; n < L.cout; ++n)
            for (int ky = 0; ky < 7; ++ky)
                for (int kx = 0; kx < 7; ++kx)
                    for (int c = 0; c < 3; ++c)
                        hw[((size_t)n * 7 + ky) * 32 + kx * 4 + c] = f32_to_bf16_host(w[(((size_t)n * 7 + ky) * 7 + kx) * 3 + c]);
    } else if (L.kind == LK_FIRST3X3) { // [8][3][3][3] -> [8][3][3][4]
        K = 36; rows = L.cout;
        hw.assign(rows * K, 0);
        for (int n = 0; n < L.cout; ++n)
            for (int t = 0; t < 9; ++t)
                for (int c = 0; c < 3; ++c) hw[(size_t)n * 36 + t * 4 + c] = f32_to_bf16_host(w[((size_t)n * 9 + t) * 3 + c]);
    } else if (L.kind == LK_DEPTHWISE) { // [C][3][3][1] -> [9][C_d]
        K = L.cout_d; rows = 9;
        hw.assign(rows * K, 0);
        for (int c = 0; c < L.cout; ++c)
            for (int t = 0; t < 9; ++t) hw[(size_t)t * K + c] = f32_to_bf16_host(w[(size_t)c * 9 + t]);
    } else {
        K = (size_t)taps * L.cin_d;
        hw.assign(rows * K, 0);
        for (int n = 0; n < L.cout; ++n)
            for (int t = 0; t < taps; ++t)
                for (int c = 0; c < L.cin; ++c)
                    hw[(size_t)n * K + (size_t)t * L.cin_d + c] = f32_to_bf16_host(w[((size_t)n * taps + t) * L.cin + c]);
    }
    RFD_HIP(hipMemcpy2DAsync(d_w + L.w_off, L.ldw * sizeof(bf16_t), hw.data(), K * sizeof(bf16_t), K * sizeof(bf16_t), rows,
                             hipMemcpyHostToDevice, s));
    std::vector<float> hw32;
    if (d_w32) { // f32 parity mode: the UNROUNDED values in the same device layout (conv0 and ordinary convs only: R50)
        hw32.assign(rows * K, 0.f);
        if (L.kind == LK_CONV0) {
            for (int n = 0; n < L.cout; ++n)
                for (int ky = 0; ky < 7; ++ky)
                    for (int kx = 0; kx < 7; ++kx)
                        for (int c = 0; c < 3; ++c) hw32[((size_t)n * 7 + ky) * 32 + kx * 4 + c] = w[(((size_t)n * 7 + ky) * 7 + kx) * 3 + c];
        } else if (L.kind == LK_CONV) {
            for (int n = 0; n < L.cout; ++n)
                for (int t = 0; t < taps; ++t)
                    for (int c = 0; c < L.cin; ++c) hw32[(size_t)n * K + (size_t)t * L.cin_d + c] = w[((size_t)n * taps + t) * L.cin + c];
        }
        RFD_HIP(hipMemcpy2DAsync(d_w32 + L.w_off, L.ldw * sizeof(float), hw32.data(), K * sizeof(float), K * sizeof(float), rows,
                                 hipMemcpyHostToDevice, s));
    }
    std::vector<float> hb(L.cout_d, 0.f);
    if (bias) {
        memcpy(hb.data(), bias, L.cout * sizeof(float));
        RFD_HIP(hipMemcpyAsync(d_b + L.b_off, hb.data(), L.cout_d * sizeof(float), hipMemcpyHostToDevice, s));
    }
    RFD_HIP(hipStreamSynchronize(s)); // hw / hb go out of scope
    return RFD_OK;
}

int Network::get_layer(int idx, float *w, float *bias, hipStream_t s)
{
    if (idx < 0 || idx >= (int)g.layers.size()) { set_error("layer index %d out of range", idx); return RFD_ERR_INVALID_ARG; }
    const Layer &L = g.layers[idx];
    const int taps = L.kh * L.kw;
    if (w && d_w32 && (L.kind == LK_CONV0 || L.kind == LK_CONV)) { // f32 parity mode: the values the f32 kernels use
        size_t rows = L.cout_d, K = (size_t)taps * L.cin_d;
        if (L.kind == LK_CONV0) { rows = L.cout; K = 7 * 32; }
        std::vector<float> hw(rows * K);
        RFD_HIP(hipMemcpy2DAsync(hw.data(), K * sizeof(float), d_w32 + L.w_off, L.ldw * sizeof(float), K * sizeof(float), rows, hipMemcpyDeviceToHost, s));
        RFD_HIP(hipStreamSynchronize(s));
        if (L.kind == LK_CONV0) {
            for (int n = 0; n < L.cout; ++n)
                for (int ky = 0; ky < 7; ++ky)
                    for (int kx = 0; kx < 7; ++kx)
                        for (int c = 0; c < 3; ++c) w[(((size_t)n * 7 + ky) * 7 + kx) * 3 + c] = hw[((size_t)n * 7 + ky) * 32 + kx * 4 + c];
        } else {
            for (int n = 0; n < L.cout; ++n)
                for (int t = 0; t < taps; ++t)
                    for (int c = 0; c < L.cin; ++c) w[((size_t)n * taps + t) * L.cin + c] = hw[(size_t)n * K + (size_t)t * L.cin_d + c];
        }
    } else if (w) {
        size_t rows = L.cout_d, K = (size_t)taps * L.cin_d;
        if (L.kind == LK_CONV0) { rows = L.cout; K = 7 * 32; }
        else if (L.kind == LK_FIRST3X3) { rows = L.cout; K = 36; }
        else if (L.kind == LK_DEPTHWISE) { rows = 9; K = L.cout_d; }
        std::vector<bf16_t> hw(rows * K);
        RFD_HIP(hipMemcpy2DAsync(hw.data(), K * sizeof(bf16_t), d_w + L.w_off, L.ldw * sizeof(bf16_t), K * sizeof(bf16_t), rows,
                                 hipMemcpyDeviceToHost, s));
        RFD_HIP(hipStreamSynchronize(s));
        if (L.kind == LK_CONV0) {
            for (int n = 0; n < L.cout; ++n)
                for (int ky = 0; ky < 7; ++ky)
                    for (int kx = 0; kx < 7; ++kx)
                        for (int c = 0; c < 3; ++c)
                            w[(((size_t)n * 7 + ky) * 7 + kx) * 3 + c] = bf16_to_f32_host(hw[((size_t)n * 7 + ky) * 32 + kx * 4 + c]);
        } else if (L.kind == LK_FIRST3X3) {
            for (int n = 0; n < L.cout; ++n)
                for (int t = 0; t < 9; ++t)
                    for (int c = 0; c < 3; ++c) w[((size_t)n * 9 + t) * 3 + c] = bf16_to_f32_host(hw[(size_t)n * 36 + t * 4 + c]);
        } else if (L.kind == LK_DEPTHWISE) {
            for (int c = 0; c < L.cout; ++c)
                for (int t = 0; t < 9; ++t) w[(size_t)c * 9 + t] = bf16_to_f32_host(hw[(size_t)t * K + c]);
        } else {
            for (int n = 0; n < L.cout; ++n)
                for (int t = 0; t < taps; ++t)
                    for (int c = 0; c < L.cin; ++c)
                        w[((size_t)n * taps + t) * L.cin + c] = bf16_to_f32_host(hw[(size_t)n * K + (size_t)t * L.cin_d + c]);
        }
    }
    if (bias) {
        RFD_HIP(hipMemcpyAsync(bias, d_b + L.b_off, L.cout * sizeof(float), hipMemcpyDeviceToHost, s));
        RFD_HIP(hipStreamSynchronize(s));
    }
    return RFD_OK;
}

int Network::set_affine(int idx, const float *scale, const float *shift, hipStream_t s)
{
    if (idx < 0 || idx >= (int)g.layers.size() || !g.layers[idx].has_affine) { set_error("layer %d has no affine", idx); return RFD_ERR_INVALID_ARG; }
    const Layer &L = g.layers[idx];
    RFD_HIP(hipMemcpyAsync(d_b + g.b_total + L.a_off, scale, L.cout * sizeof(float), hipMemcpyHostToDevice, s));
    RFD_HIP(hipMemcpyAsync(d_b + g.b_total + L.a_off + L.cout_d, shift, L.cout * sizeof(float), hipMemcpyHostToDevice, s));
    RFD_HIP(hipStreamSynchronize(s));
    return RFD_OK;
}

int Network::get_affine(int idx, float *scale, float *shift, hipStream_t s)
{
    if (idx < 0 || idx >= (int)g.layers.size() || !g.layers[idx].has_affine) { set_error("layer %d has no affine", idx); return RFD_ERR_INVALID_ARG; }
    const Layer &L = g.layers[idx];
    RFD_HIP(hipMemcpyAsync(scale, d_b + g.b_total + L.a_off, L.cout * sizeof(float), hipMemcpyDeviceToHost, s));
    RFD_HIP(hipMemcpyAsync(shift, d_b + g.b_total + L.a_off + L.cout_d, L.cout * sizeof(float), hipMemcpyDeviceToHost, s));
    RFD_HIP(hipStreamSynchronize(s));
    return RFD_OK;
}

// The parameters op i of a chain of B images at image batch_off launches with -- nothing is launched and no kernel chosen here
// (launch_op runs them; op_kernels asks conv_select.hip which kernels that takes).
void Network::op_launch(int i, int B, int batch_off, int part, bool offer_conv1, OpLaunch *out) const
{
    const Op &o = g.ops[i];
    const Layer &L = g.layers[o.layer];
    const TensorDesc &tin = g.tensors[o.in];
    OpLaunch &l = *out;
    memset(&l, 0, sizeof l);
    l.kind = o.kind;
    l.force_tile = force_tile;
    if (o.kind == OP_FIRST || o.kind == OP_DW || o.kind == OP_STEM) {
        l.x = (const bf16_t *)tensor_ptr(o.in, batch_off);
        l.w = d_w + L.w_off;
        l.bias = d_b + L.b_off;
        l.y = (bf16_t *)tensor_ptr(o.out, batch_off);
        l.B = B; l.H = tin.H; l.W = tin.W;
        l.C = o.kind == OP_FIRST ? g.tensors[o.out].C : tin.C;
        l.stride = L.stride;
    }
    if (o.kind == OP_STEM) {
        l.scale = d_b + g.b_total + L.a_off;
        l.shift = d_b + g.b_total + L.a_off + L.cout_d;
        // Peephole (round 4): when the next op of the range is the first unit's conv1 -- a plain 1x1 64 -> 64 conv + bias + ReLU
        // on the stem's output -- the persistent stem kernel computes it on the pooled tile (choose_stem decides whether that
        // form runs); the conv's own op is then skipped.  Bit-identical (tests/test_persistent_gpu.py).
        if (offer_conv1 && i + 1 < (int)g.ops.size()) {
            const Op &n = g.ops[i + 1];
            const Layer &Ln = g.layers[n.layer];
            const bool plain = n.kind == OP_CONV && n.in == o.out && Ln.kh == 1 && Ln.kw == 1 && Ln.stride == 1 && Ln.cin_d == 64 &&
                               Ln.cout_d == 64 && n.relu && n.in_affine < 0 && n.res < 0 && n.layer2 < 0 && n.layer_n2 < 0 && n.out2 < 0 &&
                               n.outf < 0 && n.out >= 0 && n.x_coff == 0 && n.y_coff == 0 && n.branch == o.branch &&
                               g.tensors[n.out].C == 64 && n.n_valid >= 64 && n.y_split >= 64;
            if (plain) { l.w1 = d_w + Ln.w_off; l.bias1 = d_b + Ln.b_off; l.t1 = (bf16_t *)tensor_ptr(n.out, batch_off); }
        }
    } else if (o.kind == OP_B2B && L.cin_d == 64 && g.layers[o.layer_b].cout_d == 64) {
        l.b2b_s1 = true;
        B2BParams &bp = l.b2b;
        const Layer &Lb = g.layers[o.layer_b];
        bp.x = (const bf16_t *)tensor_ptr(o.in, batch_off);
        bp.w3 = d_w + L.w_off;
        bp.bias3 = d_b + L.b_off;
        if (o.layer2 >= 0) {
            const Layer &L2 = g.layers[o.layer2];
            bp.x2 = (const bf16_t *)tensor_ptr(o.in2, batch_off);
            bp.bias3b = d_b + L2.b_off;
            bp.Cin2 = L2.cin_d;
        }
        bp.res = o.res >= 0 ? (const bf16_t *)tensor_ptr(o.res, batch_off) : nullptr;
        bp.scale = d_b + g.b_total + L.a_off;
        bp.shift = d_b + g.b_total + L.a_off + L.cout_d;
        bp.raw = (bf16_t *)tensor_ptr(o.out, batch_off);
        bp.w1 = d_w + Lb.w_off;
        bp.bias1 = d_b + Lb.b_off;
        bp.t1 = (bf16_t *)tensor_ptr(o.out_b, batch_off);
        bp.B = B; bp.H = tin.H; bp.W = tin.W; bp.Cin = L.cin_d;
        bp.force_tile = force_tile;
    } else if (o.kind == OP_CONV || o.kind == OP_B2B) {
        const int tout = o.out >= 0 ? o.out : (o.out2 >= 0 ? o.out2 : o.outf);
        ConvParams &p = l.conv;
        p.x = (const bf16_t *)tensor_ptr(o.in, batch_off);
        p.w = d_w + L.w_off;
        p.bias = d_b + L.b_off;
        p.zero = d_zero;
        p.force_tile = force_tile;
        p.co_running = co_running;
        p.fail = d_fail;
        if (latency_pass(B) && !co_running && batch_off == 0 && part == 0 && !sk_cnt_n.empty()) {
            const int br = std::min(std::max(o.branch, 0), 2);
            p.latency = 1;
            p.sk_ws = d_sk_ws[br]; p.sk_ws_bytes = sk_ws_bytes[br];
            p.sk_cnt = d_sk_cnt + sk_cnt_off[i]; p.sk_cnt_n = sk_cnt_n[i];
        }
        p.res = o.res >= 0 ? (const bf16_t *)tensor_ptr(o.res, batch_off) : nullptr;
        if (o.layer2 >= 0) {
            const Layer &L2 = g.layers[o.layer2];
            const TensorDesc &t2 = g.tensors[o.in2];
            p.x2 = (const bf16_t *)tensor_ptr(o.in2, batch_off);
            p.bias2 = d_b + L2.b_off;
            p.H2 = t2.H; p.W2 = t2.W; p.Cin2 = L2.cin_d; p.stride2 = L2.stride;
        }
        if (o.in_affine >= 0) {
            const Layer &La = g.layers[o.in_affine];
            p.in_scale = d_b + g.b_total + La.a_off;
            p.in_shift = d_b + g.b_total + La.a_off + La.cout_d;
        }
        p.scale2 = d_b + g.b_total + L.a_off;
        p.shift2 = d_b + g.b_total + L.a_off + L.cout_d;
        p.y = o.out >= 0 ? (bf16_t *)tensor_ptr(o.out, batch_off) : nullptr;
        p.y2 = o.out2 >= 0 ? (bf16_t *)tensor_ptr(o.out2, batch_off) : nullptr;
        p.yf = o.outf >= 0 ? (float *)tensor_ptr(o.outf, batch_off) : nullptr;
        p.B = B; p.H = tin.H; p.W = tin.W; p.Cin = L.cin_d;
        p.Cout = L.cout_d + (o.layer_n2 >= 0 ? g.layers[o.layer_n2].cout_d : 0); // N-fused sibling: its rows follow
        p.n_valid = o.n_valid;
        p.ldx = tin.C; p.x_coff = o.x_coff; p.y_split = o.y_split; p.y_split_add = o.y_split_add;
        p.KH = L.kh; p.KW = L.kw; p.stride = L.stride; p.pad = L.pad;
        p.Ho = g.tensors[tout].H; p.Wo = g.tensors[tout].W;
        p.ldy = o.out >= 0 ? g.tensors[o.out].C : p.Cout;
        p.y_coff = o.y_coff;
        p.relu = o.relu; p.res_up2 = o.res_up2; p.res_post = o.res_post; p.head_softmax = o.head_softmax;
        if (o.kind == OP_B2B) { // beyond stage 1: the pair runs through launch_conv (a fused pair kernel, or two launches)
            const Layer &Lb = g.layers[o.layer_b];
            p.w1 = d_w + Lb.w_off;
            p.bias1 = d_b + Lb.b_off;
            p.t1 = (bf16_t *)tensor_ptr(o.out_b, batch_off);
            p.n1 = Lb.cout_d;
        }
    }
}

int launch_op(const OpLaunch &l, hipStream_t s, bool *fused)
{
    *fused = false;
    switch (l.kind) {
    case OP_FIRST: return launch_first3x3(l.x, l.w, l.bias, l.y, l.B, l.H, l.W, l.C, s);
    case OP_DW: return launch_dwconv3x3(l.x, l.w, l.bias, l.y, l.B, l.H, l.W, l.C, l.stride, s);
    case OP_STEM: return launch_stem(l.x, l.w, l.bias, l.scale, l.shift, l.y, l.B, l.H, l.W, s, l.force_tile, l.w1, l.bias1, l.t1, l.w1 ? fused : nullptr);
    default: return l.b2b_s1 ? launch_conv_b2b_s1(l.b2b, s) : launch_conv(l.conv, s);
    }
}

// the kernels launch_op(l) runs, " + "-separated (display names, conv_kernel_name); *fused as launch_op reports it
int op_kernels(const OpLaunch &l, int cus, std::string *names, bool *fused)
{
    *fused = false;
    ConvPlan plan;
    plan.steps = 1;
    switch (l.kind) {
    case OP_FIRST: plan.step[0].kernel = K_FIRST3X3; break;
    case OP_DW: plan.step[0].kernel = K_DWCONV3X3; break;
    case OP_STEM:
        plan.step[0].kernel = choose_stem(l.B, l.H, l.W, l.w1 && l.t1, l.force_tile, cus);
        *fused = plan.step[0].kernel == K_STEM_PERSISTENT_CONV1;
        break;
    default:
        if (l.b2b_s1) choose_b2b_s1(l.b2b, bank_behind(l.b2b.w3, l.b2b.w1), &plan.step[0]);
        else RFD_TRY(choose_conv(l.conv, bank_behind(l.conv.w, l.conv.w1), &plan));
    }
    names->clear();
    for (int i = 0; i < plan.steps; ++i) {
        if (i) *names += " + ";
        *names += conv_kernel_name(plan.step[i].kernel);
    }
    return RFD_OK;
}

// rfd_debug_op_kernels' answer for op `op` of a chain of n images.  The stem and the conv behind it may run as ONE launch when a
// pass runs them back to back: the stem is asked with the conv on offer, and the conv reports "(fused into ...)" when it was taken.
int Network::op_kernel_names(int n, int op, int cus, std::string *out) const
{
    OpLaunch l;
    bool fused = false;
    if (op > 0 && g.ops[op - 1].kind == OP_STEM) {
        std::string stem;
        op_launch(op - 1, n, 0, 0, true, &l);
        RFD_TRY(op_kernels(l, cus, &stem, &fused));
        if (fused) { *out = "(fused into " + stem + ")"; return RFD_OK; }
    }
    op_launch(op, n, 0, 0, g.ops[op].kind == OP_STEM, &l);
    return op_kernels(l, cus, out, &fused);
}

int Network::run(int B, hipStream_t s, int first_op, int last_op, int batch_off, int part)
{
    if (!weights_ready) { set_error("network weights are not initialised (rfd_init_synthetic_weights / rfd_set_layer_weights)"); return RFD_ERR_STATE; }
    if (B < 1 || batch_off + B > max_batch) { set_error("batch %d exceeds max_batch_size %d", batch_off + B, max_batch); return RFD_ERR_CAPACITY; }
    if (precision != 0) return run_f32(B, s, first_op, last_op, batch_off);
    const int nops = (int)g.ops.size();
    if (profiling && (int)ev.size() < 2 * nops) {
        const size_t old = ev.size();
        ev.resize(2 * nops);
        for (size_t i = old; i < ev.size(); ++i) RFD_HIP(hipEventCreate(&ev[i]));
    }
    if (last_op < 0 || last_op >= nops) last_op = nops - 1;
    if (part == 0) { prof_first = std::max(first_op, 0); prof_last = last_op; }
    hipStream_t main_stream = s;
    const bool fork_ok = multi_stream && !profiling && first_op <= 0 && last_op == nops - 1 && side[part][0] && side[part][1];
    bool forked[2] = {false, false};
    // timing-only experiment (results are garbage): RFD_SKIP_OPS="42,45" leaves those ops out of the pass -- the step time without
    // them bounds what ANY faster kernel for them could buy end to end in the overlapped two-chain pass (tools/ab_bench.sh).
    // Compiled only into diagnostic builds (tools/build_variant.sh ... -DRFD_DIAG): a shipped library never drops an op, whatever
    // the environment says (the reference returns Err on every failure and never silently wrong detections).
#ifdef RFD_DIAG
    static const std::vector<int> skip_ops = [] {
        std::vector<int> v;
        if (const char *e = getenv("RFD_SKIP_OPS"))
            for (const char *q = e; *q;) { v.push_back(atoi(q)); while (*q && *q != ',') ++q; if (*q == ',') ++q; }
        return v;
    }();
#else
    static const std::vector<int> skip_ops;
#endif
    for (int i = std::max(first_op, 0); i <= last_op; ++i) {
        const Op &o = g.ops[i];
        s = main_stream;
        if (!skip_ops.empty() && std::find(skip_ops.begin(), skip_ops.end(), i) != skip_ops.end()) {
            if (profiling) { RFD_HIP(hipEventRecord(ev[2 * i], s)); RFD_HIP(hipEventRecord(ev[2 * i + 1], s)); }
            continue;
        }
        if (fork_ok && o.branch > 0) {
            const int bidx = o.branch - 1;
            if (!forked[bidx]) { // everything this chain reads was enqueued on the main stream before this point
                RFD_HIP(hipEventRecord(ev_fork[part][bidx], main_stream));
                RFD_HIP(hipStreamWaitEvent(side[part][bidx], ev_fork[part][bidx], 0));
                forked[bidx] = true;
            }
            s = side[part][bidx];
        }
        if (profiling) RFD_HIP(hipEventRecord(ev[2 * i], s));
        // the stem is offered the conv behind it when that conv is the next op of the range (op_launch)
        OpLaunch L;
        op_launch(i, B, batch_off, part, !profiling && i + 1 <= last_op && skip_ops.empty(), &L);
        bool fused = false;
        RFD_TRY(launch_op(L, s, &fused));
        if (profiling) RFD_HIP(hipEventRecord(ev[2 * i + 1], s));
        if (fused) ++i; // the conv ran inside the stem kernel
    }
    for (int bidx = 0; bidx < 2; ++bidx)
        if (forked[bidx]) { // join
            RFD_HIP(hipEventRecord(ev_join[part][bidx], side[part][bidx]));
            RFD_HIP(hipStreamWaitEvent(main_stream, ev_join[part][bidx], 0));
        }
    return RFD_OK;
}

// The op list in f32 (kernels_f32.hip): the same parameters run() builds, f32 pointers, one stream.  The fused stem runs as
// conv0 -> max pool (+ affine + ReLU) through the stem's own output buffer region is NOT possible (different sizes), so the
// conv0 activation goes to a scratch allocation made on first use; the stage-1 back-to-back op runs as its two convolutions.
int Network::run_f32(int B, hipStream_t s, int first_op, int last_op, int batch_off)
{
    const int nops = (int)g.ops.size();
    if (last_op < 0 || last_op >= nops) last_op = nops - 1;
    const float *aff = d_b + g.b_total;
    for (int i = std::max(first_op, 0); i <= last_op; ++i) {
        const Op &o = g.ops[i];
        const Layer &L = g.layers[o.layer];
        const TensorDesc &tin = g.tensors[o.in];
        if (o.kind == OP_STEM) {
            const size_t need = (size_t)max_batch * (tin.H / 2) * (tin.W / 2) * 64 * sizeof(float);
            if (!d_stem32) RFD_HIP(hipMalloc(&d_stem32, need));
            float *c0 = (float *)d_stem32 + (size_t)batch_off * (tin.H / 2) * (tin.W / 2) * 64;
            RFD_TRY(launch_conv0_f32((const bf16_t *)tensor_ptr(o.in, batch_off), d_w32 + L.w_off, d_b + L.b_off, c0, B, tin.H, tin.W, s));
            RFD_TRY(launch_maxpool_f32(c0, (float *)tensor_ptr32(o.out, batch_off), aff + L.a_off, aff + L.a_off + L.cout_d, B, tin.H / 2,
                                       tin.W / 2, 64, s));
            continue;
        }
        if (o.kind != OP_CONV && o.kind != OP_B2B) { set_error("f32 parity mode: op kind %d has no f32 kernel", o.kind); return RFD_ERR_INVALID_ARG; }
        const int tout = o.out >= 0 ? o.out : (o.out2 >= 0 ? o.out2 : o.outf);
        ConvF32Params p;
        memset(&p, 0, sizeof p);
        p.x = (const float *)tensor_ptr32(o.in, batch_off);
        p.w = d_w32 + L.w_off;
        p.ldw = (int)L.ldw;
        p.bias = d_b + L.b_off;
        p.res = o.res >= 0 ? (const float *)tensor_ptr32(o.res, batch_off) : nullptr;
        if (o.layer2 >= 0) {
            const Layer &L2 = g.layers[o.layer2];
            const TensorDesc &t2 = g.tensors[o.in2];
            p.x2 = (const float *)tensor_ptr32(o.in2, batch_off);
            p.bias2 = d_b + L2.b_off;
            p.H2 = t2.H; p.W2 = t2.W; p.Cin2 = L2.cin_d; p.stride2 = L2.stride;
        }
        if (o.in_affine >= 0) {
            const Layer &La = g.layers[o.in_affine];
            p.in_scale = aff + La.a_off;
            p.in_shift = aff + La.a_off + La.cout_d;
        }
        p.scale2 = aff + L.a_off;
        p.shift2 = aff + L.a_off + L.cout_d;
        p.y = o.out >= 0 ? (float *)tensor_ptr32(o.out, batch_off) : nullptr;
        p.y2 = o.out2 >= 0 ? (float *)tensor_ptr32(o.out2, batch_off) : nullptr;
        p.yf = o.outf >= 0 ? (float *)tensor_ptr32(o.outf, batch_off) : nullptr;
        p.B = B; p.H = tin.H; p.W = tin.W; p.Cin = L.cin_d;
        p.Cout = L.cout_d + (o.layer_n2 >= 0 ? g.layers[o.layer_n2].cout_d : 0);
        p.n_valid = o.n_valid;
        p.ldx = tin.C; p.x_coff = o.x_coff; p.y_split = o.y_split; p.y_split_add = o.y_split_add;
        p.KH = L.kh; p.KW = L.kw; p.stride = L.stride; p.pad = L.pad;
        p.Ho = g.tensors[tout].H; p.Wo = g.tensors[tout].W;
        p.ldy = o.out >= 0 ? g.tensors[o.out].C : p.Cout;
        p.y_coff = o.y_coff;
        p.relu = o.relu; p.res_up2 = o.res_up2; p.res_post = o.res_post; p.head_softmax = o.head_softmax;
        if (o.kind == OP_B2B) { // raw = conv3(x) [+ shortcut(x2)] + bias (+ res); t1 = relu(conv1(relu(raw * scale + shift)) + bias1)
            const bool act_out = o.out < 0; // last unit of a stage: only the activated output exists and conv1 reads it as it is
            p.relu = 0; p.yf = nullptr;
            if (!act_out) p.y2 = nullptr;
            p.n_valid = p.Cout; p.y_split = 1 << 30; p.y_split_add = 0; p.y_coff = 0; p.ldy = p.Cout;
            RFD_TRY(launch_conv_f32(p, s));
            const Layer &Lb = g.layers[o.layer_b];
            ConvF32Params q;
            memset(&q, 0, sizeof q);
            q.x = (const float *)tensor_ptr32(act_out ? o.out2 : o.out, batch_off);
            q.w = d_w32 + Lb.w_off; q.ldw = (int)Lb.ldw; q.bias = d_b + Lb.b_off;
            if (!act_out) { q.in_scale = aff + L.a_off; q.in_shift = aff + L.a_off + L.cout_d; }
            q.y = (float *)tensor_ptr32(o.out_b, batch_off);
            q.B = B; q.H = q.Ho = tin.H; q.W = q.Wo = tin.W; q.Cin = Lb.cin_d; q.Cout = Lb.cout_d;
            q.KH = q.KW = 1; q.stride = 1; q.pad = 0;
            q.ldx = g.tensors[act_out ? o.out2 : o.out].C; q.ldy = g.tensors[o.out_b].C; q.n_valid = q.Cout; q.y_split = 1 << 30; q.relu = 1;
            RFD_TRY(launch_conv_f32(q, s));
            continue;
        }
        RFD_TRY(launch_conv_f32(p, s));
    }
    return RFD_OK;
}

int Network::ensure_alt_heads()
{
    if (!d_alt.empty()) return RFD_OK;
    d_alt.assign(d_buffers.size(), nullptr);
    for (int l = 0; l < 3; ++l) {
        const int bi = g.tensors[g.heads[l]].buffer;
        RFD_HIP(hipMalloc(&d_alt[bi], g.buffer_bytes_per_image[bi] * (size_t)max_batch));
        RFD_HIP(hipMemset(d_alt[bi], 0, g.buffer_bytes_per_image[bi] * (size_t)max_batch));
    }
    RFD_HIP(hipDeviceSynchronize()); // the fills run on the NULL stream (see Network::create)
    return RFD_OK;
}

// chain streams a, b (, c) for parts 0 / 1 (/ 2); the side streams (and further parts) take the rest of the pool in order
void Network::assign_streams(int a, int b, int c)
{
    part_stream[0] = pool[a];
    part_stream[1] = pool[b];
    if (c >= 0) part_stream[2] = pool[c];
    int k = 0;
    auto next = [&]() {
        while (k == a || k == b || k == c) ++k;
        return pool[k++ % kPool];
    };
    const int nchain = c >= 0 ? 3 : 2;
    for (int hh = 0; hh < nchain; ++hh)
        for (int i = 0; i < 2; ++i) side[hh][i] = next();
    for (int hh = nchain; hh < kMaxParts; ++hh) {
        part_stream[hh] = next();
        for (int i = 0; i < 2; ++i) side[hh][i] = next();
    }
}

// Round 3 tried a HYBRID split on the verdict's suggestion -- two 16-image chains up to stage 4, then stage 4 + the stride-32 /
// stride-16 pyramid levels ONCE over the whole batch (their launches cost a 32-image batch about what they cost 16 images),
// optionally re-split for the stride-8 tail, or pipelined on a third stream under the next call's chains with the workspace
// doubled.  All three forms measured SLOWER than two independent chains (7 445 / 7 278, 7 422 / 7 395, 7 249 / 7 275 against
// 7 643 / 7 499 / 7 301 / 7 405 img/s on the same boxes: profiles/r03_ab_safe_waits_hybrid.jsonl, r03_ab_pipelined_hybrid.jsonl):
// stage 4's kernels occupy 100-200 CUs and the other chain already fills the rest, so joining only removes overlap.  The
// joined range also picks kernels by its own batch size, which for two layers means another f32 summation order, i.e. heads
// that differ in the last bf16 bit from the split pass (tests/test_concurrency_gpu.py fails with it).  Removed.

int Network::split_body(int B, hipStream_t s)
{
    int sizes[kMaxParts];
    const int P = pass_chains(B, sizes);
    RFD_HIP(hipEventRecord(ev_part_fork, s));
    co_running = 1;
    int off = 0, st = RFD_OK;
    for (int p = 0; p < P && st == RFD_OK; ++p) {
        const int Bp = sizes[p];
        RFD_HIP(hipStreamWaitEvent(part_stream[p], ev_part_fork, 0));
        st = run(Bp, part_stream[p], 0, -1, off, p);
        if (st == RFD_OK) RFD_HIP(hipEventRecord(ev_part_join[p], part_stream[p]));
        off += Bp;
    }
    co_running = 0;
    RFD_TRY(st);
    for (int p = 0; p < P; ++p) RFD_HIP(hipStreamWaitEvent(s, ev_part_join[p], 0));
    return RFD_OK;
}

// The streams of a process share a few hardware queues, handed out in creation order across ALL its streams (torch's
// and RCCL's included), and two chains that land on the same queue run one after the other: with fixed streams the
// same build measured anywhere between 4.9 k and 6.2 k img/s at B = 32 depending on what else had created streams
// before.  So the first split pass times the real pass (idempotent: it only rewrites the workspace) with each pair
// of pool streams as the two chain streams and keeps the fastest -- 28 pairs x 3 passes, about half a second, once.
int Network::tune_streams(int B, int P, hipStream_t s)
{
    hipEvent_t e0 = nullptr, e1 = nullptr;
    RFD_HIP(hipEventCreate(&e0));
    RFD_HIP(hipEventCreate(&e1));
    int st = RFD_OK;
    auto time_set = [&](int a, int b, int c, int reps, float *out) { // median of `reps` synchronous passes after one warm pass
        assign_streams(a, b, c);
        std::vector<float> ts;
        for (int rep = 0; rep <= reps && st == RFD_OK; ++rep) {
            if (hipEventRecord(e0, s) != hipSuccess) st = RFD_ERR_HIP;
            if (st == RFD_OK) st = split_body(B, s);
            if (st == RFD_OK && (hipEventRecord(e1, s) != hipSuccess || hipEventSynchronize(e1) != hipSuccess)) st = RFD_ERR_HIP;
            float ms = 0.f;
            if (st == RFD_OK && hipEventElapsedTime(&ms, e0, e1) == hipSuccess && rep > 0) ts.push_back(ms);
        }
        std::sort(ts.begin(), ts.end());
        *out = ts.empty() ? 1e30f : ts[ts.size() / 2];
    };
    // coarse scan of all pairs (triples for three parts), 2 passes each, then the four best again with 9 passes each
    struct Cand { float t; int a, b, c; };
    std::vector<Cand> cand;
    for (int a = 0; a < kPool && st == RFD_OK; ++a)
        for (int b = a + 1; b < kPool && st == RFD_OK; ++b) {
            if (P == 2) {
                float t;
                time_set(a, b, -1, 2, &t);
                cand.push_back({t, a, b, -1});
            } else {
                for (int c = b + 1; c < kPool && st == RFD_OK; ++c) {
                    float t;
                    time_set(a, b, c, 2, &t);
                    cand.push_back({t, a, b, c});
                }
            }
        }
    std::sort(cand.begin(), cand.end(), [](const Cand &x, const Cand &y) { return x.t < y.t; });
    float best = 1e30f;
    int ba = 2, bb = 5, bc = P == 3 ? 6 : -1;
    for (size_t i = 0; i < cand.size() && i < 4 && st == RFD_OK; ++i) {
        float t;
        time_set(cand[i].a, cand[i].b, cand[i].c, 9, &t);
        if (t < best) { best = t; ba = cand[i].a; bb = cand[i].b; bc = cand[i].c; }
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    RFD_TRY(st);
    assign_streams(ba, bb, bc);
    tuned_ms = best;
    tuned_a = ba; tuned_b = bb;
    if (getenv("RFD_STREAM_TUNE_VERBOSE")) fprintf(stderr, "[rfd] chain streams: pool[%d], pool[%d], pool[%d] (%.3f ms per split pass at B = %d)\n", ba, bb, bc, best, B);
    return RFD_OK;
}

// Split passes are never captured into a hipGraph (run_graphed): replayed from a graph they measured slower than the
// unsplit graph, and the nested fork/join topology (caller stream -> part stream -> side streams) makes
// hipStreamEndCapture of this ROCm (7.0 runtime) recurse without end.
int Network::run_split(int B, hipStream_t s)
{
    const int P = num_parts(B);
    co_running = 0;
    if (P <= 1) return run(B, s);
    if (!tuned && tune && (P == 2 || P == 3)) {
        tuned = true;
        if (getenv("RFD_STREAM_TUNE") && atoi(getenv("RFD_STREAM_TUNE")) == 0) return split_body(B, s);
        RFD_TRY(tune_streams(B, P, s));
    }
    return split_body(B, s);
}

int Network::run_graphed(int B, hipStream_t s)
{
    if (!use_graph || profiling || B < 1 || B > max_batch || num_parts(B) > 1) return run_split(B, s);
    if ((int)graph_exec.size() <= max_batch) { graph_exec.assign(max_batch + 1, nullptr); warmed.assign(max_batch + 1, 0); }
    if (graph_exec[B]) {
        RFD_HIP(hipGraphLaunch(graph_exec[B], s));
        return RFD_OK;
    }
    if (!warmed[B]) { // first call for this batch size runs eagerly (hipFuncSetAttribute etc. are not capturable)
        warmed[B] = 1;
        return run_split(B, s);
    }
    hipGraph_t graph = nullptr;
    // hipGraphLaunch of a graph with three parallel branches (main + two side chains) crashes inside this ROCm's
    // hip::Graph::UpdateStreams when the process was started with GPU_MAX_HW_QUEUES < 3: capture a linear graph there
    static const bool linear_graph = getenv("GPU_MAX_HW_QUEUES") && atoi(getenv("GPU_MAX_HW_QUEUES")) < 3;
    const bool ms_saved = multi_stream;
    if (linear_graph) multi_stream = false;
    RFD_HIP(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
    const int st = run_split(B, s);
    const hipError_t e = hipStreamEndCapture(s, &graph);
    multi_stream = ms_saved;
    if (st != RFD_OK || e != hipSuccess || !graph) {
        if (graph) (void)hipGraphDestroy(graph);
        use_graph = false; // capture unsupported here: stay eager
        return st != RFD_OK ? st : run_split(B, s);
    }
    hipGraphExec_t exec = nullptr;
    const hipError_t ei = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    if (ei != hipSuccess || !exec) {
        use_graph = false;
        return run_split(B, s);
    }
    graph_exec[B] = exec;
    RFD_HIP(hipGraphLaunch(exec, s));
    return RFD_OK;
}

int Network::collect_profile()
{
    const int nops = (int)g.ops.size();
    op_ms.assign(nops, 0.f);
    if (!profiling || (int)ev.size() < 2 * nops) return RFD_OK;
    for (int i = prof_first; i <= prof_last && i < nops; ++i) RFD_HIP(hipEventElapsedTime(&op_ms[i], ev[2 * i], ev[2 * i + 1]));
    return RFD_OK;
}

} // namespace rfd
