// face_plan.h -- the host decisions of the face stage (include/rfd.h: selection, alignment, model inputs, the packed face list,
// the quality and normalisation rules, liveness): cv::resize's scale bookkeeping, the config defaults, the argument checks, the
// bound of a face list, which configs the warp writes itself, the tile table of the liveness crops, and where each part of
// the stage's staging buffers lies.  Plain host code: nothing of HIP is included, so tests/cpp/face_plan_check.cpp builds it
// with the host compiler alone.  face_host.hip does what is decided here.
//
// A check returns RFD_OK, or the status of the refusal with the call's error message in msg; the entry hands that to set_error.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <cmath>

#include "../../include/rfd.h"

namespace rfd {

constexpr int kFaceMaxSide = 4096; // of an aligned crop and of every model input

// ---- cv::resize's scale bookkeeping: 1 / (dst / src) in f64, as cv::resize computes it, and OpenCV's INTER_LINEAR ->
//      INTER_AREA switch, taken when both factors are exactly 2 (the 2x2 mean).  All four sizes >= 1. ----
struct ResizeScale {
    double scale_x, scale_y;
    int area_fast;
};

inline ResizeScale resize_scale(int src_w, int src_h, int dst_w, int dst_h)
{
    ResizeScale r;
    const double inv_x = (double)dst_w / src_w, inv_y = (double)dst_h / src_h;
    r.scale_x = 1.0 / inv_x;
    r.scale_y = 1.0 / inv_y;
    const int ix = (int)lrint(r.scale_x), iy = (int)lrint(r.scale_y);
    r.area_fast = fabs(r.scale_x - ix) < 2.220446049250313e-16 && fabs(r.scale_y - iy) < 2.220446049250313e-16 && ix == 2 && iy == 2;
    return r;
}

// ---- config defaults ----
inline void selection_config_default(rfd_selection_config *cfg)
{
    cfg->margin_center_left_ratio = 0.3f;  // config.rs:110
    cfg->margin_center_right_ratio = 0.3f; // config.rs:111
    cfg->margin_edge_ratio = 0.1f;         // config.rs:112
    cfg->minimum_face_ratio = 0.0075f;     // config.rs:113
}

inline void alignment_config_default(rfd_alignment_config *cfg)
{
    memset(cfg, 0, sizeof *cfg);
    cfg->out_w = 112; cfg->out_h = 112; // config.rs:46
    static const float tmpl[10] = {38.2946f, 51.6963f, 73.5318f, 51.5014f, 56.0252f, 71.7366f, 41.5493f, 92.3655f, 70.7299f, 92.2041f}; // :47-52
    memcpy(cfg->standard_landmarks, tmpl, sizeof tmpl);
}

inline void face_tensor_config_quality(rfd_face_tensor_config *cfg)
{
    memset(cfg, 0, sizeof *cfg);
    cfg->out_w = 112; cfg->out_h = 112;
    static const float mean[3] = {123.675f, 116.28f, 103.53f};          // face_quality.rs:43
    static const float scale[3] = {0.01712475f, 0.017507f, 0.01742919f}; // :44 (named `std`, applied as a factor :93)
    memcpy(cfg->mean, mean, sizeof mean);
    memcpy(cfg->scale, scale, sizeof scale);
}

inline void face_tensor_config_extraction(rfd_face_tensor_config *cfg)
{
    memset(cfg, 0, sizeof *cfg);
    cfg->out_w = 112; cfg->out_h = 112;
    for (int i = 0; i < 3; ++i) { cfg->mean[i] = 127.5f; cfg->scale[i] = 0.0078125f; } // face_extraction.rs:38-39
}

inline void face_tensor_config_quality_assessment(rfd_face_tensor_config *cfg, int w, int h)
{
    memset(cfg, 0, sizeof *cfg);
    cfg->out_w = w; cfg->out_h = h;
    for (int i = 0; i < 3; ++i) { cfg->mean[i] = 127.5f; cfg->scale[i] = 0.00784313725f; } // face_quality_assessment.rs:76
}

inline void face_list_config_default(rfd_face_list_config *cfg)
{
    memset(cfg, 0, sizeof *cfg);
    cfg->max_faces = RFD_GALLERY_MAX_K; // one gallery search pass (32 queries) per frame
    cfg->min_face_px = 0.0f;
    cfg->min_score = 0.0f;
}

inline void liveness_config_default(rfd_liveness_config *cfg)
{
    memset(cfg, 0, sizeof *cfg);
    // face_antispoofing.rs:448-485, the only place that names the models: miniFAS_4, miniFAS_2_7, miniFAS_2, miniFAS_1
    static const float scale[4] = {4.0f, 2.7f, 2.0f, 1.0f};
    static const int32_t size[4] = {80, 80, 256, 128};
    cfg->k = 4;
    for (int j = 0; j < 4; ++j) { cfg->scale[j] = scale[j]; cfg->out_w[j] = cfg->out_h[j] = size[j]; }
}

// ---- checks ----
inline bool face_side_ok(int v) { return v >= 1 && v <= kFaceMaxSide; }

inline int check_align_cfg(const rfd_alignment_config &c, char *msg, size_t cap)
{
    if (face_side_ok(c.out_w) && face_side_ok(c.out_h)) return RFD_OK;
    snprintf(msg, cap, "alignment output size %dx%d out of range", c.out_w, c.out_h);
    return RFD_ERR_INVALID_ARG;
}

// k tensor configs, of which an entry needs k_min at least
inline int check_face_tensor_count(int k, int k_min, char *msg, size_t cap)
{
    if (k > RFD_MAX_FACE_TENSORS) {
        snprintf(msg, cap, "%d tensor configs exceed RFD_MAX_FACE_TENSORS (%d)", k, RFD_MAX_FACE_TENSORS);
        return RFD_ERR_CAPACITY;
    }
    if (k >= k_min) return RFD_OK;
    snprintf(msg, cap, "invalid argument: too few tensor configs (k >= k_min)");
    return RFD_ERR_INVALID_ARG;
}

inline int check_face_tensor_size(const rfd_face_tensor_config &c, int j, char *msg, size_t cap)
{
    if (face_side_ok(c.out_w) && face_side_ok(c.out_h)) return RFD_OK;
    snprintf(msg, cap, "tensor config %d: size %dx%d out of range", j, c.out_w, c.out_h);
    return RFD_ERR_INVALID_ARG;
}

inline int check_crop_size(int crop_w, int crop_h, char *msg, size_t cap)
{
    if (face_side_ok(crop_w) && face_side_ok(crop_h)) return RFD_OK;
    snprintf(msg, cap, "invalid argument: crop size out of range (crop_w >= 1 && crop_h >= 1 && crop_w <= 4096 && crop_h <= 4096)");
    return RFD_ERR_INVALID_ARG;
}

// every refusal names its field
inline int check_list_cfg(const rfd_face_list_config &c, int list_cap, char *msg, size_t cap)
{
    if (c.max_faces < 1) snprintf(msg, cap, "invalid argument: max_faces %d < 1", c.max_faces);
    else if (!std::isfinite(c.min_face_px) || c.min_face_px < 0.0f) snprintf(msg, cap, "invalid argument: min_face_px %g is negative or not finite", (double)c.min_face_px);
    else if (!std::isfinite(c.min_score)) snprintf(msg, cap, "invalid argument: min_score %g is not finite", (double)c.min_score);
    else if (list_cap < 1) snprintf(msg, cap, "invalid argument: cap %d < 1", list_cap);
    else return RFD_OK;
    return RFD_ERR_INVALID_ARG;
}

inline int check_liveness_cfg(const rfd_liveness_config &c, char *msg, size_t cap)
{
    if (c.k > RFD_MAX_FACE_TENSORS) {
        snprintf(msg, cap, "liveness config: k = %d exceeds RFD_MAX_FACE_TENSORS (%d)", c.k, RFD_MAX_FACE_TENSORS);
        return RFD_ERR_CAPACITY;
    }
    if (c.k < 1) { snprintf(msg, cap, "invalid argument: liveness config: k = %d, at least one model is needed", c.k); return RFD_ERR_INVALID_ARG; }
    for (int j = 0; j < c.k; ++j) {
        if (!face_side_ok(c.out_w[j])) snprintf(msg, cap, "invalid argument: liveness config: out_w[%d] = %d out of range", j, c.out_w[j]);
        else if (!face_side_ok(c.out_h[j])) snprintf(msg, cap, "invalid argument: liveness config: out_h[%d] = %d out of range", j, c.out_h[j]);
        else if (!(c.scale[j] > 0.0f && c.scale[j] <= 3.402823466e38f)) snprintf(msg, cap, "invalid argument: liveness config: scale[%d] = %g is not finite and positive", j, (double)c.scale[j]);
        else continue;
        return RFD_ERR_INVALID_ARG;
    }
    return RFD_OK;
}

// the counts of the quality rule, the normalisation and the liveness rule
inline int check_quality_counts(int n, int classes, char *msg, size_t cap)
{
    if (n >= 1 && classes >= 1) return RFD_OK;
    snprintf(msg, cap, "invalid argument: n < 1 or classes < 1 (n >= 1 && classes >= 1)");
    return RFD_ERR_INVALID_ARG;
}

inline int check_normalize_counts(int n, int dim, char *msg, size_t cap)
{
    if (n >= 1 && dim >= 1) return RFD_OK;
    snprintf(msg, cap, "invalid argument: n < 1 or dim < 1 (n >= 1 && dim >= 1)");
    return RFD_ERR_INVALID_ARG;
}

inline int check_liveness_decide_counts(int k, int n, int classes, char *msg, size_t cap)
{
    if (k >= 1 && n >= 1 && classes >= 2) return RFD_OK;
    snprintf(msg, cap, "invalid argument: k < 1, n < 1 or classes < 2 (k >= 1 && n >= 1 && classes >= 2)");
    return RFD_ERR_INVALID_ARG;
}

// ---- the faces a list call can list at most: what its set-up and warp launches are sized by (the true count stays in HBM) ----
inline int face_list_bound(int n, int max_faces, int max_det, int cap)
{
    const long long all = (long long)n * (max_faces < max_det ? max_faces : max_det);
    return (int)(all < cap ? all : cap);
}

// ---- configs of the crop's own size are written by the warp itself, from the registers that hold the pixel (fused); the others
//      are resized from the crop in HBM (rest).  Both groups in the order of j. ----
struct FaceSplit {
    int fused[RFD_MAX_FACE_TENSORS], rest[RFD_MAX_FACE_TENSORS];
    int n_fused, n_rest;
};

inline FaceSplit face_split(int align_w, int align_h, const rfd_face_tensor_config *cfgs, int k)
{
    FaceSplit s = {};
    for (int j = 0; j < k; ++j) {
        if (cfgs[j].out_w == align_w && cfgs[j].out_h == align_h) s.fused[s.n_fused++] = j;
        else s.rest[s.n_rest++] = j;
    }
    return s;
}

// ---- the flat table of 256-pixel tiles of one face's liveness crops: model j owns [tile0[j], tile0[j + 1]) ----
struct LiveTiles {
    int tile0[RFD_MAX_FACE_TENSORS];
    int total;
};

inline LiveTiles live_tiles(const rfd_liveness_config &c)
{
    LiveTiles t = {};
    for (int j = 0; j < c.k; ++j) {
        t.tile0[j] = t.total;
        t.total += (c.out_w[j] * c.out_h[j] + 255) / 256;
    }
    return t;
}

// ---- where each part of a staging buffer lies, in 4-byte words from its start, and the words of the whole ----
// the selection of n frames: box [n][5] | kps [n][10] | found [n]
struct SelLayout { size_t box, kps, found, words; };
inline SelLayout sel_layout(int n)
{
    const size_t N = (size_t)n;
    return SelLayout{0, 5 * N, 15 * N, 16 * N};
}

// the list of a host-output call over n frames: total [1] | first [n + 1] | frame, row, status [bound] each | box [bound][5] |
// kps [bound][10]
struct ListLayout { size_t total, first, frame, row, status, box, kps, words; };
inline ListLayout list_layout(int n, int bound)
{
    const size_t N = (size_t)n, B = (size_t)bound;
    return ListLayout{0, 1, N + 2, N + 2 + B, N + 2 + 2 * B, N + 2 + 3 * B, N + 2 + 8 * B, N + 2 + 18 * B};
}

// the host form of the liveness tensors: box [n][5] | found [n] | weights [n][k] | rois [n][k][4] | status [n]
struct LiveTensorLayout { size_t box, found, weights, rois, status, words; };
inline LiveTensorLayout live_tensor_layout(int n, int k)
{
    const size_t N = (size_t)n, K = (size_t)k;
    return LiveTensorLayout{0, 5 * N, 6 * N, 6 * N + N * K, 6 * N + 5 * N * K, 7 * N + 5 * N * K};
}

// the host form of the liveness rule: logits [k][n][classes] | weights [n][k] | score [n] | live [n]
struct LiveDecideLayout { size_t logits, weights, score, live, words; };
inline LiveDecideLayout live_decide_layout(int n, int k, int classes)
{
    const size_t N = (size_t)n, K = (size_t)k, one = N * (size_t)classes;
    return LiveDecideLayout{0, K * one, K * one + N * K, K * one + N * K + N, K * one + N * K + 2 * N};
}

} // namespace rfd
