// rfd.hpp -- C++17 host facade over the C ABI of librfd_hip.so (include/rfd.h), header-only.
//
// The reference's host code is a compiled Rust crate; no Rust toolchain exists in the build image, so this is the
// compiled-language mirror of the types a maintainer's Rust facade would expose (INTEGRATION.md shows that Rust side).
// Names, argument meaning and error behaviour follow the reference:
//   rfd::FaceDetectionConfig          <- FaceDetectionConfig::new            src/pipeline/face_pipeline/config.rs:13-33
//   rfd::RetinaFaceDetection          <- struct RetinaFaceDetection + ::new  src/pipeline/module/face_detection.rs:19-129
//   RetinaFaceDetection::call         <- ::call(&self, image:&Mat, is_debug) face_detection.rs:496-513
//                                        -> (Array2<f32> [K,5], Option<Array3<f32>> [K,5,2])
//   rfd::FaceSelection::call          <- FaceSelection::call                 src/pipeline/module/face_selection.rs:72-189
//   rfd::FaceAlignment::call          <- FaceAlignment::call                 src/pipeline/module/face_alignment.rs:27-141
//   rfd::decode_jpeg / _device        <- byte_data_to_opencv (imdecode)      src/utils/utils.rs:8-52
//   rfd::encode_jpeg / _device        (no counterpart: the reference hands raw frames on)
//   rfd::Error                        <- anyhow::Error: every failing entry point throws it (status + message)
// What changed against the reference constructor: the Triton client / model config / model name arguments are gone
// (the network runs in-process); device_id, max_det and the backbone are new.
#ifndef RFD_HPP
#define RFD_HPP

#include <algorithm>
#include <array>
#include <cstdint>
#include <limits>
#include <optional>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "rfd.h"

namespace rfd {

struct Error : std::runtime_error {
    int status;
    std::string message; // the library's text alone
    Error(int st, const std::string &what) : std::runtime_error("rfd status " + std::to_string(st) + ": " + what), status(st), message(what) {}
};
inline void check(int status)
{
    if (status < 0) throw Error(status, rfd_last_error() ? rfd_last_error() : "");
}

// config.rs:13-33
struct FaceDetectionConfig {
    std::string model_name = "face_detection_retina"; // kept for source compatibility; unused (no Triton)
    std::pair<int, int> image_size{640, 640};          // (w, h)
    int max_batch_size = 1;
    float confidence_threshold = 0.7f;
    float iou_threshold = 0.45f;
    int timeout = 20;                                  // unused (no RPC)
};

// the decoded frame the reference passes around as opencv::core::Mat (CV_8UC3, BGR; utils.rs:8-52)
struct Mat {
    const uint8_t *data = nullptr;
    int rows = 0, cols = 0;
    std::ptrdiff_t step = 0; // bytes per row
    int channels = 3;
    Mat() = default;
    Mat(const uint8_t *d, int r, int c, std::ptrdiff_t s = 0, int ch = 3) : data(d), rows(r), cols(c), step(s ? s : (std::ptrdiff_t)c * ch), channels(ch) {}
};

// (Array2<f32> [K,5], Array3<f32> [K,5,2]) of face_detection.rs:496, row-major
struct Detections {
    std::size_t k = 0;
    std::vector<float> det; // k x 5: x1, y1, x2, y2, score in source-image pixels, descending score
    std::vector<float> kps; // k x 5 x 2
    const float *box(std::size_t i) const { return det.data() + 5 * i; }
    const float *landmarks(std::size_t i) const { return kps.data() + 10 * i; }
};

class RetinaFaceDetection {
  public:
    // RetinaFaceDetection::new(client, model_cfg, model_name, image_size, max_batch_size, conf, iou) minus the Triton
    // arguments (face_detection.rs:41-49)
    RetinaFaceDetection(std::pair<int, int> image_size, int max_batch_size, float confidence_threshold, float iou_threshold,
                        int device_id = 0, int max_det = 1024, int backbone = RFD_BACKBONE_R50, int precision = RFD_PRECISION_BF16,
                        int schedule = RFD_SCHEDULE_THROUGHPUT)
    {
        rfd_config cfg;
        rfd_config_default(&cfg);
        cfg.image_w = image_size.first; cfg.image_h = image_size.second;
        cfg.max_batch_size = max_batch_size;
        cfg.confidence_threshold = confidence_threshold;
        cfg.iou_threshold = iou_threshold;
        cfg.device_id = device_id;
        cfg.max_det = max_det;
        cfg.backbone = backbone;
        cfg.precision = precision; // RFD_PRECISION_F32: the f32 parity mode (the reference's FP32 tensor contract, face_detection.rs:261)
        cfg.schedule = schedule;   // RFD_SCHEDULE_LATENCY: split-K convolutions for passes of <= RFD_LATENCY_MAX_BATCH images (bits of their own, see rfd.h)
        check(rfd_create(&cfg, &ctx_));
        max_det_ = (std::size_t)max_det;
        max_batch_ = max_batch_size;
    }
    explicit RetinaFaceDetection(const FaceDetectionConfig &c, int device_id = 0, int max_det = 1024, int backbone = RFD_BACKBONE_R50)
        : RetinaFaceDetection(c.image_size, c.max_batch_size, c.confidence_threshold, c.iou_threshold, device_id, max_det, backbone) {}
    RetinaFaceDetection(const RetinaFaceDetection &) = delete;
    RetinaFaceDetection &operator=(const RetinaFaceDetection &) = delete;
    ~RetinaFaceDetection() { rfd_destroy(ctx_); }

    void init_synthetic_weights(uint64_t seed) { check(rfd_init_synthetic_weights(ctx_, seed)); }
    void load_weights(const std::string &path) { check(rfd_load_weights(ctx_, path.c_str())); }
    void save_weights(const std::string &path) { check(rfd_save_weights(ctx_, path.c_str())); }

    // RetinaFaceDetection::call (face_detection.rs:496).  A non-3-channel image is an error, as in the reference
    // (at_2d::<Vec3b> fails, face_detection.rs:226).  Empty result: k = 0 (reference: (0,5) and (0,5,2), :413-419).
    Detections call(const Mat &image, std::optional<bool> /*is_debug*/ = std::nullopt) { return call_batch({image}).at(0); }

    // batch form: one call for n frames (the throughput entry; n <= max_batch_size)
    std::vector<Detections> call_batch(const std::vector<Mat> &images)
    {
        const int n = (int)images.size();
        std::vector<rfd_image> im(images.size());
        for (int i = 0; i < n; ++i) {
            if (images[i].channels != 3) throw Error(RFD_ERR_INVALID_ARG, "face_detection - expected a CV_8UC3 image");
            im[i] = rfd_image{images[i].data, images[i].rows, images[i].cols, images[i].step};
        }
        std::vector<float> boxes((std::size_t)n * max_det_ * 5), lmk((std::size_t)n * max_det_ * 10);
        std::vector<int32_t> count(n), total(n);
        rfd_dets out{boxes.data(), lmk.data(), count.data(), total.data()};
        check(rfd_detect_batch(ctx_, im.data(), n, &out));
        std::vector<Detections> res(n);
        for (int i = 0; i < n; ++i) {
            const std::size_t k = (std::size_t)count[i];
            res[i].k = k;
            res[i].det.assign(boxes.begin() + (std::size_t)i * max_det_ * 5, boxes.begin() + (std::size_t)i * max_det_ * 5 + k * 5);
            res[i].kps.assign(lmk.begin() + (std::size_t)i * max_det_ * 10, lmk.begin() + (std::size_t)i * max_det_ * 10 + k * 10);
        }
        return res;
    }

    rfd_ctx *raw() const { return ctx_; }
    std::size_t max_det() const { return max_det_; }

  private:
    rfd_ctx *ctx_ = nullptr;
    std::size_t max_det_ = 0;
    int max_batch_ = 0;
};

// FaceSelectionConfig::new (config.rs:98-117) + FaceSelection::call (face_selection.rs:72-189) on the device
struct FaceSelectionConfig {
    float margin_center_left_ratio = 0.3f, margin_center_right_ratio = 0.3f, margin_edge_ratio = 0.1f, minimum_face_ratio = 0.0075f;
};
struct SelectedFace {
    std::optional<std::array<float, 5>> bbox;                // None: no face passed the filters
    std::optional<std::array<float, 10>> key_points;         // None: no detection within 2 px of the chosen box
};
class FaceSelection {
  public:
    explicit FaceSelection(FaceSelectionConfig c = {}) : cfg_(c) {}
    // call(&self, img, bboxes, kps, is_enroll) -> (Option<bbox>, Option<kps>): here over the detector's output
    SelectedFace call(RetinaFaceDetection &det, const Mat &image, const Detections &d, bool is_enroll = false) const
    {
        const std::size_t md = det.max_det();
        std::vector<float> boxes(md * 5, 0.f), lmk(md * 10, 0.f);
        std::copy(d.det.begin(), d.det.end(), boxes.begin());
        std::copy(d.kps.begin(), d.kps.end(), lmk.begin());
        int32_t count = (int32_t)d.k, total = (int32_t)d.k;
        rfd_dets in{boxes.data(), lmk.data(), &count, &total};
        rfd_selection_config sc{cfg_.margin_center_left_ratio, cfg_.margin_center_right_ratio, cfg_.margin_edge_ratio, cfg_.minimum_face_ratio};
        const int h = image.rows, w = image.cols;
        float ob[5], ok[10];
        int32_t found = 0;
        check(rfd_select_faces(det.raw(), &in, &h, &w, 1, &sc, is_enroll ? 1 : 0, ob, ok, &found));
        SelectedFace s;
        if (found & 1) { s.bbox.emplace(); std::copy(ob, ob + 5, s.bbox->begin()); }
        if (found == 3) { s.key_points.emplace(); std::copy(ok, ok + 10, s.key_points->begin()); }
        return s;
    }

  private:
    FaceSelectionConfig cfg_;
};

// FaceAlignmentConfig::new (config.rs:37-56) + FaceAlignment::call (face_alignment.rs:27-141) on the device
class FaceAlignment {
  public:
    FaceAlignment() { rfd_alignment_config_default(&cfg_); }
    FaceAlignment(std::pair<int, int> image_size, const std::array<float, 10> &standard_landmarks)
    {
        rfd_alignment_config_default(&cfg_);
        cfg_.out_w = image_size.first; cfg_.out_h = image_size.second;
        std::copy(standard_landmarks.begin(), standard_landmarks.end(), cfg_.standard_landmarks);
    }
    // -> the aligned out_h x out_w x 3 u8 BGR crop (the reference returns a Mat); throws where the reference returns Err
    std::vector<uint8_t> call(RetinaFaceDetection &det, const Mat &img, const SelectedFace &face) const
    {
        rfd_image im{img.data, img.rows, img.cols, img.step};
        float box[5] = {0, 0, 0, 0, 0}, kps[10] = {0};
        int32_t found = 0, status = 0;
        if (face.bbox) { std::copy(face.bbox->begin(), face.bbox->end(), box); found |= 1; }
        if (face.key_points) { std::copy(face.key_points->begin(), face.key_points->end(), kps); found |= 2; }
        std::vector<uint8_t> crop((std::size_t)cfg_.out_w * cfg_.out_h * 3);
        check(rfd_align_faces(det.raw(), &im, 1, box, kps, &found, &cfg_, crop.data(), &status));
        if (status < 0) throw Error(RFD_ERR_INVALID_ARG, "face_alignment - no key points / no face / crop outside the image (status " + std::to_string(status) + ")");
        return crop;
    }

  private:
    rfd_alignment_config cfg_;
};

// The inputs of the two models after alignment and what follows them: FaceQuality::call (face_quality.rs:40-186) and
// FaceExtraction::call (face_extraction.rs:30-150) minus the remote models themselves.
struct FaceTensorConfig : rfd_face_tensor_config {
    static FaceTensorConfig quality() { FaceTensorConfig c; rfd_face_tensor_config_quality(&c); return c; }       // face_quality.rs:43-44
    static FaceTensorConfig extraction() { FaceTensorConfig c; rfd_face_tensor_config_extraction(&c); return c; } // face_extraction.rs:38-39
};
// crops [n][crop_h][crop_w][3] u8 BGR -> one [n][3][out_h][out_w] f32 tensor (R, G, B planes) per config
inline std::vector<std::vector<float>> face_tensors(RetinaFaceDetection &det, const uint8_t *crops, int n, int crop_w, int crop_h,
                                                    const std::vector<FaceTensorConfig> &cfgs)
{
    std::vector<rfd_face_tensor_config> c(cfgs.begin(), cfgs.end());
    std::vector<std::vector<float>> out(cfgs.size());
    std::vector<float *> ptrs(cfgs.size());
    for (std::size_t j = 0; j < cfgs.size(); ++j) {
        out[j].resize((std::size_t)n * 3 * (cfgs[j].out_w > 0 ? cfgs[j].out_w : 0) * (cfgs[j].out_h > 0 ? cfgs[j].out_h : 0));
        ptrs[j] = out[j].data();
    }
    check(rfd_face_tensors(det.raw(), crops, n, crop_w, crop_h, c.data(), (int)c.size(), ptrs.data()));
    return out;
}
// face_quality.rs:159-168 on logits [n][classes] -> (scores, classes); throws where the reference panics (a NaN logit)
inline std::pair<std::vector<float>, std::vector<int32_t>> quality_decide(RetinaFaceDetection &det, const std::vector<float> &logits,
                                                                           int n, int classes, float threshold)
{
    std::vector<float> score(n);
    std::vector<int32_t> klass(n);
    check(rfd_quality_decide(det.raw(), logits.data(), n, classes, threshold, score.data(), klass.data()));
    return {score, klass};
}
// normalize_outputs (utils.rs:148-154): every row of emb [n][dim] divided by its L2 norm
inline std::vector<float> normalize_embeddings(RetinaFaceDetection &det, const std::vector<float> &emb, int n, int dim)
{
    std::vector<float> out(emb.size());
    check(rfd_normalize_embeddings(det.raw(), emb.data(), n, dim, out.data()));
    return out;
}

// Every detected face of a frame (rfd.h, "the packed face list"): up to max_faces detections per frame as one dense list of
// aligned crops and model inputs.  Vectors are sized for `cap` faces; the library writes the first valid() of them.
struct FaceListConfig : rfd_face_list_config {
    FaceListConfig() { rfd_face_list_config_default(this); }   // 32 faces per frame, no size or score floor
};
struct FaceList {
    int32_t total = 0;                         // T, not clamped to cap
    int cap = 0;
    std::vector<int32_t> first, frame, row, status;   // [n + 1], [cap] x 3
    std::vector<float> box, kps;               // [cap][5], [cap][10]
    std::vector<uint8_t> crops;                // [cap][out_h][out_w][3], empty if not asked for
    std::vector<std::vector<float>> tensors;   // per config: [cap][3][out_h][out_w]
    int valid() const { return total < cap ? total : cap; }
};
namespace detail {
inline rfd_face_list face_list_pointers(FaceList &r, std::size_t n, int cap, const rfd_alignment_config &ac,
                                        const std::vector<FaceTensorConfig> &cfgs, bool want_crops)
{
    const std::size_t c = cap > 0 ? (std::size_t)cap : 1, k = cfgs.size() <= RFD_MAX_FACE_TENSORS ? cfgs.size() : 0;
    r.cap = cap;
    r.first.assign(n + 1, 0); r.frame.assign(c, 0); r.row.assign(c, 0); r.status.assign(c, 0);
    r.box.assign(c * 5, 0.f); r.kps.assign(c * 10, 0.f);
    if (want_crops) r.crops.assign(c * 3 * (ac.out_w > 0 ? ac.out_w : 0) * (ac.out_h > 0 ? ac.out_h : 0), 0);
    r.tensors.resize(k);
    rfd_face_list p = {&r.total, r.first.data(), r.frame.data(), r.row.data(), r.box.data(), r.kps.data(), r.status.data(),
                       want_crops ? r.crops.data() : nullptr, {}};
    for (std::size_t j = 0; j < k; ++j) {
        r.tensors[j].assign(c * 3 * (cfgs[j].out_w > 0 ? cfgs[j].out_w : 0) * (cfgs[j].out_h > 0 ? cfgs[j].out_h : 0), 0.f);
        p.tensors[j] = r.tensors[j].data();
    }
    return p;
}
} // namespace detail
// frames + the detections rfd_detect_batch returned for them -> the list (stage level: the kernels of detect_align_all)
inline FaceList align_detections(RetinaFaceDetection &det, const std::vector<rfd_image> &imgs, const rfd_dets &dets,
                                 const std::vector<FaceTensorConfig> &cfgs, int cap, const FaceListConfig &lc = FaceListConfig(),
                                 const rfd_alignment_config *ac = nullptr, bool want_crops = true)
{
    rfd_alignment_config a;
    rfd_alignment_config_default(&a);
    if (ac) a = *ac;
    FaceList r;
    rfd_face_list p = detail::face_list_pointers(r, imgs.size(), cap, a, cfgs, want_crops);
    std::vector<rfd_face_tensor_config> c(cfgs.begin(), cfgs.end());
    check(rfd_align_detections(det.raw(), imgs.data(), (int)imgs.size(), &dets, &lc, &a, c.data(), (int)c.size(), cap, &p));
    return r;
}
// detect, list, align, tensorise: host frames in, host list out; the frames cross PCIe once
inline FaceList detect_align_all(RetinaFaceDetection &det, const std::vector<rfd_image> &imgs, const std::vector<FaceTensorConfig> &cfgs,
                                 int cap, const FaceListConfig &lc = FaceListConfig(), const rfd_alignment_config *ac = nullptr,
                                 bool want_crops = true)
{
    rfd_alignment_config a;
    rfd_alignment_config_default(&a);
    if (ac) a = *ac;
    FaceList r;
    rfd_face_list p = detail::face_list_pointers(r, imgs.size(), cap, a, cfgs, want_crops);
    std::vector<rfd_face_tensor_config> c(cfgs.begin(), cfgs.end());
    check(rfd_detect_align_all_batch(det.raw(), imgs.data(), (int)imgs.size(), &lc, &a, c.data(), (int)c.size(), cap, &p));
    return r;
}
// the device-resident form: frames and every pointer of `out` in device memory; async: no host synchronisation
inline void detect_all_faces_device(RetinaFaceDetection &det, const std::vector<rfd_image> &imgs, const std::vector<FaceTensorConfig> &cfgs,
                                    int cap, rfd_face_list &out, const FaceListConfig &lc = FaceListConfig(),
                                    const rfd_alignment_config *ac = nullptr, bool async = false)
{
    std::vector<rfd_face_tensor_config> c(cfgs.begin(), cfgs.end());
    check(rfd_detect_all_faces_device(det.raw(), imgs.data(), (int)imgs.size(), &lc, ac, c.data(), (int)c.size(), cap, &out, async ? 1 : 0));
}

// FaceAntiSpoofing (face_antispoofing.rs) minus the remote miniFAS models: FAS config, the model inputs, the decision rule.
// Defined per face (rfd.h: the reference's two bugs are not copied).
struct LivenessConfig : rfd_liveness_config {
    LivenessConfig() { rfd_liveness_config_default(this); }   // the four models the reference names (:448-485)
};
struct LivenessInputs {
    std::vector<std::vector<float>> tensors;   // per model: [n][3][out_h][out_w], B, G, R planes, raw 0..255
    std::vector<float> weights;                // [n][k]
    std::vector<int32_t> rois;                 // [n][k][4] ltx, lty, rbx, rby
    std::vector<int32_t> status;               // [n]: 0 ok, -2 no face, -3 a ROI outside the frame (the reference returns Err)
};
// _get_scale_image + _preprocess for n frames and their selected boxes [n][5] / flags [n]
inline LivenessInputs liveness_tensors(RetinaFaceDetection &det, const std::vector<rfd_image> &imgs, const float *boxes,
                                       const int32_t *found, const LivenessConfig &cfg = LivenessConfig())
{
    const std::size_t n = imgs.size(), k = cfg.k > 0 && cfg.k <= RFD_MAX_FACE_TENSORS ? (std::size_t)cfg.k : 0;
    LivenessInputs r;
    r.tensors.resize(k);
    std::vector<float *> ptrs(k ? k : 1, nullptr);
    for (std::size_t j = 0; j < k; ++j) {
        r.tensors[j].resize(n * 3 * (cfg.out_w[j] > 0 ? cfg.out_w[j] : 0) * (cfg.out_h[j] > 0 ? cfg.out_h[j] : 0));
        ptrs[j] = r.tensors[j].data();
    }
    r.weights.resize(n * k); r.rois.resize(n * k * 4); r.status.resize(n);
    check(rfd_liveness_tensors(det.raw(), imgs.data(), (int)n, boxes, found, &cfg, ptrs.data(), r.weights.data(), r.rois.data(),
                               r.status.data()));
    return r;
}
// _postprocess on logits[j] = [n][classes] of every model -> (scores, live flags); the reference's literal threshold is 0.55
inline std::pair<std::vector<float>, std::vector<int32_t>> liveness_decide(RetinaFaceDetection &det,
                                                                            const std::vector<std::vector<float>> &logits, int n,
                                                                            int classes, const std::vector<float> &weights,
                                                                            float threshold = 0.55f)
{
    std::vector<const float *> ptrs;
    for (const std::vector<float> &l : logits) ptrs.push_back(l.data());
    std::vector<float> score(n);
    std::vector<int32_t> live(n);
    check(rfd_liveness_decide(det.raw(), ptrs.data(), (int)ptrs.size(), n, classes, weights.data(), threshold, score.data(), live.data()));
    return {score, live};
}

// The face gallery (rfd.h, "gallery"): what FacePipeline::extract's facial_feature is enrolled into and compared with.  Owns the
// rfd_gallery; destroy it before the detector it was made from.
class Gallery {
  public:
    struct Matches {
        int n = 0, k = 0;
        std::vector<float> scores;  // [n][k], descending; -inf where the gallery has fewer than k rows
        std::vector<int32_t> rows;  // [n][k], equal scores by ascending row; -1 in that tail
    };
    Gallery(RetinaFaceDetection &det, int dim, int capacity) : dim_(dim) { check(rfd_gallery_create(det.raw(), dim, capacity, &g_)); }
    // a gallery read from a file that save() wrote; capacity 0 = the file's rows
    Gallery(RetinaFaceDetection &det, const std::string &path, int capacity = 0)
    {
        check(rfd_gallery_load(det.raw(), path.c_str(), capacity, &g_));
        check(rfd_gallery_size(g_, nullptr, nullptr, &dim_));
    }
    Gallery(const Gallery &) = delete;
    Gallery &operator=(const Gallery &) = delete;
    ~Gallery() { rfd_gallery_destroy(g_); }
    rfd_gallery *raw() { return g_; }
    int dim() const { return dim_; }
    int size() const
    {
        int rows = 0;
        check(rfd_gallery_size(g_, &rows, nullptr, nullptr));
        return rows;
    }
    void clear() { check(rfd_gallery_clear(g_)); }
    // emb [n][dim], unit vectors -> the row the first one got
    int add(const std::vector<float> &emb)
    {
        int first = 0;
        check(rfd_gallery_add(g_, emb.data(), (int)(emb.size() / (std::size_t)dim_), &first));
        return first;
    }
    // rows (duplicates allowed) are erased and never found again; add does not reuse their numbers
    void remove(const std::vector<int32_t> &rows) { check(rfd_gallery_remove(g_, rows.data(), (int)rows.size())); }
    // row rows[i] takes emb[i] and is live afterwards, whether it was live or removed; rows must be distinct
    void replace(const std::vector<int32_t> &rows, const std::vector<float> &emb)
    {
        if (emb.size() != rows.size() * (std::size_t)dim_) throw Error(RFD_ERR_INVALID_ARG, "replace: one embedding per row");
        check(rfd_gallery_replace(g_, rows.data(), emb.data(), (int)rows.size()));
    }
    // the same with emb [rows.size()][dim] in device memory (16-byte aligned); enqueued, no synchronisation
    void replace_device(const std::vector<int32_t> &rows, const float *emb) { check(rfd_gallery_replace_device(g_, rows.data(), emb, (int)rows.size())); }
    int live() const
    {
        int n = 0;
        check(rfd_gallery_live(g_, &n));
        return n;
    }
    // the removed rows, ascending
    std::vector<int32_t> removed() const
    {
        int n = 0;
        check(rfd_gallery_removed(g_, nullptr, 0, &n));
        std::vector<int32_t> out((std::size_t)n);
        check(rfd_gallery_removed(g_, out.data(), n, &n));
        return out;
    }
    // writes path + ".tmp", then renames it over path
    void save(const std::string &path) { check(rfd_gallery_save(g_, path.c_str())); }
    // the stored (bf16) values of rows [row0, row0 + n); a removed row reads as zeros
    std::vector<float> rows(int row0, int n)
    {
        std::vector<float> out((std::size_t)(n > 0 ? n : 0) * (std::size_t)dim_);
        check(rfd_gallery_get_rows(g_, row0, n, out.data()));
        return out;
    }
    // queries [n][dim] -> the k best rows of each
    Matches search(const std::vector<float> &queries, int k)
    {
        Matches m;
        m.n = (int)(queries.size() / (std::size_t)dim_);
        m.k = k;
        m.scores.resize((std::size_t)m.n * (std::size_t)(k > 0 ? k : 0));
        m.rows.resize(m.scores.size());
        check(rfd_gallery_search(g_, queries.data(), m.n, k, m.scores.data(), m.rows.data()));
        return m;
    }
    // identities (rfd.h, "identities"): rows[i] gets ids[i] (>= 0, or RFD_GALLERY_NO_IDENTITY); enqueued, no synchronisation
    struct IdentityMatches : Matches {
        std::vector<int32_t> ids;  // [n][k], the identity of each entry; -1 for an unlabelled row and in the empty tail
    };
    void set_identities(const std::vector<int32_t> &rows, const std::vector<int32_t> &ids)
    {
        if (ids.size() != rows.size()) throw Error(RFD_ERR_INVALID_ARG, "set_identities: one identity per row");
        check(rfd_gallery_set_identities(g_, rows.data(), ids.data(), (int)rows.size()));
    }
    // the identities of rows [row0, row0 + n)
    std::vector<int32_t> identities(int row0, int n) const
    {
        std::vector<int32_t> out((std::size_t)(n > 0 ? n : 0));
        check(rfd_gallery_get_identities(g_, row0, n, out.data()));
        return out;
    }
    // the number of live rows that carry an identity >= 0
    int labelled() const
    {
        int n = 0;
        check(rfd_gallery_identities(g_, &n));
        return n;
    }
    // queries [n][dim] -> the k best identities of each, every identity under its best row; entries below min_score are empty
    IdentityMatches search_identities(const std::vector<float> &queries, int k, float min_score = -std::numeric_limits<float>::infinity())
    {
        IdentityMatches m;
        m.n = (int)(queries.size() / (std::size_t)dim_);
        m.k = k;
        m.scores.resize((std::size_t)m.n * (std::size_t)(k > 0 ? k : 0));
        m.rows.resize(m.scores.size());
        m.ids.resize(m.scores.size());
        check(rfd_gallery_search_identities(g_, queries.data(), m.n, k, min_score, m.scores.data(), m.rows.data(), m.ids.data()));
        return m;
    }
    // tags (rfd.h, "tags"): rows[i] (live, distinct) gets the tag tags[i], any 32-bit value; enqueued, no synchronisation
    void set_tags(const std::vector<int32_t> &rows, const std::vector<uint32_t> &tags)
    {
        if (tags.size() != rows.size()) throw Error(RFD_ERR_INVALID_ARG, "set_tags: one tag per row");
        check(rfd_gallery_set_tags(g_, rows.data(), tags.data(), (int)rows.size()));
    }
    // the tags of rows [row0, row0 + n); 0 for a row that never got one and for a removed row
    std::vector<uint32_t> tags(int row0, int n) const
    {
        std::vector<uint32_t> out((std::size_t)(n > 0 ? n : 0));
        check(rfd_gallery_get_tags(g_, row0, n, out.data()));
        return out;
    }
    // search_identities among the rows r with (tag[r] & mask[q]) == value[q] for query q; one mask and one value per query
    IdentityMatches search_filtered(const std::vector<float> &queries, int k, const std::vector<uint32_t> &mask, const std::vector<uint32_t> &value,
                                    float min_score = -std::numeric_limits<float>::infinity())
    {
        IdentityMatches m;
        m.n = (int)(queries.size() / (std::size_t)dim_);
        if (mask.size() != (std::size_t)m.n || value.size() != (std::size_t)m.n) throw Error(RFD_ERR_INVALID_ARG, "search_filtered: one mask and one value per query");
        m.k = k;
        m.scores.resize((std::size_t)m.n * (std::size_t)(k > 0 ? k : 0));
        m.rows.resize(m.scores.size());
        m.ids.resize(m.scores.size());
        check(rfd_gallery_search_filtered(g_, queries.data(), m.n, k, min_score, mask.data(), value.data(), m.scores.data(), m.rows.data(), m.ids.data()));
        return m;
    }
    // the same with every pointer in device memory (queries 16-byte aligned; mask, value [n]; scores, rows, ids [n][k]);
    // enqueued, and with async no synchronisation
    void search_filtered_device(const float *queries, int n, int k, float min_score, const uint32_t *mask, const uint32_t *value, float *scores, int32_t *rows,
                                int32_t *ids, bool async = false)
    {
        check(rfd_gallery_search_filtered_device(g_, queries, n, k, min_score, mask, value, scores, rows, ids, async ? 1 : 0));
    }
    // nearest (rfd.h, "nearest"): for every row a of [row0, row0 + n) the best live row b != a that cfg allows; entry i belongs to
    // row row0 + i, and is (-inf, -1, -1) where a is removed or nothing qualifies
    struct Nearest {
        std::vector<float> scores;
        std::vector<int32_t> rows, ids;
    };
    static rfd_gallery_nearest_config nearest_config(int mode = RFD_GALLERY_NEAREST_OTHER_ROW, float min_score = -std::numeric_limits<float>::infinity(),
                                                     uint32_t tag_mask = 0)
    {
        rfd_gallery_nearest_config cfg;
        rfd_gallery_nearest_config_default(&cfg);
        cfg.mode = mode;
        cfg.min_score = min_score;
        cfg.tag_mask = tag_mask;
        return cfg;
    }
    Nearest nearest(int row0, int n, const rfd_gallery_nearest_config &cfg = nearest_config())
    {
        Nearest r;
        r.scores.resize((std::size_t)(n > 0 ? n : 0));
        r.rows.resize(r.scores.size());
        r.ids.resize(r.scores.size());
        check(rfd_gallery_nearest(g_, row0, n, &cfg, r.scores.data(), r.rows.data(), r.ids.data()));
        return r;
    }
    // the same with the outputs in device memory ([n] each; ids may be null); enqueued, and with async no synchronisation
    void nearest_device(int row0, int n, const rfd_gallery_nearest_config &cfg, float *scores, int32_t *rows, int32_t *ids, bool async = false)
    {
        check(rfd_gallery_nearest_device(g_, row0, n, &cfg, scores, rows, ids, async ? 1 : 0));
    }

  private:
    rfd_gallery *g_ = nullptr;
    int dim_;
};

// JPEG decode on the device (rfd.h, "JPEG decode"): byte_data_to_opencv (utils.rs:8-52), the first line of FacePipeline::extract.
struct JpegInfo {
    int width = 0, height = 0, components = 0;
    int sampling = RFD_JPEG_GRAY; // rfd_jpeg_sampling
    int restart_interval = 0;
};
// host only: the whole marker validation; throws with RFD_ERR_UNSUPPORTED / RFD_ERR_INVALID_ARG and the cause
inline JpegInfo jpeg_info(const std::vector<uint8_t> &file)
{
    struct rfd_jpeg_info i;
    check(rfd_jpeg_info(file.data(), file.size(), &i));
    JpegInfo r;
    r.width = i.width; r.height = i.height; r.components = i.components; r.sampling = i.sampling; r.restart_interval = i.restart_interval;
    return r;
}
// a decoded frame that owns its pixels: rows x cols x 3 u8 BGR (a grey file: B = G = R)
struct DecodedImage {
    std::vector<uint8_t> pixels;
    int rows = 0, cols = 0;
    Mat mat() const { return Mat(pixels.data(), rows, cols); }
};
inline void set_decode_threads(RetinaFaceDetection &det, int threads) { check(rfd_set_decode_threads(det.raw(), threads)); }
// files -> host frames, decoded on the device; throws where the reference's imdecode fails.  oriented: the context is in
// RFD_JPEG_ORIENTATION_APPLY mode (set_jpeg_orientation below), so the frames are allocated in the oriented size; denom: the
// context's set_jpeg_scale, so they are allocated in the scaled size.  Both repeat what the context was told: where they differ
// from it, the decode refuses the call by its size rule (RFD_ERR_INVALID_ARG naming the frame) and writes nothing
inline std::vector<DecodedImage> decode_jpeg(RetinaFaceDetection &det, const std::vector<std::vector<uint8_t>> &files, bool oriented = false, int denom = 1)
{
    const std::size_t n = files.size();
    std::vector<DecodedImage> out(n);
    std::vector<const uint8_t *> ptrs(n);
    std::vector<std::size_t> lens(n);
    std::vector<rfd_image> im(n);
    for (std::size_t i = 0; i < n; ++i) {
        JpegInfo info;
        try {
            info = jpeg_info(files[i]);
            if (oriented) {
                struct rfd_jpeg_orientation o;
                check(rfd_jpeg_orientation(files[i].data(), files[i].size(), &o));
                info.width = o.width; info.height = o.height;
            }
            if (denom != 1) {
                struct rfd_jpeg_scaled_size z;
                check(rfd_jpeg_scaled_size(files[i].data(), files[i].size(), denom, oriented ? RFD_JPEG_ORIENTATION_APPLY : RFD_JPEG_ORIENTATION_IGNORE, &z));
                info.width = z.width; info.height = z.height;
            }
        } catch (const Error &e) { // name the file, as the batch call itself does
            throw Error(e.status, "file " + std::to_string(i) + ": " + e.message);
        }
        out[i].rows = info.height; out[i].cols = info.width;
        out[i].pixels.resize((std::size_t)info.height * (std::size_t)info.width * 3);
        ptrs[i] = files[i].data(); lens[i] = files[i].size();
        im[i] = rfd_image{out[i].pixels.data(), info.height, info.width, (std::ptrdiff_t)info.width * 3};
    }
    check(rfd_decode_jpeg_batch(det.raw(), ptrs.data(), lens.data(), (int)n, im.data()));
    return out;
}
// files -> caller-allocated DEVICE frames (frames[i].data is device memory the library writes); the same array then feeds
// rfd_detect_batch_device / rfd_detect_faces_device.  async: no host synchronisation (rfd_sync before reading).
inline void decode_jpeg_device(RetinaFaceDetection &det, const std::vector<std::vector<uint8_t>> &files, const std::vector<rfd_image> &frames,
                               bool async = false)
{
    if (files.size() != frames.size()) throw Error(RFD_ERR_INVALID_ARG, "decode_jpeg_device: one frame per file");
    std::vector<const uint8_t *> ptrs(files.size());
    std::vector<std::size_t> lens(files.size());
    for (std::size_t i = 0; i < files.size(); ++i) { ptrs[i] = files[i].data(); lens[i] = files[i].size(); }
    check(rfd_decode_jpeg_batch_device(det.raw(), ptrs.data(), lens.data(), (int)files.size(), frames.data(), async ? 1 : 0));
}
// The library's default encode settings (quality 90, 4:2:0, one restart row) with the given fields replaced (rfd.h, "JPEG encode")
inline rfd_jpeg_encode_config jpeg_encode_config(int quality = 90, rfd_jpeg_sampling sampling = RFD_JPEG_420, int restart_rows = 1)
{
    rfd_jpeg_encode_config c;
    check(rfd_jpeg_encode_config_default(&c));
    c.quality = quality; c.sampling = (int32_t)sampling; c.restart_rows = restart_rows;
    return c;
}
// host BGR frames -> baseline JPEG files, encoded on the device, byte for byte what libjpeg-turbo's default compressor writes.
// slot_bytes: the room of a file (0: the largest rfd_jpeg_encode_bound of the frames); a file that does not fit comes back empty
inline std::vector<std::vector<uint8_t>> encode_jpeg(RetinaFaceDetection &det, const std::vector<rfd_image> &frames, const rfd_jpeg_encode_config &cfg,
                                                     std::size_t slot_bytes = 0)
{
    const std::size_t n = frames.size();
    if (slot_bytes == 0)
        for (const rfd_image &f : frames) {
            std::size_t b = 0;
            check(rfd_jpeg_encode_bound(f.width, f.height, &cfg, &b));
            slot_bytes = std::max(slot_bytes, b);
        }
    std::vector<uint8_t> slots(n * slot_bytes);
    std::vector<int32_t> size(n, 0);
    check(rfd_encode_jpeg_batch(det.raw(), frames.data(), (int)n, &cfg, slots.data(), slot_bytes, size.data()));
    std::vector<std::vector<uint8_t>> out(n);
    for (std::size_t i = 0; i < n; ++i)
        if (size[i] > 0) out[i].assign(slots.begin() + (std::ptrdiff_t)(i * slot_bytes), slots.begin() + (std::ptrdiff_t)(i * slot_bytes + (std::size_t)size[i]));
    return out;
}
// DEVICE frames or crops -> files in DEVICE slots of slot_bytes each, size_dev[i] their lengths (-1: does not fit); count_dev
// (device, may be null): images at and past it are left alone, e.g. rfd_face_list.total for its crops.  async: no host wait.
inline void encode_jpeg_device(RetinaFaceDetection &det, const std::vector<rfd_image> &frames, const rfd_jpeg_encode_config &cfg, uint8_t *out, std::size_t slot_bytes,
                               int32_t *size_dev, const int32_t *count_dev = nullptr, bool async = false)
{
    check(rfd_encode_jpeg_batch_device(det.raw(), frames.data(), (int)frames.size(), count_dev, &cfg, out, slot_bytes, size_dev, async ? 1 : 0));
}
// RFD_JPEG_ENTROPY_DEVICE: files with a restart interval are Huffman-decoded on the device (rfd.h, "entropy decoding on the
// device"); every other file, and everything in RFD_JPEG_ENTROPY_HOST (the default), on the host threads
inline void set_jpeg_entropy(RetinaFaceDetection &det, rfd_jpeg_entropy mode) { check(rfd_set_jpeg_entropy(det.raw(), (int)mode)); }
// per frame of the last decode call: 0 host, 1 device, 2 host after the device refused the frame
// RFD_JPEG_ORIENTATION_APPLY: frames are written upright, through the file's EXIF orientation tag and in the oriented size (rfd.h,
// "EXIF orientation"); RFD_JPEG_ORIENTATION_IGNORE (the default): as the file stores them
inline void set_jpeg_orientation(RetinaFaceDetection &det, rfd_jpeg_orientation_mode mode) { check(rfd_set_jpeg_orientation(det.raw(), (int)mode)); }

struct JpegOrientation {
    int orientation = 1;                    // 1..8
    int width = 0, height = 0;              // of the frame an APPLY-mode decode writes
    int stored_width = 0, stored_height = 0;
};
inline JpegOrientation jpeg_orientation(const std::vector<uint8_t> &file)
{
    struct rfd_jpeg_orientation o;
    check(rfd_jpeg_orientation(file.data(), file.size(), &o));
    JpegOrientation r;
    r.orientation = o.orientation; r.width = o.width; r.height = o.height;
    r.stored_width = o.stored_width; r.stored_height = o.stored_height;
    return r;
}

// 1 / denom of the stored size, denom 1 (the default), 2, 4 or 8, built by libjpeg's reduced inverse DCTs (rfd.h, "JPEG decode,
// reduced size"); applies to every frame of the calls that follow
inline void set_jpeg_scale(RetinaFaceDetection &det, int denom) { check(rfd_set_jpeg_scale(det.raw(), denom)); }
struct JpegScaledSize {
    int denom = 1;
    int width = 0, height = 0;              // of the frame a decode with that denominator and orientation mode writes
    int stored_width = 0, stored_height = 0;
    int orientation = 1;                    // the one that will be applied
};
inline JpegScaledSize jpeg_scaled_size(const std::vector<uint8_t> &file, int denom, rfd_jpeg_orientation_mode mode = RFD_JPEG_ORIENTATION_IGNORE)
{
    struct rfd_jpeg_scaled_size z;
    check(rfd_jpeg_scaled_size(file.data(), file.size(), denom, (int)mode, &z));
    JpegScaledSize r;
    r.denom = z.denom; r.width = z.width; r.height = z.height;
    r.stored_width = z.stored_width; r.stored_height = z.stored_height; r.orientation = z.orientation;
    return r;
}

inline std::vector<int32_t> jpeg_last_paths(RetinaFaceDetection &det)
{
    int n = 0;
    const int st = rfd_jpeg_last_paths(det.raw(), nullptr, 0, &n);
    if (st != RFD_ERR_CAPACITY) check(st);
    std::vector<int32_t> out((std::size_t)n);
    check(rfd_jpeg_last_paths(det.raw(), out.data(), n, &n));
    return out;
}

// ---- views (rfd.h, "views"): detection over overlapping views of a frame, merged on the device ----
// the defaults for a network of net_w x net_h: tile = the network size, overlap = net_w / 5, the full view, a margin of 4 px
inline rfd_view_config view_config(int net_w = 640, int net_h = 640)
{
    rfd_view_config c;
    rfd_view_config_default(&c, net_w, net_h);
    return c;
}
// the views of one frame: the whole frame first where there is more than one tile, then the tiles row-major; host only
inline std::vector<rfd_view> view_plan(int frame_w, int frame_h, const rfd_view_config &cfg, int frame = 0)
{
    int n = 0;
    const int st = rfd_view_plan(frame, frame_w, frame_h, &cfg, nullptr, 0, &n);
    if (st != RFD_ERR_CAPACITY) check(st);
    std::vector<rfd_view> out((std::size_t)n);
    check(rfd_view_plan(frame, frame_w, frame_h, &cfg, out.data(), n, &n));
    return out;
}
// DEVICE frames and DEVICE slabs [frames.size()][max_det] (out.total required), views sorted by frame; the slabs feed the
// selection, alignment and face-list calls as those of rfd_detect_batch_device do.  async: no host synchronisation
inline void detect_views_device(RetinaFaceDetection &det, const std::vector<rfd_image> &frames, const std::vector<rfd_view> &views, float edge_margin,
                                rfd_dets out, bool async = false)
{
    check(rfd_detect_views_batch_device(det.raw(), frames.data(), (int)frames.size(), views.data(), (int)views.size(), edge_margin, &out, async ? 1 : 0));
}
// host frames and host slabs, synchronous
inline void detect_views(RetinaFaceDetection &det, const std::vector<rfd_image> &frames, const std::vector<rfd_view> &views, float edge_margin, rfd_dets out)
{
    check(rfd_detect_views_batch(det.raw(), frames.data(), (int)frames.size(), views.data(), (int)views.size(), edge_margin, &out));
}

// ---- tracker (rfd.h, "tracker"): faces followed over the frames of a video stream ----
// Owns the rfd_tracker; destroy it before the detector it was made from.
class Tracker {
  public:
    // one frame's answer of the host form: a serial (0 = none) and RFD_TRACK_* flags per row of the frame
    struct Frame {
        std::vector<int32_t> track;
        std::vector<uint32_t> flags;
        int matched = 0, born = 0, dropped = 0;
        std::vector<int32_t> ended;  // serials of the tracks that ended at this frame, in ascending slot order
        std::vector<int32_t> due;    // the rows that are RFD_TRACK_DUE, in row order: the faces to hand to the models
    };
    static rfd_tracker_config default_config(RetinaFaceDetection &det)
    {
        rfd_tracker_config c;
        check(rfd_tracker_config_default(det.raw(), &c));
        return c;
    }
    explicit Tracker(RetinaFaceDetection &det) : max_det_(det.max_det()), cfg_(default_config(det)) { check(rfd_tracker_create(det.raw(), &cfg_, &t_)); }
    Tracker(RetinaFaceDetection &det, const rfd_tracker_config &cfg) : max_det_(det.max_det()), cfg_(cfg) { check(rfd_tracker_create(det.raw(), &cfg_, &t_)); }
    Tracker(const Tracker &) = delete;
    Tracker &operator=(const Tracker &) = delete;
    ~Tracker() { rfd_tracker_destroy(t_); }
    rfd_tracker *raw() { return t_; }
    const rfd_tracker_config &config() const { return cfg_; }
    // frames[i] = the detections of a frame of camera streams[i] as call_batch returns them; frames of one camera in time order.
    // quality (optional): one value per row of every frame
    std::vector<Frame> update(const std::vector<int32_t> &streams, const std::vector<Detections> &frames,
                              const std::vector<std::vector<float>> *quality = nullptr)
    {
        const std::size_t n = frames.size(), md = max_det_, mt = (std::size_t)cfg_.max_tracks;
        if (streams.size() != n || (quality && quality->size() != n)) throw Error(RFD_ERR_INVALID_ARG, "tracker - one stream (and quality list) per frame");
        std::vector<float> boxes(n * md * 5), lmk(n * md * 10), q(quality ? n * md : 0);
        std::vector<int32_t> count(n), track(n * md), stats(n * 4), ended(n * mt);
        std::vector<uint32_t> flags(n * md);
        for (std::size_t i = 0; i < n; ++i) {
            const std::size_t k = std::min(frames[i].k, md);
            std::copy(frames[i].det.begin(), frames[i].det.begin() + (std::ptrdiff_t)(k * 5), boxes.begin() + (std::ptrdiff_t)(i * md * 5));
            std::copy(frames[i].kps.begin(), frames[i].kps.begin() + (std::ptrdiff_t)(k * 10), lmk.begin() + (std::ptrdiff_t)(i * md * 10));
            count[i] = (int32_t)k;
            if (quality) {
                if ((*quality)[i].size() < k) throw Error(RFD_ERR_INVALID_ARG, "tracker - a quality value per row");
                std::copy((*quality)[i].begin(), (*quality)[i].begin() + (std::ptrdiff_t)k, q.begin() + (std::ptrdiff_t)(i * md));
            }
        }
        const rfd_dets dets{boxes.data(), lmk.data(), count.data(), nullptr};
        rfd_track_out out{};
        out.track = track.data(); out.flags = flags.data(); out.stats = stats.data(); out.ended = ended.data();
        check(rfd_tracker_update(t_, streams.data(), &dets, quality ? q.data() : nullptr, (int)n, &out));
        std::vector<Frame> res(n);
        for (std::size_t i = 0; i < n; ++i) {
            Frame &f = res[i];
            const std::size_t k = (std::size_t)count[i];
            f.track.assign(track.begin() + (std::ptrdiff_t)(i * md), track.begin() + (std::ptrdiff_t)(i * md + k));
            f.flags.assign(flags.begin() + (std::ptrdiff_t)(i * md), flags.begin() + (std::ptrdiff_t)(i * md + k));
            f.matched = stats[i * 4]; f.born = stats[i * 4 + 1]; f.dropped = stats[i * 4 + 3];
            f.ended.assign(ended.begin() + (std::ptrdiff_t)(i * mt), ended.begin() + (std::ptrdiff_t)(i * mt) + stats[i * 4 + 2]);
            for (std::size_t r = 0; r < k; ++r)
                if (f.flags[r] & RFD_TRACK_DUE) f.due.push_back((int32_t)r);
        }
        return res;
    }
    // DEVICE slabs and outputs, enqueued on the detector's stream; async: no host synchronisation
    void update_device(const std::vector<int32_t> &streams, const rfd_dets &dets, const float *quality, const rfd_track_out &out, bool async = false)
    {
        check(rfd_tracker_update_device(t_, streams.data(), &dets, quality, (int)streams.size(), &out, async ? 1 : 0));
    }
    void reset(int stream = -1) { check(rfd_tracker_reset(t_, stream)); }
    // the live tracks of a stream in ascending slot order (waits for the stream)
    std::vector<rfd_track> tracks(int stream)
    {
        int n = 0;
        check(rfd_tracker_get_tracks(t_, stream, nullptr, 0, &n));
        std::vector<rfd_track> out((std::size_t)n);
        check(rfd_tracker_get_tracks(t_, stream, out.data(), n, &n));
        return out;
    }

    // ---- track identities (rfd.h, "track identities"): a template and a name per track, an answer per detection row ----
    static rfd_track_identity_config default_identity_config()
    {
        rfd_track_identity_config c;
        check(rfd_track_identity_config_default(&c));
        return c;
    }
    // once per tracker
    void enable_identities(const rfd_track_identity_config &cfg)
    {
        check(rfd_tracker_identity_enable(t_, &cfg));
        id_cfg_ = cfg;
    }
    void enable_identities() { enable_identities(default_identity_config()); }
    const rfd_track_identity_config &identity_config() const { return id_cfg_; }
    // One observation of the host forms: the embedding (or gallery answer) of slab row `row` of frame `frame`, whose track is
    // `serial`; observations in (frame, row) order.
    struct Observation {
        int32_t frame, row, serial;
    };
    struct Fused {
        std::vector<float> query;     // [m][dim]: what to search the gallery with
        std::vector<int32_t> status;  // [m]: RFD_TRACK_FUSE_*
    };
    // emb: [m][dim], the ID model's raw output; weight: [m] or empty for 1
    Fused fuse(const std::vector<int32_t> &streams, const std::vector<Observation> &obs, const std::vector<float> &emb,
               const std::vector<float> &weight = {})
    {
        const std::size_t m = obs.size(), dim = (std::size_t)id_cfg_.dim;
        if (emb.size() != m * dim || (!weight.empty() && weight.size() != m)) throw Error(RFD_ERR_INVALID_ARG, "tracker - an embedding (and weight) per observation");
        ObsArrays a = obs_arrays(streams, obs);
        Fused out{std::vector<float>(m * dim), std::vector<int32_t>(m, RFD_TRACK_FUSE_NO_TRACK)};
        const rfd_track_obs o{nullptr, a.first.data(), a.row.data(), a.serial.data()};
        check(rfd_tracker_fuse(t_, streams.data(), (int)streams.size(), &o, (int)m, emb.data(), weight.empty() ? nullptr : weight.data(),
                               out.query.data(), out.status.data()));
        return out;
    }
    // scores, rows, ids: [m][k] as Gallery's identity search returned them for Fused::query; status: Fused::status
    void label(const std::vector<int32_t> &streams, const std::vector<Observation> &obs, int k, const std::vector<float> &scores,
               const std::vector<int32_t> &rows, const std::vector<int32_t> &ids, const std::vector<int32_t> &status)
    {
        const std::size_t m = obs.size(), mk = m * (std::size_t)(k > 0 ? k : 0);
        if (scores.size() != mk || rows.size() != mk || (!ids.empty() && ids.size() != mk) || status.size() != m)
            throw Error(RFD_ERR_INVALID_ARG, "tracker - k results and a status per observation");
        ObsArrays a = obs_arrays(streams, obs);
        const rfd_track_obs o{nullptr, a.first.data(), a.row.data(), a.serial.data()};
        check(rfd_tracker_label(t_, streams.data(), (int)streams.size(), &o, (int)m, k, scores.data(), rows.data(), ids.empty() ? nullptr : ids.data(),
                                status.data()));
    }
    // one frame's answer of who: per row the flags with RFD_TRACK_NAMED added, the identity (-1) and its score (-inf)
    struct Who {
        std::vector<uint32_t> who;
        std::vector<int32_t> identity;
        std::vector<float> score;
    };
    // frames: what update returned for the same streams; every row of every frame is answered
    std::vector<Who> who(const std::vector<int32_t> &streams, const std::vector<Frame> &frames)
    {
        const std::size_t n = frames.size(), md = max_det_;
        if (streams.size() != n) throw Error(RFD_ERR_INVALID_ARG, "tracker - one stream per frame");
        std::vector<int32_t> track(n * md), count(n), identity(n * md);
        std::vector<uint32_t> flags(n * md);
        std::vector<float> score(n * md);
        for (std::size_t i = 0; i < n; ++i) {
            const std::size_t k = std::min(frames[i].track.size(), md);
            std::copy(frames[i].track.begin(), frames[i].track.begin() + (std::ptrdiff_t)k, track.begin() + (std::ptrdiff_t)(i * md));
            std::copy(frames[i].flags.begin(), frames[i].flags.begin() + (std::ptrdiff_t)k, flags.begin() + (std::ptrdiff_t)(i * md));
            count[i] = (int32_t)k;
        }
        check(rfd_tracker_who(t_, streams.data(), (int)n, track.data(), count.data(), flags.data(), flags.data(), identity.data(), score.data()));
        std::vector<Who> res(n);
        for (std::size_t i = 0; i < n; ++i) {
            const std::ptrdiff_t at = (std::ptrdiff_t)(i * md), k = (std::ptrdiff_t)count[i];
            res[i].who.assign(flags.begin() + at, flags.begin() + at + k);
            res[i].identity.assign(identity.begin() + at, identity.begin() + at + k);
            res[i].score.assign(score.begin() + at, score.begin() + at + k);
        }
        return res;
    }
    // DEVICE pointers throughout (stream list: host), enqueued on the detector's stream; async: no host synchronisation
    void fuse_device(const std::vector<int32_t> &streams, const rfd_track_obs &obs, int m, const float *emb, const float *weight, float *query,
                     int32_t *status, bool async = false)
    {
        check(rfd_tracker_fuse_device(t_, streams.data(), (int)streams.size(), &obs, m, emb, weight, query, status, async ? 1 : 0));
    }
    void label_device(const std::vector<int32_t> &streams, const rfd_track_obs &obs, int m, int k, const float *scores, const int32_t *rows,
                      const int32_t *ids, const int32_t *status, bool async = false)
    {
        check(rfd_tracker_label_device(t_, streams.data(), (int)streams.size(), &obs, m, k, scores, rows, ids, status, async ? 1 : 0));
    }
    void who_device(const std::vector<int32_t> &streams, const int32_t *track, const int32_t *count, const uint32_t *flags_in, uint32_t *who,
                    int32_t *identity, float *id_score, bool async = false)
    {
        check(rfd_tracker_who_device(t_, streams.data(), (int)streams.size(), track, count, flags_in, who, identity, id_score, async ? 1 : 0));
    }
    // the entries of the live, fused tracks of a stream in ascending slot order (waits for the stream)
    std::vector<rfd_track_identity> identities(int stream)
    {
        int n = 0;
        check(rfd_tracker_get_identities(t_, stream, nullptr, 0, &n));
        std::vector<rfd_track_identity> out((std::size_t)n);
        check(rfd_tracker_get_identities(t_, stream, out.data(), n, &n));
        return out;
    }
    // the template of a live, fused track; throws for "no such track"
    std::vector<float> track_template(int stream, int32_t serial)
    {
        std::vector<float> out((std::size_t)id_cfg_.dim);
        check(rfd_tracker_get_template(t_, stream, serial, out.data()));
        return out;
    }

    // ---- track shots (rfd.h, "track shots"): the best aligned crop of every track, ended tracks as records ----
    static rfd_track_shot_config default_shot_config()
    {
        rfd_track_shot_config c;
        check(rfd_track_shot_config_default(&c));
        return c;
    }
    // once per tracker
    void enable_shots(const rfd_track_shot_config &cfg)
    {
        check(rfd_tracker_shots_enable(t_, &cfg));
        shot_cfg_ = cfg;
    }
    void enable_shots() { enable_shots(default_shot_config()); }
    const rfd_track_shot_config &shot_config() const { return shot_cfg_; }
    std::size_t shot_bytes() const { return (std::size_t)shot_cfg_.crop_w * (std::size_t)shot_cfg_.crop_h * 3; }
    // crops: [m][crop_h][crop_w][3], the aligned crop of each observation; face_status: [m] or empty; q: [m] or empty (every
    // valid shot is kept); stamps: one per frame or empty for 0 -> [m] RFD_TRACK_SHOT_*
    std::vector<int32_t> keep_shots(const std::vector<int32_t> &streams, const std::vector<Observation> &obs, const std::vector<uint8_t> &crops,
                                    const std::vector<float> &q = {}, const std::vector<int32_t> &face_status = {},
                                    const std::vector<int64_t> &stamps = {})
    {
        const std::size_t m = obs.size();
        if (crops.size() != m * shot_bytes() || (!q.empty() && q.size() != m) || (!face_status.empty() && face_status.size() != m) ||
            (!stamps.empty() && stamps.size() != streams.size()))
            throw Error(RFD_ERR_INVALID_ARG, "tracker - a crop (and q, face status) per observation, a stamp per frame");
        ObsArrays a = obs_arrays(streams, obs);
        std::vector<int32_t> status(m, RFD_TRACK_SHOT_NO_TRACK);
        const rfd_track_obs o{nullptr, a.first.data(), a.row.data(), a.serial.data()};
        check(rfd_tracker_keep_shots(t_, streams.data(), stamps.empty() ? nullptr : stamps.data(), (int)streams.size(), &o, (int)m, crops.data(),
                                     face_status.empty() ? nullptr : face_status.data(), q.empty() ? nullptr : q.data(), status.data()));
        return status;
    }
    // the records of the tracks that `frames` (what update returned for the same streams) ended, with their crops
    struct Records {
        int total = 0;                       // untruncated
        std::vector<int32_t> first;          // [n + 1]
        std::vector<rfd_track_record> rec;   // [min(total, cap)]
        std::vector<uint8_t> crops;          // [min(total, cap)][crop_h][crop_w][3]
    };
    Records collect_ended(const std::vector<int32_t> &streams, const std::vector<Frame> &frames, int cap, const std::vector<int64_t> &stamps = {})
    {
        const std::size_t n = frames.size(), mt = (std::size_t)cfg_.max_tracks;
        if (streams.size() != n || (!stamps.empty() && stamps.size() != n) || cap < 1) throw Error(RFD_ERR_INVALID_ARG, "tracker - one stream (and stamp) per frame, cap >= 1");
        std::vector<int32_t> stats(n * 4, 0), ended(n * mt, 0);
        for (std::size_t i = 0; i < n; ++i) {
            const std::size_t k = std::min(frames[i].ended.size(), mt);
            stats[i * 4 + 2] = (int32_t)k;
            std::copy(frames[i].ended.begin(), frames[i].ended.begin() + (std::ptrdiff_t)k, ended.begin() + (std::ptrdiff_t)(i * mt));
        }
        Records out;
        out.first.assign(n + 1, 0);
        out.rec.resize((std::size_t)cap);
        out.crops.resize((std::size_t)cap * shot_bytes());
        int32_t total = 0;
        const rfd_track_records r{&total, out.first.data(), out.rec.data(), out.crops.data()};
        check(rfd_tracker_collect_ended(t_, streams.data(), stamps.empty() ? nullptr : stamps.data(), (int)n, stats.data(), ended.data(), cap, &r));
        out.total = total;
        const std::size_t have = (std::size_t)std::min(std::max(total, 0), cap);
        out.rec.resize(have);
        out.crops.resize(have * shot_bytes());
        return out;
    }
    // DEVICE pointers throughout (stream list and stamps: host), enqueued on the detector's stream; async: no host synchronisation
    void keep_shots_device(const std::vector<int32_t> &streams, const int64_t *stamps, const rfd_track_obs &obs, int m, const uint8_t *crops,
                           const int32_t *face_status, const float *q, int32_t *status, bool async = false)
    {
        check(rfd_tracker_keep_shots_device(t_, streams.data(), stamps, (int)streams.size(), &obs, m, crops, face_status, q, status, async ? 1 : 0));
    }
    void collect_ended_device(const std::vector<int32_t> &streams, const int64_t *stamps, const int32_t *stats, const int32_t *ended, int cap,
                              const rfd_track_records &out, bool async = false)
    {
        check(rfd_tracker_collect_ended_device(t_, streams.data(), stamps, (int)streams.size(), stats, ended, cap, &out, async ? 1 : 0));
    }
    // the entries of the live tracks of a stream that have a kept shot, in ascending slot order (waits for the stream)
    std::vector<rfd_track_shot> shots(int stream)
    {
        int n = 0;
        check(rfd_tracker_get_shots(t_, stream, nullptr, 0, &n));
        std::vector<rfd_track_shot> out((std::size_t)n);
        check(rfd_tracker_get_shots(t_, stream, out.data(), n, &n));
        return out;
    }
    // the stored crop of a live track; throws for "no such track"
    std::vector<uint8_t> shot_crop(int stream, int32_t serial)
    {
        std::vector<uint8_t> out(shot_bytes());
        check(rfd_tracker_get_shot_crop(t_, stream, serial, out.data()));
        return out;
    }

  private:
    struct ObsArrays {
        std::vector<int32_t> first, row, serial;
    };
    ObsArrays obs_arrays(const std::vector<int32_t> &streams, const std::vector<Observation> &obs) const
    {
        const std::size_t n = streams.size(), md = max_det_;
        ObsArrays a{std::vector<int32_t>(n + 1, 0), std::vector<int32_t>(obs.size()), std::vector<int32_t>(n * md, 0)};
        for (std::size_t t = 0; t < obs.size(); ++t) {
            const Observation &o = obs[t];
            if (o.frame < 0 || (std::size_t)o.frame >= n || (t > 0 && o.frame < obs[t - 1].frame))
                throw Error(RFD_ERR_INVALID_ARG, "tracker - observations in frame order, each of a frame of the call");
            for (std::size_t b = (std::size_t)o.frame + 1; b <= n; ++b) ++a.first[b];
            a.row[t] = o.row;
            if (o.row >= 0 && (std::size_t)o.row < md) a.serial[(std::size_t)o.frame * md + (std::size_t)o.row] = o.serial;
        }
        return a;
    }
    rfd_tracker *t_ = nullptr;
    std::size_t max_det_ = 0;
    rfd_tracker_config cfg_{};
    rfd_track_identity_config id_cfg_{};
    rfd_track_shot_config shot_cfg_{};
};

// The device-resident form of the face list over caller-made DEVICE slabs (rfd_align_detections_device): with a tracker's
// `due` slab as dets, only the faces worth a model call are aligned.
inline void align_detections_device(RetinaFaceDetection &det, const std::vector<rfd_image> &imgs, const rfd_dets &dets,
                                    const rfd_face_list_config *list_cfg, const rfd_alignment_config *align_cfg,
                                    const std::vector<rfd_face_tensor_config> &cfgs, int cap, rfd_face_list out, bool async = false)
{
    check(rfd_align_detections_device(det.raw(), imgs.data(), (int)imgs.size(), &dets, list_cfg, align_cfg, cfgs.data(), (int)cfgs.size(), cap, &out, async ? 1 : 0));
}

// ---- shot quality (rfd.h, "shot quality"): a figure of merit in [0, 1] per detection row, the tracker's `quality` ----
// one frame's answer of the host form, a value per row of the frame
struct ShotQuality {
    std::vector<float> quality;
    std::vector<std::array<float, RFD_SHOT_QUALITY_PARTS>> parts; // sharp, mean, expo, yaw, roll, pitch, pose, size
    std::vector<int32_t> status;                                  // 1 = unmeasured: the region is below 32 x 32 pixels
};
inline rfd_shot_quality_config shot_quality_default_config()
{
    rfd_shot_quality_config c;
    check(rfd_shot_quality_config_default(&c));
    return c;
}
// frames[i] with its detections dets[i] as call_batch returns them; cfg = nullptr: the default
inline std::vector<ShotQuality> shot_quality(RetinaFaceDetection &det, const std::vector<rfd_image> &frames, const std::vector<Detections> &dets,
                                             const rfd_shot_quality_config *cfg = nullptr)
{
    const std::size_t n = frames.size(), md = det.max_det();
    if (dets.size() != n) throw Error(RFD_ERR_INVALID_ARG, "shot quality - one detection list per frame");
    std::vector<float> boxes(n * md * 5), lmk(n * md * 10), q(n * md), parts(n * md * RFD_SHOT_QUALITY_PARTS);
    std::vector<int32_t> count(n), status(n * md);
    for (std::size_t i = 0; i < n; ++i) {
        const std::size_t k = std::min(dets[i].k, md);
        std::copy(dets[i].det.begin(), dets[i].det.begin() + (std::ptrdiff_t)(k * 5), boxes.begin() + (std::ptrdiff_t)(i * md * 5));
        std::copy(dets[i].kps.begin(), dets[i].kps.begin() + (std::ptrdiff_t)(k * 10), lmk.begin() + (std::ptrdiff_t)(i * md * 10));
        count[i] = (int32_t)k;
    }
    const rfd_dets d{boxes.data(), lmk.data(), count.data(), nullptr};
    check(rfd_shot_quality(det.raw(), frames.data(), (int)n, &d, cfg, q.data(), parts.data(), status.data()));
    std::vector<ShotQuality> res(n);
    for (std::size_t i = 0; i < n; ++i) {
        const std::size_t k = (std::size_t)count[i];
        res[i].quality.assign(q.begin() + (std::ptrdiff_t)(i * md), q.begin() + (std::ptrdiff_t)(i * md + k));
        res[i].status.assign(status.begin() + (std::ptrdiff_t)(i * md), status.begin() + (std::ptrdiff_t)(i * md + k));
        res[i].parts.resize(k);
        for (std::size_t r = 0; r < k; ++r)
            std::copy_n(parts.begin() + (std::ptrdiff_t)((i * md + r) * RFD_SHOT_QUALITY_PARTS), RFD_SHOT_QUALITY_PARTS, res[i].parts[r].begin());
    }
    return res;
}
// DEVICE frames, slabs and outputs (parts and status may be null), enqueued on the detector's stream; async: no host
// synchronisation.  `quality` is what Tracker::update_device takes.
inline void shot_quality_device(RetinaFaceDetection &det, const std::vector<rfd_image> &imgs, const rfd_dets &dets, const rfd_shot_quality_config *cfg,
                                float *quality, float *parts = nullptr, int32_t *status = nullptr, bool async = false)
{
    check(rfd_shot_quality_device(det.raw(), imgs.data(), (int)imgs.size(), &dets, cfg, quality, parts, status, async ? 1 : 0));
}

// ---- redaction (rfd.h, "redaction"): pixelate or fill the faces of detection rows in frames ----
inline rfd_redact_config redact_default_config()
{
    rfd_redact_config c;
    check(rfd_redact_config_default(&c));
    return c;
}
// Host frames[i] with their detections dets[i] as call_batch returns them, painted into dst[i] (frames of the same sizes), or in
// place when dst is empty: the frames' data is then written through.  sel: empty, or one word per frame and row (rfd.h);
// cfg = nullptr: the default.  -> applied per frame.
inline std::vector<int32_t> redact_faces(RetinaFaceDetection &det, const std::vector<rfd_image> &frames, const std::vector<rfd_image> &dst,
                                         const std::vector<Detections> &dets, const std::vector<std::vector<uint32_t>> &sel = {},
                                         const rfd_redact_config *cfg = nullptr)
{
    const std::size_t n = frames.size(), md = det.max_det();
    if (dets.size() != n) throw Error(RFD_ERR_INVALID_ARG, "redact faces - one detection list per frame");
    if (!dst.empty() && dst.size() != n) throw Error(RFD_ERR_INVALID_ARG, "redact faces - one dst per frame, or none");
    if (!sel.empty() && sel.size() != n) throw Error(RFD_ERR_INVALID_ARG, "redact faces - one sel list per frame, or none");
    std::vector<float> boxes(n * md * 5);
    std::vector<int32_t> count(n), applied(n);
    std::vector<uint32_t> words(sel.empty() ? 0 : n * md);
    for (std::size_t i = 0; i < n; ++i) {
        const std::size_t k = std::min(dets[i].k, md);
        std::copy(dets[i].det.begin(), dets[i].det.begin() + (std::ptrdiff_t)(k * 5), boxes.begin() + (std::ptrdiff_t)(i * md * 5));
        count[i] = (int32_t)k;
        if (!sel.empty()) std::copy_n(sel[i].begin(), std::min(sel[i].size(), md), words.begin() + (std::ptrdiff_t)(i * md));
    }
    const rfd_dets d{boxes.data(), nullptr, count.data(), nullptr};
    check(rfd_redact_faces(det.raw(), frames.data(), dst.empty() ? nullptr : dst.data(), (int)n, &d, sel.empty() ? nullptr : words.data(), cfg, applied.data()));
    return applied;
}
// DEVICE frames, slabs, sel and applied (either may be null; dst null: in place), enqueued on the detector's stream; async: no
// host synchronisation.  The tracker's flags array is a ready `sel`.
inline void redact_faces_device(RetinaFaceDetection &det, const std::vector<rfd_image> &imgs, const rfd_image *dst, const rfd_dets &dets,
                                const uint32_t *sel, const rfd_redact_config *cfg, int32_t *applied = nullptr, bool async = false)
{
    check(rfd_redact_faces_device(det.raw(), imgs.data(), dst, (int)imgs.size(), &dets, sel, cfg, applied, async ? 1 : 0));
}

// ---- annotation (rfd.h, "annotation"): box outlines, landmarks and text labels drawn into frames ----
inline rfd_annotate_config annotate_default_config()
{
    rfd_annotate_config c;
    check(rfd_annotate_config_default(&c));
    return c;
}
// The seven rows of glyph 0 .. 13 of the library's font (0-9 - ? % space), top first, bit 4 the left column.
inline std::array<uint8_t, 7> annotate_glyph(int glyph)
{
    std::array<uint8_t, 7> rows{};
    check(rfd_debug_annotate_glyph(glyph, rows.data()));
    return rows;
}
// Host frames[i] with their detections dets[i] as call_batch returns them (boxes, landmarks, scores), drawn into dst[i] (frames
// of the same sizes), or in place when dst is empty: the frames' data is then written through.  sel, label, value: empty, or one
// entry per frame and row (rfd.h); cfg = nullptr: the default.  -> applied per frame.
inline std::vector<int32_t> annotate_faces(RetinaFaceDetection &det, const std::vector<rfd_image> &frames, const std::vector<rfd_image> &dst,
                                           const std::vector<Detections> &dets, const std::vector<std::vector<uint32_t>> &sel = {},
                                           const std::vector<std::vector<int32_t>> &label = {}, const std::vector<std::vector<float>> &value = {},
                                           const rfd_annotate_config *cfg = nullptr)
{
    const std::size_t n = frames.size(), md = det.max_det();
    if (dets.size() != n) throw Error(RFD_ERR_INVALID_ARG, "annotate faces - one detection list per frame");
    if (!dst.empty() && dst.size() != n) throw Error(RFD_ERR_INVALID_ARG, "annotate faces - one dst per frame, or none");
    if ((!sel.empty() && sel.size() != n) || (!label.empty() && label.size() != n) || (!value.empty() && value.size() != n))
        throw Error(RFD_ERR_INVALID_ARG, "annotate faces - one sel, label and value list per frame, or none");
    std::vector<float> boxes(n * md * 5), lmk(n * md * 10), values(value.empty() ? 0 : n * md);
    std::vector<int32_t> count(n), applied(n), labels(label.empty() ? 0 : n * md);
    std::vector<uint32_t> words(sel.empty() ? 0 : n * md);
    for (std::size_t i = 0; i < n; ++i) {
        const std::size_t k = std::min(dets[i].k, md);
        std::copy(dets[i].det.begin(), dets[i].det.begin() + (std::ptrdiff_t)(k * 5), boxes.begin() + (std::ptrdiff_t)(i * md * 5));
        std::copy(dets[i].kps.begin(), dets[i].kps.begin() + (std::ptrdiff_t)(k * 10), lmk.begin() + (std::ptrdiff_t)(i * md * 10));
        count[i] = (int32_t)k;
        if (!sel.empty()) std::copy_n(sel[i].begin(), std::min(sel[i].size(), md), words.begin() + (std::ptrdiff_t)(i * md));
        if (!label.empty()) std::copy_n(label[i].begin(), std::min(label[i].size(), md), labels.begin() + (std::ptrdiff_t)(i * md));
        if (!value.empty()) std::copy_n(value[i].begin(), std::min(value[i].size(), md), values.begin() + (std::ptrdiff_t)(i * md));
    }
    const rfd_dets d{boxes.data(), lmk.data(), count.data(), nullptr};
    check(rfd_annotate_faces(det.raw(), frames.data(), dst.empty() ? nullptr : dst.data(), (int)n, &d, sel.empty() ? nullptr : words.data(),
                             label.empty() ? nullptr : labels.data(), value.empty() ? nullptr : values.data(), cfg, applied.data()));
    return applied;
}
// DEVICE frames, slabs, sel, label, value and applied (each may be null where rfd.h lets it; dst null: in place), enqueued on the
// detector's stream; async: no host synchronisation.  The tracker's flags or `who` array is a ready `sel`, `identity` a ready
// `label`, `id_score` a ready `value`.
inline void annotate_faces_device(RetinaFaceDetection &det, const std::vector<rfd_image> &imgs, const rfd_image *dst, const rfd_dets &dets,
                                  const uint32_t *sel, const int32_t *label, const float *value, const rfd_annotate_config *cfg,
                                  int32_t *applied = nullptr, bool async = false)
{
    check(rfd_annotate_faces_device(det.raw(), imgs.data(), dst, (int)imgs.size(), &dets, sel, label, value, cfg, applied, async ? 1 : 0));
}

} // namespace rfd
#endif
