// track_identity_demo.cpp -- compiled-language user of the track identities through include/rfd.hpp: three tracks are born from
// one frame, four observations (two of them of one track) are fused, the answers of a gallery search written by hand are
// labelled, and every row of the frame is asked who it is.  Prints every status and, with %a, every query element, score, weight
// and template element, so that tests/test_track_identity_cpp_gpu.py can compare with tests/track_identity_ref.py bit for bit.
// usage: track_identity_demo   (no arguments: the scenario is fixed; max_det 16, dim 96)
#include <cstdio>
#include <limits>

#include "rfd.hpp"

static std::vector<float> grid_box(int k)
{
    const float x = 20.0f * (float)(k % 16), y = 20.0f * (float)(k / 16);
    return {x, y, x + 9.0f, y + 9.0f, 0.9f};
}

int main()
{
    const int rows = 16, dim = 96;
    const float ninf = -std::numeric_limits<float>::infinity();
    try {
        rfd::FaceDetectionConfig dc;
        dc.image_size = {128, 128};
        dc.max_batch_size = 4;
        rfd::RetinaFaceDetection det(dc, 0, rows, 1);
        rfd_tracker_config cfg = rfd::Tracker::default_config(det);
        cfg.iou_min = 0.5f; cfg.max_missed = 0; cfg.min_score = 0.5f; cfg.new_score = 0.5f; cfg.min_hits = 1; cfg.improve = 1.1f;
        rfd::Tracker tracker(det, cfg);
        try {
            tracker.identities(0);
            std::printf("not enabled accepted\n");
        } catch (const rfd::Error &e) {
            std::printf("not enabled rejected %d\n", e.status);
        }
        rfd_track_identity_config ic = rfd::Tracker::default_identity_config();
        ic.dim = dim; ic.accept = 0.5f; ic.release = 0.25f; ic.margin = 0.125f;
        tracker.enable_identities(ic);
        try {
            tracker.enable_identities(ic);
            std::printf("second enable accepted\n");
        } catch (const rfd::Error &e) {
            std::printf("second enable rejected %d\n", e.status);
        }

        rfd::Detections frame;
        frame.k = 3;
        for (int k = 0; k < 3; ++k) {
            const std::vector<float> b = grid_box(k);
            frame.det.insert(frame.det.end(), b.begin(), b.end());
        }
        frame.kps.assign(3 * 10, 0.0f);
        const std::vector<rfd::Tracker::Frame> res = tracker.update({0}, {frame});
        std::printf("track");
        for (int32_t t : res[0].track) std::printf(" %d", t);
        std::printf("\n");

        // (3, 4), 2 e0, (0, 5, 12), 7 e1: tracks 1, 2, 3 and 2 again (slab row 5)
        const std::vector<rfd::Tracker::Observation> obs = {{0, 0, 1}, {0, 1, 2}, {0, 2, 3}, {0, 5, 2}};
        std::vector<float> emb(4 * (std::size_t)dim, 0.0f);
        emb[0] = 3.0f; emb[1] = 4.0f;
        emb[(std::size_t)dim] = 2.0f;
        emb[2 * (std::size_t)dim + 1] = 5.0f; emb[2 * (std::size_t)dim + 2] = 12.0f;
        emb[3 * (std::size_t)dim + 1] = 7.0f;
        const rfd::Tracker::Fused fused = tracker.fuse({0}, obs, emb, {1.0f, 3.0f, 2.0f, 4.0f});
        for (std::size_t t = 0; t < obs.size(); ++t) {
            std::printf("fuse %zu status %d query", t, fused.status[t]);
            for (int i = 0; i < dim; ++i) std::printf(" %a", fused.query[t * (std::size_t)dim + (std::size_t)i]);
            std::printf("\n");
        }
        // k = 2: named 7; below accept; an unlabelled row with an empty runner-up; the margin fails
        const std::vector<float> scores = {0.75f, 0.2f, 0.3f, 0.1f, 0.875f, ninf, 0.75f, 0.6875f};
        const std::vector<int32_t> grows = {3, 8, 3, 8, 4, -1, 5, 3}, ids = {7, 9, 7, 9, -1, -1, 8, 7};
        tracker.label({0}, obs, 2, scores, grows, ids, fused.status);
        const std::vector<rfd::Tracker::Who> who = tracker.who({0}, res);
        for (std::size_t r = 0; r < who[0].who.size(); ++r) std::printf("who %zu %u %d %a\n", r, who[0].who[r], who[0].identity[r], who[0].score[r]);
        for (const rfd_track_identity &e : tracker.identities(0))
            std::printf("entry slot %d serial %d identity %d row %d score %a named %d shots %d weight %a\n", e.slot, e.serial, e.identity, e.row, e.score,
                        e.named, e.shots, e.weight);
        const std::vector<float> tmpl = tracker.track_template(0, 2);
        std::printf("template 2");
        for (float v : tmpl) std::printf(" %a", v);
        std::printf("\n");
        try {
            tracker.track_template(0, 9);
            std::printf("unknown serial accepted\n");
        } catch (const rfd::Error &e) {
            std::printf("unknown serial rejected %d\n", e.status);
        }
    } catch (const rfd::Error &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
