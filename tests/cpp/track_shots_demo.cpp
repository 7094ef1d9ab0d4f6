// track_shots_demo.cpp -- compiled-language user of the track shots through include/rfd.hpp: two tracks are born from one frame,
// three crops (two of them of one track) are offered with their q, both tracks miss the next frame and end, and the ended tracks
// are collected as records.  Prints every status, entry, record and crop byte, so that tests/test_track_shots_cpp_gpu.py can
// compare with tests/track_shots_ref.py.
// usage: track_shots_demo   (no arguments: the scenario is fixed; max_det 16, crops 4 x 3)
#include <cstdio>

#include "rfd.hpp"

static std::vector<float> grid_box(int k)
{
    const float x = 20.0f * (float)(k % 16), y = 20.0f * (float)(k / 16);
    return {x, y, x + 9.0f, y + 9.0f, 0.9f};
}

static void print_bytes(const char *what, int which, const uint8_t *p, std::size_t n)
{
    std::printf("%s %d", what, which);
    for (std::size_t i = 0; i < n; ++i) std::printf(" %u", (unsigned)p[i]);
    std::printf("\n");
}

int main()
{
    const int rows = 16;
    try {
        rfd::FaceDetectionConfig dc;
        dc.image_size = {128, 128};
        dc.max_batch_size = 4;
        rfd::RetinaFaceDetection det(dc, 0, rows, 1);
        rfd_tracker_config cfg = rfd::Tracker::default_config(det);
        cfg.iou_min = 0.5f; cfg.max_missed = 0; cfg.min_score = 0.5f; cfg.new_score = 0.5f; cfg.min_hits = 1; cfg.improve = 1.1f;
        rfd::Tracker tracker(det, cfg);
        try {
            tracker.shots(0);
            std::printf("not enabled accepted\n");
        } catch (const rfd::Error &e) {
            std::printf("not enabled rejected %d\n", e.status);
        }
        rfd_track_shot_config sc = rfd::Tracker::default_shot_config();
        std::printf("default %d %d\n", sc.crop_w, sc.crop_h);
        sc.crop_w = 4; sc.crop_h = 3;
        tracker.enable_shots(sc);
        try {
            tracker.enable_shots(sc);
            std::printf("second enable accepted\n");
        } catch (const rfd::Error &e) {
            std::printf("second enable rejected %d\n", e.status);
        }
        const std::size_t cb = tracker.shot_bytes();

        rfd::Detections frame;
        frame.k = 2;
        for (int k = 0; k < 2; ++k) {
            const std::vector<float> b = grid_box(k);
            frame.det.insert(frame.det.end(), b.begin(), b.end());
        }
        frame.kps.assign(2 * 10, 0.0f);
        const std::vector<rfd::Tracker::Frame> born = tracker.update({0}, {frame});
        std::printf("track");
        for (int32_t t : born[0].track) std::printf(" %d", t);
        std::printf("\n");

        // crops named 10, 11, 12: byte i of crop `tag` is (tag * 37 + i) % 251
        const std::vector<rfd::Tracker::Observation> obs = {{0, 0, 1}, {0, 1, 2}, {0, 5, 1}};
        std::vector<uint8_t> crops(3 * cb);
        for (std::size_t t = 0; t < 3; ++t)
            for (std::size_t i = 0; i < cb; ++i) crops[t * cb + i] = (uint8_t)(((10 + t) * 37 + i) % 251);
        const std::vector<int32_t> status = tracker.keep_shots({0}, obs, crops, {0.5f, 0.25f, 0.75f}, {}, {1000});
        std::printf("status");
        for (int32_t s : status) std::printf(" %d", s);
        std::printf("\n");
        for (const rfd_track_shot &e : tracker.shots(0))
            std::printf("entry slot %d serial %d shots %d kept %d q %a first %lld best %lld\n", e.slot, e.serial, e.shots, e.kept, e.q,
                        (long long)e.first_stamp, (long long)e.best_stamp);
        const std::vector<uint8_t> one = tracker.shot_crop(0, 1);
        print_bytes("crop", 1, one.data(), one.size());
        try {
            tracker.shot_crop(0, 9);
            std::printf("unknown serial accepted\n");
        } catch (const rfd::Error &e) {
            std::printf("unknown serial rejected %d\n", e.status);
        }

        rfd::Detections empty;
        empty.k = 0;
        const std::vector<rfd::Tracker::Frame> gone = tracker.update({0}, {empty});
        std::printf("ended");
        for (int32_t s : gone[0].ended) std::printf(" %d", s);
        std::printf("\n");
        const rfd::Tracker::Records recs = tracker.collect_ended({0}, gone, 4, {2000});
        std::printf("total %d first %d %d\n", recs.total, recs.first[0], recs.first[1]);
        for (std::size_t r = 0; r < recs.rec.size(); ++r) {
            const rfd_track_record &x = recs.rec[r];
            std::printf("record %zu stream %d serial %d frame %d shots %d kept %d q %a first %lld best %lld end %lld identity %d row %d score %a named %d\n", r,
                        x.stream, x.serial, x.frame, x.shots, x.kept, x.q, (long long)x.first_stamp, (long long)x.best_stamp, (long long)x.end_stamp,
                        x.identity, x.row, x.id_score, x.named);
            print_bytes("picture", (int)r, recs.crops.data() + r * cb, cb);
        }
    } catch (const rfd::Error &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
