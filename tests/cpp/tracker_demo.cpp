// tracker_demo.cpp -- compiled-language user of the tracker through include/rfd.hpp: frames of detections from a file go through
// rfd::Tracker::update in calls of up to four frames, then a reset and one more round.  Prints every id, flag and, with %a, every
// shot quality, so that tests/test_tracker_cpp_gpu.py can compare with tests/tracker_ref.py bit for bit.
// usage: tracker_demo <boxes.f32 [n][rows][5]> <counts.i32 [n]> <streams.i32 [n]> <rows> <streams> <max_tracks> <iou_min>
//                     <max_missed> <min_score> <new_score> <min_hits> <improve>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>

#include "rfd.hpp"

template <class T> static std::vector<T> read_all(const char *path)
{
    std::ifstream f(path, std::ios::binary);
    const std::vector<char> b((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    std::vector<T> out(b.size() / sizeof(T));
    std::memcpy(out.data(), b.data(), out.size() * sizeof(T));
    return out;
}

static void print_tracks(rfd::Tracker &tracker, int streams)
{
    for (int s = 0; s < streams; ++s)
        for (const rfd_track &t : tracker.tracks(s))
            std::printf("state %d slot %d serial %d box %a %a %a %a missed %d hits %d shot %a\n", s, t.slot, t.serial, t.box[0], t.box[1], t.box[2],
                        t.box[3], t.missed, t.hits, t.shot_q);
}

static void run(rfd::Tracker &tracker, const std::vector<float> &boxes, const std::vector<int32_t> &counts, const std::vector<int32_t> &streams, std::size_t rows)
{
    const std::size_t n = counts.size();
    for (std::size_t at = 0; at < n; at += 4) {
        const std::size_t m = std::min<std::size_t>(4, n - at);
        std::vector<rfd::Detections> frames(m);
        for (std::size_t i = 0; i < m; ++i) {
            const std::size_t k = (std::size_t)counts[at + i];
            frames[i].k = k;
            frames[i].det.assign(boxes.begin() + (std::ptrdiff_t)((at + i) * rows * 5), boxes.begin() + (std::ptrdiff_t)((at + i) * rows * 5 + k * 5));
            frames[i].kps.assign(k * 10, 0.0f);
        }
        const std::vector<int32_t> st(streams.begin() + (std::ptrdiff_t)at, streams.begin() + (std::ptrdiff_t)(at + m));
        const std::vector<rfd::Tracker::Frame> res = tracker.update(st, frames);
        for (std::size_t i = 0; i < m; ++i) {
            const rfd::Tracker::Frame &f = res[i];
            std::printf("frame %zu stream %d matched %d born %d dropped %d track", at + i, st[i], f.matched, f.born, f.dropped);
            for (int32_t t : f.track) std::printf(" %d", t);
            std::printf(" flags");
            for (uint32_t t : f.flags) std::printf(" %u", t);
            std::printf(" ended");
            for (int32_t t : f.ended) std::printf(" %d", t);
            std::printf(" due");
            for (int32_t t : f.due) std::printf(" %d", t);
            std::printf("\n");
        }
    }
}

int main(int argc, char **argv)
{
    if (argc < 13) { std::fprintf(stderr, "usage: %s boxes.f32 counts.i32 streams.i32 rows streams max_tracks iou_min max_missed min_score new_score min_hits improve\n", argv[0]); return 2; }
    const std::vector<float> boxes = read_all<float>(argv[1]);
    const std::vector<int32_t> counts = read_all<int32_t>(argv[2]), streams = read_all<int32_t>(argv[3]);
    const std::size_t rows = (std::size_t)std::atoi(argv[4]);
    if (rows < 1 || streams.size() != counts.size() || boxes.size() != counts.size() * rows * 5) { std::fprintf(stderr, "sizes do not match\n"); return 2; }
    try {
        rfd::FaceDetectionConfig dc;
        dc.image_size = {128, 128};
        dc.max_batch_size = 4;
        rfd::RetinaFaceDetection det(dc, 0, (int)rows, 1);
        rfd_tracker_config cfg = rfd::Tracker::default_config(det);
        cfg.streams = std::atoi(argv[5]);
        cfg.max_tracks = std::atoi(argv[6]);
        cfg.iou_min = std::strtof(argv[7], nullptr);
        cfg.max_missed = std::atoi(argv[8]);
        cfg.min_score = std::strtof(argv[9], nullptr);
        cfg.new_score = std::strtof(argv[10], nullptr);
        cfg.min_hits = std::atoi(argv[11]);
        cfg.improve = std::strtof(argv[12], nullptr);
        rfd::Tracker tracker(det, cfg);
        run(tracker, boxes, counts, streams, rows);
        print_tracks(tracker, cfg.streams);
        tracker.reset(0);
        std::printf("reset 0\n");
        run(tracker, boxes, counts, streams, rows);
        print_tracks(tracker, cfg.streams);
        try {
            tracker.update({cfg.streams}, {rfd::Detections()}); // a stream outside [0, streams)
            std::printf("bad stream accepted\n");
        } catch (const rfd::Error &e) {
            std::printf("bad stream rejected %d\n", e.status);
        }
    } catch (const rfd::Error &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
