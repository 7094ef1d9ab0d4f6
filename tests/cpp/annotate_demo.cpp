// annotate_demo.cpp -- compiled-language user of the annotation through include/rfd.hpp: two host frames of different sizes with
// three detection rows are annotated out of place with two styles, labels and values, then the first in place with the default
// config.  Prints the default config, the font, every applied count and every byte of the painted frames in hex, so that
// tests/test_annotate_cpp_gpu.py can compare with tests/annotate_ref.py.
// usage: annotate_demo   (no arguments: the scenario is fixed; max_det 16)
#include <cstdio>

#include "rfd.hpp"

static std::vector<uint8_t> pattern(int b, int h, int w)
{
    std::vector<uint8_t> f((std::size_t)h * w * 3);
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x)
            for (int c = 0; c < 3; ++c) f[((std::size_t)y * w + x) * 3 + c] = (uint8_t)((x * 7 + y * 13 + c * 5 + b * 31) % 251);
    return f;
}

static void print_frame(const char *what, int which, const std::vector<uint8_t> &f)
{
    std::printf("%s %d ", what, which);
    for (uint8_t v : f) std::printf("%02x", (unsigned)v);
    std::printf("\n");
}

static rfd::Detections rows(std::initializer_list<std::array<float, 15>> list)
{
    rfd::Detections d;
    for (const auto &r : list) {
        d.det.insert(d.det.end(), r.begin(), r.begin() + 5);
        d.kps.insert(d.kps.end(), r.begin() + 5, r.end());
        ++d.k;
    }
    return d;
}

int main()
{
    try {
        rfd::FaceDetectionConfig dc;
        dc.image_size = {128, 128};
        dc.max_batch_size = 4;
        rfd::RetinaFaceDetection det(dc, 0, 16, 1);
        rfd_annotate_config cfg = rfd::annotate_default_config();
        std::printf("default %d %d %d %d %d %d %d colour %u %u %u\n", cfg.n_styles, cfg.thickness, cfg.mark_radius, cfg.label_source, cfg.value_source,
                    cfg.text_scale, cfg.alpha, (unsigned)cfg.style[0].colour[0], (unsigned)cfg.style[0].colour[1], (unsigned)cfg.style[0].colour[2]);
        for (int g = 0; g < 14; ++g) {
            const std::array<uint8_t, 7> r = rfd::annotate_glyph(g);
            std::printf("glyph %d %u %u %u %u %u %u %u\n", g, (unsigned)r[0], (unsigned)r[1], (unsigned)r[2], (unsigned)r[3], (unsigned)r[4], (unsigned)r[5], (unsigned)r[6]);
        }
        try {
            rfd::annotate_glyph(14);
            std::printf("glyph 14 accepted\n");
        } catch (const rfd::Error &e) {
            std::printf("glyph 14 rejected %d\n", e.status);
        }

        const int H[2] = {40, 30}, W[2] = {50, 33};
        std::vector<std::vector<uint8_t>> src = {pattern(0, H[0], W[0]), pattern(1, H[1], W[1])};
        std::vector<std::vector<uint8_t>> out = {std::vector<uint8_t>(src[0].size(), 0xA5), std::vector<uint8_t>(src[1].size(), 0xA5)};
        std::vector<rfd_image> frames, dst;
        for (int b = 0; b < 2; ++b) {
            frames.push_back(rfd_image{src[b].data(), H[b], W[b], (ptrdiff_t)W[b] * 3});
            dst.push_back(rfd_image{out[b].data(), H[b], W[b], (ptrdiff_t)W[b] * 3});
        }
        // x1 y1 x2 y2 score, five landmarks
        const std::vector<rfd::Detections> dets = {
            rows({{5.5f, 14.0f, 30.25f, 33.0f, 0.875f, 10, 18, 20, 18, 15, 24, 11, 29, 19, 29},
                  {22.0f, 10.0f, 47.0f, 38.5f, 0.5f, 28, 15, 40, 15, 34, 22, 29, 30, 39, 30}}),
            rows({{-4.0f, 3.0f, 20.0f, 36.0f, 0.25f, 2, 10, 12, 10, 7, 15, 3, 20, 11, 20}}),
        };
        const std::vector<std::vector<uint32_t>> sel = {{2, 0}, {3}};
        const std::vector<std::vector<int32_t>> label = {{17, -1}, {204}};
        const std::vector<std::vector<float>> value = {{0.83f, 0.07f}, {1.5f}};
        cfg.n_styles = 2;
        cfg.style[0] = rfd_annotate_style{2, 2, {0, 0, 255, 0}};
        cfg.style[1] = rfd_annotate_style{0, 0, {255, 128, 0, 0}};
        cfg.thickness = 1; cfg.mark_radius = 1; cfg.label_source = RFD_ANNOTATE_ARRAY; cfg.value_source = RFD_ANNOTATE_ARRAY;
        cfg.text_scale = 1; cfg.alpha = 200;
        cfg.text_colour[0] = 255; cfg.text_colour[1] = 255; cfg.text_colour[2] = 255;
        std::vector<int32_t> applied = rfd::annotate_faces(det, frames, dst, dets, sel, label, value, &cfg);
        std::printf("applied %d %d\n", applied[0], applied[1]);
        for (int b = 0; b < 2; ++b) print_frame("dst", b, out[(std::size_t)b]);
        for (int b = 0; b < 2; ++b) print_frame("source", b, src[(std::size_t)b]);

        // in place, the default config: box, landmarks, score %
        applied = rfd::annotate_faces(det, {frames[0]}, {}, {dets[0]});
        std::printf("applied %d\n", applied[0]);
        print_frame("in place", 0, src[0]);

        cfg.thickness = 17;
        try {
            rfd::annotate_faces(det, frames, dst, dets, sel, label, value, &cfg);
            std::printf("thickness 17 accepted\n");
        } catch (const rfd::Error &e) {
            std::printf("thickness 17 rejected %d\n", e.status);
        }
    } catch (const rfd::Error &e) {
        std::fprintf(stderr, "rfd error %d: %s\n", e.status, e.what());
        return 1;
    }
    return 0;
}
