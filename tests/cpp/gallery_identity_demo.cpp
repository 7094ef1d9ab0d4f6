// gallery_identity_demo.cpp -- compiled-language user of the gallery's identity calls through include/rfd.hpp: enrol rows,
// label them, search the k best identities, remove a row, search again.  Prints every score with %.9g so that
// tests/test_gallery_identity_cpp_gpu.py can compare bit for bit with tests/gallery_identity_ref.py.
// usage: gallery_identity_demo <gallery.f32> <queries.f32> <ids.i32> <dim> <k> <min_score> <row to remove>
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

static void print(const char *tag, const rfd::Gallery::IdentityMatches &m)
{
    for (int q = 0; q < m.n; ++q) {
        std::printf("%s %d", tag, q);
        for (int j = 0; j < m.k; ++j) {
            const std::size_t at = (std::size_t)q * (std::size_t)m.k + (std::size_t)j;
            std::printf(" %.9g %d %d", m.scores[at], m.rows[at], m.ids[at]);
        }
        std::printf("\n");
    }
}

int main(int argc, char **argv)
{
    if (argc < 8) { std::fprintf(stderr, "usage: %s gallery.f32 queries.f32 ids.i32 dim k min_score remove_row\n", argv[0]); return 2; }
    const std::vector<float> g = read_all<float>(argv[1]), q = read_all<float>(argv[2]);
    const std::vector<int32_t> ids = read_all<int32_t>(argv[3]);
    const int dim = std::atoi(argv[4]), k = std::atoi(argv[5]), gone = std::atoi(argv[7]);
    const float min_score = std::strtof(argv[6], nullptr);
    const int rows = (int)ids.size();
    if (dim < 1 || g.size() != (std::size_t)rows * (std::size_t)dim) { std::fprintf(stderr, "sizes do not match\n"); return 2; }
    try {
        rfd::RetinaFaceDetection det(rfd::FaceDetectionConfig(), 0, 16, 1);
        rfd::Gallery gallery(det, dim, rows);
        std::printf("first %d\n", gallery.add(g));
        print("unlabelled", gallery.search_identities(q, k));          // the plain search plus ids = -1
        std::vector<int32_t> all((std::size_t)rows);
        for (int r = 0; r < rows; ++r) all[(std::size_t)r] = r;
        gallery.set_identities(all, ids);
        std::printf("labelled %d\n", gallery.labelled());
        print("all", gallery.search_identities(q, k));
        print("min", gallery.search_identities(q, k, min_score));
        gallery.remove({gone});
        std::printf("labelled %d identity %d\n", gallery.labelled(), gallery.identities(gone, 1)[0]);
        print("removed", gallery.search_identities(q, k));
        try {
            gallery.set_identities({gone}, {3});                        // a removed row cannot be labelled
            std::printf("removed row accepted\n");
        } catch (const rfd::Error &e) {
            std::printf("removed row rejected %d\n", e.status);
        }
    } catch (const rfd::Error &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
