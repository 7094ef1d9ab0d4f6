// gallery_file_check.cpp -- the gallery file parser (csrc/gallery_file.h) alone, built with the host compiler under
// -fsanitize=address,undefined by tests/test_gallery_file_cpu.py and run as a program: a valid file, every malformed case of
// rfd.h's "gallery file" with its status, and the valid file cut at every byte.  No HIP, no device, nothing loaded into Python.
//   usage: gallery_file_check <scratch directory>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../rs-face-detection_amd/csrc/gallery_file.h"

static int failures = 0;

static void write_file(const std::string &path, const std::vector<unsigned char> &bytes)
{
    FILE *f = fopen(path.c_str(), "wb");
    if (!f || (bytes.size() && fwrite(bytes.data(), 1, bytes.size(), f) != bytes.size())) { std::perror(path.c_str()); std::exit(2); }
    fclose(f);
}

static void expect(const std::string &path, const std::vector<unsigned char> &bytes, int status, const char *needle, const char *what)
{
    write_file(path, bytes);
    int dim = -1, rows = -1, live = -1;
    char msg[256] = "";
    const int st = rfd::gallery_file_info(path.c_str(), &dim, &rows, &live, msg, sizeof msg);
    const bool ok = st == status && (status == RFD_OK || std::string(msg).find(needle) != std::string::npos);
    if (!ok) {
        ++failures;
        std::printf("FAIL %s: status %d (want %d), message \"%s\" (want \"%s\")\n", what, st, status, msg, needle);
    }
}

int main(int argc, char **argv)
{
    if (argc < 2) { std::fprintf(stderr, "usage: %s <scratch directory>\n", argv[0]); return 2; }
    const std::string path = std::string(argv[1]) + "/check.rfdg";
    // dim 32, 11 rows, rows 1 and 9 removed; values 1.0 (0x3f80), zeros in the removed rows
    const int dim = 32, rows = 11;
    std::vector<unsigned char> good = {'R', 'F', 'D', 'G', 1, 0, 0, 0, 32, 0, 0, 0, 11, 0, 0, 0, 0, 0, 0, 0, 0xfd, 0x05};
    for (int r = 0; r < rows; ++r)
        for (int d = 0; d < dim; ++d) {
            const bool live = r != 1 && r != 9;
            good.push_back(live ? 0x80 : 0);
            good.push_back(live ? 0x3f : 0);
        }
    expect(path, good, RFD_OK, "", "valid file");
    {
        int d = 0, r = 0, l = 0;
        char msg[256];
        if (rfd::gallery_file_info(path.c_str(), &d, &r, &l, msg, sizeof msg) != RFD_OK || d != 32 || r != 11 || l != 9) {
            ++failures;
            std::printf("FAIL valid file: dim %d rows %d live %d\n", d, r, l);
        }
    }
    auto with = [&](size_t at, unsigned char v) { std::vector<unsigned char> b = good; b[at] = v; return b; };
    expect(path, with(0, 'X'), RFD_ERR_INVALID_ARG, "magic", "wrong magic");
    expect(path, with(4, 2), RFD_ERR_INVALID_ARG, "version", "wrong version");
    expect(path, with(8, 48), RFD_ERR_INVALID_ARG, "dim", "dim 48");
    expect(path, with(8, 0), RFD_ERR_INVALID_ARG, "dim", "dim 0");
    expect(path, with(9, 8), RFD_ERR_INVALID_ARG, "dim", "dim 2080");
    expect(path, with(16, 1), RFD_ERR_INVALID_ARG, "reserved", "reserved field");
    expect(path, with(12, 12), RFD_ERR_INVALID_ARG, "length", "rows 12 in the header");
    expect(path, with(15, 0x7f), RFD_ERR_INVALID_ARG, "rows", "rows beyond 2^30");
    expect(path, with(21, 0x0d), RFD_ERR_INVALID_ARG, "beyond", "liveness bit of row 11");
    expect(path, with(22 + 2 * (4 * dim + 7) + 1, 0x7f), RFD_ERR_INVALID_ARG, "row 4", "infinity in row 4");
    expect(path, with(22 + 2 * (4 * dim + 7) + 1, 0x7f), RFD_ERR_INVALID_ARG, "element 7", "infinity at element 7");
    expect(path, with(22 + 2 * (10 * dim + 31) + 1, 0xff), RFD_ERR_INVALID_ARG, "row 10", "NaN in the last value");
    {
        std::vector<unsigned char> longer = good;
        longer.push_back(0);
        expect(path, longer, RFD_ERR_INVALID_ARG, "length", "one byte too many");
    }
    for (size_t cut = 0; cut < good.size(); ++cut) // every truncation, the empty file included
        expect(path, std::vector<unsigned char>(good.begin(), good.begin() + (long)cut), RFD_ERR_INVALID_ARG, "length", "truncated file");
    {
        char msg[256] = "";
        const int st = rfd::gallery_file_info((std::string(argv[1]) + "/no/such/file").c_str(), nullptr, nullptr, nullptr, msg, sizeof msg);
        if (st != RFD_ERR_IO || std::string(msg).find("cannot open") == std::string::npos) { ++failures; std::printf("FAIL missing path: status %d, \"%s\"\n", st, msg); }
    }
    // the writer's bytes are the hand-written ones
    {
        FILE *f = fopen(path.c_str(), "wb");
        const unsigned char bits[2] = {0xfd, 0x05};
        std::vector<uint16_t> v((size_t)rows * dim, 0x3f80);
        for (int d = 0; d < dim; ++d) v[(size_t)1 * dim + d] = v[(size_t)9 * dim + d] = 0;
        const bool ok = f && rfd::gallery_file_write_head(f, dim, rows, bits) && rfd::gallery_file_write_values(f, v.data(), v.size());
        if (f) fclose(f);
        std::vector<unsigned char> back(good.size() + 1);
        f = fopen(path.c_str(), "rb");
        const size_t n = f ? fread(back.data(), 1, back.size(), f) : 0;
        if (f) fclose(f);
        back.resize(n);
        if (!ok || back != good) { ++failures; std::printf("FAIL writer: %zu bytes, want %zu\n", n, good.size()); }
    }
    std::remove(path.c_str());
    std::printf("gallery_file_check: %d failures\n", failures);
    return failures ? 1 : 0;
}
