// jpeg_exif_check.cpp -- the EXIF reader of the JPEG front end (csrc/jpeg_parse.h: jpeg_exif_orientation under jpeg_parse_header)
// alone, built with the host compiler under -fsanitize=address,undefined by tests/test_jpeg_orientation_cpu.py and run as a
// program.  The file named on the command line carries an Exif APP1 segment whose payload is bytes [at, at + n) of the file.
// Every payload byte is replaced by 0x00, 0x7F, 0x80 and 0xFF in turn, and the payload is cut at every length 0 .. n with the
// segment's length field adjusted to match, so that the file stays well-formed around it.  Each run must return RFD_OK with the
// stored size unchanged and an orientation in 1 .. 8: EXIF damage never refuses a file.  The input of every run is a heap block
// of exactly the file's size, so a read past it aborts the program.  No HIP, no device, nothing loaded into Python.
//   usage: jpeg_exif_check <file.jpg> <payload offset> <payload length>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "../../rs-face-detection_amd/csrc/jpeg_parse.h"

static int failures = 0;
static long calls = 0, upright = 0;
static int width = 0, height = 0;

static void check(const std::vector<unsigned char> &bytes, const char *what, size_t k, int v)
{
    ++calls;
    std::unique_ptr<unsigned char[]> data(new unsigned char[bytes.size()]);
    std::copy(bytes.begin(), bytes.end(), data.get());
    struct rfd_jpeg_orientation o;
    char msg[256] = "";
    const int st = rfd::jpeg_orientation(data.get(), bytes.size(), &o, msg, sizeof msg);
    if (st != RFD_OK) { ++failures; std::printf("FAIL %s %zu (0x%02x): status %d, %s\n", what, k, v, st, msg); return; }
    if (o.stored_width != width || o.stored_height != height) { ++failures; std::printf("FAIL %s %zu (0x%02x): stored size %d x %d\n", what, k, v, o.stored_width, o.stored_height); }
    if (o.orientation < 1 || o.orientation > 8) { ++failures; std::printf("FAIL %s %zu (0x%02x): orientation %d\n", what, k, v, o.orientation); }
    const bool swapped = o.orientation >= 5;
    if (o.width != (swapped ? height : width) || o.height != (swapped ? width : height)) { ++failures; std::printf("FAIL %s %zu (0x%02x): oriented size %d x %d\n", what, k, v, o.width, o.height); }
    upright += o.orientation == 1;
}

int main(int argc, char **argv)
{
    if (argc != 4) { std::fprintf(stderr, "usage: %s <file.jpg> <payload offset> <payload length>\n", argv[0]); return 2; }
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) { std::perror(argv[1]); return 2; }
    std::vector<unsigned char> good;
    for (int ch; (ch = std::fgetc(f)) != EOF;) good.push_back((unsigned char)ch);
    std::fclose(f);
    const size_t at = (size_t)std::strtoul(argv[2], nullptr, 10), n = (size_t)std::strtoul(argv[3], nullptr, 10);
    if (at < 6 || at + n > good.size() || good[at - 4] != 0xff || good[at - 3] != 0xe1 || ((size_t)good[at - 2] << 8 | good[at - 1]) != n + 2) {
        std::fprintf(stderr, "bytes [%zu, %zu) are not the payload of an APP1 segment\n", at, at + n);
        return 2;
    }
    struct rfd_jpeg_orientation o;
    char msg[256] = "";
    if (rfd::jpeg_orientation(good.data(), good.size(), &o, msg, sizeof msg) != RFD_OK || o.orientation == 1) {
        std::printf("FAIL the file itself: %s, orientation %d\n", msg, o.orientation);
        return 1;
    }
    width = o.stored_width; height = o.stored_height;
    static const int values[4] = {0x00, 0x7f, 0x80, 0xff};
    for (size_t k = 0; k < n; ++k)
        for (int v : values) {
            if (good[at + k] == v) continue;
            std::vector<unsigned char> b = good;
            b[at + k] = (unsigned char)v;
            check(b, "byte", k, v);
        }
    for (size_t cut = 0; cut <= n; ++cut) {
        std::vector<unsigned char> b(good.begin(), good.begin() + (long)(at + cut));
        b[at - 2] = (unsigned char)((cut + 2) >> 8); b[at - 1] = (unsigned char)(cut + 2);
        b.insert(b.end(), good.begin() + (long)(at + n), good.end());
        check(b, "cut", cut, 0);
    }
    std::printf("jpeg_exif_check: %ld calls, %ld upright, %d failures\n", calls, upright, failures);
    return failures ? 1 : 0;
}
