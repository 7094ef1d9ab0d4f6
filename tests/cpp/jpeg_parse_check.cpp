// jpeg_parse_check.cpp -- the JPEG front end (csrc/jpeg_parse.h: marker parser and Huffman decoder) alone, built with the host
// compiler under -fsanitize=address,undefined by tests/test_jpeg_cpu.py and run as a program.  For every file named on the
// command line: the whole file must decode; the file cut at every byte, and the file with each single byte of its first 700
// replaced by 0x00 and by 0xFF, must each return a status -- any status -- with the sanitizers silent.  The output buffers are
// heap blocks of exactly the documented size, so a write past them aborts the program.  No HIP, no device, nothing loaded
// into Python.
//   usage: jpeg_parse_check <file.jpg>...
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "../../rs-face-detection_amd/csrc/jpeg_parse.h"

static int failures = 0;
static long calls = 0, refused = 0;

// parse + entropy-decode as the library does: records and coefficients sized from the header alone
static int decode(const std::vector<unsigned char> &bytes)
{
    ++calls;
    // an exact-size copy: a read past the end of the file is a heap overflow the sanitizer sees
    std::unique_ptr<unsigned char[]> data(new unsigned char[bytes.size() ? bytes.size() : 1]);
    std::copy(bytes.begin(), bytes.end(), data.get());
    std::unique_ptr<rfd::JpegHeader> h(new rfd::JpegHeader);
    int st = rfd::jpeg_parse_header(data.get(), bytes.size(), *h);
    if (st == RFD_OK && (uint64_t)h->nblocks * 64 > rfd::kJpegMaxCoefs) st = rfd::jpeg_decode_scan(data.get(), bytes.size(), *h, nullptr, nullptr, nullptr); // refused before it writes
    else if (st == RFD_OK) {
        std::unique_ptr<uint32_t[]> rec(new uint32_t[(size_t)h->nblocks]);
        std::unique_ptr<int16_t[]> coef(new int16_t[(size_t)h->nblocks * 64]);
        uint32_t used = 0;
        st = rfd::jpeg_decode_scan(data.get(), bytes.size(), *h, rec.get(), coef.get(), &used);
        if (st == RFD_OK) {
            if (used > (uint32_t)h->nblocks * 64) { ++failures; std::printf("FAIL %u values in %d blocks\n", used, h->nblocks); }
            for (int b = 0; b < h->nblocks; ++b) {
                const uint32_t off = rec[b] >> rfd::kJpegRecCountBits, count = rec[b] & 127u;
                if (count > 64 || off + count > used) { ++failures; std::printf("FAIL record %d: offset %u count %u of %u\n", b, off, count, used); break; }
            }
        }
    }
    if (st != RFD_OK) {
        ++refused;
        if (st != RFD_ERR_INVALID_ARG && st != RFD_ERR_UNSUPPORTED && st != RFD_ERR_CAPACITY) { ++failures; std::printf("FAIL status %d\n", st); }
        if (!h->msg[0]) { ++failures; std::printf("FAIL status %d without a message\n", st); }
    }
    return st;
}

int main(int argc, char **argv)
{
    if (argc < 2) { std::fprintf(stderr, "usage: %s <file.jpg>...\n", argv[0]); return 2; }
    for (int a = 1; a < argc; ++a) {
        FILE *f = std::fopen(argv[a], "rb");
        if (!f) { std::perror(argv[a]); return 2; }
        std::vector<unsigned char> good;
        for (int ch; (ch = std::fgetc(f)) != EOF;) good.push_back((unsigned char)ch);
        std::fclose(f);
        if (decode(good) != RFD_OK) { ++failures; std::printf("FAIL %s does not decode\n", argv[a]); continue; }
        for (size_t cut = 0; cut < good.size(); ++cut) decode(std::vector<unsigned char>(good.begin(), good.begin() + (long)cut));
        const size_t head = good.size() < 700 ? good.size() : 700;
        for (size_t at = 0; at < head; ++at)
            for (int v = 0; v <= 0xff; v += 0xff) {
                if (good[at] == v) continue;
                std::vector<unsigned char> b = good;
                b[at] = (unsigned char)v;
                decode(b);
            }
        // the two debug / info helpers on the same input
        struct rfd_jpeg_info info;
        char msg[256];
        size_t blocks = 0;
        if (rfd::jpeg_info(good.data(), good.size(), &info, msg, sizeof msg) != RFD_OK || info.width < 1) { ++failures; std::printf("FAIL jpeg_info: %s\n", msg); }
        if (rfd::jpeg_debug_coefficients(good.data(), good.size(), nullptr, 0, &blocks, msg, sizeof msg) != RFD_ERR_CAPACITY || blocks == 0) { ++failures; std::printf("FAIL block count\n"); }
        std::vector<int16_t> out(blocks * 64);
        if (rfd::jpeg_debug_coefficients(good.data(), good.size(), out.data(), blocks, &blocks, msg, sizeof msg) != RFD_OK) { ++failures; std::printf("FAIL coefficients: %s\n", msg); }
    }
    std::printf("jpeg_parse_check: %ld calls, %ld refused, %d failures\n", calls, refused, failures);
    return failures ? 1 : 0;
}
