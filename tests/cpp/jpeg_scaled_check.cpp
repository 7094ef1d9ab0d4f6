// jpeg_scaled_check.cpp -- the host half of the reduced-size JPEG decode (csrc/jpeg_parse.h: the entropy decoder told each
// component's inverse-DCT size, jpeg_scaled_size, the block-count hook) alone, built with the host compiler under
// -fsanitize=address,undefined by tests/test_jpeg_scaled_cpu.py and run as a program.  For every file named on the command line and
// every denominator 1, 2, 4, 8: the whole file must decode, with every record inside the values written and no longer than at
// full size; the file cut at every byte, and the file with each single byte of its first 700 replaced by 0x00 and by 0xFF, must
// each return a status -- any status -- with the sanitizers silent.  The output buffers are heap blocks of exactly the documented
// size, so a write past them aborts the program.  No HIP, no device, nothing loaded into Python.
//   usage: jpeg_scaled_check <file.jpg>...
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../../rs-face-detection_amd/csrc/jpeg_parse.h"

static int failures = 0;
static long calls = 0, refused = 0;
static const int kDenoms[4] = {1, 2, 4, 8};

// parse + entropy-decode at 1 / denom as the library does; counts (may be null) receives the records' counts
static int decode(const std::vector<unsigned char> &bytes, int denom, std::vector<uint32_t> *counts)
{
    ++calls;
    std::unique_ptr<unsigned char[]> data(new unsigned char[bytes.size() ? bytes.size() : 1]); // exact size: a read past the file is a heap overflow
    std::copy(bytes.begin(), bytes.end(), data.get());
    std::unique_ptr<rfd::JpegHeader> h(new rfd::JpegHeader);
    int st = rfd::jpeg_parse_header(data.get(), bytes.size(), *h);
    if (st == RFD_OK && (uint64_t)h->nblocks * 64 <= rfd::kJpegMaxCoefs) {
        std::unique_ptr<uint32_t[]> rec(new uint32_t[(size_t)h->nblocks]);
        std::unique_ptr<int16_t[]> coef(new int16_t[(size_t)h->nblocks * 64]);
        uint32_t used = 0;
        int n[3];
        rfd::jpeg_idct_sizes(*h, denom, n);
        for (int c = 0; c < h->ncomp; ++c)
            if (n[c] != 8 && n[c] != 4 && n[c] != 2 && n[c] != 1) { ++failures; std::printf("FAIL size %d of component %d at 1/%d\n", n[c], c, denom); }
        st = rfd::jpeg_decode_scan(data.get(), bytes.size(), *h, rec.get(), coef.get(), &used, denom == 1 ? nullptr : n);
        if (st == RFD_OK) {
            if (used > (uint32_t)h->nblocks * 64) { ++failures; std::printf("FAIL %u values in %d blocks\n", used, h->nblocks); }
            if (counts) counts->assign((size_t)h->nblocks, 0);
            for (int b = 0; b < h->nblocks; ++b) {
                const uint32_t off = rec[b] >> rfd::kJpegRecCountBits, count = rec[b] & 127u;
                if (count > 64 || off + count > used) { ++failures; std::printf("FAIL record %d at 1/%d: offset %u count %u of %u\n", b, denom, off, count, used); break; }
                if (count && coef[off + count - 1] == 0) { ++failures; std::printf("FAIL record %d at 1/%d ends on a zero\n", b, denom); break; }
                if (counts) (*counts)[(size_t)b] = count;
            }
        }
    } else if (st == RFD_OK) st = RFD_ERR_CAPACITY;
    if (st != RFD_OK) {
        ++refused;
        if (st != RFD_ERR_INVALID_ARG && st != RFD_ERR_UNSUPPORTED && st != RFD_ERR_CAPACITY) { ++failures; std::printf("FAIL status %d\n", st); }
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
        std::vector<uint32_t> full, part;
        if (decode(good, 1, &full) != RFD_OK) { ++failures; std::printf("FAIL %s does not decode\n", argv[a]); continue; }
        for (int d = 0; d < 4; ++d) {
            const int denom = kDenoms[d];
            if (decode(good, denom, &part) != RFD_OK || part.size() != full.size()) { ++failures; std::printf("FAIL %s does not decode at 1/%d\n", argv[a], denom); continue; }
            for (size_t b = 0; b < full.size(); ++b)
                if (part[b] > full[b]) { ++failures; std::printf("FAIL %s block %zu: count %u at 1/%d, %u at full size\n", argv[a], b, part[b], denom, full[b]); break; }
            for (size_t cut = 0; cut < good.size(); ++cut) decode(std::vector<unsigned char>(good.begin(), good.begin() + (long)cut), denom, nullptr);
            const size_t head = good.size() < 700 ? good.size() : 700;
            for (size_t at = 0; at < head; ++at)
                for (int v = 0; v <= 0xff; v += 0xff) {
                    if (good[at] == v) continue;
                    std::vector<unsigned char> b = good;
                    b[at] = (unsigned char)v;
                    decode(b, denom, nullptr);
                }
            // the two helpers on the same input
            struct rfd_jpeg_scaled_size z;
            char msg[256];
            size_t blocks = 0;
            if (rfd::jpeg_scaled_size(good.data(), good.size(), denom, RFD_JPEG_ORIENTATION_APPLY, &z, msg, sizeof msg) != RFD_OK || z.denom != denom ||
                z.width < 1 || z.height < 1 || z.reserved[0] || z.reserved[1]) { ++failures; std::printf("FAIL jpeg_scaled_size: %s\n", msg); }
            std::memset(&z, 0x5a, sizeof z);
            if (rfd::jpeg_scaled_size(good.data(), good.size() / 4, denom, RFD_JPEG_ORIENTATION_APPLY, &z, msg, sizeof msg) == RFD_OK || z.width != 0x5a5a5a5a) { ++failures; std::printf("FAIL a refused file changed the struct\n"); }
            if (rfd::jpeg_debug_coefficients(good.data(), good.size(), nullptr, 0, &blocks, msg, sizeof msg, denom, nullptr) != RFD_ERR_CAPACITY || blocks != full.size()) { ++failures; std::printf("FAIL block count\n"); }
            std::unique_ptr<uint8_t[]> count(new uint8_t[blocks]);
            if (rfd::jpeg_debug_coefficients(good.data(), good.size(), nullptr, blocks, &blocks, msg, sizeof msg, denom, count.get()) != RFD_OK) { ++failures; std::printf("FAIL counts: %s\n", msg); }
            else
                for (size_t b = 0; b < blocks; ++b)
                    if (count[b] != part[b]) { ++failures; std::printf("FAIL the hook's count of block %zu\n", b); break; }
        }
    }
    std::printf("jpeg_scaled_check: %ld calls, %ld refused, %d failures\n", calls, refused, failures);
    return failures ? 1 : 0;
}
