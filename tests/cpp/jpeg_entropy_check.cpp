// jpeg_entropy_check.cpp -- the interval decoder the device runs (csrc/jpeg_entropy.h: jpeg_decode_interval, one function for host
// and device) and the marker pre-scan, built with the host compiler under -fsanitize=address,undefined by
// tests/test_jpeg_entropy_cpu.py and run as a program.  Records, coefficients, interval tables and the file itself are heap
// blocks of exactly their size, so a read or write past them aborts the program.
//
// For every file on the command line, then for the file cut at every byte of its scan and with each of the first 700 scan bytes
// replaced by 0x00, 0xFF and 0xD0 in turn:
//   every interval the pre-scan finds is decoded by jpeg_decode_interval; it is either refused, or its blocks equal what the host
//   decoder (jpeg_parse.h: jpeg_decode_scan) makes of the same bytes taken as a scan of their own -- counts and coefficients;
//   where the file is eligible and no interval is refused, jpeg_decode_scan must accept the whole file with the same blocks.
// A file named before `--damaged` must itself be eligible and decode without a refusal; one named after it need not.
//   usage: jpeg_entropy_check <file.jpg>... [--damaged <file.jpg>...]
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../../rs-face-detection_amd/csrc/jpeg_entropy.h"

static int failures = 0;
static long calls = 0, intervals_run = 0, intervals_refused = 0, files_whole = 0;

static void fail(const char *what, long a = 0, long b = 0)
{
    if (++failures <= 20) std::printf("FAIL %s (%ld, %ld)\n", what, a, b);
}

// true: eligible and every interval accepted
static bool check(const std::vector<unsigned char> &bytes)
{
    using namespace rfd;
    ++calls;
    std::unique_ptr<unsigned char[]> data(new unsigned char[bytes.size() ? bytes.size() : 1]);
    std::copy(bytes.begin(), bytes.end(), data.get());
    const size_t len = bytes.size();
    std::unique_ptr<JpegHeader> h(new JpegHeader);
    if (jpeg_parse_header(data.get(), len, *h) != RFD_OK) return false;
    const int R = h->restart_interval, mcus = h->mcux * h->mcuy;
    if (R < 1 || (uint64_t)h->nblocks * 64 > kJpegMaxCoefs || h->nblocks > (1 << 16)) return false;
    const size_t want = ((size_t)mcus + (size_t)R - 1) / (size_t)R, nb = (size_t)h->nblocks;
    std::unique_ptr<uint32_t[]> begin(new uint32_t[want]), end(new uint32_t[want]);
    bool seq = true;
    const size_t found = jpeg_prescan(data.get(), len, h->scan, begin.get(), end.get(), want, &seq);
    for (size_t k = 0; k < found && k < want; ++k)
        if (begin[k] > end[k] || end[k] > len || begin[k] < h->scan || (k && begin[k] < end[k - 1] + 2)) fail("interval table", (long)k, (long)begin[k]);
    {   // the eligibility rule agrees with the pre-scan it is made of
        std::unique_ptr<uint32_t[]> b2(new uint32_t[want]), e2(new uint32_t[want]);
        size_t count = 0;
        char msg[200] = "";
        const bool el = jpeg_device_eligible(data.get(), len, *h, b2.get(), e2.get(), want, &count, msg, sizeof msg);
        if (el != (R <= kJpegDeviceMaxInterval && found == want && seq)) fail("eligibility", (long)found, (long)want);
        if (!el && !msg[0]) fail("not eligible without a message");
    }
    std::unique_ptr<uint32_t[]> rec(new uint32_t[nb]), hrec(new uint32_t[nb]), srec(new uint32_t[nb]);
    std::unique_ptr<int16_t[]> coef(new int16_t[nb * 64]), hcoef(new int16_t[nb * 64]), scoef(new int16_t[nb * 64]);
    uint32_t hused = 0;
    std::unique_ptr<JpegHeader> whole(new JpegHeader(*h)), strip(new JpegHeader(*h));
    const int hst = jpeg_decode_scan(data.get(), len, *whole, hrec.get(), hcoef.get(), &hused);
    JpegScanGeom g;
    std::unique_ptr<JpegDevHuff[]> tab(new JpegDevHuff[6]);
    jpeg_scan_geom(*h, g, tab.get(), tab.get() + 3);
    bool all = found == want && seq;
    for (size_t k = 0; k < found && k < want; ++k) {
        const int mcu0 = (int)k * R, mcu1 = mcu0 + R < mcus ? mcu0 + R : mcus, nm = mcu1 - mcu0;
        ++intervals_run;
        if (!jpeg_decode_interval(data.get(), begin[k], end[k], mcu0, mcu1, g, tab.get(), tab.get() + 3, rec.get(), coef.get())) {
            ++intervals_refused;
            all = false;
            continue;
        }
        // the host decoder on the interval's bytes as a scan of their own: nm MCUs in one row
        strip->restart_interval = 0;
        strip->mcux = nm; strip->mcuy = 1;
        strip->nblocks = 0;
        for (int c = 0; c < h->ncomp; ++c) {
            strip->comp[c].bw = nm * h->comp[c].h; strip->comp[c].bh = h->comp[c].v;
            strip->comp[c].blk0 = strip->nblocks;
            strip->nblocks += strip->comp[c].bw * strip->comp[c].bh;
        }
        strip->scan = begin[k];
        uint32_t sused = 0;
        if (jpeg_decode_scan(data.get(), end[k], *strip, srec.get(), scoef.get(), &sused) != RFD_OK) { fail("accepted an interval the host decoder refuses", (long)k); continue; }
        for (int j = 0; j < nm; ++j) {
            const int mcu = mcu0 + j, my = mcu / h->mcux, mx = mcu - my * h->mcux;
            for (int c = 0; c < h->ncomp; ++c) {
                const JpegComponent &q = h->comp[c], &s = strip->comp[c];
                for (int v = 0; v < q.v; ++v)
                    for (int u = 0; u < q.h; ++u) {
                        const int blk = q.blk0 + (my * q.v + v) * q.bw + mx * q.h + u, sb = s.blk0 + v * s.bw + j * q.h + u;
                        const uint32_t count = rec[blk] & 127u, off = rec[blk] >> kJpegRecCountBits;
                        if (off != (uint32_t)blk * 64 || count > 64) { fail("record", blk, (long)rec[blk]); continue; }
                        if (count != (srec[sb] & 127u)) { fail("count", blk, (long)count); continue; }
                        if (std::memcmp(coef.get() + off, scoef.get() + (srec[sb] >> kJpegRecCountBits), count * sizeof(int16_t))) fail("coefficients", blk, (long)k);
                    }
            }
        }
    }
    if (all) {
        ++files_whole;
        if (hst != RFD_OK) fail("every interval accepted, the host decoder refuses the file");
        else
            for (size_t b = 0; b < nb; ++b) {
                const uint32_t count = rec[b] & 127u;
                if (count != (hrec[b] & 127u) || std::memcmp(coef.get() + (rec[b] >> kJpegRecCountBits), hcoef.get() + (hrec[b] >> kJpegRecCountBits), count * sizeof(int16_t))) {
                    fail("whole file", (long)b);
                    break;
                }
            }
    }
    return all;
}

int main(int argc, char **argv)
{
    if (argc < 2) { std::fprintf(stderr, "usage: %s <file.jpg>... [--damaged <file.jpg>...]\n", argv[0]); return 2; }
    bool damaged = false;
    for (int a = 1; a < argc; ++a) {
        if (!std::strcmp(argv[a], "--damaged")) { damaged = true; continue; }
        FILE *f = std::fopen(argv[a], "rb");
        if (!f) { std::perror(argv[a]); return 2; }
        std::vector<unsigned char> good;
        for (int ch; (ch = std::fgetc(f)) != EOF;) good.push_back((unsigned char)ch);
        std::fclose(f);
        if (!check(good) && !damaged) { fail("a good file is not eligible, or an interval of it is refused"); std::printf("     %s\n", argv[a]); continue; }
        std::unique_ptr<rfd::JpegHeader> h(new rfd::JpegHeader);
        if (rfd::jpeg_parse_header(good.data(), good.size(), *h) != RFD_OK) { if (!damaged) fail("header"); continue; }
        for (size_t cut = h->scan; cut < good.size(); ++cut) check(std::vector<unsigned char>(good.begin(), good.begin() + (long)cut));
        const size_t head = good.size() - h->scan < 700 ? good.size() - h->scan : 700;
        const int values[3] = {0x00, 0xff, 0xd0};
        for (size_t at = h->scan; at < h->scan + head; ++at)
            for (int v : values) {
                if (good[at] == v) continue;
                std::vector<unsigned char> b = good;
                b[at] = (unsigned char)v;
                check(b);
            }
    }
    std::printf("jpeg_entropy_check: %ld inputs, %ld whole, %ld intervals, %ld refused, %d failures\n", calls, files_whole, intervals_run, intervals_refused, failures);
    return failures ? 1 : 0;
}
