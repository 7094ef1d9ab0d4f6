// kernels_jpeg_entropy.hip -- Huffman decoding of restart-interval JPEG files on the device (rfd.h, "JPEG decode",
// RFD_JPEG_ENTROPY_DEVICE), gfx950.
//
// One launch per batch.  One THREAD decodes one restart interval with jpeg_decode_interval (csrc/jpeg_entropy.h), the same
// function the host check program runs under the sanitizers: intervals are independent by construction (byte-aligned, DC
// predictors zero), so no thread waits for another, no workgroup for another workgroup, and every loop is bounded by the
// interval's bytes.  A workgroup is one wave that serves 64 consecutive intervals of ONE frame; it finds the frame in the
// descriptor table by its own index, as the IDCT and colour kernels do, and stages that frame's Huffman tables (per component
// DC and AC: fast[512], maxcode, valoff, vals) in LDS once.  A thread writes its blocks' coefficients and records straight into
// the frame's slice of the pools the IDCT kernel reads (dense layout: block b at coef[b * 64]); a refused interval ORs a 1 into
// the frame's status word with an ordinary vector atomic, and the host then decodes that frame itself.
// The 2-byte coefficient stores of neighbouring lanes are far apart (uncoalesced); profiles/jpeg_entropy_device.txt.
#include "jpeg_entropy.h"
#include "kernels.h"

namespace rfd {

namespace {

constexpr int kHuffWords = (int)(sizeof(JpegDevHuff) / 4);

__global__ __launch_bounds__(kJpegEntropyGroup) void jpeg_entropy_kernel(JpegEntropyParams p)
{
    __shared__ JpegDevHuff tab[6]; // dc[3] | ac[3]
    const int g = blockIdx.x;
    int lo = 0, hi = p.n - 1; // the frame whose first workgroup is the last one <= g
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (p.frames[mid].group0 <= g) lo = mid; else hi = mid - 1;
    }
    const JpegEntropyFrame &f = p.frames[lo];
    {
        const uint32_t *src = reinterpret_cast<const uint32_t *>(f.dc);
        uint32_t *dst = reinterpret_cast<uint32_t *>(tab);
        for (int i = (int)threadIdx.x; i < 6 * kHuffWords; i += kJpegEntropyGroup) dst[i] = src[i];
    }
    __syncthreads();
    const int k = (g - f.group0) * kJpegEntropyGroup + (int)threadIdx.x;
    if (k >= f.intervals) return;
    const uint32_t *iv = p.intervals + f.interval0;
    const uint32_t begin = iv[k] - f.file_scan, end = iv[f.intervals + k] - f.file_scan;
    const int mcu0 = k * f.geom.restart, mcu1 = min(mcu0 + f.geom.restart, f.geom.mcus);
    // begin <= end <= scan_bytes by the pre-scan; checked again so that a damaged table cannot make the reader leave the pool
    const bool ok = begin <= end && end <= f.scan_bytes &&
                    jpeg_decode_interval(p.scan + f.scan0, begin, end, mcu0, mcu1, f.geom, tab, tab + 3, p.rec + f.rec0, p.coef + f.rec0 * 64);
    if (!ok) atomicOr(p.status + f.frame, 1u);
}

} // namespace

int launch_jpeg_entropy(const JpegEntropyParams &p, hipStream_t s)
{
    if (p.n < 1) return RFD_OK;
    hipLaunchKernelGGL(jpeg_entropy_kernel, dim3((unsigned)p.groups), dim3(kJpegEntropyGroup), 0, s, p);
    RFD_HIP(hipGetLastError());
    return RFD_OK;
}

} // namespace rfd
