#!/usr/bin/env python3
"""JPEG decode (rfd.h, "JPEG decode") on 32 files of 1920x1080, 4:2:0, quality 90.  Each figure from its own source:
  (a) host: wall time of an ASYNCHRONOUS rfd_decode_jpeg_batch_device call, which returns when the entropy decoding is done and
      the copies and kernels are enqueued, per batch and per frame at 1, 4 and 16 decode threads; and the wall time of the
      synchronous call (host clock around work that ends in a stream synchronise) as the end-to-end figure;
  (b) device: the two kernels' time from a CHILD run of this script under `rocprofv3 --kernel-trace --memory-copy-trace --stats`
      (a run of its own: tracing slows the host, so nothing else is timed there), jpeg_idct_kernel and jpeg_color_kernel read
      from the kernel statistics, against the HBM floor (<= 19 MB per frame over the streaming rate); the host-to-device copies
      of the same run as their own line against the PCIe link (63 GB/s), never against the HBM floor;
  (c) bytes that cross PCIe per frame (records + coefficients up to each block's last non-zero one), counted from the
      coefficients, against the 6.2 MB of a decoded frame;
  (d) Pillow's full decode time on the same host, where Pillow is installed, as the yardstick.
Files: generated with Pillow where it is installed, or every *.jpg of a directory given as the argument.
--entropy device selects RFD_JPEG_ENTROPY_DEVICE (rfd.h, "entropy decoding on the device"): (a) is then the call with the entropy
kernel inside, (b) adds jpeg_entropy_kernel, (c) counts the scan bytes and interval tables that cross PCIe instead, and the
per-frame paths are printed, so that a run in which the kernel never ran cannot pass for one.  --restart rows writes the
generated files with a restart interval of one MCU row (Pillow's restart_marker_rows = 1), --restart max with one of
kJpegDeviceMaxInterval MCUs (restart_marker_blocks); without it the files have no restart interval and stay on the host.
--orientation N (1..8, default 1) writes an Exif APP1 with that orientation into the generated files and selects
RFD_JPEG_ORIENTATION_APPLY (rfd.h, "EXIF orientation"), so that the colour stage of (b) is jpeg_color_oriented_kernel for 2..8;
the files of a directory keep the tags they have.  --no-host skips (a), (c) and (d): the traced child alone.
--scale D (1, 2, 4, 8; default 1) selects rfd_set_jpeg_scale(D) (rfd.h, "JPEG decode, reduced size"): the kernels of (b) are then
jpeg_idct_reduced_kernel and jpeg_color_scaled_kernel (jpeg_color_scaled_oriented_kernel for tagged files), each against the
floor of its OWN bytes; (c) counts the shortened runs; the plane and frame bytes per frame are printed.

    python tools/jpeg_bench.py [directory] [--files 32] [--reps 5] [--no-trace] [--entropy host|device] [--restart none|rows|max|MCUs]
                               [--orientation 1..8] [--scale 1|2|4|8] [--no-host]
Record the output in profiles/jpeg_decode.txt, profiles/jpeg_entropy_device.txt, profiles/jpeg_orientation.txt and
profiles/jpeg_scaled.txt."""
import argparse
import glob
import io
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rs-face-detection_amd", "python"))
STREAM_TBS = 6.3   # float4 copy rate of the chip, TB/s
MAX_INTERVAL = 128   # kJpegDeviceMaxInterval (csrc/jpeg_entropy.h)


def exif_app1(orientation):
    """an Exif APP1 segment whose IFD0 holds the orientation alone: "Exif\\0\\0", II, 42, IFD0 at 8, one SHORT entry"""
    import struct
    payload = b"Exif\0\0II" + struct.pack("<HIHHHIHHI", 42, 8, 1, 0x0112, 3, 1, orientation, 0, 0)
    return b"\xff\xe1" + struct.pack(">H", len(payload) + 2) + payload


def make_files(n, restart="none", orientation=1):
    from PIL import Image
    out = []
    for i in range(n):
        rng = np.random.default_rng(i)
        y, x = np.mgrid[0:1080, 0:1920]
        img = np.stack([(x * 255 // 1919), (y * 255 // 1079), ((x + y) * 255 // 2998)], -1).astype(np.float64)
        for _ in range(40):   # blobs and a noisy band: a photograph-like mix of smooth and busy blocks
            cx, cy, r = rng.integers(0, 1920), rng.integers(0, 1080), rng.integers(20, 200)
            img[(x - cx) ** 2 + (y - cy) ** 2 < r * r] = rng.integers(0, 256, 3)
        img[:, 1400:] += rng.normal(0, 12, (1080, 520, 3))
        buf = io.BytesIO()
        kw = {"none": {}, "rows": dict(restart_marker_rows=1), "max": dict(restart_marker_blocks=MAX_INTERVAL)}.get(restart) if not str(restart).isdigit() else dict(restart_marker_blocks=int(restart))
        Image.fromarray(np.clip(img, 0, 255).astype(np.uint8)).save(buf, "JPEG", quality=90, subsampling=2, **kw)
        data = buf.getvalue()
        out.append(data[:2] + exif_app1(orientation) + data[2:] if orientation != 1 else data)
    return out


def load_files(a):
    if a.directory:
        return [open(f, "rb").read() for f in sorted(glob.glob(os.path.join(a.directory, "*.jpg")))[:a.files]]
    return make_files(a.files, a.restart, a.orientation)


def plane_bytes(info, scale):
    """bytes of the component planes of one frame at 1 / scale: per block n x n samples, n per component as jdmaster.c chooses it"""
    h, v = {0: (1, 1), 1: (1, 1), 2: (2, 1), 3: (2, 2)}[info["sampling"]]
    mx, my = -(-info["width"] // (8 * h)), -(-info["height"] // (8 * v))
    m = 8 // scale
    luma = mx * h * my * v * m * m
    if info["components"] == 1:
        return luma
    n = 2 * m if (h, v) == (2, 2) and scale != 1 else m   # 4:2:0 chroma grows through its inverse DCT instead of being upsampled
    return luma + 2 * mx * my * n * n


def open_detector(R, files, entropy="host", orientation=1, scale=1):
    """the frames are allocated in the size the decode writes: the oriented one when --orientation selects APPLY, the scaled one
    when --scale is not 1"""
    import torch
    infos = [R.jpeg_info(f) for f in files]
    det = R.RetinaFaceDetection(max_batch_size=len(files), max_src=(max(i["width"] for i in infos), max(i["height"] for i in infos)))
    det.set_jpeg_entropy(entropy)
    if orientation != 1:
        det.set_jpeg_orientation("apply")
        infos = [dict(i, **{k: v for k, v in R.jpeg_orientation(f).items() if k in ("width", "height")}) for i, f in zip(infos, files)]
    if scale != 1:
        det.set_jpeg_scale(scale)
        mode = "apply" if orientation != 1 else "ignore"
        infos = [dict(i, **{k: v for k, v in R.jpeg_scaled_size(f, scale, mode).items() if k in ("width", "height")}) for i, f in zip(infos, files)]
    dev = torch.device("cuda", 0)
    bufs = [torch.zeros((i["height"], i["width"] * 3), dtype=torch.uint8, device=dev) for i in infos]
    torch.cuda.synchronize()
    return det, infos, bufs, [b.data_ptr() for b in bufs], [(i["height"], i["width"]) for i in infos]


def traced_child(a):
    """what runs under the profiler: one warm-up call, then --reps synchronous calls; prints how many calls it made"""
    import torch  # noqa: F401  (first: librfd_hip.so then binds to the HIP runtime torch ships)
    import rfd_hip as R
    files = load_files(a)
    det, infos, bufs, ptrs, shapes = open_detector(R, files, a.entropy, a.orientation, a.scale)
    for _ in range(1 + a.reps):
        det.decode_jpeg_device(files, ptrs, shapes)
    print("traced calls %d frames %d orientations %s" % (1 + a.reps, len(files), sorted(set(det.jpeg_last_orientations()))))
    det.close()


def read_stats(directory, suffix):
    """rows of the first *<suffix> under directory as dicts, or None"""
    import csv
    for d, _, fs in os.walk(directory):
        for f in sorted(fs):
            if f.endswith(suffix):
                with open(os.path.join(d, f), newline="") as fh:
                    return list(csv.DictReader(fh))
    return None


def scaled_kernel_lines(rows, a, infos, h2d_bytes_per_call):
    """(b) at --scale 2, 4, 8: each reduced kernel against the floor of its own bytes.  The inverse DCT reads the records and runs
    that crossed PCIe and writes the planes; the colour kernel reads the planes and writes the frames."""
    n = len(infos)
    planes = sum(plane_bytes(i, a.scale) for i in infos)
    frames = sum(-(-i["width"] // a.scale) * -(-i["height"] // a.scale) * 3 for i in infos)
    colour = "jpeg_color_scaled_kernel" if a.orientation == 1 else "jpeg_color_scaled_oriented_kernel"
    for name, moved in (("jpeg_entropy_kernel", None), ("jpeg_idct_reduced_kernel", h2d_bytes_per_call + planes), (colour, planes + frames)):
        hit = [x for x in rows if name in x["Name"]]
        if not hit:
            if moved is not None or a.entropy == "device":
                print("(b) %s is not in the kernel statistics" % name)
            continue
        us = float(hit[0]["AverageNs"]) / 1e3
        line = "(b) %s: %d launches, %.1f us per launch = %.2f us per frame (min %.1f, max %.1f us per launch)" % (
            name, int(hit[0]["Calls"]), us, us / n, float(hit[0]["MinNs"]) / 1e3, float(hit[0]["MaxNs"]) / 1e3)
        if moved is not None:
            floor = moved / (STREAM_TBS * 1e12) * 1e6
            line += "; its bytes %.1f MB per launch = %.2f TB/s, floor %.1f us at %.1f TB/s: %.0f %% of the floor's rate" % (
                moved / 1e6, moved / us / 1e6, floor, STREAM_TBS, 100 * floor / us)
        print(line)
    for other in ("jpeg_idct_kernel", "jpeg_color_kernel", "jpeg_color_oriented_kernel"):
        if [x for x in rows if other in x["Name"]]:
            print("(b) UNEXPECTED: %s ran in a scaled window" % other)


def kernel_pass(files, a, h2d_bytes_per_call, infos):
    """(b): a child of this script under rocprofv3, a process of its own started with subprocess; prints the figures"""
    import shutil
    import subprocess
    import tempfile
    exe = shutil.which("rocprofv3")
    if exe is None:
        print("(b) rocprofv3 is not installed here: kernel time not measured")
        return
    tmp = tempfile.mkdtemp(prefix="rfd_jpeg_")
    try:
        for i, f in enumerate(files):
            with open(os.path.join(tmp, "%03d.jpg" % i), "wb") as fh:
                fh.write(f)
        out = os.path.join(tmp, "trace")
        r = subprocess.run([exe, "--kernel-trace", "--memory-copy-trace", "--stats", "--output-format", "csv", "-d", out, "--", sys.executable,
                            os.path.abspath(__file__), tmp, "--files", str(len(files)), "--reps", str(a.reps), "--entropy", a.entropy, "--orientation",
                            str(a.orientation), "--scale", str(a.scale), "--child"],
                           capture_output=True, text=True, timeout=600)
        if r.returncode != 0 or "traced calls" not in r.stdout:
            print("(b) the traced child failed (exit %d): kernel time not measured\n%s" % (r.returncode, (r.stdout + r.stderr)[-600:]))
            return
        calls, n = 1 + a.reps, len(files)
        rows = read_stats(out, "kernel_stats.csv")
        if not rows:
            print("(b) no kernel statistics were written: kernel time not measured")
            return
        floor_us = 19e6 / (STREAM_TBS * 1e12) * 1e6
        total = 0.0
        print("(b) %s" % [l for l in r.stdout.splitlines() if "traced calls" in l][0])
        if a.scale != 1:
            return scaled_kernel_lines(rows, a, infos, h2d_bytes_per_call)
        colour = "jpeg_color_kernel" if a.orientation == 1 else "jpeg_color_oriented_kernel"   # every file carries the same tag
        for name in ("jpeg_entropy_kernel", "jpeg_idct_kernel", "jpeg_color_kernel", "jpeg_color_oriented_kernel"):
            hit = [x for x in rows if name in x["Name"]]
            if not hit:
                if name == colour or name == "jpeg_idct_kernel" or (name == "jpeg_entropy_kernel" and a.entropy == "device"):
                    print("(b) %s is not in the kernel statistics" % name)
                continue
            us = float(hit[0]["AverageNs"]) / 1e3
            if name != "jpeg_entropy_kernel":   # the HBM floor below is that of the two parallel kernels
                total += us
            print("(b) %s: %d launches, %.1f us per launch = %.2f us per frame (min %.1f, max %.1f us per launch)" %
                  (name, int(hit[0]["Calls"]), us, us / n, float(hit[0]["MinNs"]) / 1e3, float(hit[0]["MaxNs"]) / 1e3))
        print("(b) idct + colour: %.2f us per frame against the HBM floor of %.1f us per frame (19 MB at %.1f TB/s): %.0f %% of the floor's rate" %
              (total / n, floor_us, STREAM_TBS, 100 * floor_us / (total / n) if total else 0))
        copies = read_stats(out, "memory_copy_stats.csv")
        h2d = [x for x in copies or [] if "HOST_TO_DEVICE" in x["Name"].upper() or "H2D" in x["Name"].upper()]
        if h2d:
            ns = sum(float(x["TotalDurationNs"]) for x in h2d) / calls
            print("(b) host-to-device copies: %.1f us per call for %.2f MB = %.1f GB/s against the 63 GB/s of the PCIe link" %
                  (ns / 1e3, h2d_bytes_per_call / 1e6, h2d_bytes_per_call / ns))
        else:
            print("(b) no host-to-device copy statistics were written: copy time not measured")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("directory", nargs="?")
    ap.add_argument("--files", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-trace", action="store_true", help="skip (b), the child run under rocprofv3")
    ap.add_argument("--entropy", choices=("host", "device"), default="host", help="where eligible files are entropy-decoded")
    ap.add_argument("--restart", default="none", help="restart interval of the generated files: none, rows (one MCU row), max (kJpegDeviceMaxInterval MCUs) or a number of MCUs")
    ap.add_argument("--orientation", type=int, choices=range(1, 9), default=1, help="EXIF orientation written into the generated files; 2..8 select APPLY mode")
    ap.add_argument("--scale", type=int, choices=(1, 2, 4, 8), default=1, help="rfd_set_jpeg_scale: decode at 1 / this")
    ap.add_argument("--no-host", action="store_true", help="skip (a), (c) and (d): only the child run under rocprofv3")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return traced_child(a)
    import torch  # noqa: F401  (first: librfd_hip.so then binds to the HIP runtime torch ships)
    import rfd_hip as R
    files = load_files(a)
    n = len(files)
    infos = stored = [R.jpeg_info(f) for f in files]   # stored: the files' own sizes, whatever size the frames below get
    print("%d files, %.0f KB each on average, first %dx%d sampling %d, orientation %d" %
          (n, sum(map(len, files)) / n / 1e3, infos[0]["width"], infos[0]["height"], infos[0]["sampling"], R.jpeg_orientation(files[0])["orientation"]))
    # (c) transport bytes: 4 per block + 2 per coefficient up to the last non-zero one of its block (in zigzag order)
    zz = np.argsort(np.array([0, 1, 5, 6, 14, 15, 27, 28, 2, 4, 7, 13, 16, 26, 29, 42, 3, 8, 12, 17, 25, 30, 41, 43, 9, 11, 18, 24, 31, 40, 44, 53, 10, 19, 23, 32,
                              39, 45, 52, 54, 20, 22, 33, 38, 46, 51, 55, 60, 21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63]))
    h2d = []
    for f in files:
        if a.scale != 1:   # the runs end at the last non-zero coefficient the reduced inverse DCT reads: the decoder's own counts
            counts = R.jpeg_block_counts(f, a.scale)
            h2d.append(counts.shape[0] * 4 + 2 * int(counts.astype(np.int64).sum()))
            continue
        nz = R.jpeg_coefficients(f)[:, zz] != 0
        h2d.append(nz.shape[0] * 4 + 2 * int(np.where(nz.any(1), 64 - np.argmax(nz[:, ::-1], 1), 0).sum()))
    decoded = [-(-i["width"] // a.scale) * -(-i["height"] // a.scale) * 3 for i in infos]
    print("scale 1/%d: %.3f MB of planes and %.3f MB of frame per frame (full size: %.3f and %.3f MB)" %
          (a.scale, np.mean([plane_bytes(i, a.scale) for i in infos]) / 1e6, np.mean(decoded) / 1e6, np.mean([plane_bytes(i, 1) for i in infos]) / 1e6,
           np.mean([i["width"] * i["height"] * 3 for i in infos]) / 1e6))
    if a.no_host:
        return kernel_pass(files, a, float(np.sum(h2d)) + n * 496, stored)
    print("(c) H2D bytes per frame: %.2f MB (records + truncated runs) against %.2f MB decoded = %.1f %%" %
          (np.mean(h2d) / 1e6, np.mean(decoded) / 1e6, 100 * np.sum(h2d) / np.sum(decoded)))
    det, infos, bufs, ptrs, shapes = open_detector(R, files, a.entropy, a.orientation, a.scale)
    det.decode_jpeg_device(files, ptrs, shapes)   # allocates the staging, loads the code objects
    paths = det.jpeg_last_paths()
    print("entropy mode %s, restart interval of the first file %d MCUs; paths of the batch: %d host, %d device, %d refused by the device" %
          (a.entropy, infos[0]["restart_interval"], paths.count(0), paths.count(1), paths.count(2)))
    if a.entropy == "device":   # (c) for the frames that took the device path: the scan bytes and 8 B per interval, plus one descriptor
        dev, scan = [], []
        for f, p in zip(files, paths):
            if p == 1:
                iv = R.jpeg_intervals(f)
                dev.append(iv[-1][1] - iv[0][0] + 8 * len(iv) + 8600)
                scan.append(len(iv))
        if dev:
            print("(c) device path: %.3f MB per frame (scan bytes + interval table + descriptor, %d intervals per frame) against %.2f MB on the host path = %.1f %%" %
                  (np.mean(dev) / 1e6, int(np.mean(scan)), np.mean(h2d) / 1e6, 100 * np.mean(dev) / np.mean(h2d)))
    for threads in (1, 4, 16):
        det.set_decode_threads(threads)
        enq, whole = [], []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            det.decode_jpeg_device(files, ptrs, shapes, async_=True)
            enq.append(time.perf_counter() - t0)
            det.sync()
            t0 = time.perf_counter()
            det.decode_jpeg_device(files, ptrs, shapes)
            whole.append(time.perf_counter() - t0)
        e, w = float(np.median(enq)) * 1e3, float(np.median(whole)) * 1e3
        print("(a) %2d threads: entropy decode + enqueue %.2f ms per batch of %d = %.3f ms per frame (min %.2f, max %.2f ms); synchronous call %.2f ms = %.0f frames/s" %
              (threads, e, n, e / n, min(enq) * 1e3, max(enq) * 1e3, w, n / w * 1e3))
    det.close()
    try:
        from PIL import Image
        t0 = time.perf_counter()
        for f in files:
            Image.open(io.BytesIO(f)).load()
        print("(d) Pillow full decode, one thread: %.2f ms per frame" % ((time.perf_counter() - t0) / n * 1e3))
    except ImportError:
        print("(d) Pillow is not installed here")
    if not a.no_trace:
        kernel_pass(files, a, float(np.sum(h2d)) + n * 496, stored)


if __name__ == "__main__":
    main()
