#!/usr/bin/env python3
"""Frame conversion (rfd.h, "frames in camera and decoder formats") on 32 frames of 1920x1080 per call.  Each figure from its own
source:
  (a) device: frame_convert_kernel's time per launch for NV12, I420, YUYV and BGRA from a CHILD run of this script under
      `rocprofv3 --kernel-trace` (a run of its own: tracing slows the host, so nothing else is timed there).  The child makes
      1 + --reps rfd_convert_frames_device calls per format, in that order, so the dispatches of the one kernel are told apart by
      their order in the trace; the first of each group is dropped as the warm-up.  Each against the bytes it moves (planes
      read + frames written) over the 6.3 TB/s streaming rate.  jpeg_color_kernel on 4:2:0 files of the same size (Pillow writes
      them; without Pillow that line is not measured) is timed in the same run: it moves the bytes of NV12 and does more
      arithmetic.
  (b) host: rfd_upload_frames_device of NV12 from page-locked memory against the status-quo route, the host-to-device copies of
      the same 32 frames as BGR with tight rows (what place_frames enqueues for host frames), from page-locked memory too.  Alternating
      windows, --repeats per series; a window is --steps calls enqueued back to back and one synchronisation, milliseconds per
      call = host clock over the window / steps.  The spread of the baseline's windows is the yardstick for a difference.

    python tools/frame_convert_bench.py [--reps 20] [--steps 10] [--repeats 5] [--no-trace] [--no-host]
Record the output in profiles/frame_convert.txt."""
import argparse
import ctypes as C
import io
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rs-face-detection_amd", "python"))
STREAM_TBS = 6.3   # float4 copy rate of the chip, TB/s (README)
N, W, H = 32, 1920, 1080
FORMATS = ("nv12", "i420", "yuyv", "bgra")


def plane_sizes(R, fmt):
    l = R.frame_layout(fmt, W, H)
    return [rb * rows for rb, rows in zip(l["row_bytes"], l["rows"])]


def device_frames(R, torch, fmt):
    """N frames of fmt in HBM, random bytes, tight rows -> (tensors to keep, rfd_frame list)"""
    dev = torch.device("cuda", 0)
    keep, frames = [], []
    for i in range(N):
        planes = [torch.randint(0, 256, (s,), dtype=torch.uint8, device=dev) for s in plane_sizes(R, fmt)]
        keep.append(planes)
        frames.append(R.frame(fmt, W, H, [p.data_ptr() for p in planes]))
    return keep, frames


def jpeg_files():
    from PIL import Image
    out = []
    for i in range(N):
        rng = np.random.default_rng(i)
        y, x = np.mgrid[0:H, 0:W]
        img = np.stack([(x * 255 // (W - 1)), (y * 255 // (H - 1)), ((x + y) * 255 // (W + H - 2))], -1).astype(np.float64)
        img[:, W // 2:] += rng.normal(0, 12, (H, W - W // 2, 3))
        buf = io.BytesIO()
        Image.fromarray(np.clip(img, 0, 255).astype(np.uint8)).save(buf, "JPEG", quality=90, subsampling=2)
        out.append(buf.getvalue())
    return out


def traced_child(a):
    """what runs under the profiler; prints how many calls it made"""
    import torch
    import rfd_hip as R
    det = R.RetinaFaceDetection(image_size=(128, 128), max_batch_size=N, max_src=(W, H))
    dev = torch.device("cuda", 0)
    outs = [torch.zeros((H, W * 3), dtype=torch.uint8, device=dev) for _ in range(N)]
    ptrs = [o.data_ptr() for o in outs]
    for fmt in FORMATS:
        keep, frames = device_frames(R, torch, fmt)
        torch.cuda.synchronize()
        for _ in range(1 + a.reps):
            det.convert_frames_device(frames, ptrs)
    jpeg = 0
    try:
        files = jpeg_files()
        for _ in range(1 + a.reps):
            det.decode_jpeg_device(files, ptrs, [(H, W)] * N)
        jpeg = 1 + a.reps
    except ImportError:
        pass
    print("traced calls %d per format, %d decode calls, frames %d" % (1 + a.reps, jpeg, N))
    det.close()


def kernel_pass(a):
    import csv
    import shutil
    import subprocess
    import tempfile
    import rfd_hip as R
    exe = shutil.which("rocprofv3")
    if exe is None:
        print("(a) rocprofv3 is not installed here: kernel time not measured")
        return
    tmp = tempfile.mkdtemp(prefix="rfd_frames_")
    try:
        r = subprocess.run([exe, "--kernel-trace", "--output-format", "csv", "-d", tmp, "--", sys.executable, os.path.abspath(__file__),
                            "--reps", str(a.reps), "--child"], capture_output=True, text=True, timeout=900)
        if r.returncode != 0 or "traced calls" not in r.stdout:
            print("(a) the traced child failed (exit %d): kernel time not measured\n%s" % (r.returncode, (r.stdout + r.stderr)[-600:]))
            return
        rows = None
        for d, _, fs in os.walk(tmp):
            for f in sorted(fs):
                if f.endswith("kernel_trace.csv"):
                    with open(os.path.join(d, f), newline="") as fh:
                        rows = list(csv.DictReader(fh))
        if not rows:
            print("(a) no kernel trace was written: kernel time not measured")
            return
        print("(a) %s" % [l for l in r.stdout.splitlines() if "traced calls" in l][0])
        us = lambda x: (int(x["End_Timestamp"]) - int(x["Start_Timestamp"])) / 1e3
        conv = sorted((x for x in rows if "frame_convert_kernel" in x["Kernel_Name"]), key=lambda x: int(x["Start_Timestamp"]))
        per = 1 + a.reps
        if len(conv) != per * len(FORMATS):
            print("(a) %d dispatches of frame_convert_kernel in the trace, %d expected: kernel time not measured" % (len(conv), per * len(FORMATS)))
            return
        frame_bytes = W * H * 3
        for k, fmt in enumerate(FORMATS):
            t = [us(x) for x in conv[k * per + 1:(k + 1) * per]]
            moved = N * (sum(plane_sizes(R, fmt)) + frame_bytes)
            floor = moved / (STREAM_TBS * 1e12) * 1e6
            print("(a) frame_convert_kernel %s: %d launches, median %.1f us per launch = %.2f us per frame (min %.1f, max %.1f); %.2f MB per frame, "
                  "%.1f MB per launch = %.2f TB/s, floor %.1f us at %.1f TB/s: %.0f %% of the floor's rate" %
                  (fmt, len(t), float(np.median(t)), float(np.median(t)) / N, min(t), max(t), moved / N / 1e6, moved / 1e6, moved / float(np.median(t)) / 1e6,
                   floor, STREAM_TBS, 100 * floor / float(np.median(t))))
        col = sorted((x for x in rows if "jpeg_color_kernel" in x["Kernel_Name"]), key=lambda x: int(x["Start_Timestamp"]))
        if len(col) != per:
            print("(a) jpeg_color_kernel: %d dispatches in the trace, %d expected: not measured" % (len(col), per))
        else:
            t = [us(x) for x in col[1:]]
            print("(a) jpeg_color_kernel on 4:2:0 files of %d x %d, same run: %d launches, median %.1f us per launch (min %.1f, max %.1f)" %
                  (W, H, len(t), float(np.median(t)), min(t), max(t)))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def host_pass(a):
    import torch
    import rfd_hip as R
    det = R.RetinaFaceDetection(image_size=(128, 128), max_batch_size=N, max_src=(W, H))
    L = det._L
    dev = torch.device("cuda", 0)
    outs = [torch.zeros((H, W * 3), dtype=torch.uint8, device=dev) for _ in range(N)]
    ptrs = [o.data_ptr() for o in outs]
    sizes = plane_sizes(R, "nv12")
    nv12_bytes, bgr_bytes = sum(sizes), W * H * 3
    pin = C.c_void_p()
    R._check(L.rfd_host_alloc(N * nv12_bytes, C.byref(pin)))
    block = np.frombuffer((C.c_uint8 * (N * nv12_bytes)).from_address(pin.value), np.uint8)
    block[:] = np.random.default_rng(1).integers(0, 256, block.size, dtype=np.uint8)
    frames = [R.frame("nv12", W, H, [pin.value + i * nv12_bytes, pin.value + i * nv12_bytes + sizes[0]]) for i in range(N)]
    bgr_src = [torch.randint(0, 256, (H, W * 3), dtype=torch.uint8).pin_memory() for _ in range(N)]
    stream = torch.cuda.Stream()       # the baseline's copies run on a stream of torch's, the upload on the context's
    torch.cuda.synchronize()

    def upload_nv12():
        det.upload_frames_device(frames, ptrs, async_=True)

    def copy_bgr():   # what place_frames enqueues for host frames: one copy of tight rows per frame
        with torch.cuda.stream(stream):
            for o, s in zip(outs, bgr_src):
                o.copy_(s, non_blocking=True)

    def drain():
        det.sync()
        stream.synchronize()

    def window(call):
        t0 = time.perf_counter()
        for _ in range(a.steps):
            call()
        drain()
        return (time.perf_counter() - t0) * 1e3 / a.steps

    for call in (upload_nv12, copy_bgr):
        for _ in range(3):
            call()
        drain()
    up, base = [], []
    for _ in range(a.repeats):                                          # alternating windows
        up.append(round(window(upload_nv12), 4))
        base.append(round(window(copy_bgr), 4))
    stats = lambda w: {"windows_ms": w, "median_ms": round(float(np.median(w)), 4), "min_ms": min(w), "max_ms": max(w)}
    print("(b) " + json.dumps({"frames_per_call": N, "frame_size": [W, H], "steps_per_window": a.steps, "repeats": a.repeats,
                               "nv12_bytes_per_call": N * nv12_bytes, "bgr_bytes_per_call": N * bgr_bytes,
                               "upload_nv12_and_convert": stats(up), "copy_bgr": stats(base), "copy_bgr_spread_ms": round(max(base) - min(base), 4),
                               "upload_minus_copy_median_ms": round(float(np.median(up) - np.median(base)), 4),
                               "upload_gb_per_s": round(N * nv12_bytes / float(np.median(up)) / 1e6, 1),
                               "copy_gb_per_s": round(N * bgr_bytes / float(np.median(base)) / 1e6, 1)}))
    det.sync()
    det.close()
    L.rfd_host_free(pin)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20, help="timed launches per format in the traced child")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5, help="timed windows per series")
    ap.add_argument("--no-trace", action="store_true", help="skip (a), the child run under rocprofv3")
    ap.add_argument("--no-host", action="store_true", help="skip (b)")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return traced_child(a)
    import torch  # noqa: F401  (first: librfd_hip.so then binds to the HIP runtime torch ships)
    if not a.no_host:
        host_pass(a)
    if not a.no_trace:
        kernel_pass(a)


if __name__ == "__main__":
    main()
