#!/usr/bin/env python3
"""JPEG encode (rfd.h, "JPEG encode").  Two workloads: 32 frames of 1920x1080 at quality 90, 4:2:0, one MCU row per restart
interval; and 256 crops of 112x112 with restart_rows = 0, the one-workgroup-per-image form of the entropy kernels.  Each figure
from its own source:
  (a) device: the time of each kernel per launch from a CHILD run of this script under `rocprofv3 --kernel-trace` (a run of its
      own: tracing slows the host, so nothing else is timed there).  The child makes 1 + --reps rfd_encode_jpeg_batch_device calls
      per workload, in that order; the first call of each is dropped as the warm-up.  The block kernel against its byte floor:
      pixels in (once) plus coefficients out, over the 6.3 TB/s streaming rate.
  (b) host: the whole call (enqueue to drained stream) against the route callers have today, the device-to-host copy of the same
      frames as raw BGR into page-locked memory.  Alternating windows, --repeats per series; a window is --steps calls enqueued
      back to back and one synchronisation, milliseconds per call = host clock over the window / steps.  The spread of the
      baseline's windows is the yardstick for a difference.  Then the bytes each route puts on PCIe, and Pillow's encode of the
      same frames on this host on one thread (the work the copy route leaves to the host).

    python tools/jpeg_encode_bench.py [--reps 10] [--steps 5] [--repeats 5] [--no-trace] [--no-host]
Record the output in profiles/jpeg_encode.txt."""
import argparse
import io
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rs-face-detection_amd", "python"))
STREAM_TBS = 6.3   # float4 copy rate of the chip, TB/s (README)
# as the trace names them, demangled or not
KERNELS = (("jpeg_encode_blocks_kernel",), ("jpeg_encode_entropy_kernel<false>", "jpeg_encode_entropy_kernelILb0"), ("jpeg_encode_assemble_kernel",),
           ("jpeg_encode_entropy_kernel<true>", "jpeg_encode_entropy_kernelILb1"))
WORKLOADS = [dict(name="frames", n=32, w=1920, h=1080, restart=1, slot=1 << 21), dict(name="crops", n=256, w=112, h=112, restart=0, slot=1 << 14)]


def pictures(n, w, h):
    """n frames: ramps, the right half with noise, so that the files are neither empty nor incompressible"""
    y, x = np.mgrid[0:h, 0:w]
    base = np.stack([(x * 255 // max(w - 1, 1)), (y * 255 // max(h - 1, 1)), ((x + y) * 255 // max(w + h - 2, 1))], -1).astype(np.float32)
    out = []
    for i in range(n):
        img = np.roll(base, 37 * i, 1).copy()
        img[:, w // 2:] += np.random.default_rng(i).normal(0, 12, (h, w - w // 2, 3)).astype(np.float32)
        out.append(np.clip(img, 0, 255).astype(np.uint8))
    return out


class Workload:
    def __init__(self, R, torch, det, wl):
        dev = torch.device("cuda", 0)
        self.wl, self.det = wl, det
        self.host = pictures(wl["n"], wl["w"], wl["h"])
        self.frames = [torch.from_numpy(f).to(dev) for f in self.host]
        self.out = torch.zeros(wl["n"] * wl["slot"], dtype=torch.uint8, device=dev)
        self.size = torch.zeros(wl["n"], dtype=torch.int32, device=dev)
        self.cfg = R.jpeg_encode_config(90, R.JPEG_420, wl["restart"])
        self.ptrs, self.shapes = [f.data_ptr() for f in self.frames], [(wl["h"], wl["w"])] * wl["n"]
        torch.cuda.synchronize()

    def encode(self, async_=True):
        self.det.encode_jpeg_device(self.ptrs, self.shapes, self.out.data_ptr(), self.wl["slot"], self.size.data_ptr(), cfg=self.cfg, async_=async_)


def detector(R):
    return R.RetinaFaceDetection(image_size=(128, 128), max_batch_size=256, max_src=(1920, 1080))


def traced_child(a):
    import torch
    import rfd_hip as R
    det = detector(R)
    for wl in WORKLOADS:
        w = Workload(R, torch, det, wl)
        for _ in range(1 + a.reps):
            w.encode(async_=False)
        sizes = w.size.cpu().numpy()
        print("traced %s: %d calls, file bytes min %d median %d max %d" % (wl["name"], 1 + a.reps, sizes.min(), int(np.median(sizes)), sizes.max()))
    det.close()


def kernel_pass(a):
    import csv
    import shutil
    import subprocess
    import tempfile
    exe = shutil.which("rocprofv3")
    if exe is None:
        print("(a) rocprofv3 is not installed here: kernel time not measured")
        return
    tmp = tempfile.mkdtemp(prefix="rfd_encode_")
    try:
        r = subprocess.run([exe, "--kernel-trace", "--output-format", "csv", "-d", tmp, "--", sys.executable, os.path.abspath(__file__),
                            "--reps", str(a.reps), "--child"], capture_output=True, text=True, timeout=900)
        if r.returncode != 0 or "traced crops" not in r.stdout:
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
        for line in r.stdout.splitlines():
            if line.startswith("traced"):
                print("(a) " + line)
        us = lambda x: (int(x["End_Timestamp"]) - int(x["Start_Timestamp"])) / 1e3
        per = 1 + a.reps
        for key in KERNELS:
            hits = sorted((x for x in rows if any(k in x["Kernel_Name"] for k in key)), key=lambda x: int(x["Start_Timestamp"]))
            key = key[0]
            if len(hits) != per * len(WORKLOADS):
                print("(a) %s: %d dispatches in the trace, %d expected: not measured" % (key, len(hits), per * len(WORKLOADS)))
                continue
            for k, wl in enumerate(WORKLOADS):
                t = [us(x) for x in hits[k * per + 1:(k + 1) * per]]
                line = "(a) %s, %s (%d x %d x %d): %d launches, median %.1f us per launch (min %.1f, max %.1f)" % (
                    key, wl["name"], wl["n"], wl["w"], wl["h"], len(t), float(np.median(t)), min(t), max(t))
                if key == KERNELS[0][0]:
                    mx, my = -(-wl["w"] // 16), -(-wl["h"] // 16)
                    moved = wl["n"] * (wl["w"] * wl["h"] * 3 + mx * my * 6 * 128)
                    floor = moved / (STREAM_TBS * 1e12) * 1e6
                    line += "; pixels in + coefficients out %.1f MB, floor %.1f us at %.1f TB/s: %.0f %% of the floor's rate" % (
                        moved / 1e6, floor, STREAM_TBS, 100 * floor / float(np.median(t)))
                print(line)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def host_pass(a):
    import torch
    import rfd_hip as R
    det = detector(R)
    stream = torch.cuda.Stream()
    stats = lambda w: {"windows_ms": w, "median_ms": round(float(np.median(w)), 4), "min_ms": min(w), "max_ms": max(w)}
    for wl in WORKLOADS:
        w = Workload(R, torch, det, wl)
        pinned = [torch.zeros((wl["h"], wl["w"], 3), dtype=torch.uint8).pin_memory() for _ in range(wl["n"])]

        def copy_raw():   # the route callers have today: the raw frames to the host, one copy each
            with torch.cuda.stream(stream):
                for p, f in zip(pinned, w.frames):
                    p.copy_(f, non_blocking=True)

        def drain():
            det.sync()
            stream.synchronize()

        def window(call):
            t0 = time.perf_counter()
            for _ in range(a.steps):
                call()
            drain()
            return (time.perf_counter() - t0) * 1e3 / a.steps

        for call in (w.encode, copy_raw):
            for _ in range(2):
                call()
            drain()
        enc, base = [], []
        for _ in range(a.repeats):                                          # alternating windows
            enc.append(round(window(w.encode), 4))
            base.append(round(window(copy_raw), 4))
        sizes = w.size.cpu().numpy()
        assert (sizes > 0).all(), sizes
        out = {"workload": wl["name"], "images_per_call": wl["n"], "image_size": [wl["w"], wl["h"]], "restart_rows": wl["restart"], "steps_per_window": a.steps,
               "repeats": a.repeats, "encode_call": stats(enc), "copy_raw_bgr": stats(base), "copy_raw_bgr_spread_ms": round(max(base) - min(base), 4),
               "encode_minus_copy_median_ms": round(float(np.median(enc) - np.median(base)), 4),
               "pcie_bytes_per_call_files": int(sizes.sum()), "pcie_bytes_per_call_raw": wl["n"] * wl["w"] * wl["h"] * 3,
               "file_bytes_median": int(np.median(sizes))}
        try:
            from PIL import Image
            k = min(wl["n"], 8)
            t0 = time.perf_counter()
            for f in w.host[:k]:
                Image.fromarray(f[..., ::-1]).save(io.BytesIO(), "JPEG", quality=90, subsampling=2, **({"restart_marker_rows": 1} if wl["restart"] else {}))
            out["pillow_one_thread_ms_per_image"] = round((time.perf_counter() - t0) * 1e3 / k, 4)
            out["pillow_one_thread_ms_per_call"] = round(out["pillow_one_thread_ms_per_image"] * wl["n"], 2)
        except ImportError:
            out["pillow_one_thread_ms_per_image"] = "not measured (no Pillow)"
        print("(b) " + json.dumps(out))
        del w, pinned
    det.sync()
    det.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10, help="timed calls per workload in the traced child")
    ap.add_argument("--steps", type=int, default=5)
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
