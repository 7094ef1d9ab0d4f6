"""What the shot quality (include/rfd.h, "shot quality") costs beside the detection call it follows.

Input: 32 device frames of --size (1080p), RetinaFace-R50 640x640 with synthetic weights in a context of 32; the quality call
reads SYNTHETIC slabs of --rows rows per frame -- square boxes of --sides pixels spread over the frame (side 0: the whole frame),
the template's landmarks scaled into each -- while the detector writes slabs of its own.  Eight workgroups share the rows of a
frame and a workgroup reads a whole region, so the cost grows with rows x area; combinations whose regions exceed --max-mb
megabytes per workgroup are skipped (1024 whole-frame rows would be 800 MB through each of 256 workgroups).

Timing, in one process, by the method of tools/track_bench.py: alternating windows, detection + quality then detection alone,
--repeats windows each; a window is --steps calls enqueued back to back (async) and one synchronisation, milliseconds per call
= host clock over the window / steps.  The spread of the baseline's windows is the yardstick for what a difference means.
Prints one JSON line per (rows, side): the added time per call, per row, and the bytes per second one workgroup achieved
(rows of a workgroup x region bytes over the added time; DESIGN.md section 6 gives 95-125 GB/s for one CU)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rs-face-detection_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

STANDARD = [38.2946, 51.6963, 73.5318, 51.5014, 56.0252, 71.7366, 41.5493, 92.3655, 70.7299, 92.2041]
GROUPS_PER_FRAME = 8      # kSqGroupsPerFrame of csrc/shot_quality_host.h


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5, help="timed windows per series")
    ap.add_argument("--size", type=int, nargs=2, default=[1920, 1080], metavar=("W", "H"))
    ap.add_argument("--rows", type=int, nargs="+", default=[8, 64, 1024])
    ap.add_argument("--sides", type=int, nargs="+", default=[40, 112, 400, 0], help="0 = the whole frame")
    ap.add_argument("--max-mb", type=float, default=16.0, help="skip a combination that reads more than this per workgroup")
    args = ap.parse_args()

    import numpy as np
    import torch
    import helpers
    import rfd_hip

    n, md = 32, 1024
    W, H = args.size
    det = rfd_hip.RetinaFaceDetection(image_size=(640, 640), max_batch_size=n, max_det=md)
    det.init_synthetic_weights(1234)
    dev = torch.device("cuda", 0)
    bufs = [torch.from_numpy(helpers.make_image(10 + f, H, W)).to(dev) for f in range(n)]
    ptrs, shapes = [b.data_ptr() for b in bufs], [(H, W)] * n
    frames = [(p, H, W) for p in ptrs]
    zeros = lambda *shape, dt=torch.float32: torch.zeros(shape, dtype=dt, device=dev)
    own = (zeros(n, md, 5), zeros(n, md, 10), zeros(n, dt=torch.int32), zeros(n, dt=torch.int32))      # the detector's slabs
    q, parts, status = zeros(n, md), zeros(n, md, 8), zeros(n, md, dt=torch.int32)

    def detect_only():
        det.detect_device(ptrs, shapes, *[t.data_ptr() for t in own], async_=True)

    for side in args.sides:
        bw, bh = (side, side) if side else (W, H)
        k = np.arange(md)
        box = np.zeros((md, 5), np.float32)
        box[:, 0], box[:, 1] = (k * 37) % max(W - bw, 1), (k * 53) % max(H - bh, 1)
        box[:, 2], box[:, 3], box[:, 4] = box[:, 0] + bw - 1, box[:, 1] + bh - 1, 0.9
        lmk = (np.asarray(STANDARD, np.float32).reshape(1, 5, 2) / 112.0 * [bw, bh] + box[:, None, :2]).reshape(md, 10).astype(np.float32)
        s_boxes, s_lmk = torch.from_numpy(np.tile(box, (n, 1, 1))).to(dev), torch.from_numpy(np.tile(lmk, (n, 1, 1))).to(dev)
        region_bytes = bw * bh * 3
        for rows in args.rows:
            per_group = -(-rows // GROUPS_PER_FRAME)
            if per_group * region_bytes > args.max_mb * 1e6:
                print(json.dumps({"rows_per_frame": rows, "box": [bw, bh], "skipped": "%.0f MB per workgroup" % (per_group * region_bytes / 1e6)}))
                continue
            s_count = torch.full((n,), rows, dtype=torch.int32, device=dev)
            torch.cuda.synchronize()

            def detect_quality():
                detect_only()
                det.shot_quality(frames, (s_boxes.data_ptr(), s_lmk.data_ptr(), s_count.data_ptr()), device=True,
                                 out=(q.data_ptr(), parts.data_ptr(), status.data_ptr()), async_=True)

            def window(call):
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    call()
                det.sync()
                return (time.perf_counter() - t0) * 1e3 / args.steps

            for call in (detect_quality, detect_only):
                for _ in range(args.warmup):
                    call()
                det.sync()
            q_ms, d_ms = [], []
            for _ in range(args.repeats):                                   # alternating windows
                q_ms.append(round(window(detect_quality), 4))
                d_ms.append(round(window(detect_only), 4))
            stats = lambda w: {"windows_ms": w, "median_ms": round(float(np.median(w)), 4), "min_ms": min(w), "max_ms": max(w)}
            added = float(np.median(q_ms) - np.median(d_ms))
            st, qq = status.cpu().numpy(), q.cpu().numpy()
            print(json.dumps({"frames_per_call": n, "rows_per_frame": rows, "box": [bw, bh], "frame_size": [W, H], "steps_per_window": args.steps,
                              "repeats": args.repeats, "detect_then_quality": stats(q_ms), "detect_alone": stats(d_ms),
                              "detect_alone_spread_ms": round(max(d_ms) - min(d_ms), 4), "quality_minus_alone_median_ms": round(added, 4),
                              "us_per_row": round(added * 1e3 / (rows * n), 4) if added > 0 else None,
                              "rows_per_workgroup": per_group, "region_bytes": region_bytes,
                              "one_workgroup_GB_per_s": round(per_group * region_bytes / (added * 1e-3) / 1e9, 2) if added > 0 else None,
                              "measured_rows_frame_0": int((st[0, :rows] == 0).sum()), "quality_row_0": float(qq[0, 0])}))
    det.close()


if __name__ == "__main__":
    main()
