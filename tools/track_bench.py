"""What a tracker update (include/rfd.h, "tracker") costs beside the detection call it follows.

Input: 32 device frames of --size, one per stream, RetinaFace-R50 640x640 with synthetic weights in a context of 32; the tracker
(32 streams, --max-tracks slots) reads SYNTHETIC slabs of 8, 64 and 1024 rows per frame -- non-overlapping 10 x 10 boxes on a
grid, the same in every call, so after the first call every row that has a slot matches it at IoU 1 and the rest are refused a
birth: the steady state of a full scene -- while the detector writes slabs of its own.  One workgroup of one wave per stream
walks its frame's rows one after the other, so the update is latency-bound and its cost grows with the rows.

Timing, in one process: alternating windows, detection + update then detection alone, --repeats windows each; a window is
--steps calls enqueued back to back (async) and one synchronisation, milliseconds per call = host clock over the window / steps.
The spread of the baseline's windows is the yardstick for what a difference means.  Prints one JSON line per row count."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rs-face-detection_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5, help="timed windows per series")
    ap.add_argument("--size", type=int, nargs=2, default=[640, 480], metavar=("W", "H"))
    ap.add_argument("--max-tracks", type=int, default=256)
    ap.add_argument("--rows", type=int, nargs="+", default=[8, 64, 1024])
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
    zeros = lambda *shape, dt=torch.float32: torch.zeros(shape, dtype=dt, device=dev)
    own = (zeros(n, md, 5), zeros(n, md, 10), zeros(n, dt=torch.int32), zeros(n, dt=torch.int32))      # the detector's slabs
    z = dict(track=zeros(n, md, dt=torch.int32), flags=zeros(n, md, dt=torch.int32), stats=zeros(n, 4, dt=torch.int32),
             ended=zeros(n, args.max_tracks, dt=torch.int32), due_boxes=zeros(n, md, 5), due_lmk=zeros(n, md, 10),
             due_count=zeros(n, dt=torch.int32), due_track=zeros(n, md, dt=torch.int32))
    out = rfd_hip.rfd_track_out(z["track"].data_ptr(), z["flags"].data_ptr(), z["stats"].data_ptr(), z["ended"].data_ptr(),
                                rfd_hip.rfd_dets(z["due_boxes"].data_ptr(), z["due_lmk"].data_ptr(), z["due_count"].data_ptr(), None),
                                z["due_track"].data_ptr())
    grid = np.zeros((md, 5), np.float32)
    k = np.arange(md)
    grid[:, 0], grid[:, 1] = 20 * (k % 32), 20 * (k // 32)
    grid[:, 2], grid[:, 3], grid[:, 4] = grid[:, 0] + 9, grid[:, 1] + 9, 0.9
    s_boxes, s_lmk = torch.from_numpy(np.tile(grid, (n, 1, 1))).to(dev), zeros(n, md, 10)
    streams = list(range(n))

    def detect_only():
        det.detect_device(ptrs, shapes, *[t.data_ptr() for t in own], async_=True)

    for rows in args.rows:
        tracker = det.tracker(streams=n, max_tracks=args.max_tracks, min_score=0.5, new_score=0.5)
        s_count = torch.full((n,), rows, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()

        def detect_track():
            detect_only()
            tracker.update_device(streams, s_boxes.data_ptr(), s_lmk.data_ptr(), s_count.data_ptr(), out, async_=True)

        def window(call):
            t0 = time.perf_counter()
            for _ in range(args.steps):
                call()
            det.sync()
            return (time.perf_counter() - t0) * 1e3 / args.steps

        for call in (detect_track, detect_only):
            for _ in range(args.warmup):
                call()
            det.sync()
        t_ms, d_ms = [], []
        for _ in range(args.repeats):                                   # alternating windows
            t_ms.append(round(window(detect_track), 4))
            d_ms.append(round(window(detect_only), 4))
        stats = lambda w: {"windows_ms": w, "median_ms": round(float(np.median(w)), 4), "min_ms": min(w), "max_ms": max(w)}
        st = z["stats"].cpu().numpy()
        print(json.dumps({"streams": n, "frames_per_call": n, "rows_per_frame": rows, "max_tracks": args.max_tracks, "frame_size": [W, H],
                          "steps_per_window": args.steps, "repeats": args.repeats, "detect_then_track": stats(t_ms), "detect_alone": stats(d_ms),
                          "detect_alone_spread_ms": round(max(d_ms) - min(d_ms), 4),
                          "track_minus_alone_median_ms": round(float(np.median(t_ms) - np.median(d_ms)), 4),
                          "last_call_matched_per_frame": int(st[0, 0]), "last_call_dropped_per_frame": int(st[0, 3])}))
        tracker.close()
    det.close()


if __name__ == "__main__":
    main()
