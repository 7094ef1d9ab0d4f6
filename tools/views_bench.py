"""Detection over views (include/rfd.h, "views") against the only route the library had to the same pixels before it: one
rfd_detect_batch_device call on the same regions as separate images, which leaves one unmerged slab per region.

Input: --frames device frames of --size (1080p), each planned with the default configuration (9 views at 640x640: 4 x 2 tiles
and the full view), 3 frames = 27 views in a context of 32; RetinaFace-R50 with synthetic weights, the confidence threshold set
to a quantile of the scores so that the post path has candidates to work on.  Preprocess and network work are identical on both
routes -- the same 27 regions, one pass of 27 images -- so a difference is the post path's: one decode into per-frame lists, one
sort and one NMS workgroup per FRAME over Vmax x 16 800 candidate slots (the streaming form), against 27 register-form ones.

Timing, in one process: alternating windows, views then regions, --repeats windows each; a window is --steps calls enqueued
back to back (async) and one synchronisation, milliseconds per call = host clock over the window / steps.  The spread of the
baseline's windows is the yardstick for what a difference means.  The decode / sort / NMS times are the library's own HIP events
(rfd_get_stats) of synchronous calls, the median of --repeats.  Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rs-face-detection_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5, help="timed windows per series")
    ap.add_argument("--frames", type=int, default=3)
    ap.add_argument("--size", type=int, nargs=2, default=[1920, 1080], metavar=("W", "H"))
    ap.add_argument("--quantile", type=float, default=0.995, help="the confidence threshold, as a quantile of the scores")
    args = ap.parse_args()

    import numpy as np
    import torch
    import helpers
    import rfd_hip

    W, H = args.size
    cfg = rfd_hip.view_config((640, 640))
    views = [v for f in range(args.frames) for v in rfd_hip.view_plan(W, H, cfg, frame=f)]
    n = len(views)
    det = rfd_hip.RetinaFaceDetection(image_size=(640, 640), max_batch_size=32, max_det=1024)
    det.init_synthetic_weights(1234)
    frames = [helpers.make_image(10 + f, H, W, n_blobs=40) for f in range(args.frames)]
    dev = torch.device("cuda", 0)
    bufs = [torch.from_numpy(f).to(dev) for f in frames]
    # the threshold: a quantile of the scores of the first frame's views
    rois = [frames[v.frame][v.y:v.y + v.h, v.x:v.x + v.w] for v in views if v.frame == 0]
    heads = det.forward(det.preprocess(rois)[1])
    fg = np.concatenate([heads[3 * l][:, 2:4].reshape(len(rois), -1) for l in range(3)], 1)
    thr = float(np.quantile(fg, args.quantile))
    det.set_thresholds(thr, 0.45)

    md = det.max_det
    slab = lambda k: (torch.zeros((k, md, 5), dtype=torch.float32, device=dev), torch.zeros((k, md, 10), dtype=torch.float32, device=dev),
                      torch.zeros(k, dtype=torch.int32, device=dev), torch.zeros(k, dtype=torch.int32, device=dev))
    merged, separate = slab(args.frames), slab(n)
    regions = (rfd_hip.rfd_image * n)()
    for i, v in enumerate(views):
        regions[i].data = bufs[v.frame].data_ptr() + v.y * W * 3 + v.x * 3
        regions[i].height, regions[i].width, regions[i].stride = v.h, v.w, W * 3
    sep = rfd_hip.rfd_dets(*[t.data_ptr() for t in separate])
    torch.cuda.synchronize()

    def by_views(async_):
        det.detect_views_device([b.data_ptr() for b in bufs], [(H, W)] * args.frames, views, *[t.data_ptr() for t in merged],
                                edge_margin=cfg.edge_margin, async_=async_)

    def by_regions(async_):
        rfd_hip._check(det._L.rfd_detect_batch_device(det._ctx, regions, n, C.byref(sep), int(async_)))

    def window(call):
        t0 = time.perf_counter()
        for _ in range(args.steps):
            call(True)
        det.sync()
        return (time.perf_counter() - t0) * 1e3 / args.steps

    def stages():
        rows = {by_views: [], by_regions: []}
        for _ in range(args.repeats):                               # alternating here too: a synchronous call starts on an idle chip
            for call in (by_views, by_regions):
                call(False)
                s = det.stats()
                rows[call].append([s["ms_preprocess"], s["ms_network"], s["ms_decode"], s["ms_sort"], s["ms_nms"], s["candidates"]])
        out = []
        for call in (by_views, by_regions):
            m = np.median(np.array(rows[call], np.float64), 0)
            out.append({"preprocess_ms": round(m[0], 4), "network_ms": round(m[1], 4), "decode_ms": round(m[2], 4), "sort_ms": round(m[3], 4),
                        "nms_ms": round(m[4], 4), "candidates": int(m[5])})
        return out

    for call in (by_views, by_regions):
        for _ in range(args.warmup):
            call(True)
        det.sync()
    v_ms, r_ms = [], []
    for _ in range(args.repeats):                                   # alternating windows
        v_ms.append(round(window(by_views), 4))
        r_ms.append(round(window(by_regions), 4))
    stats = lambda w: {"windows_ms": w, "median_ms": round(float(np.median(w)), 4), "min_ms": min(w), "max_ms": max(w)}
    views_stages, regions_stages = stages()
    res = {"frames": args.frames, "frame_size": [W, H], "views": n, "views_per_frame": n // args.frames, "confidence_threshold": round(thr, 6),
           "steps_per_window": args.steps, "repeats": args.repeats,
           "views_call": stats(v_ms), "regions_call": stats(r_ms), "regions_spread_ms": round(max(r_ms) - min(r_ms), 4),
           "views_minus_regions_median_ms": round(float(np.median(v_ms) - np.median(r_ms)), 4),
           "views_stages": views_stages, "regions_stages": regions_stages,
           "merged_detections": [int(x) for x in merged[3].cpu().numpy()], "unmerged_detections": int(separate[3].cpu().numpy().sum())}
    print(json.dumps(res))
    det.close()


if __name__ == "__main__":
    main()
