"""What the annotation (include/rfd.h, "annotation") costs beside the detection call it follows, next to the nearest existing
kernel -- rfd_redact_faces_device in FILL / RECT mode on the same rows: the same tiles and the same bytes -- and next to the route
callers had before it: the frames over PCIe to the host and back.

Input: 32 device frames of --size (1080p), RetinaFace-R50 640x640 with synthetic weights in a context of 32; the annotation reads
SYNTHETIC slabs of --rows rows per frame -- square boxes of --sides pixels spread over the frame, five landmarks inside each --
while the detector writes slabs of its own.  The config is the default (outline 2, marks 2, the score as text at scale 2, opaque),
and the same without text.

Timing, in one process, by the method of tools/redact_bench.py: alternating windows -- detection + annotation, detection alone,
the annotation calls alone back to back, the redaction calls alone back to back -- --repeats windows each; a window is --steps
calls enqueued back to back (async) and one synchronisation, milliseconds per call = host clock over the window / steps.  The
spread of the baseline's windows is the yardstick for what a difference means.  Last, the copy route: device -> page-locked host
-> device of the same frames, the copies alone, with no painting on the host.
Prints one JSON line per (rows, side, form, text) and one for the copy route."""
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
    ap.add_argument("--size", type=int, nargs=2, default=[1920, 1080], metavar=("W", "H"))
    ap.add_argument("--rows", type=int, nargs="+", default=[8, 64, 1024])
    ap.add_argument("--sides", type=int, nargs="+", default=[40, 400])
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
    outs = [torch.zeros(H * W * 3, dtype=torch.uint8, device=dev) for _ in range(n)]
    ptrs, shapes = [b.data_ptr() for b in bufs], [(H, W)] * n
    frames, dsts = [(p, H, W) for p in ptrs], [(t.data_ptr(), H, W) for t in outs]
    zeros = lambda *shape, dt=torch.float32: torch.zeros(shape, dtype=dt, device=dev)
    own = (zeros(n, md, 5), zeros(n, md, 10), zeros(n, dt=torch.int32), zeros(n, dt=torch.int32))      # the detector's slabs
    applied = zeros(n, dt=torch.int32)
    with_text = rfd_hip.annotate_config()
    without = rfd_hip.annotate_config(value_source=rfd_hip.ANNOTATE_NONE)
    fill = rfd_hip.redact_config(mode=rfd_hip.REDACT_FILL, shape=rfd_hip.REDACT_RECT, margin_x=0.0, margin_top=0.0, margin_bottom=0.0)
    frame_bytes = n * H * W * 3

    def window(call, sync):
        t0 = time.perf_counter()
        for _ in range(args.steps):
            call()
        sync()
        return (time.perf_counter() - t0) * 1e3 / args.steps

    def series(calls, sync):
        for call in calls:
            for _ in range(args.warmup):
                call()
            sync()
        ms = [[] for _ in calls]
        for _ in range(args.repeats):                                           # alternating windows
            for k, call in enumerate(calls):
                ms[k].append(round(window(call, sync), 4))
        return ms

    stats = lambda w: {"windows_ms": w, "median_ms": round(float(np.median(w)), 4), "min_ms": min(w), "max_ms": max(w)}

    def detect_only():
        det.detect_device(ptrs, shapes, *[t.data_ptr() for t in own], async_=True)

    for side in args.sides:
        k = np.arange(md)
        box = np.zeros((md, 5), np.float32)
        box[:, 0], box[:, 1] = (k * 37) % max(W - side, 1), (k * 53) % max(H - side, 1)
        box[:, 2], box[:, 3], box[:, 4] = box[:, 0] + side - 1, box[:, 1] + side - 1, 0.9
        lmk = np.zeros((md, 5, 2), np.float32)
        for m, (fx, fy) in enumerate(((0.3, 0.35), (0.7, 0.35), (0.5, 0.55), (0.35, 0.75), (0.65, 0.75))):
            lmk[:, m, 0], lmk[:, m, 1] = box[:, 0] + fx * side, box[:, 1] + fy * side
        s_boxes, s_lmk = torch.from_numpy(np.tile(box, (n, 1, 1))).to(dev), torch.from_numpy(np.tile(lmk.reshape(md, 10), (n, 1, 1))).to(dev)
        for rows in args.rows:
            s_count = torch.full((n,), rows, dtype=torch.int32, device=dev)
            for in_place in (True, False):
                for text, cfg in ((True, with_text), (False, without)):
                    def annotate():
                        det.annotate_faces(frames, (s_boxes.data_ptr(), s_lmk.data_ptr(), s_count.data_ptr()), cfg=cfg, device=True,
                                           dst=None if in_place else dsts, applied=applied.data_ptr(), async_=True)

                    def redact():
                        det.redact_faces(frames, (s_boxes.data_ptr(), s_count.data_ptr()), cfg=fill, device=True, dst=None if in_place else dsts,
                                         applied=applied.data_ptr(), async_=True)

                    def detect_annotate():
                        detect_only()
                        annotate()
                    torch.cuda.synchronize()
                    r_ms, d_ms, a_ms, f_ms = series((detect_annotate, detect_only, annotate, redact), det.sync)
                    added, alone, redaction = float(np.median(r_ms) - np.median(d_ms)), float(np.median(a_ms)), float(np.median(f_ms))
                    annotate()
                    det.sync()
                    got = applied.cpu().numpy()
                    print(json.dumps({"frames_per_call": n, "rows_per_frame": rows, "box": [side, side], "frame_size": [W, H],
                                      "form": "in place" if in_place else "out of place", "text": text, "steps_per_window": args.steps, "repeats": args.repeats,
                                      "detect_then_annotate": stats(r_ms), "detect_alone": stats(d_ms), "detect_alone_spread_ms": round(max(d_ms) - min(d_ms), 4),
                                      "annotate_minus_alone_median_ms": round(added, 4), "annotate_calls_alone_back_to_back": stats(a_ms),
                                      "redact_fill_rect_calls_alone_back_to_back": stats(f_ms),
                                      "annotate_over_redact_fill": round(alone / redaction, 3) if redaction > 0 else None,
                                      "applied_frame_0": int(got[0])}), flush=True)

    # the route callers had: the frames to page-locked host memory and back, the copies alone
    host = [torch.empty(H * W * 3, dtype=torch.uint8).pin_memory() for _ in range(n)]

    def round_trip():
        for b, h in zip(bufs, host):
            h.copy_(b.view(-1), non_blocking=True)
        for b, h in zip(bufs, host):
            b.view(-1).copy_(h, non_blocking=True)
    torch.cuda.synchronize()
    rt_ms, = series((round_trip,), torch.cuda.synchronize)
    print(json.dumps({"copy_route": "device -> page-locked host -> device, %d frames of %d x %d, copies alone" % (n, W, H), "bytes_each_way": frame_bytes,
                      "round_trip": stats(rt_ms), "GB_per_s_round_trip": round(2 * frame_bytes / (float(np.median(rt_ms)) * 1e-3) / 1e9, 1)}), flush=True)
    det.close()


if __name__ == "__main__":
    main()
