#!/usr/bin/env python3
"""Cost of listing, aligning and tensorising EVERY face of a frame instead of one, at the bench's operating point: 32 resident
frames of 1080p, RetinaFace-R50, the calibrated cls bias of bench.py (raised until every frame holds at least FACES detections).

In one run, wall clock around calls that end with rfd_sync, medians of --calls calls after --warmup warm-ups:

  one_face_ms_before   rfd_detect_faces_device, quality + extraction presets        (one face per frame)
  all_faces_ms         rfd_detect_all_faces_device, max_faces = FACES, cap = 32 * FACES, the same presets
  one_face_ms_after    the first window again

and from them: the difference per extra face, (all_faces - mean of the two one-face windows) / (T - 32), with the spread of
the two one-face windows -- the same code, minutes apart -- as the yardstick for what a difference means.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "rs-face-detection_amd", "python"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

B, H, W, MAX_DET, FACES = 32, 1080, 1920, 1024, 8


def shift_cls_bias(det, graph, frames, rate):
    """bench.py's calibrate_cls_bias: shift the fg logits so that `rate` of the anchors clear the 0.7 threshold"""
    _, tensor, _ = det.preprocess(frames[:2])
    heads = det.forward(tensor)
    p = np.clip(np.concatenate([heads[3 * l][:, 2:4].reshape(-1) for l in range(3)]).astype(np.float64), 1e-7, 1 - 1e-7)
    delta = float(np.log(0.7 / 0.3) - np.quantile(np.log(p / (1 - p)), 1.0 - rate))
    for i, L in enumerate(graph.layers):
        if L.name.decode().startswith("head"):
            w, b = det.get_layer(i, L)
            b[2:4] += delta
            det.set_layer(i, w, b)


def median_ms(fn, warmup, calls):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return round(float(np.median(ts)) * 1e3, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    import torch
    import helpers
    import rfd_hip
    det = rfd_hip.RetinaFaceDetection(image_size=(640, 640), max_batch_size=B, max_det=MAX_DET)
    frames = [helpers.make_image(1000 + i, H, W) for i in range(B)]
    cfgs = [rfd_hip.face_tensor_config_quality(), rfd_hip.face_tensor_config_extraction()]
    det.init_synthetic_weights(1234)
    graph = rfd_hip.Graph(rfd_hip.BACKBONE_R50, 640, 640)
    for rate in (0.006, 0.02, 0.06):   # bench.py's rate first; denser only if some frame holds fewer than FACES detections
        shift_cls_bias(det, graph, frames, rate)
        counts = [len(b) for b, _ in det.call_batch(frames)]
        if min(counts) >= FACES:
            break
    res = {"batch": B, "frame": [H, W], "calls": args.calls, "warmup": args.warmup, "cand_rate": rate,
           "detections_per_frame_min": min(counts), "detections_per_frame_max": max(counts), "max_faces": FACES}
    if min(counts) < FACES:
        raise SystemExit("a frame holds only %d detections: %s" % (min(counts), json.dumps(res)))
    dev = torch.device("cuda", 0)
    fr = torch.from_numpy(np.stack(frames)).to(dev)
    ptrs = [fr.data_ptr() + i * H * W * 3 for i in range(B)]
    shapes = [(H, W)] * B
    cap = B * FACES
    i32 = lambda n: torch.zeros(n, dtype=torch.int32, device=dev)
    one = dict(box=torch.zeros(B, 5, device=dev), kps=torch.zeros(B, 10, device=dev), found=i32(B), status=i32(B),
               tensors=[torch.zeros(B, 3, 112, 112, device=dev) for _ in cfgs])
    many = dict(total=i32(1), first=i32(B + 1), frame=i32(cap), row=i32(cap), status=i32(cap), box=torch.zeros(cap, 5, device=dev),
                kps=torch.zeros(cap, 10, device=dev), tensors=[torch.zeros(cap, 3, 112, 112, device=dev) for _ in cfgs])
    lc = rfd_hip.face_list_config(max_faces=FACES)
    torch.cuda.synchronize()

    def one_face():
        det.detect_faces_device(ptrs, shapes, cfgs, one["box"].data_ptr(), one["kps"].data_ptr(), one["found"].data_ptr(), None,
                                one["status"].data_ptr(), [t.data_ptr() for t in one["tensors"]], async_=True)
        det.sync()

    def all_faces():
        det.detect_all_faces_device(ptrs, shapes, cfgs, cap, many["total"].data_ptr(), many["first"].data_ptr(), many["frame"].data_ptr(),
                                    many["row"].data_ptr(), many["box"].data_ptr(), many["kps"].data_ptr(), many["status"].data_ptr(), None,
                                    [t.data_ptr() for t in many["tensors"]], list_cfg=lc, async_=True)
        det.sync()

    res["one_face_ms_before"] = median_ms(one_face, args.warmup, args.calls)
    res["all_faces_ms"] = median_ms(all_faces, args.warmup, args.calls)
    res["one_face_ms_after"] = median_ms(one_face, args.warmup, args.calls)
    T = int(many["total"].cpu()[0])
    res["faces_listed"] = T
    res["faces_one_face_path"] = int((one["status"].cpu().numpy() >= 0).sum())
    base = 0.5 * (res["one_face_ms_before"] + res["one_face_ms_after"])
    res["extra_ms_per_batch"] = round(res["all_faces_ms"] - base, 3)
    res["extra_us_per_extra_face"] = round(1e3 * (res["all_faces_ms"] - base) / max(T - B, 1), 3)
    res["one_face_window_spread_ms"] = round(abs(res["one_face_ms_before"] - res["one_face_ms_after"]), 3)
    print(json.dumps(res))
    det.close()


if __name__ == "__main__":
    main()
