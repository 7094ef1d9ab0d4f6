#!/usr/bin/env python3
"""Time of the model-input epilogue (rfd_face_tensors and friends) at the bench's operating point: 32 frames of 1080p,
RetinaFace-R50, the calibrated cls bias of bench.py.  Medians of --calls calls after --warmup warm-ups, wall clock around
calls that end with a host synchronisation:

  align          rfd_detect_select_align_batch                     (what existed before: crops only)
  align_tensors  rfd_detect_select_align_tensors_batch, both presets, with and without the u8 crops
  device         rfd_detect_faces_device, async = 1, then rfd_sync  (frames and every output in HBM)

--kernels runs only the alignment epilogue on fixed selections, a few times each way -- rfd_align_faces + rfd_face_tensors
(align_warp_kernel, then face_tensor_kernel on the crops) and rfd_align_faces_tensors (align_warp_tensor_kernel) -- so that
`rocprofv3 --kernel-trace --stats -- python tools/face_tensor_bench.py --kernels` prices the kernels themselves.
Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "rs-face-detection_amd", "python"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

B, H, W, MAX_DET = 32, 1080, 1920, 1024
CAND_RATE = 0.006   # bench.py's TARGET_CAND_RATE


def calibrate(det, graph, frames):
    """bench.py's calibrate_cls_bias: shift the fg logits so that CAND_RATE of the anchors clear the 0.7 threshold"""
    _, tensor, _ = det.preprocess(frames[:2])
    heads = det.forward(tensor)
    p = np.clip(np.concatenate([heads[3 * l][:, 2:4].reshape(-1) for l in range(3)]).astype(np.float64), 1e-7, 1 - 1e-7)
    delta = float(np.log(0.7 / 0.3) - np.quantile(np.log(p / (1 - p)), 1.0 - CAND_RATE))
    for i, L in enumerate(graph.layers):
        if L.name.decode().startswith("head"):
            w, b = det.get_layer(i, L)
            b[2:4] += delta
            det.set_layer(i, w, b)
    return delta


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
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--kernels", action="store_true")
    args = ap.parse_args()
    import torch
    import helpers
    import rfd_hip
    det = rfd_hip.RetinaFaceDetection(image_size=(640, 640), max_batch_size=B, max_det=MAX_DET)
    frames = [helpers.make_image(1000 + i, H, W) for i in range(B)]
    cfgs = [rfd_hip.face_tensor_config_quality(), rfd_hip.face_tensor_config_extraction()]
    if args.kernels:
        sel = [helpers.make_face_kps(50 + i, H, W)[::-1] for i in range(B)]
        for _ in range(5):
            crops, _ = det.align_faces(frames, sel)
            det.face_tensors(crops, cfgs)
            det.align_faces_tensors(frames, sel, cfgs)
            det.align_faces_tensors(frames, sel, cfgs, want_crops=False)
        print(json.dumps({"kernels": True, "faces": B, "frame": [H, W]}))
        det.close()
        return
    det.init_synthetic_weights(1234)
    delta = calibrate(det, rfd_hip.Graph(rfd_hip.BACKBONE_R50, 640, 640), frames)
    res = {"batch": B, "frame": [H, W], "calls": args.calls, "warmup": args.warmup, "cls_bias": round(delta, 3)}
    _, _, status = det.detect_select_align(frames)
    res["aligned_faces"] = int((status >= 0).sum())
    res["align_ms"] = median_ms(lambda: det.detect_select_align(frames), args.warmup, args.calls)
    res["align_tensors_ms"] = median_ms(lambda: det.detect_select_align_tensors(frames, cfgs), args.warmup, args.calls)
    res["align_tensors_no_crops_ms"] = median_ms(lambda: det.detect_select_align_tensors(frames, cfgs, want_crops=False), args.warmup, args.calls)
    dev = torch.device("cuda", 0)
    fr = torch.from_numpy(np.stack(frames)).to(dev)
    ptrs = [fr.data_ptr() + i * H * W * 3 for i in range(B)]
    shapes = [(H, W)] * B
    o = dict(box=torch.zeros(B, 5, device=dev), kps=torch.zeros(B, 10, device=dev), found=torch.zeros(B, dtype=torch.int32, device=dev),
             crops=torch.zeros(B, 112, 112, 3, dtype=torch.uint8, device=dev), status=torch.zeros(B, dtype=torch.int32, device=dev),
             tensors=[torch.zeros(B, 3, 112, 112, device=dev) for _ in cfgs])
    torch.cuda.synchronize()

    def device_call(crops=True):
        det.detect_faces_device(ptrs, shapes, cfgs, o["box"].data_ptr(), o["kps"].data_ptr(), o["found"].data_ptr(),
                                o["crops"].data_ptr() if crops else None, o["status"].data_ptr(), [t.data_ptr() for t in o["tensors"]], async_=True)
        det.sync()

    res["device_ms"] = median_ms(device_call, args.warmup, args.calls)
    res["device_no_crops_ms"] = median_ms(lambda: device_call(False), args.warmup, args.calls)
    slab = torch.zeros(B * MAX_DET * 15 + 2 * B, dtype=torch.float32, device=dev)
    base = slab.data_ptr()
    dp = (base, base + B * MAX_DET * 5 * 4, base + B * MAX_DET * 15 * 4, base + B * MAX_DET * 15 * 4 + B * 4)

    def detect_only():
        det.detect_device(ptrs, shapes, *dp, async_=1)
        det.sync()

    res["device_detect_only_ms"] = median_ms(detect_only, args.warmup, args.calls)   # the same pass without any epilogue
    print(json.dumps(res))
    det.close()


if __name__ == "__main__":
    main()
