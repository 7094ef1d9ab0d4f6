#!/usr/bin/env python3
"""Time of the liveness model inputs (rfd_liveness_tensors_device) at 32 faces in 1080p frames resident in HBM, default config
(the four miniFAS inputs: 80x80, 80x80, 256x256, 128x128), against the yardstick: the existing face_tensor_kernel producing
the same four output sizes from 112x112 crops (rfd_face_tensors).

Default mode: HIP events on the context's stream around --calls device-resident calls after --warmup warm-ups -> milliseconds
per call (descriptor copy + both kernels), output bytes per call and output GB/s.  rfd_face_tensors has host pointers only, so
its wall clock includes PCIe copies and is reported as such; the kernel-to-kernel comparison comes from

  rocprofv3 --kernel-trace --stats --output-format csv -- python tools/liveness_bench.py --kernels

which runs both paths a few times in one process: liveness_geometry_kernel + liveness_tensor_kernel against face_tensor_kernel.
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

B, H, W = 32, 1080, 1920
DISTINCT = 4   # distinct synthetic frames; every face still reads a frame copy of its own in HBM


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--kernels", action="store_true")
    args = ap.parse_args()
    import torch
    import helpers
    import rfd_hip
    det = rfd_hip.RetinaFaceDetection(image_size=(640, 640), max_batch_size=B, max_det=64)
    cfg = rfd_hip.liveness_config()
    sizes = [(cfg.out_w[j], cfg.out_h[j]) for j in range(cfg.k)]
    out_bytes = B * 3 * 4 * sum(w * h for w, h in sizes)
    distinct = [helpers.make_image(1000 + i, H, W) for i in range(DISTINCT)]
    boxes = np.stack([helpers.make_face_kps(50 + i, H, W)[1] for i in range(B)])
    dev = torch.device("cuda", 0)
    fr = torch.from_numpy(np.stack([distinct[i % DISTINCT] for i in range(B)])).to(dev)
    ptrs, shapes = [fr.data_ptr() + i * H * W * 3 for i in range(B)], [(H, W)] * B
    d_box, d_found = torch.from_numpy(boxes).to(dev), torch.ones(B, dtype=torch.int32, device=dev)
    t = [torch.zeros(B, 3, h, w, device=dev) for w, h in sizes]
    d_w, d_r, d_s = torch.zeros(B, cfg.k, device=dev), torch.zeros(B, cfg.k, 4, dtype=torch.int32, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)
    tp = [x.data_ptr() for x in t]
    torch.cuda.synchronize()

    def live(async_=True):
        det.liveness_tensors_device(ptrs, shapes, d_box.data_ptr(), d_found.data_ptr(), tp, d_w.data_ptr(), d_r.data_ptr(), d_s.data_ptr(),
                                    cfg=cfg, async_=async_)

    # the yardstick: 112x112 crops -> the same four sizes through face_tensor_kernel (parent-commit code)
    e = rfd_hip.face_tensor_config_extraction()
    ycfgs = [rfd_hip.face_tensor_config(s, list(e.mean), list(e.scale)) for s in sizes]
    crops = np.random.default_rng(3).integers(0, 256, size=(B, 112, 112, 3), dtype=np.uint8)

    live(False)
    status, rois = d_s.cpu().numpy(), d_r.cpu().numpy()
    res = {"faces": B, "frame": [H, W], "sizes": sizes, "out_bytes": out_bytes, "status_ok": int((status == 0).sum()),
           "mean_roi_w": [round(float((rois[:, j, 2] - rois[:, j, 0] + 1).mean()), 1) for j in range(cfg.k)]}
    if args.kernels:
        for _ in range(20):
            live(False)
            det.face_tensors(crops, ycfgs)
        res["kernels"] = True
        print(json.dumps(res))
        det.close()
        return
    stream = torch.cuda.Stream()
    det.set_stream(stream.cuda_stream)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(args.warmup):
        live()
    det.sync()
    with torch.cuda.stream(stream):
        e0.record()
        for _ in range(args.calls):
            live()
        e1.record()
    e1.synchronize()
    ms = e0.elapsed_time(e1) / args.calls
    det.set_stream(None)
    res.update({"calls": args.calls, "warmup": args.warmup, "liveness_device_ms": round(ms, 4),
                "liveness_out_GBps": round(out_bytes / ms / 1e6, 1)})
    ts = []
    for i in range(args.warmup // 4 + 13):
        t0 = time.perf_counter()
        det.face_tensors(crops, ycfgs)
        ts.append(time.perf_counter() - t0)
    res["yardstick_host_form_wall_ms_incl_pcie"] = round(float(np.median(ts[-10:])) * 1e3, 3)
    print(json.dumps(res))
    det.close()


if __name__ == "__main__":
    main()
