#!/usr/bin/env python3
"""Time of one gallery search (rfd_gallery_search_device: 32 queries, k = 5, dim 512) over 100 k and 1 M enrolled rows, against
its floor and against torch on the same bf16 data on the same GPU.

Per size: the gallery is filled from device memory (rfd_gallery_add_device, seeded unit vectors), then --warmup searches, then
--steps searches enqueued back to back and one synchronisation; milliseconds per search = host clock over that window / steps
(scan launch + merge launch, no copies: queries and results stay in HBM).  Bytes streamed = padded rows * dim * 2 (the gallery is
read once per search); the floor is those bytes / 6.2 TB/s, the rate a streaming global_load_dwordx4 kernel reaches on the
MI355X.  The yardstick is torch.topk(q @ G.T, k) on bf16 copies of the same rows and queries, timed the same way; its product is
rounded to bf16 before the top-k, so its rows are compared with the library's only as a fraction of equal best rows.
Prints one JSON line per size."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rs-face-detection_amd", "python"))

DIM, NQ, K = 512, 32, 5
STREAM_RATE = 6.2e12   # bytes / s
CHUNK = 100_000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rows", type=int, nargs="*", default=[100_000, 1_000_000])
    args = ap.parse_args()
    import torch
    import rfd_hip
    det = rfd_hip.RetinaFaceDetection(image_size=(640, 640), max_batch_size=1, max_det=16)
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev)
    for rows in args.rows:
        gal = det.gallery(DIM, rows)
        g16 = torch.empty(rows, DIM, dtype=torch.bfloat16, device=dev)
        gen.manual_seed(rows)
        for at in range(0, rows, CHUNK):
            m = min(CHUNK, rows - at)
            x = torch.randn(m, DIM, device=dev, generator=gen)
            x = x / x.norm(dim=1, keepdim=True)
            g16[at:at + m] = x.to(torch.bfloat16)
            torch.cuda.synchronize()
            gal.add_device(x.data_ptr(), m)
            det.sync()
        assert gal.size() == rows
        q = g16[:NQ].float() + 0.02 * torch.randn(NQ, DIM, device=dev, generator=gen)   # noisy copies of enrolled rows
        q = (q / q.norm(dim=1, keepdim=True)).contiguous()
        q16 = q.to(torch.bfloat16)
        d_s = torch.zeros(NQ, K, device=dev)
        d_r = torch.zeros(NQ, K, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()

        def ours(n):
            for _ in range(n):
                gal.search_device(q.data_ptr(), NQ, K, d_s.data_ptr(), d_r.data_ptr(), async_=True)
            det.sync()

        def theirs(n):
            out = None
            for _ in range(n):
                out = torch.topk(q16 @ g16.T, K)
            torch.cuda.synchronize()
            return out

        ours(args.warmup)
        t0 = time.perf_counter()
        ours(args.steps)
        ms = (time.perf_counter() - t0) * 1e3 / args.steps
        theirs(args.warmup)
        t0 = time.perf_counter()
        ref = theirs(args.steps)
        ms_torch = (time.perf_counter() - t0) * 1e3 / args.steps
        streamed = (rows + 15) // 16 * 16 * DIM * 2
        floor_ms = streamed / STREAM_RATE * 1e3
        same_best = float((d_r[:, 0].cpu() == ref.indices[:, 0].cpu().int()).float().mean())
        found_self = float((d_r[:, 0].cpu() == torch.arange(NQ, dtype=torch.int32)).float().mean())
        print(json.dumps({"rows": rows, "dim": DIM, "queries": NQ, "k": K, "steps": args.steps, "warmup": args.warmup,
                          "search_ms": round(ms, 4), "bytes_streamed": streamed, "streamed_TB_per_s": round(streamed / ms / 1e9, 3),
                          "floor_ms_at_6.2_TB_per_s": round(floor_ms, 4), "fraction_of_floor_rate": round(floor_ms / ms, 3),
                          "torch_matmul_topk_ms": round(ms_torch, 4), "best_row_equals_torch": same_best,
                          "query_finds_its_row": found_self}), flush=True)
        gal.close()
        del g16
    det.close()


if __name__ == "__main__":
    main()
