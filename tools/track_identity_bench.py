"""What the track identities (include/rfd.h, "track identities") add to a detection + tracker call, and what the route callers had
before them costs in the same run.

Input: 32 device frames of --size, one per stream, RetinaFace-R50 640x640 with synthetic weights in a context of 32, followed by
rfd_tracker_update_device on SYNTHETIC slabs of --due rows per frame (non-overlapping boxes on a grid, the same in every call:
after the first call every row matches its track at IoU 1).  Every one of those rows is treated as a due face whose embedding
(dim 512, seeded) has come back: m = 32 x due observations per call, described by a synthetic face list.  The gallery holds 1024
seeded rows of 256 identities; k = 4.

Four series, in one process, in alternating windows of --steps calls enqueued back to back and one synchronisation at the end
(milliseconds per call = host clock over the window / steps):
  alone    detection + tracker update;
  search   the same, then rfd_normalize_embeddings_device and rfd_gallery_search_identities_device on the m embeddings: what the
           gallery costs either way, so that the rows below can be read as "beside the search";
  device   detection + update, then rfd_tracker_fuse_device, rfd_gallery_search_identities_device on the fused queries,
           rfd_tracker_label_device and rfd_tracker_who_device: no host wait before the window's end;
  host     the same detection + update, then what a caller did before: normalise the embeddings and search each on its own on the
           device, WAIT, copy track, flags, due_track and the search results to the host (the embeddings too, as a caller that
           reconciles a track's shots needs them), join them by serial in numpy into a sel array, copy sel back.
The spread of the `alone` windows is the yardstick for what a difference means.  No time is fixed in advance.  Prints one JSON line
per due count."""
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
    ap.add_argument("--due", type=int, nargs="+", default=[1, 8, 64], help="due faces per stream and call")
    args = ap.parse_args()

    import numpy as np
    import torch
    import helpers
    import rfd_hip

    n, md, dim, k, accept = 32, 1024, 512, 4, 0.05
    W, H = args.size
    det = rfd_hip.RetinaFaceDetection(image_size=(640, 640), max_batch_size=n, max_det=md)
    det.init_synthetic_weights(1234)
    L = det._L
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(3)
    bufs = [torch.from_numpy(helpers.make_image(10 + f, H, W)).to(dev) for f in range(n)]
    ptrs, shapes = [b.data_ptr() for b in bufs], [(H, W)] * n
    zeros = lambda *shape, dt=torch.float32: torch.zeros(shape, dtype=dt, device=dev)
    i32 = torch.int32
    own = (zeros(n, md, 5), zeros(n, md, 10), zeros(n, dt=i32), zeros(n, dt=i32))                     # the detector's slabs
    z = dict(track=zeros(n, md, dt=i32), flags=zeros(n, md, dt=i32), stats=zeros(n, 4, dt=i32), ended=zeros(n, args.max_tracks, dt=i32),
             due_track=zeros(n, md, dt=i32))
    out = rfd_hip.rfd_track_out(z["track"].data_ptr(), z["flags"].data_ptr(), z["stats"].data_ptr(), z["ended"].data_ptr(), rfd_hip.rfd_dets(),
                                z["due_track"].data_ptr())
    grid = np.zeros((md, 5), np.float32)
    r = np.arange(md)
    grid[:, 0], grid[:, 1] = 20 * (r % 32), 20 * (r // 32)
    grid[:, 2], grid[:, 3], grid[:, 4] = grid[:, 0] + 9, grid[:, 1] + 9, 0.9
    s_boxes, s_lmk = torch.from_numpy(np.tile(grid, (n, 1, 1))).to(dev), zeros(n, md, 10)
    streams = list(range(n))
    enrolled = rng.standard_normal((1024, dim)).astype(np.float32)
    enrolled /= np.linalg.norm(enrolled, axis=1, keepdims=True)
    gallery = det.gallery(dim=dim, capacity=1024)
    gallery.add(enrolled)
    gallery.set_identities(np.arange(1024), np.arange(1024) // 4)
    who, identity, id_score, sel = zeros(n, md, dt=i32), zeros(n, md, dt=i32), zeros(n, md), zeros(n, md, dt=i32)

    def detect_only():
        det.detect_device(ptrs, shapes, *[t.data_ptr() for t in own], async_=True)

    for due in args.due:
        m = n * due
        tracker = det.tracker(streams=n, max_tracks=args.max_tracks, min_score=0.5, new_score=0.5, min_hits=1)
        tracker.enable_identities(dim=dim, accept=accept, release=0.0, margin=0.0)
        s_count = torch.full((n,), due, dtype=i32, device=dev)
        # the synthetic face list: frame b owns observations [b due, (b + 1) due), rows 0 .. due - 1, whose tracks are serials 1 .. due
        serial = np.zeros((n, md), np.int32)
        serial[:, :due] = np.arange(1, due + 1)
        o = dict(total=torch.tensor([m], dtype=i32, device=dev), first=torch.arange(0, m + 1, due, dtype=i32, device=dev),
                 row=torch.arange(due, dtype=i32, device=dev).repeat(n), serial=torch.from_numpy(serial).to(dev))
        obs = rfd_hip.rfd_track_obs(o["total"].data_ptr(), o["first"].data_ptr(), o["row"].data_ptr(), o["serial"].data_ptr())
        emb = torch.from_numpy(rng.standard_normal((m, dim)).astype(np.float32)).to(dev)
        query, status = zeros(m, dim), zeros(m, dt=i32)
        scores, rows, ids = zeros(m, k), zeros(m, k, dt=i32), zeros(m, k, dt=i32)
        torch.cuda.synchronize()

        def alone():
            detect_only()
            tracker.update_device(streams, s_boxes.data_ptr(), s_lmk.data_ptr(), s_count.data_ptr(), out, async_=True)

        def device_route():
            alone()
            tracker.fuse_device(streams, obs, m, emb.data_ptr(), query.data_ptr(), status.data_ptr(), async_=True)
            gallery.search_identities_device(query.data_ptr(), m, k, -np.inf, scores.data_ptr(), rows.data_ptr(), ids.data_ptr(), async_=True)
            tracker.label_device(streams, obs, m, k, scores.data_ptr(), rows.data_ptr(), ids.data_ptr(), status.data_ptr(), async_=True)
            tracker.who_device(streams, z["track"].data_ptr(), s_count.data_ptr(), who.data_ptr(), flags_ptr=z["flags"].data_ptr(),
                               identity_ptr=identity.data_ptr(), id_score_ptr=id_score.data_ptr(), async_=True)

        def search_route():
            alone()
            rfd_hip._check(L.rfd_normalize_embeddings_device(det._ctx, emb.data_ptr(), m, dim, query.data_ptr()))
            gallery.search_identities_device(query.data_ptr(), m, k, -np.inf, scores.data_ptr(), rows.data_ptr(), ids.data_ptr(), async_=True)

        def host_route():
            alone()
            rfd_hip._check(L.rfd_normalize_embeddings_device(det._ctx, emb.data_ptr(), m, dim, query.data_ptr()))
            gallery.search_identities_device(query.data_ptr(), m, k, -np.inf, scores.data_ptr(), rows.data_ptr(), ids.data_ptr(), async_=True)
            det.sync()                                                                               # the wait the device route has not
            h_track, h_flags, h_due = z["track"].cpu().numpy(), z["flags"].cpu().numpy().view(np.uint32), o["serial"].cpu().numpy()
            h_emb, h_scores, h_ids = emb.cpu().numpy(), scores.cpu().numpy(), ids.cpu().numpy()
            h_sel = h_flags.copy()
            named = (h_scores[:, 0] >= accept) & (h_ids[:, 0] >= 0)
            for b in range(n):                                                                       # the join by serial
                t = np.arange(b * due, (b + 1) * due)
                good = h_due[b, :due][named[t]]
                h_sel[b, :due] |= np.where(np.isin(h_track[b, :due], good), np.uint32(8), np.uint32(0))
            sel.copy_(torch.from_numpy(h_sel.view(np.int32)))
            return h_emb

        def window(call):
            t0 = time.perf_counter()
            for _ in range(args.steps):
                call()
            det.sync()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3 / args.steps

        series = (("alone", alone), ("search", search_route), ("device", device_route), ("host", host_route))
        for _, call in series:
            for _ in range(args.warmup):
                call()
            det.sync()
        ms = {name: [] for name, _ in series}
        for _ in range(args.repeats):                                   # alternating windows
            for name, call in series:
                ms[name].append(round(window(call), 4))
        stats = lambda w: {"windows_ms": w, "median_ms": round(float(np.median(w)), 4), "min_ms": min(w), "max_ms": max(w)}
        med = {name: float(np.median(w)) for name, w in ms.items()}
        fused = int((status.cpu().numpy() == 0).sum())
        print(json.dumps({"streams": n, "frames_per_call": n, "due_per_stream": due, "observations_per_call": m, "dim": dim, "k": k,
                          "gallery_rows": 1024, "max_tracks": args.max_tracks, "frame_size": [W, H], "steps_per_window": args.steps,
                          "repeats": args.repeats, "alone": stats(ms["alone"]), "search_route": stats(ms["search"]), "device_route": stats(ms["device"]), "host_route": stats(ms["host"]),
                          "alone_spread_ms": round(max(ms["alone"]) - min(ms["alone"]), 4),
                          "device_minus_alone_median_ms": round(med["device"] - med["alone"], 4),
                          "host_minus_alone_median_ms": round(med["host"] - med["alone"], 4),
                          "search_minus_alone_median_ms": round(med["search"] - med["alone"], 4),
                          "device_minus_search_median_ms": round(med["device"] - med["search"], 4),
                          "host_minus_search_median_ms": round(med["host"] - med["search"], 4),
                          "last_call_fused": fused, "last_call_named_rows": int(((who.cpu().numpy() & 8) != 0).sum())}))
        tracker.close()
    gallery.close()
    det.close()


if __name__ == "__main__":
    main()
