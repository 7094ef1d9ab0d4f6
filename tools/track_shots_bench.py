"""What the track shots (include/rfd.h, "track shots") add to a detection + tracker call, what the route callers had before them
costs in the same run, and the copy kernel's time against its byte floor.

Input: 32 device frames of --size, one per stream, RetinaFace-R50 640x640 with synthetic weights in a context of 32, followed by
rfd_tracker_update_device on SYNTHETIC slabs of max(due, ended) rows per frame (non-overlapping boxes on a grid, the same in every
call: after the first call every row matches its track at IoU 1).  The first --due of those rows per frame are treated as due
faces whose aligned 112 x 112 crops are at hand (seeded bytes): m = 32 x due observations per call, described by a synthetic face
list, with q NULL, so every one of them is kept and its crop moves.  `ended` tracks are synthetic too: the `ended` list of every
frame names --ended serials of its stream that hold a shot (collect reads the state and changes nothing, so the same list yields
the same records in every call): 32 x ended records per call, each with its crop.

Three series, in one process, in alternating windows of --steps calls enqueued back to back and one synchronisation at the end
(milliseconds per call = host clock over the window / steps):
  alone    detection + tracker update;
  device   detection + update, then rfd_tracker_collect_ended_device and rfd_tracker_keep_shots_device: no host wait before the
           window's end;
  host     the same detection + update, then what a caller did before: WAIT, copy the due crops, due_track, first, row, stats and
           ended to the host, and keep the best crop per (stream, serial) in a dict, popping the ended ones.
The spread of the `alone` windows is the yardstick for what a difference means.
The copy kernel: windows of collect calls alone between two events, over an `ended` list that names every track of every stream
(32 x max(due, ended) records), once with `crops` set and once with `crops` NULL: the same list kernel, and the copy kernel's
launch is the only difference.  The difference per call is the copy's time with its launch, held against 2 x the bytes moved at
6.3 TB/s, the rate this project measured for a streaming kernel.
No time is fixed in advance.  Prints one JSON line per (due, ended)."""
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
    ap.add_argument("--ended", type=int, nargs="+", default=[1, 8], help="ended tracks per stream and call")
    args = ap.parse_args()

    import numpy as np
    import torch
    import helpers
    import rfd_hip

    n, md, side = 32, 1024, 112
    cb = side * side * 3
    W, H = args.size
    det = rfd_hip.RetinaFaceDetection(image_size=(640, 640), max_batch_size=n, max_det=md)
    det.init_synthetic_weights(1234)
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
    stamp = list(range(n))

    def face_list(rows):
        """frame b owns observations [b rows, (b + 1) rows), slab rows 0 .. rows - 1, whose tracks are serials 1 .. rows"""
        m = n * rows
        serial = np.zeros((n, md), np.int32)
        serial[:, :rows] = np.arange(1, rows + 1)
        o = dict(total=torch.tensor([m], dtype=i32, device=dev), first=torch.arange(0, m + 1, rows, dtype=i32, device=dev),
                 row=torch.arange(rows, dtype=i32, device=dev).repeat(n), serial=torch.from_numpy(serial).to(dev))
        return m, o, rfd_hip.rfd_track_obs(o["total"].data_ptr(), o["first"].data_ptr(), o["row"].data_ptr(), o["serial"].data_ptr())

    def detect_only():
        det.detect_device(ptrs, shapes, *[t.data_ptr() for t in own], async_=True)

    for due in args.due:
        for ended in args.ended:
            tracks = max(due, ended)
            m, o, obs = face_list(due)
            tracker = det.tracker(streams=n, max_tracks=args.max_tracks, min_score=0.5, new_score=0.5, min_hits=1)
            tracker.enable_shots(crop_w=side, crop_h=side)
            s_count = torch.full((n,), tracks, dtype=i32, device=dev)
            crops = torch.from_numpy(rng.integers(0, 256, size=(n * tracks, side, side, 3), dtype=np.uint8)).to(dev)
            status = zeros(n * tracks, dt=i32)
            # the synthetic `ended`: serials 1 .. ended of every stream, each of which gets a shot below
            h_stats, h_ended = np.zeros((n, 4), np.int32), np.zeros((n, args.max_tracks), np.int32)
            h_stats[:, 2], h_ended[:, :ended] = ended, np.arange(1, ended + 1)
            e_stats, e_ended = torch.from_numpy(h_stats).to(dev), torch.from_numpy(h_ended).to(dev)
            rcap = n * ended
            rec = dict(total=zeros(1, dt=i32), first=zeros(n + 1, dt=i32), rec=torch.zeros(rcap * 80, dtype=torch.uint8, device=dev),
                       crops=torch.zeros((rcap, side, side, 3), dtype=torch.uint8, device=dev))
            records = rfd_hip.rfd_track_records(rec["total"].data_ptr(), rec["first"].data_ptr(), rec["rec"].data_ptr(), rec["crops"].data_ptr())
            # the copy measurement's list: every track of every stream, with and without crops
            c_stats, c_ended = np.zeros((n, 4), np.int32), np.zeros((n, args.max_tracks), np.int32)
            c_stats[:, 2], c_ended[:, :tracks] = tracks, np.arange(1, tracks + 1)
            c_stats, c_ended = torch.from_numpy(c_stats).to(dev), torch.from_numpy(c_ended).to(dev)
            ccap = n * tracks
            crec = dict(total=zeros(1, dt=i32), first=zeros(n + 1, dt=i32), rec=torch.zeros(ccap * 80, dtype=torch.uint8, device=dev),
                        crops=torch.zeros((ccap, side, side, 3), dtype=torch.uint8, device=dev))
            with_crops = rfd_hip.rfd_track_records(crec["total"].data_ptr(), crec["first"].data_ptr(), crec["rec"].data_ptr(), crec["crops"].data_ptr())
            without = rfd_hip.rfd_track_records(crec["total"].data_ptr(), crec["first"].data_ptr(), crec["rec"].data_ptr(), None)
            torch.cuda.synchronize()

            def alone():
                detect_only()
                tracker.update_device(streams, s_boxes.data_ptr(), s_lmk.data_ptr(), s_count.data_ptr(), out, async_=True)

            # every track that the timed calls name holds a shot before they start
            alone()
            m_all, o_all, obs_all = face_list(tracks)
            tracker.keep_shots_device(streams, obs_all, m_all, crops.data_ptr(), status.data_ptr(), stamp=stamp)
            assert int((status.cpu().numpy()[:m_all] == 0).sum()) == m_all

            def keep():
                tracker.keep_shots_device(streams, obs, m, crops.data_ptr(), status.data_ptr(), stamp=stamp, async_=True)

            def collect_all(records_):
                tracker.collect_ended_device(streams, c_stats.data_ptr(), c_ended.data_ptr(), ccap, records_, stamp=stamp, async_=True)

            def device_route():
                alone()
                tracker.collect_ended_device(streams, e_stats.data_ptr(), e_ended.data_ptr(), rcap, records, stamp=stamp, async_=True)
                keep()

            best = {}

            def host_route():
                alone()
                det.sync()                                                                           # the wait the device route has not
                h_crops, h_due = crops[:m].cpu().numpy(), o["serial"].cpu().numpy()
                h_first, h_row = o["first"].cpu().numpy(), o["row"].cpu().numpy()
                hs, he = e_stats.cpu().numpy(), e_ended.cpu().numpy()
                done = []
                for b in range(n):                                                                   # the join by (stream, serial)
                    for e in range(hs[b, 2]):
                        done.append(best.pop((streams[b], int(he[b, e])), None))
                    for t in range(h_first[b], h_first[b + 1]):
                        best[(streams[b], int(h_due[b, h_row[t]]))] = h_crops[t]
                return done

            def window(call):
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    call()
                det.sync()
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) * 1e3 / args.steps

            def event_window(call):
                """milliseconds per call between two events on the context's stream (torch's current stream is set to it)"""
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(args.steps):
                    call()
                b.record()
                b.synchronize()
                return a.elapsed_time(b) / args.steps

            series = (("alone", alone), ("device", device_route), ("host", host_route))
            for _, call in series:
                for _ in range(args.warmup):
                    call()
                det.sync()
            ms = {name: [] for name, _ in series}
            for _ in range(args.repeats):                                   # alternating windows
                for name, call in series:
                    ms[name].append(round(window(call), 4))
            # the copy kernel: collect calls alone, on a torch stream lent to the context so that torch's events bracket them
            lent = torch.cuda.Stream(device=dev)
            det.sync()
            det.set_stream(lent.cuda_stream)
            moved, still = [], []
            try:
                with torch.cuda.stream(lent):
                    for _ in range(args.warmup):
                        collect_all(with_crops)
                        collect_all(without)
                    for _ in range(args.repeats):
                        moved.append(round(event_window(lambda: collect_all(with_crops)), 5))
                        still.append(round(event_window(lambda: collect_all(without)), 5))
                det.sync()
            finally:
                det.set_stream(None)
            kept_last = int((status.cpu().numpy()[:m] == 0).sum())              # the last keep call kept every observation
            copied = int(crec["total"].cpu().numpy()[0])
            assert copied == ccap and bool((crec["crops"][ccap - 1] == crops[(n - 1) * tracks + tracks - 1]).all())
            stats = lambda w: {"windows_ms": w, "median_ms": round(float(np.median(w)), 4), "min_ms": min(w), "max_ms": max(w)}
            med = {name: float(np.median(w)) for name, w in ms.items()}
            spread = max(ms["alone"]) - min(ms["alone"])
            copy_ms = float(np.median(moved)) - float(np.median(still))
            floor_ms = 2.0 * copied * cb / 6.3e12 * 1e3
            print(json.dumps({"streams": n, "frames_per_call": n, "due_per_stream": due, "ended_per_stream": ended, "observations_per_call": m,
                              "records_per_call": int(rec["total"].cpu().numpy()[0]), "crop": [side, side], "max_tracks": args.max_tracks,
                              "frame_size": [W, H], "steps_per_window": args.steps, "repeats": args.repeats,
                              "alone": stats(ms["alone"]), "device_route": stats(ms["device"]), "host_route": stats(ms["host"]),
                              "alone_spread_ms": round(spread, 4),
                              "device_minus_alone_median_ms": round(med["device"] - med["alone"], 4),
                              "device_minus_alone_in_spreads": round((med["device"] - med["alone"]) / spread, 1) if spread > 0 else None,
                              "host_minus_alone_median_ms": round(med["host"] - med["alone"], 4),
                              "host_minus_alone_in_spreads": round((med["host"] - med["alone"]) / spread, 1) if spread > 0 else None,
                              "collect_alone_with_crops_ms": stats(moved), "collect_alone_without_crops_ms": stats(still),
                              "copy_rows": copied, "copy_kernel_ms": round(copy_ms, 5), "copy_bytes_moved": copied * cb,
                              "copy_floor_ms": round(floor_ms, 5), "copy_over_floor": round(copy_ms / floor_ms, 1) if floor_ms > 0 else None,
                              "last_call_kept": kept_last}))
            tracker.close()
    det.close()


if __name__ == "__main__":
    main()
