#!/usr/bin/env python3
"""Time of one gallery search (rfd_gallery_search_device: 32 queries, k = 5, dim 512) over 100 k and 1 M enrolled rows, against
its floor and against torch on the same bf16 data on the same GPU.

Per size: the gallery is filled from device memory (rfd_gallery_add_device, seeded unit vectors), then --warmup searches, then
--steps searches enqueued back to back and one synchronisation; milliseconds per search = host clock over that window / steps
(scan launch + merge launch, no copies: queries and results stay in HBM).  Bytes streamed = padded rows * dim * 2 (the gallery is
read once per search); the floor is those bytes / 6.2 TB/s, the rate a streaming global_load_dwordx4 kernel reaches on the
MI355X.  The yardstick is torch.topk(q @ G.T, k) on bf16 copies of the same rows and queries, timed the same way; its product is
rounded to bf16 before the top-k, so its rows are compared with the library's only as a fraction of equal best rows.

--removed FRACTION measures the scan that skips removed rows against the plain one on the same gallery in the same process:
--repeats windows of --steps plain searches (their spread is the yardstick), then that share of the rows, drawn at random, is
removed (rfd_gallery_remove) and the same windows are timed on the masked scan, then the rows are put back
(rfd_gallery_replace_device with their own embeddings) and the plain windows are timed again, so a drift of the machine shows
as a difference between the two plain series.  The masked scan reads 2 more bytes per block of 16 rows.

--identities M measures the identity search (rfd_gallery_search_identities_device) against the plain one on the same gallery in
the same process: --repeats windows of plain searches, then the rows are labelled with M identities as row % M (an identity's
rows lie M apart, in every wave's walk) and the identity search is timed, then with M contiguous runs of rows (an identity's rows
arrive together), then the plain windows again; the spread of the two plain series is the yardstick.  The identity scan reads
4 bytes of identity for a key that passes a list's filter and nothing else beyond the plain scan's bytes.

--tenants T measures the filtered search (rfd_gallery_search_filtered_device) against the plain one on the same gallery in the
same process: --repeats windows of plain searches, then for each --tenant-layout the rows are tagged with T tenants, as row % T
(mod: a tenant's rows lie T apart, in every wave's walk) or in T contiguous runs (runs: a tenant's rows arrive together, and
most blocks hold nothing of it), and the filtered search is timed with mask = 0xFFFFFFFF and, per query, the tenant of the row
the query is a noisy copy of; then the plain windows again; the spread of the two plain series is the yardstick.  The filtered
scan reads the 64 bytes of a block's tags only in a block with a key that passes a list's filter.

--nearest N [N ...] measures the self-join (rfd_gallery_nearest_device of the first N rows: every row's best other row) against
the route the interface offered before it, in the same process: rfd_gallery_search_device of those rows' stored values with k = 2
(one pass over the gallery per 32 of them; the caller then drops the self-match).  Windows of the two alternate, --repeats of
each, a window holding as many calls as fit about half a second (at most --steps); the spread of the search route's windows is the
noise.  Both answers are compared.  Two floors: the matrix work N * rows * dim * 2 at 2.5 PFLOP/s, and the bytes the scan reads,
ceil(N / tile_rows) times the gallery, at the streaming rate above.  Keep N <= 65 536 at 1 M rows.
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
MFMA_RATE = 2.5e15     # bf16 FLOP / s, dense peak
CHUNK = 100_000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rows", type=int, nargs="*", default=[100_000, 1_000_000])
    ap.add_argument("--removed", type=float, default=0.0, help="share of the rows to remove at random before timing the masked scan")
    ap.add_argument("--identities", type=int, default=0, help="label the rows with this many identities and time the identity search")
    ap.add_argument("--tenants", type=int, default=0, help="tag the rows with this many tenants and time the filtered search of one tenant per query")
    ap.add_argument("--tenant-layout", nargs="+", choices=("mod", "runs"), default=["mod", "runs"], help="row %% T, or T contiguous runs of rows")
    ap.add_argument("--nearest", type=int, nargs="+", default=[], help="time the self-join of the first N rows against the search route to the same answer")
    ap.add_argument("--repeats", type=int, default=5, help="timed windows per series of a --removed, --identities, --tenants or --nearest run")
    args = ap.parse_args()
    assert 0.0 <= args.removed < 1.0 and args.identities >= 0 and args.tenants >= 0
    import torch
    import rfd_hip
    det = rfd_hip.RetinaFaceDetection(image_size=(640, 640), max_batch_size=1, max_det=16)
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev)
    for rows in args.rows:
        gal = det.gallery(DIM, rows)
        g16 = torch.empty(rows, DIM, dtype=torch.bfloat16, device=dev)
        g32 = torch.empty(rows, DIM, device=dev) if args.removed > 0 else None   # the embeddings, to put removed rows back
        gen.manual_seed(rows)
        for at in range(0, rows, CHUNK):
            m = min(CHUNK, rows - at)
            x = torch.randn(m, DIM, device=dev, generator=gen)
            x = x / x.norm(dim=1, keepdim=True)
            g16[at:at + m] = x.to(torch.bfloat16)
            if g32 is not None:
                g32[at:at + m] = x
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

        def window():
            t0 = time.perf_counter()
            ours(args.steps)
            return (time.perf_counter() - t0) * 1e3 / args.steps

        ours(args.warmup)
        ms = window()
        masked = {}
        if args.removed > 0:
            import numpy as np
            series = lambda: [round(window(), 4) for _ in range(args.repeats)]
            stats = lambda w: {"windows_ms": w, "median_ms": round(float(np.median(w)), 4), "min_ms": min(w), "max_ms": max(w)}
            plain = series()
            gone = np.sort(np.random.default_rng(rows).choice(rows, max(1, int(rows * args.removed)), replace=False)).astype(np.int32)
            gal.remove(gone)
            assert gal.live() == rows - len(gone)
            ours(args.warmup)                      # the masked instantiation's first launches
            with_mask = series()
            assert not bool(torch.isin(d_r.cpu(), torch.from_numpy(gone)).any())
            back = g32[torch.from_numpy(gone).to(dev).long()].contiguous()
            torch.cuda.synchronize()
            gal.replace_device(gone, back.data_ptr())
            det.sync()
            assert gal.live() == rows
            ours(args.warmup)
            plain_again = series()
            spread = max(plain + plain_again) - min(plain + plain_again)
            masked = {"removed_rows": int(len(gone)), "repeats": args.repeats, "plain": stats(plain), "masked": stats(with_mask),
                      "plain_again": stats(plain_again), "plain_spread_ms": round(spread, 4),
                      "masked_minus_plain_median_ms": round(float(np.median(with_mask) - np.median(plain + plain_again)), 4),
                      "masked_extra_bytes": (rows + 15) // 16 * 2}
        if args.identities > 0:
            import numpy as np
            m_ids = min(args.identities, rows)
            d_i = torch.zeros(NQ, K, dtype=torch.int32, device=dev)
            torch.cuda.synchronize()

            def ours_ids(n):
                for _ in range(n):
                    gal.search_identities_device(q.data_ptr(), NQ, K, float("-inf"), d_s.data_ptr(), d_r.data_ptr(), d_i.data_ptr(), async_=True)
                det.sync()

            def id_window():
                t0 = time.perf_counter()
                ours_ids(args.steps)
                return (time.perf_counter() - t0) * 1e3 / args.steps

            stats = lambda w: {"windows_ms": w, "median_ms": round(float(np.median(w)), 4), "min_ms": min(w), "max_ms": max(w)}
            plain = [round(window(), 4) for _ in range(args.repeats)]
            every = np.arange(rows)
            series = {}
            for name, ids in (("row_mod_m", every % m_ids), ("runs", every * m_ids // rows)):
                gal.set_identities(every, ids)
                det.sync()
                assert gal.labelled() == rows
                ours_ids(args.warmup)                  # the identity instantiation's first launches
                series[name] = [round(id_window(), 4) for _ in range(args.repeats)]
                got_r, got_i = d_r.cpu().numpy(), d_i.cpu().numpy()
                assert (got_r >= 0).all() or m_ids < K
                assert all(len(set(row[row >= 0].tolist())) == int((row >= 0).sum()) for row in got_i)   # k distinct identities per query
                assert (got_i[got_r >= 0] == ids[got_r[got_r >= 0]]).all()
            ours(args.warmup)
            plain_again = [round(window(), 4) for _ in range(args.repeats)]
            both = plain + plain_again
            masked.update({"identities": m_ids, "repeats": args.repeats, "plain": stats(plain), "identity_row_mod_m": stats(series["row_mod_m"]),
                           "identity_runs": stats(series["runs"]), "plain_again": stats(plain_again), "plain_spread_ms": round(max(both) - min(both), 4),
                           "row_mod_m_minus_plain_median_ms": round(float(np.median(series["row_mod_m"]) - np.median(both)), 4),
                           "runs_minus_plain_median_ms": round(float(np.median(series["runs"]) - np.median(both)), 4),
                           "identity_array_bytes": rows * 4})
        if args.tenants > 0:
            import numpy as np
            t_n = min(args.tenants, rows)
            d_i = torch.zeros(NQ, K, dtype=torch.int32, device=dev)
            d_mask = torch.full((NQ,), -1, dtype=torch.int32, device=dev)   # 0xFFFFFFFF: the whole word
            d_value = torch.zeros(NQ, dtype=torch.int32, device=dev)
            torch.cuda.synchronize()

            def ours_filtered(n):
                for _ in range(n):
                    gal.search_filtered_device(q.data_ptr(), NQ, K, float("-inf"), d_mask.data_ptr(), d_value.data_ptr(), d_s.data_ptr(), d_r.data_ptr(),
                                               d_i.data_ptr(), async_=True)
                det.sync()

            def filtered_window():
                t0 = time.perf_counter()
                ours_filtered(args.steps)
                return (time.perf_counter() - t0) * 1e3 / args.steps

            stats = lambda w: {"windows_ms": w, "median_ms": round(float(np.median(w)), 4), "min_ms": min(w), "max_ms": max(w)}
            plain = [round(window(), 4) for _ in range(args.repeats)]
            every = np.arange(rows)
            series = {}
            for name in args.tenant_layout:
                tags = every % t_n if name == "mod" else every * t_n // rows
                gal.set_tags(every, tags)
                d_value.copy_(torch.from_numpy(tags[:NQ].astype(np.int32)))   # query i is a noisy copy of row i
                det.sync()
                torch.cuda.synchronize()
                ours_filtered(args.warmup)             # the filtered instantiation's first launches
                series[name] = [round(filtered_window(), 4) for _ in range(args.repeats)]
                got_r = d_r.cpu().numpy()
                assert (got_r[:, 0] == np.arange(NQ)).all()                              # every query finds its row, in its tenant
                assert all((tags[row[row >= 0]] == tags[a]).all() for a, row in enumerate(got_r))   # and rows of its tenant alone
                assert (got_r >= 0).all() or rows // t_n < K
            ours(args.warmup)
            plain_again = [round(window(), 4) for _ in range(args.repeats)]
            both = plain + plain_again
            base = float(np.median(both))
            masked.update({"tenants": t_n, "repeats": args.repeats, "plain": stats(plain), "plain_again": stats(plain_again),
                           "plain_spread_ms": round(max(both) - min(both), 4), "tag_array_bytes": (rows + 15) // 16 * 64})
            for name, w in series.items():
                masked.update({"filtered_" + name: stats(w), name + "_minus_plain_median_ms": round(float(np.median(w)) - base, 4),
                               name + "_over_plain": round(float(np.median(w)) / base, 3)})
        if args.nearest:
            import numpy as np
            cus = torch.cuda.get_device_properties(0).multi_processor_count
            masked["nearest"] = []
            for n_a in args.nearest:
                n_a = min(n_a, rows)
                plan = rfd_hip.gallery_nearest_plan(rows, 0, n_a, DIM, cus)
                qa = g16[:n_a].float().contiguous()                  # the stored values of the rows: what get_rows returns
                n_s, n_r, n_i = (torch.zeros(n_a, dtype=t, device=dev) for t in (torch.float32, torch.int32, torch.int32))
                s_s, s_r = torch.zeros(n_a, 2, device=dev), torch.zeros(n_a, 2, dtype=torch.int32, device=dev)
                torch.cuda.synchronize()

                def join(n):
                    for _ in range(n):
                        gal.nearest_device(0, n_a, n_s.data_ptr(), n_r.data_ptr(), n_i.data_ptr(), async_=True)
                    det.sync()

                def route(n):
                    for _ in range(n):
                        gal.search_device(qa.data_ptr(), n_a, 2, s_s.data_ptr(), s_r.data_ptr(), async_=True)
                    det.sync()

                def timed(f):
                    f(1)                                                 # first launches, and how many calls a window holds
                    t0 = time.perf_counter()
                    f(1)
                    calls = max(1, min(args.steps, int(0.5 / max(time.perf_counter() - t0, 1e-6))))
                    return lambda: _window(f, calls), calls

                def _window(f, calls):
                    t0 = time.perf_counter()
                    f(calls)
                    return (time.perf_counter() - t0) * 1e3 / calls

                join_w, join_calls = timed(join)
                route_w, route_calls = timed(route)
                joins, routes = [], []
                for _ in range(args.repeats):                           # alternating windows
                    joins.append(round(join_w(), 4))
                    routes.append(round(route_w(), 4))
                # the two answers: the search's two best rows with the row itself dropped
                sr, ss, nr, ns = s_r.cpu().numpy(), s_s.cpu().numpy(), n_r.cpu().numpy(), n_s.cpu().numpy()
                other = np.where(sr[:, 0] == np.arange(n_a), 1, 0)
                same_rows = float((sr[np.arange(n_a), other] == nr).mean())
                same_bits = float((ss[np.arange(n_a), other].view(np.uint32) == ns.view(np.uint32)).mean())
                stats = lambda w: {"windows_ms": w, "median_ms": round(float(np.median(w)), 4), "min_ms": min(w), "max_ms": max(w)}
                j_ms, r_ms = float(np.median(joins)), float(np.median(routes))
                gallery_bytes = (rows + 15) // 16 * 16 * DIM * 2
                mfma_floor = n_a * float(rows) * DIM * 2 / MFMA_RATE * 1e3
                stream_floor = plan["tiles"] * gallery_bytes / STREAM_RATE * 1e3
                masked["nearest"].append({
                    "n": n_a, "form": plan["form"], "tile_rows": plan["tile_rows"], "tiles": plan["tiles"], "splits": plan["splits"], "grid": plan["grid"],
                    "repeats": args.repeats, "nearest_calls_per_window": join_calls, "search_route_calls_per_window": route_calls,
                    "nearest": stats(joins), "search_route_k2_groups_of_32": stats(routes), "search_route_spread_ms": round(max(routes) - min(routes), 4),
                    "search_route_over_nearest": round(r_ms / j_ms, 2),
                    "mfma_floor_ms_at_2.5_PF": round(mfma_floor, 4), "fraction_of_mfma_floor": round(mfma_floor / j_ms, 3),
                    "stream_floor_ms_at_6.2_TB_per_s": round(stream_floor, 4), "fraction_of_stream_floor": round(stream_floor / j_ms, 3),
                    "achieved_TFLOP_per_s": round(n_a * float(rows) * DIM * 2 / j_ms / 1e9, 1),
                    "rows_equal_search_route": same_rows, "score_bits_equal_search_route": same_bits})
                del qa, n_s, n_r, n_i, s_s, s_r
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
                          "query_finds_its_row": found_self, **masked}), flush=True)
        gal.close()
        del g16, g32
    det.close()


if __name__ == "__main__":
    main()
