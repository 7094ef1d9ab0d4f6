#!/usr/bin/env python3
"""bench.py -- the headline benchmark of BASELINE.json on MI355X.

metric : images/s (+ p50 latency) of the whole detection hot path -- letterbox preprocess, RetinaFace-R50
         forward (bf16 MFMA implicit-GEMM convs), decode, sort, NMS, rescale -- on 640x640 frames, batch 32
         per GPU (BASELINE.json configs[2]), frames already resident in HBM when the clock starts.
N > 1  : one process per GPU (torch.distributed, backend nccl = RCCL), every rank runs its own shard of 32
         frames (weak scaling) and the per-rank detection slabs are all-gathered over xGMI each step.
         `python bench.py --gpus N` without a launcher spawns the N ranks itself (the parent never touches the GPU).
Prints ONE JSON line on rank 0.  A plain run sets up, warms up, times --steps steps and reports the headline figure
(`value`, `ms_per_step`, `config`); --dump-outputs DIR also writes the detections of the last timed step as .npy files
(seeded synthetic inputs: identical from run to run, so that two builds can be compared output for output).
--full adds everything beside the headline figure, each leg after the timed steps:  `sustained` (>= 3 s of the same
step), `p50_ms`, `stage_ms`; `roofline`, measured live with HIP events (rfd_set_profiling / rfd_stats) and two child
`rocprofv3 --pmc` runs for its traffic; `value_host_path`, the PCIe-inclusive rate of the same workload through
rfd_submit_batch / rfd_collect_batch (page-locked host frames in, host detections out, two batches in flight) --
reported beside `value`, never as it; `cpu_baseline`, the restated CPU path (plain f32 torch-CPU forward + the C
oracle) timed on a bounded sample on rank 0 at N = 1.
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
for p in (ROOT, os.path.join(ROOT, "rs-face-detection_amd", "python"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

ASYNC_MODE = int(os.environ.get("RFD_BENCH_ASYNC", "2"))  # 1: every step ordered on one stream; 2: cross-step overlap
BATCH = int(os.environ.get("RFD_BENCH_BATCH", "32"))  # 32 is the headline configuration
IMAGE = 640
# source frame size (h, w); default = the network size.  RFD_BENCH_SRC=1080x1920 gives BASELINE.json configs[3]'s per-GPU slice
SRC_H, SRC_W = (int(v) for v in os.environ.get("RFD_BENCH_SRC", "640x640").split("x"))
MAX_DET = 1024
PEAK_BF16_TFLOPS = 2500.0  # dense bf16 MFMA peak, /opt/skills/guides/MI355X_MICROARCH.md
TARGET_CAND_RATE = 0.006   # ~100 candidates / image, a realistic operating point


def calibrate_cls_bias(det, graph, frames_np):
    """Random weights give arbitrary score statistics: shift the fg logits of the three heads so that
    TARGET_CAND_RATE of the anchors clear the 0.7 threshold (setup, outside the timed region)."""
    _, tensor, _ = det.preprocess(frames_np[:2])
    heads = det.forward(tensor)
    p = np.concatenate([heads[3 * l][:, 2:4].reshape(-1) for l in range(3)]).astype(np.float64)
    p = np.clip(p, 1e-7, 1 - 1e-7)
    d = np.log(p / (1 - p))
    delta = float(np.log(0.7 / 0.3) - np.quantile(d, 1.0 - TARGET_CAND_RATE))
    for i, L in enumerate(graph.layers):
        if L.name.decode().startswith("head"):
            w, b = det.get_layer(i, L)
            b[2:4] += delta
            det.set_layer(i, w, b)
    return delta


def cpu_baseline(frames_np, thr):
    """The reference's CPU path restated (kind "port"): C oracle preprocess (1 thread, as the reference) -> plain f32
    forward of the RetinaFace-R50 of SURVEY Appendix B on torch-CPU (BatchNorm folded, channels_last, inference_mode, all
    host threads: stands in for a Triton-CPU backend) -> C oracle decode + NMS (1 thread).  Batch 1 is the reference's
    operating point (config.rs:28); batch 32 is the metric's.  Bounded to ~15 s of wall time."""
    import unfolded_ref
    from oracle import oracle as O
    model = unfolded_ref.FoldedF32(unfolded_ref.make_params(1234))
    # threads = the CPU share this process really has (cgroup quota / affinity), not the host's core count: torch would
    # otherwise start one thread per host core and oversubscribe its share
    cores = len(os.sched_getaffinity(0))
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()
        if q != "max":
            cores = max(1, min(cores, int(int(q) / int(per))))
    except (OSError, ValueError):
        pass
    torch.set_num_threads(cores)

    def timed_pass(n):
        t0 = time.perf_counter()
        pre = [O.preprocess(f, IMAGE, IMAGE) for f in frames_np[:n]]
        t1 = time.perf_counter()
        heads = [h.contiguous().numpy() for h in model.forward(torch.from_numpy(np.stack([p[1] for p in pre])))]
        t2 = time.perf_counter()
        for b in range(n):
            O.decode_nms([h[b] for h in heads], IMAGE, IMAGE, np.float32(thr), 0.45, float(pre[b][2]))
        t3 = time.perf_counter()
        return t3 - t0, (t1 - t0, t2 - t1, t3 - t2)

    res = {}
    for n, warm, budget, min_reps in ((1, 5, 4.0, 5), (32, 1, 8.0, 2)):
        for _ in range(warm):
            timed_pass(n)
        ts, parts, t_start = [], [], time.perf_counter()
        while len(ts) < min_reps or (time.perf_counter() - t_start < budget and len(ts) < 50):
            t, pr = timed_pass(n)
            ts.append(t)
            parts.append(pr)
        med = float(np.median(ts))
        pm = np.median(np.asarray(parts), axis=0)
        res[n] = {"images_per_s": round(n / med, 3), "p50_ms": round(med * 1e3, 2), "passes": len(ts), "warmup": warm,
                  "stage_ms": {"preprocess": round(pm[0] * 1e3, 2), "network": round(pm[1] * 1e3, 2), "decode_nms": round(pm[2] * 1e3, 2)}}
    return {"value": res[32]["images_per_s"], "unit": "images/s", "cores": cores, "kind": "port",
            "sample": "batch 32: %d passes after %d warm-up (p50 %.0f ms / batch); batch 1 (the reference's operating point): "
                      "%d passes after 5 warm-up; C oracle preprocess + plain f32 torch-CPU R50 forward (BN folded, "
                      "channels_last, inference_mode, %d threads: stands in for Triton-CPU) + C oracle decode/NMS; random "
                      "weights of the same architecture" % (res[32]["passes"], res[32]["warmup"], res[32]["p50_ms"],
                                                            res[1]["passes"], cores),
            "batch32": res[32], "batch1": res[1], "value_batch1": res[1]["images_per_s"]}


def measure_traffic_live():
    """Two child runs of this script under `rocprofv3 --pmc` (FETCH_SIZE, then WRITE_SIZE) -> HBM bytes per forward pass of the
    network kernels, or None.  The children are ordinary child processes started with subprocess (no exec from this process);
    under the profiler the program after `--` is python3 itself."""
    import shutil
    import tempfile
    exe = shutil.which("rocprofv3")
    if exe is None or os.environ.get("RFD_BENCH_CHILD") or any(k.startswith("ROCPROF") for k in os.environ):
        return None
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import rocpd_summary
    except Exception:
        return None
    tmp = tempfile.mkdtemp(prefix="rfd_pmc_", dir="/tmp")
    env = dict(os.environ, RFD_BENCH_CHILD="1", RFD_BENCH_HOST_PATH="0", RFD_BENCH_SUSTAIN="0", RFD_BENCH_TRAFFIC="off",
               RFD_STREAM_TUNE="0", RFD_BENCH_ASYNC="1", TMPDIR="/tmp")
    dbs = {}
    try:
        for ctr in ("FETCH_SIZE", "WRITE_SIZE"):
            out = os.path.join(tmp, ctr)
            r = subprocess.run([exe, "--pmc", ctr, "-d", out, "--", sys.executable, os.path.abspath(__file__), "--no-cpu-baseline",
                                "--full", "--steps", "4", "--warmup", "1"], cwd=tmp, env=env, stdout=subprocess.DEVNULL,
                               stderr=subprocess.DEVNULL, timeout=240)
            if r.returncode != 0:
                return None
            found = [os.path.join(d, f) for d, _, fs in os.walk(out) for f in fs if f.endswith("_results.db")]
            if not found:
                return None
            dbs[ctr] = found[0]
        summ = os.path.join(tmp, "hbm_traffic.json")
        import contextlib
        import io
        with contextlib.redirect_stdout(io.StringIO()):  # the summariser prints; this script prints exactly one line
            rocpd_summary.pmc(dbs["FETCH_SIZE"], dbs["WRITE_SIZE"], summ)
        res = json.load(open(summ))
        try:  # keep the per-kernel table of this run next to the other outputs (scratch; copied to profiles/ by hand)
            os.makedirs(os.path.join(ROOT, "gpurun_out"), exist_ok=True)
            shutil.copy(summ, os.path.join(ROOT, "gpurun_out", "bench_hbm_traffic_live.json"))
        except OSError:
            pass
        return float(res["conv_igemm_hbm_bytes_per_pass"])
    except Exception as e:  # noqa: BLE001
        sys.stderr.write("live PMC traffic measurement failed: %s\n" % e)
        return None
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def timed_outputs(slab, gslabs, gathered, world):
    """What a caller of the timed step receives: ([(det [K,5], kps [K,5,2]) per image], total [n]) -- the local slab at
    N = 1, every rank's slab after the all-gather (rank-major, i.e. the global image order) at N > 1."""
    from rfd_hip import parallel
    if gslabs is not None:
        return gslabs.unpack()
    if world > 1:
        g = gathered.view(world, slab.words)
        return parallel.unpack_gathered(slab, g), np.concatenate([slab.total(g[r]).cpu().numpy() for r in range(world)])
    return slab.unpack(), slab.total().cpu().numpy()


def dump_outputs(dirname, dets, totals, limit=64 << 20):
    """--dump-outputs: boxes [n, max_det, 5] and landmarks [n, max_det, 5, 2] as float32, rows past an image's count zeroed
    (the slab leaves them unspecified); count, total and image_index [n] as float64.  Above `limit` bytes a fixed seeded
    sample of the images is written, in ascending image order."""
    idx = np.arange(len(dets))
    per_image = MAX_DET * 15 * 4 + 3 * 8
    if len(idx) * per_image > limit:
        idx = np.sort(np.random.default_rng(0).choice(len(idx), limit // per_image, replace=False))
    boxes = np.zeros((len(idx), MAX_DET, 5), np.float32)
    lmk = np.zeros((len(idx), MAX_DET, 5, 2), np.float32)
    count = np.zeros(len(idx))
    for j, i in enumerate(idx):
        d, k = dets[i]
        boxes[j, :len(d)], lmk[j, :len(d)], count[j] = d, k, len(d)
    os.makedirs(dirname, exist_ok=True)
    for name, a in (("boxes", boxes), ("landmarks", lmk), ("count", count), ("total", np.asarray(totals, np.float64)[idx]),
                    ("image_index", idx.astype(np.float64))):
        np.save(os.path.join(dirname, name + ".npy"), a)


def spawn_ranks(args):
    """`python bench.py --gpus N` without a launcher: start N fresh rank processes (RANK / LOCAL_RANK / WORLD_SIZE /
    MASTER_* set) BEFORE anything in this process touches the GPU, relay rank 0's JSON line, fail if any rank fails."""
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    procs = []
    for r in range(args.gpus):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(args.gpus), LOCAL_WORLD_SIZE=str(args.gpus),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        cmd = [sys.executable, os.path.abspath(__file__), "--gpus", str(args.gpus), "--steps", str(args.steps),
               "--warmup", str(args.warmup)] + (["--no-cpu-baseline"] if args.no_cpu_baseline else [])
        cmd += (["--full"] if args.full else []) + (["--dump-outputs", args.dump_outputs] if args.dump_outputs else [])
        procs.append(subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE if r == 0 else subprocess.DEVNULL, text=True))
    out0 = procs[0].communicate()[0]
    codes = [procs[0].returncode] + [p.wait() for p in procs[1:]]
    sys.stdout.write(out0)
    sys.stdout.flush()
    bad = [c for c in codes if c != 0]
    return bad[0] if bad else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--full", action="store_true",
                    help="also measure everything beside the headline figure: sustained window, p50 latency, host path, "
                         "roofline, live PMC traffic, CPU baseline")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="write the detections of the last timed step to DIR/<name>.npy")
    args = ap.parse_args()

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        raise SystemExit(spawn_ranks(args))  # this process has made no GPU call
    if world != args.gpus:
        raise SystemExit("--gpus %d but WORLD_SIZE=%d" % (args.gpus, world))
    import torch.distributed as dist
    if os.environ.get("RFD_BENCH_DRYRUN"):
        # launcher rehearsal without a GPU (tests/test_parallel_cpu.py): rendezvous over gloo, one collective, one line
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if world > 1:
            dist.init_process_group("gloo")
        t = torch.tensor([rank + 1], dtype=torch.int64)
        if world > 1:
            dist.all_reduce(t)
            dist.destroy_process_group()
        if os.environ.get("RFD_BENCH_DRYRUN_FAIL_RANK") == str(rank):
            raise SystemExit(3)
        if rank == 0:
            print(json.dumps({"dryrun": True, "n_gpus": world, "rank_sum": int(t.item()), "steps": args.steps, "warmup": args.warmup}))
        return
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        torch.cuda.set_device(local_rank)
        dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
    else:
        torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)

    import helpers
    import rfd_hip
    from rfd_hip import parallel

    det = rfd_hip.RetinaFaceDetection(image_size=(IMAGE, IMAGE), max_batch_size=BATCH, device_id=local_rank,
                                      max_det=MAX_DET)
    det.init_synthetic_weights(1234)
    graph = rfd_hip.Graph(rfd_hip.BACKBONE_R50, IMAGE, IMAGE)

    # synthetic 640x640 BGR frames (seed 1 + global image index), resident in HBM
    frames_np = [helpers.make_image(1000 + rank * BATCH + i, SRC_H, SRC_W) for i in range(BATCH)]
    delta = calibrate_cls_bias(det, graph, frames_np)
    frames = torch.from_numpy(np.stack(frames_np)).to(dev)
    fptrs = [frames.data_ptr() + i * SRC_H * SRC_W * 3 for i in range(BATCH)]
    shapes = [(SRC_H, SRC_W)] * BATCH
    slab = parallel.DetectionSlab(BATCH, MAX_DET, device=dev)
    pb, pl, pc, pt = slab.pointers()
    gathered = torch.empty(world * slab.words, dtype=torch.int32, device=dev) if world > 1 else None
    # N > 1: the gather is the library's own RCCL all-gather behind the C ABI (rfd_comm_init / rfd_gather_detections,
    # what a Rust host would call); torch.distributed only carries the 128-byte unique id, the barrier and the timing
    # reduction.  RFD_BENCH_GATHER=torch uses torch.distributed.all_gather_into_tensor instead (same bytes, same stream).
    gather_impl, gslabs = "none", None
    if world > 1:
        gather_impl = "torch.distributed"
        if os.environ.get("RFD_BENCH_GATHER", "abi") == "abi":
            ok = torch.ones(1, dtype=torch.int32, device=dev)
            try:
                rfd_hip.RetinaFaceDetection.comm_unique_id()  # probe: can this rank load librccl at all?
            except Exception as e:  # noqa: BLE001
                sys.stderr.write("rank %d: RCCL behind the C ABI unavailable (%s); falling back to torch.distributed\n" % (rank, e))
                ok.zero_()
            dist.all_reduce(ok, op=dist.ReduceOp.MIN)
            if int(ok.item()) == 1:
                parallel.init_comm(det)
                gslabs = parallel.GatheredSlabs(world, BATCH, MAX_DET, dev)
                gather_impl = "rfd_gather_detections (RCCL ncclAllGather behind the C ABI)"

    stream = torch.cuda.current_stream()
    det.set_stream(stream.cuda_stream)  # detector, RCCL and torch share one stream order
    if os.environ.get("RFD_BENCH_TILE"):  # experiment knob: forced conv tile configuration (rfd_debug_set_conv_tile)
        det.debug_set_conv_tile(int(os.environ["RFD_BENCH_TILE"]))
    if os.environ.get("RFD_BENCH_CONC"):  # experiment knob: "multi_stream,split_min_part,split_max_parts,use_graph"
        ms, sp, mp_, gr = (int(v) for v in os.environ["RFD_BENCH_CONC"].split(","))
        det.debug_set_concurrency(bool(ms), sp, mp_, bool(gr))

    def step():
        # async 2: the frames are complete in HBM, so the chains of this step may overlap the previous step's tail
        det.detect_device(fptrs, shapes, pb, pl, pc, pt, async_=ASYNC_MODE)
        if gslabs is not None:
            det.gather_detections((pb, pl, pc, pt), BATCH, gslabs.pointers())
        elif world > 1:
            parallel.gather_detections(slab, out=gathered)

    # set-up pass, outside warm-up and timing: the network's one-off choice of chain streams (Network::tune_streams)
    # happens in the first split pass and takes about half a second
    det.detect_device(fptrs, shapes, pb, pl, pc, pt, async_=0)

    def fence():
        det.sync()
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()

    for _ in range(args.warmup):
        step()
    fence()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    det.sync()
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    if world > 1:
        dist.barrier()
    elapsed = torch.tensor([t1 - t0], dtype=torch.float64, device=dev)
    if world > 1:
        dist.all_reduce(elapsed, op=dist.ReduceOp.MAX)
    elapsed = float(elapsed.item())

    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, *timed_outputs(slab, gslabs, gathered, world))

    # rfd_stats of the last synchronous pass (in a plain run the set-up pass): same frames, same candidates as the timed steps
    stats = det.stats()
    totals = slab.total().cpu().numpy()

    # everything beside the headline figure: only with --full
    if args.full:
        # sustained rate: the same step for >= 3 s of wall time (the timed loop above is a ~0.1 s burst at the driver's default
        # K; this window is long enough for clocks / power management to settle and for an SMI sampler to see the GPU busy)
        sustained = None
        if os.environ.get("RFD_BENCH_SUSTAIN", "1") != "0":
            sus_s = float(os.environ.get("RFD_BENCH_SUSTAIN_S", "3.0"))
            chunk = max(args.steps, 10)
            fence()
            # (the stop decision is collective -- parallel.run_for_at_least: every step() of a multi-rank job holds an all-gather)
            sus_elapsed, ssteps = parallel.run_for_at_least(step, lambda: (det.sync(), torch.cuda.synchronize()), sus_s, chunk, world, dev)
            if world > 1:
                dist.barrier()
            sus = torch.tensor([sus_elapsed, float(ssteps)], dtype=torch.float64, device=dev)
            if world > 1:  # whole-job figure: all ranks' images over the slowest rank's window
                t_max = sus[:1].clone(); dist.all_reduce(t_max, op=dist.ReduceOp.MAX)
                n_sum = sus[1:].clone(); dist.all_reduce(n_sum, op=dist.ReduceOp.SUM)
                sus_t, sus_n = float(t_max.item()), float(n_sum.item())
            else:
                sus_t, sus_n = float(sus[0].item()), float(sus[1].item())
            sustained = {"seconds": round(sus_t, 3), "steps": int(ssteps), "images_per_s": round(BATCH * sus_n / sus_t, 2),
                         "ms_per_step": round(sus_t / ssteps * 1e3, 4),
                         "note": "same step() as the timed loop, synchronised every %d steps" % chunk}

        # p50 latency of one synchronous step (batch of 32 end to end)
        lat = []
        for _ in range(min(args.steps, 20)):
            fence()
            a = time.perf_counter()
            step()
            det.sync()
            torch.cuda.synchronize()
            lat.append((time.perf_counter() - a) * 1e3)
        p50 = float(np.median(lat))

        # PCIe-inclusive rate of the same workload (H2D of u8 frames ... D2H of detections): page-locked host
        # frames through rfd_submit_batch / rfd_collect_batch, two batches in flight.  Reported beside `value`, never as it.
        host_path = None
        if world == 1 and os.environ.get("RFD_BENCH_HOST_PATH", "1") != "0":
            hsets = []
            for k in range(2):
                buf = det.host_frames(BATCH, SRC_H, SRC_W)
                for i in range(BATCH):
                    buf[i] = frames_np[i]
                hsets.append([buf[i] for i in range(BATCH)])
            det.submit(hsets[0]); det.submit(hsets[1]); det.collect(); det.collect()
            hsteps = max(args.steps, 8)
            fence()
            h0 = time.perf_counter()
            det.submit(hsets[0])
            for k in range(1, hsteps):
                det.submit(hsets[k & 1])
                det.collect()
            det.collect()
            h1 = time.perf_counter()
            host_path = {"value_host_path": round(BATCH * hsteps / (h1 - h0), 2), "ms_per_step_host_path": round((h1 - h0) / hsteps * 1e3, 4),
                         "steps_host_path": hsteps}

        # roofline of the dominant kernel class (implicit-GEMM convs): HIP events around every launch
        det.set_profiling(True)
        conv_ms, conv_flops, launches = [], 0.0, 0
        op_ms = np.zeros(graph.num_ops)
        reps = 5
        for _ in range(reps):
            det.detect_device(fptrs, shapes, pb, pl, pc, pt, async_=False)
            ms, fl, nl = det.conv_profile()
            conv_ms.append(ms)
            conv_flops, launches = fl, nl
            op_ms += det.op_profile(graph.num_ops)
        det.set_profiling(False)
        stats = det.stats()
        conv_ms_med = float(np.median(conv_ms))
        serial_tflops = conv_flops / (conv_ms_med * 1e-3) / 1e12
        op_ms /= reps
        # In the timed configuration the network runs as two overlapped half-batch chains (+ side streams), so single
        # launches cannot be timed in isolation; the class is timed as a whole: HIP events on the caller's stream at the
        # fork and after the join of the network pass (rfd_stats.ms_network), all conv FLOPs of the pass over that time.
        net_ms = []
        for _ in range(10):
            det.detect_device(fptrs, shapes, pb, pl, pc, pt, async_=False)
            net_ms.append(det.stats()["ms_network"])
        net_ms_med = float(np.median(net_ms))
        net_flops = 2.0 * graph.macs * BATCH
        achieved = net_flops / (net_ms_med * 1e-3) / 1e12

        # HBM traffic of the network kernels per forward pass, from the PMC counters: FETCH_SIZE and WRITE_SIZE in SEPARATE rocprofv3
        # passes (they do not fit one pass), FETCH_SIZE x2 on gfx950 (wide reads / LDS-DMA are tallied at half their bytes), KiB ->
        # bytes -- see tools/rocpd_summary.py.  Counters cannot be read from inside the process, so
        # rank 0 runs this same script twice as a CHILD under `rocprofv3 --pmc` (4 steps each, calls ordered on one stream: under PMC
        # every dispatch runs alone anyway) and summarises the two databases: the figure belongs to THIS run on THIS box.  If the
        # profiler is missing, fails or times out, the last committed summary is reported and labelled as such.
        traffic, traffic_source = None, "none"
        if rank == 0 and world == 1 and BATCH == 32 and os.environ.get("RFD_BENCH_TRAFFIC", "live") == "live":
            traffic = measure_traffic_live()
            if traffic is not None:
                traffic_source = "measured in this run: child `rocprofv3 --pmc FETCH_SIZE` / `--pmc WRITE_SIZE` passes of bench.py --steps 4"
        tpath = os.path.join(ROOT, "profiles", "hbm_traffic_latest.json")
        if traffic is None and BATCH == 32 and os.path.exists(tpath):
            try:
                traffic = float(json.load(open(tpath))["conv_igemm_hbm_bytes_per_pass"])
                traffic_source = "committed summary profiles/hbm_traffic_latest.json (tools/profile_bench.sh), not this run"
            except Exception:
                traffic = None

    out = None
    if rank == 0:
        value = world * BATCH * args.steps / elapsed
        out = {
            "metric": "images/sec + p50 latency, RetinaFace-R50 640x640 b32 (end-to-end detect: preprocess + CNN + decode + NMS; "
                      "`value` = frames resident in HBM, `value_host_path` = SURVEY 8(d)'s H2D -> ... -> D2H figure)",
            "value": round(value, 2), "unit": "images/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(elapsed / args.steps * 1e3, 4), "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": "bf16", "data": "synthetic",
            "config": {"workload": "RetinaFace-ResNet50 640x640 batch=32 bf16 per GPU (BASELINE.json configs[2])",
                       "batch_per_gpu": BATCH, "global_batch": BATCH * world, "image_size": [IMAGE, IMAGE],
                       "source_frames": "%dx%dx3 u8 synthetic, resident in HBM" % (SRC_W, SRC_H), "max_det": MAX_DET,
                       "timed_region": "value: u8 frames already in HBM, detections left in HBM (PCIe excluded); value_host_path: "
                                       "page-locked host frames in, host detections out (PCIe included, SURVEY 8(d))",
                       "weights": "seeded synthetic (no model file exists in the reference), cls bias calibrated %+.3f" % delta,
                       "parallelism": "image-parallel x%d, RCCL all-gather of detection slabs via %s" % (world, gather_impl) if world > 1 else "single GPU",
                       "candidates_per_image": round(float(stats["candidates"]) / BATCH, 1),
                       "detections_per_image": round(float(totals.mean()), 1)},
        }
        if args.full:
            out.update({
                "p50_ms": round(p50, 4),
                "p50_ms_per_image": round(p50 / BATCH, 5),
                "stage_ms": dict({k: round(stats[k], 4) for k in ("ms_preprocess", "ms_decode", "ms_sort", "ms_nms")},
                                 ms_network=round(net_ms_med, 4)),
                "roofline": {"bound": "mfma", "achieved": round(achieved, 2), "peak": PEAK_BF16_TFLOPS, "unit": "TFLOP/s",
                             "frac": round(achieved / PEAK_BF16_TFLOPS, 4), "traffic": traffic,
                             "traffic_unit": "HBM bytes per forward pass of the network conv kernels (PMC: FETCH_SIZE x2 + WRITE_SIZE)",
                             "traffic_source": traffic_source,
                             "hbm_frac_of_8TBps": round(traffic / (net_ms_med * 1e-3) / 8e12, 4) if traffic else None,
                             "kernel": "network conv kernels of one forward pass (stem_persistent / conv_igemm / conv_ring / conv3x3_kx / conv3x3_halo / "
                                       "conv3x3_c64 / pw_stream / pw_gemm / pw_wide / pw_b2b / pw_pair / conv_b2b_s1), timed as a class: the two "
                                       "half-batch chains overlap",
                             "flops_per_pass": net_flops, "ms_per_pass": round(net_ms_med, 4),
                             "serialised": {"note": "same pass with every op on one stream, HIP events around each of the %d "
                                                    "implicit-GEMM launches (conv0/stem excluded)" % launches,
                                            "flops_per_pass": conv_flops, "ms_per_pass": round(conv_ms_med, 4),
                                            "tflops": round(serial_tflops, 2),
                                            "avg_launch_us": round(conv_ms_med * 1e3 / max(launches, 1), 2)}},
            })
            if sustained:
                out["sustained"] = sustained
                out["sustained_vs_value"] = round(sustained["images_per_s"] / value, 4)
            if host_path:
                out.update(host_path)
                out["host_path_note"] = ("same workload with frames in page-locked HOST memory and detections returned to the host "
                                         "(rfd_submit_batch / rfd_collect_batch, two batches in flight, per rank); `value` is the "
                                         "HBM-resident rate")
            if world == 1 and not args.no_cpu_baseline:
                out["cpu_baseline"] = cpu_baseline(frames_np, 0.7)
            else:
                out["cpu_baseline"] = None
            if os.environ.get("RFD_BENCH_OPS"):
                rows = []
                for i, o in enumerate(graph.ops):
                    L = graph.layers[o.layer]
                    t = graph.tensors[o.out if o.out >= 0 else (o.out2 if o.out2 >= 0 else o.outf)]
                    fl = 2.0 * o.macs * BATCH
                    rows.append("%3d %-22s k%d s%d %4d->%4d @%3dx%-3d %8.1f us %7.1f TF" % (
                        i, L.name.decode() if o.kind != 1 else "maxpool", L.kh, L.stride, L.cin, L.cout, t.height,
                        t.width, op_ms[i] * 1e3, fl / (op_ms[i] * 1e-3) / 1e12 if op_ms[i] > 0 else 0))
                sys.stderr.write("\n".join(rows) + "\n")
    if gslabs is not None:
        det.comm_destroy()
    det.set_stream(None)
    det.close()
    if world > 1:
        dist.destroy_process_group()
    if rank == 0:
        print(json.dumps(out))


if __name__ == "__main__":
    main()
