"""bench.py prints ONE JSON line with the fields the driver and the judge read."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DUMPED = ("boxes", "landmarks", "count", "total", "image_index")


def _bench(*extra, steps=4, warmup=1):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup",
                        str(warmup)] + list(extra), capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.strip().splitlines() if l.strip()]
    assert len(lines) == 1
    return json.loads(lines[0])


def _load(d):
    return {n: np.load(os.path.join(d, n + ".npy")) for n in DUMPED}


@pytest.fixture(scope="module")
def full_run(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("dump_full"))
    return _bench("--full", "--dump-outputs", out), out


def test_bench_json_contract(full_run):
    d, _ = full_run
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 4 and d["warmup"] == 1 and d["higher_is_better"] is True
    assert d["unit"] == "images/s" and d["scaling"] == "weak" and d["vs_baseline"] is None and d["dtype"] == "bf16"
    assert "workload" in d["config"] and "model" not in d["config"]
    assert abs(d["value"] - 32 * 1000.0 / d["ms_per_step"]) < 0.01 * d["value"]
    rf = d["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in rf, k
    assert rf["bound"] in ("hbm", "mfma") and rf["unit"] in ("GB/s", "TFLOP/s") and rf["peak"] == 2500.0
    assert abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-3 and 0.02 < rf["frac"] < 1.0
    # traffic: PMC bytes per pass, measured by child rocprofv3 passes of this very run when the profiler is on the box (else the
    # committed summary, labelled); either way within a sane band of the algorithmic 13 GB of the graph as fused
    assert "traffic_source" in rf
    if rf["traffic"] is not None:
        assert 10e9 < rf["traffic"] < 25e9, rf["traffic"]
    assert rf["traffic_source"].startswith(("measured in this run", "committed summary", "none")), rf["traffic_source"]
    print("roofline.traffic = %s (%s)" % (rf["traffic"], rf["traffic_source"]))
    # the sustained window (>= 3 s of the same step) next to the short timed loop
    su = d["sustained"]
    assert su["seconds"] >= 3.0 and su["steps"] >= 10 and su["images_per_s"] > 0.8 * d["value"]
    cb = d["cpu_baseline"]
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in cb, k
    assert cb["kind"] in ("reference", "port") and cb["cores"] >= 1 and cb["value"] > 0
    assert d["value"] > 100 * cb["value"]


def test_bench_plain_run_is_lean_and_dumps_the_timed_outputs(full_run, tmp_path):
    """A plain run reports the headline figure only, for the --steps it was given, and --dump-outputs writes the detections
    of the last timed step: the same arrays as the --full run's (seeded inputs, same timed path)."""
    d = _bench("--dump-outputs", str(tmp_path), steps=7, warmup=2)
    assert d["steps"] == 7 and d["warmup"] == 2 and d["n_gpus"] == 1
    assert d["unit"] == "images/s" and d["higher_is_better"] is True and d["dtype"] == "bf16"
    assert d["metric"] == full_run[0]["metric"]
    assert abs(d["value"] - 32 * 1000.0 / d["ms_per_step"]) < 0.01 * d["value"]
    for k in ("roofline", "sustained", "cpu_baseline", "p50_ms", "value_host_path"):
        assert k not in d, k
    got, want = _load(str(tmp_path)), _load(full_run[1])
    assert sum(os.path.getsize(os.path.join(str(tmp_path), n + ".npy")) for n in DUMPED) <= 64 << 20
    assert got["boxes"].shape == (32, 1024, 5) and got["landmarks"].shape == (32, 1024, 5, 2)
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert got["count"].sum() > 0 and (got["count"] <= got["total"]).all()
    np.testing.assert_array_equal(got["image_index"], np.arange(32))
    for n in ("count", "total"):
        np.testing.assert_array_equal(got[n], want[n], err_msg=n)
    for n in ("boxes", "landmarks"):
        np.testing.assert_allclose(got[n], want[n], rtol=0, atol=1e-4, err_msg=n)
