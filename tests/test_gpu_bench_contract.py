"""GPU: bench.py's one-line JSON contract on short runs.  A plain run: the driver's keys and the
roofline of the timed region, nothing that takes a run of its own, at most 30 s outside its
steps, and with --dump-outputs the last timed step's records as float64 arrays equal to what a
caller of the same path decodes.  With --full: the cpu_baseline object and the host-to-host rate
reported beside `value`, never as it."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("cpu_baseline", "value_host_to_host", "host_to_host", "stage_ms_per_step", "stage_roofline",
             "stage_ms_per_step_pipelined", "latency_ms_single_frame", "c3_hand", "network_tflops")


def _bench(args, timeout):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    t0 = time.perf_counter()
    out = subprocess.run([sys.executable, os.path.join(REPO, "bench.py")] + args,
                         cwd=REPO, env=env, capture_output=True, text=True, timeout=timeout)
    wall = time.perf_counter() - t0
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    return json.loads(lines[0]), wall


def _headline(d, steps, warmup):
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better",
              "scaling", "vs_baseline", "dtype", "data", "config", "roofline"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == steps and d["warmup"] == warmup and d["higher_is_better"] is True
    assert d["unit"] == "frames/s" and d["scaling"] == "weak" and d["vs_baseline"] is None
    assert "workload" in d["config"] and d["frames_status_nonzero"] == 0
    assert abs(d["value"] - 32 / (d["ms_per_step"] * 1e-3)) <= 1e-6 * d["value"]
    r = d["roofline"]
    assert r["bound"] == "mfma" and r["unit"] == "TFLOP/s" and 0 < r["achieved"] < r["peak"]
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-9 and "traffic" in r


def test_bench_json_contract():
    d, _ = _bench(["--full", "--steps", "2", "--warmup", "1", "--cpu-seconds", "2", "--latency-iters", "1",
                   "--host-steps", "2"], 240)
    _headline(d, 2, 1)
    assert d["full"] is True
    for k in FULL_ONLY:
        assert k in d, k
    c = d["cpu_baseline"]
    assert c["kind"] == "port" and c["unit"] == "frames/s" and c["value"] > 0 and c["cores"] >= 1 and c["sample"]
    assert d["value_host_to_host"] > 0 and d["value_host_to_host"] != d["value"]


def test_plain_run_is_lean_and_dumps_its_outputs(tmp_path):
    """`bench.py --steps 3 --warmup 1 --dump-outputs DIR`: three timed steps and nothing beside
    them (the 7x7 roofline comes from events inside the timed steps), at most 30 s of the run
    outside its steps, and DIR/{counts,candidate,subset}.npy hold frame for frame what
    Body.infer_records + decode_records return for the bench's seeded frames."""
    dump = str(tmp_path / "dump")
    d, wall = _bench(["--steps", "3", "--warmup", "1", "--dump-outputs", dump], 120)
    _headline(d, 3, 1)
    assert d["full"] is False and d["frames_total"] == 3 * 32
    for k in FULL_ONLY:
        assert k not in d, k
    outside = wall - (3 + 1) * d["ms_per_step"] * 1e-3
    print(f"plain run: {wall:.1f} s in all, {outside:.1f} s outside its steps")
    assert outside <= 30.0

    assert sorted(os.listdir(dump)) == ["candidate.npy", "counts.npy", "subset.npy"]
    assert sum(os.path.getsize(os.path.join(dump, f)) for f in os.listdir(dump)) <= 64 << 20
    counts, cand, sub = (np.load(os.path.join(dump, n + ".npy")) for n in ("counts", "candidate", "subset"))
    assert counts.dtype == cand.dtype == sub.dtype == np.float64
    assert counts.shape == (32, 3) and cand.shape[::2] == (32, 4) and sub.shape[::2] == (32, 20)
    assert np.isfinite(cand).all() and np.isfinite(sub).all()

    import torch
    from src.body import Body
    from src.weights import BENCH_OUT_SCALE, seeded_state_dict
    body = Body(seeded_state_dict("body", 0, out_scale=BENCH_OUT_SCALE))
    frames = np.random.default_rng(1).integers(0, 256, (32, 368, 656, 3), dtype=np.uint8)  # bench.py rank 0
    rec = body.infer_records(torch.from_numpy(frames).cuda())
    body.handle.synchronize()
    for f, (c, s) in enumerate(body.decode_records(rec)):
        assert counts[f].tolist() == [0, len(c), len(s)]
        assert np.array_equal(cand[f, :len(c)], c) and not cand[f, len(c):].any(), f"frame {f}: candidates differ"
        assert np.array_equal(sub[f, :len(s)], s) and not sub[f, len(s):].any(), f"frame {f}: subsets differ"
    assert counts[:, 1].min() > 100 and counts[:, 2].min() > 5  # the crowded regime the bench measures
