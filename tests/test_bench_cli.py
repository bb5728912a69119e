"""bench.py's launcher contract on the CPU: `--gpus N` is the job's rank
count. More ranks than the box has GPUs, or a launcher world size that
disagrees with --gpus, exits non-zero before touching a GPU -- never a
silent single-GPU line. A run without --full measures and
prints the headline only, and --dump-outputs writes the last timed step's
assign[] (checked on the GPU against the oracle)."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, env_extra=None):
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    env.update(env_extra or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, capture_output=True,
                          text=True, timeout=300)


def test_more_gpus_than_the_box_has_fails():
    import torch
    n = torch.cuda.device_count()  # counting does not initialise a GPU
    r = _run(["--gpus", str(n + 1), "--steps", "1", "--warmup", "0"])
    assert r.returncode != 0
    assert "GPU" in r.stderr and '"metric"' not in r.stdout


def test_world_size_disagreeing_with_gpus_fails():
    r = _run(["--gpus", "2"], {"WORLD_SIZE": "1", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode != 0
    assert "WORLD_SIZE=1" in r.stderr and '"metric"' not in r.stdout


def test_gpus_must_be_positive():
    r = _run(["--gpus", "0"])
    assert r.returncode != 0 and '"metric"' not in r.stdout


def _bench():
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    return b


def test_dump_outputs_writes_float64_npy(tmp_path):
    """--dump-outputs DIR: assign[] as DIR/assign.npy, float64, values kept
    (-1 = not placed), the directory created when missing."""
    import numpy as np
    b = _bench()
    a = np.array([3, -1, 0, 999], dtype=np.int32)
    out = tmp_path / "deep" / "dir"
    b.dump_outputs(str(out), a)
    got = np.load(out / "assign.npy")
    assert got.dtype == np.float64 and got.tolist() == [3.0, -1.0, 0.0, 999.0]
    assert sorted(os.listdir(out)) == ["assign.npy"]


def test_plain_line_has_the_headline_and_no_other_leg():
    """The line of a run without --full: built from the timed steps' figures
    alone, every contract field of the headline present, no block of a leg
    that only --full measures."""
    import json
    b = _bench()
    c2 = {"value": 1.5e7, "ms_per_step": 0.066, "nodes": 15000, "domains": 1000, "jobs": 990, "placed": 990,
          "pods_per_job": 15, "classes": 1, "shape": b.SHAPES[3], "loop_p50_us": 60.0, "loop_p99_us": 70.0}
    d = {"world": 1, "steps": 20, "warmup": 5, "cfg2": c2, "binding": {"bound": False}}
    line = json.loads(b.emit(b.build_line(d)))
    assert line["metric"] == b.METRIC and line["value"] == 1.5e7 and line["unit"] == "placements/s"
    assert line["higher_is_better"] is True and line["dtype"] == "u32" and line["ms_per_step"] == 0.066
    assert line["steps"] == 20 and line["warmup"] == 5
    for k in ("roofline", "cpu_baseline", "p99_recovery_us", "cold_recovery", "patched_step_us", "cfg1", "cfg3",
              "cfg4", "cfg5"):
        assert k not in line, k
    assert line["detail"] is None


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_the_oracle_assignment(tmp_path):
    """A plain run on the GPU: one JSON line with the headline fields, `steps`
    as asked, no --full leg and no detail file; its dumped assign[] is the
    oracle's placement of config 2 (the same in every run)."""
    import json

    import numpy as np

    from jobset_amd import synth
    from oracle import oracle as O
    want = O.place_c(synth.config2())[0].astype(np.float64)
    out = tmp_path / "out"
    r = _run(["--gpus", "1", "--steps", "3", "--warmup", "1", "--dump-outputs", str(out),
              "--detail-out", str(tmp_path / "detail.json")])
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [x for x in r.stdout.splitlines() if x.strip()]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["steps"] == 3 and line["warmup"] == 1 and line["n_gpus"] == 1
    assert line["value"] > 0 and line["ms_per_step"] > 0 and line["unit"] == "placements/s"
    placed = int((want >= 0).sum())
    assert abs(line["value"] - placed / (line["ms_per_step"] * 1e-3)) <= 1e-3 * line["value"]
    for k in ("roofline", "cpu_baseline", "p99_recovery_us", "cfg4"):
        assert k not in line, k
    assert not (tmp_path / "detail.json").exists()
    got = np.load(out / "assign.npy")
    assert got.dtype == np.float64 and np.array_equal(got, want)


def test_evidence_lookup_follows_latest():
    """The roofline's traffic and trace figures come from the evidence
    directory profiles/LATEST names (a path under profiles/), and the line
    says so (`latest`: true) -- for the compaction and the cfg4 tally kernel."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    latest = b.latest_dir()
    assert latest is not None and os.path.isdir(latest)
    assert b.evidence_dirs()[0] == latest
    for kernel, cfg in (("place_compact_kernel", 2), ("tally_wave1_kernel", 4)):
        t = b.pmc_traffic(kernel, cfg)
        assert t is not None and t["latest"], (kernel, t)
