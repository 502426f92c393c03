"""bench.py --dump-outputs: what the timed path computed in its last step, written as .npy files so that two builds can be compared
output for output.  The file writer on the CPU; end to end on the device (-m gpu): the same arguments give the same outputs, whatever
number of untimed clock-warm replays the box's speed asked for."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

NAMES = ["qp_iterations", "status", "u0", "u_iterate", "x_iterate"]


def _arrays(B, N=20, seed=3):
    rng = np.random.default_rng(seed)
    return {"u0": rng.standard_normal((B, 4)), "x_iterate": rng.standard_normal((B, N + 1, 10)), "u_iterate": rng.standard_normal((B, N, 4)),
            "status": np.zeros(B, dtype=np.int32), "qp_iterations": rng.integers(0, 5, B).astype(np.int32)}


def test_dump_writes_every_array_whole_in_float64(tmp_path):
    a = _arrays(64)
    assert bench.dump_outputs(str(tmp_path), a) == NAMES
    assert sorted(os.listdir(tmp_path)) == [n + ".npy" for n in NAMES]
    for n in NAMES:
        got = np.load(tmp_path / f"{n}.npy")
        assert got.dtype == np.float64 and np.array_equal(got, a[n])
    bench.dump_outputs(str(tmp_path / "r1"), a, "_rank1")
    assert sorted(os.listdir(tmp_path / "r1")) == [n + "_rank1.npy" for n in NAMES]


def test_dump_beyond_the_limit_is_a_fixed_sample_of_instances(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 400_000)
    a = _arrays(1000)
    for d in ("a", "b"):
        assert bench.dump_outputs(str(tmp_path / d), a) == sorted(NAMES + ["instance_index"])
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert total <= bench.DUMP_LIMIT_BYTES
    idx = np.load(tmp_path / "a" / "instance_index.npy")
    assert np.array_equal(idx, np.load(tmp_path / "b" / "instance_index.npy"))          # the same sample on every run
    idx = idx.astype(np.int64)
    assert 100 < len(idx) < 1000 and np.all(np.diff(idx) > 0)
    for n in NAMES:
        assert np.array_equal(np.load(tmp_path / "a" / f"{n}.npy"), a[n][idx])


def test_steps_below_one_is_refused():
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--steps must be at least 1" in r.stderr


@pytest.mark.gpu
def test_dump_is_the_same_whatever_the_clock_warm_up(tmp_path):
    """Two runs with the same arguments, one without the untimed clock-warm replays: the last timed step's outputs are identical bit
    for bit (the replays' effect on the engine's warm start is undone before the timed steps), and the line counts --steps steps."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    steps = 7
    got = []
    for d, warm in (("a", "30"), ("b", "0")):
        out = tmp_path / d
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "3",
                            "--only-timed", "--downwash-form", "fused", "--clock-warm-ms", warm, "--dump-outputs", str(out)],
                           env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        line = json.loads(r.stdout.strip().splitlines()[-1])
        assert line["steps"] == steps and line["value"] > 0
        assert sorted(os.listdir(out)) == [n + ".npy" for n in NAMES]
        got.append({n: np.load(out / f"{n}.npy") for n in NAMES})
    a, b = got
    assert a["u0"].shape == (1024, 4) and a["x_iterate"].shape == (1024, 21, 10) and a["u_iterate"].shape == (1024, 20, 4)
    assert all(v.dtype == np.float64 for v in a.values())
    assert np.all(np.isfinite(a["u0"])) and not a["status"].any()
    for n in NAMES:
        assert np.array_equal(a[n], b[n]), n


@pytest.mark.gpu
def test_a_plain_run_is_the_headline_alone():
    """Without --full the line is the headline form's: its figures and nothing that takes a run of its own (other forms, the
    oracle's parity check, repeated passes, the configs block and the other legs, the CPU baseline)."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5"],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["steps"] == 20 and line["warmup"] == 5 and line["value"] > 0 and line["ms_per_step"] > 0
    assert line["unit"] == "solves/s" and line["higher_is_better"] is True and line["dtype"] == "f64"
    assert line["config"]["neighbour_exchange"] == "fused" and line["instances_not_converged"] == 0
    assert line["parity_max_rel_vs_oracle"] is None and line["roofline"]["kernel_us"] > 0
    assert set(line["forms"]) == {"fused"}
    for block in ("configs", "ipm_always", "mixed", "constrained", "host", "tick", "rows", "cpu_baseline", "config1", "repeat",
                  "scaling_baseline"):
        assert block not in line, block
