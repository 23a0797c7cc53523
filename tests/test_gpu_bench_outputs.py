"""bench.py's plain run and --dump-outputs on the GPU: a plain run times --steps steps and prints the
result line without the --full legs (gate, cpu_baseline); --dump-outputs writes the last timed
step's verdicts as float arrays, one per round, and a second run with the same arguments writes the
same bytes (the history is a pure function of the arguments). 4,099 rounds: 64 whole 64-round
segments and a 3-round tail. The verdict buffer starts zeroed, so the all-ones dump asserted here is
what the step wrote; the bit order and a history with rejected rounds are covered on the CPU
(tests/test_bench_outputs.py) and by the --full gate's negative control (tests/test_gpu_bench_dist.py),
which read the bitmap through the same unpack_verdicts."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 4099
NPY_HEADER = 128  # numpy .npy version 1.0 header of a small-shape array


def _run(out_dir):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, "-u", os.path.join(ROOT, "bench.py"), "--gpus", "1", "--n", str(N), "--steps", "2",
                        "--warmup", "1", "--dump-outputs", str(out_dir)],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    recs = [json.loads(x) for x in r.stdout.splitlines() if x.startswith('{"metric"')]
    assert len(recs) == 1
    return recs[0]


@pytest.fixture(scope="module")
def first_run(tmp_path_factory):
    d = tmp_path_factory.mktemp("dump") / "out"
    return _run(d), d


def test_plain_run_dumps_last_step_verdicts(first_run):
    out, d = first_run
    assert out["steps"] == 2 and out["warmup"] == 1 and out["n_gpus"] == 1
    assert out["unit"] == "beacons/s" and out["higher_is_better"] is True
    assert out["ms_per_step"] > 0
    # value and ms_per_step are two views of the same timed region (both rounded in the line)
    assert out["value"] == pytest.approx(N / (out["ms_per_step"] * 1e-3), rel=1e-2)
    assert out["stages_ms_per_launch"]["miller"] > 0  # from the timed steps' own events
    assert out["gate"].startswith("not run") and "cpu_baseline" not in out  # --full only
    assert sorted(os.listdir(d)) == ["first_bad.npy", "ok.npy"]
    assert os.path.getsize(d / "ok.npy") == NPY_HEADER + 4 * N
    assert os.path.getsize(d / "first_bad.npy") == NPY_HEADER + 8
    ok = np.load(d / "ok.npy")
    fb = np.load(d / "first_bad.npy")
    assert ok.dtype == np.float32 and ok.shape == (N,) and (ok == 1.0).all()
    assert fb.dtype == np.float64 and fb.tolist() == [-1.0]


def test_second_run_writes_the_same_bytes(first_run, tmp_path):
    _, d = first_run
    _run(tmp_path / "again")
    for name in ("ok.npy", "first_bad.npy"):
        assert (tmp_path / "again" / name).read_bytes() == (d / name).read_bytes(), name
