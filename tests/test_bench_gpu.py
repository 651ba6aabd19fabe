"""bench.py on the GPU, in process: a plain run reports the headline figure
only, --dump-outputs writes the last timed step's arrays and they repeat from
run to run, --full adds the roofline and the per-step split."""
import json
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import bench  # noqa: E402

pytestmark = pytest.mark.gpu

ARGS = ["--gpus", "1", "--steps", "3", "--warmup", "2", "--warm-ms", "5"]
E, P, LEVELS, R = 2048, 3, 4, 3  # cfg2


def run_bench(monkeypatch, capsys, *extra):
    monkeypatch.setattr(sys, "argv", ["bench.py", *ARGS, *extra])
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    bench.main()
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_plain_run_dumps_repeatable_outputs(gpu, monkeypatch, capsys, tmp_path):
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    out = run_bench(monkeypatch, capsys, "--dump-outputs", a)
    assert out["steps"] == 3 and out["ms_per_step"] > 0
    assert out["value"] == pytest.approx(1e3 / out["ms_per_step"])
    assert out["unit"] == "update-iterations/s" and out["higher_is_better"] is True
    assert out["dtype"] == "f32" and out["metric"] == bench.METRIC
    # nothing but the headline figure is measured
    assert out["roofline"] is None and out["step_split"] is None and out["cpu_baseline"] is None
    A = load(a)
    assert sorted(A) == ["coords", "corr", "patches", "poses"]
    assert A["coords"].shape == (1, E, 2, P, P)
    assert A["corr"].shape == (1, E, (2 * R + 1) ** 2 * P * P * LEVELS)
    assert all(v.dtype == np.float32 and np.isfinite(v).all() for v in A.values())
    assert sum(v.nbytes for v in A.values()) <= 64 * 2**20
    assert np.abs(A["corr"]).max() > 0
    # a different number of untimed steps before the same timed ones: same inputs, same outputs
    run_bench(monkeypatch, capsys, "--dump-outputs", b, "--warm-ms", "20")
    B = load(b)
    for k in A:
        assert np.array_equal(A[k], B[k]), k


def test_full_run_adds_roofline_and_step_split(gpu, monkeypatch, capsys):
    out = run_bench(monkeypatch, capsys, "--full", "--no-cpu-baseline")
    assert out["steps"] == 3 and out["ms_per_step"] > 0
    assert out["roofline"]["kernel_ms"] > 0 and out["roofline"]["achieved"] > 0
    assert len(out["roofline"]["per_level"]) == LEVELS
    assert out["step_split"]["gpu_ms_median"] > 0
    assert out["cpu_baseline"] is None
