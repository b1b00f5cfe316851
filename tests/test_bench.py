"""bench.py's own options: the plain run (no --full) and --dump-outputs."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench_module():
    spec = importlib.util.spec_from_file_location("sn_bench", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("argv", [["--steps", "0"], ["--warmup", "-1"]])
def test_bench_rejects_step_counts_it_cannot_time(monkeypatch, argv):
    bench = _bench_module()
    monkeypatch.setattr(sys, "argv", ["bench.py"] + argv)
    with pytest.raises(SystemExit) as e:
        bench.main()
    assert e.value.code == 2


def _plain_run(out_dir, workload):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--workload", workload, "--batch", "8",
           "--steps", "3", "--warmup", "1", "--dump-outputs", str(out_dir)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
def test_plain_bench_run_dumps_the_same_outputs_twice(tmp_path):
    """Two plain runs with the same arguments: the line has the headline fields, no verification or CPU leg, and
    --dump-outputs writes the same float32 planes (a history-carrying 16-bit clip: the unsigned samples of int16 tensors)."""
    lines, dumps = [], []
    for i in range(2):
        d = tmp_path / f"run{i}"
        lines.append(_plain_run(d, "480p-YUV420P16"))
        dumps.append({f: np.load(d / f) for f in sorted(os.listdir(d))})
    for line in lines:
        assert line["steps"] == 3 and line["ms_per_step"] > 0 and line["dtype"] == "u16"
        assert {"metric", "value", "unit", "higher_is_better"} <= set(line)
        assert line["verified"]["ok"] is None and "cpu_baseline" not in line and "single_frame" not in line
        assert line["dumped"]["frames"] == list(range(8))
    assert sorted(dumps[0]) == ["plane0.npy", "plane1.npy", "plane2.npy"]
    shapes = [(8, 480, 720), (8, 240, 360), (8, 240, 360)]
    for p, name in enumerate(sorted(dumps[0])):
        a, b = dumps[0][name], dumps[1][name]
        assert a.dtype == np.float32 and a.shape == shapes[p]
        assert a.min() >= 0 and a.max() <= 65535 and np.array_equal(a, np.round(a))
        assert a.max() > 255  # 16-bit samples, not bytes
        assert np.array_equal(a, b), f"{name} differs between two runs with the same arguments"
