"""bench.py's plain N = 1 run on the GPU, in this process and at a small
nreduce: it launches the combine kernel warmup + steps times and nothing
else, reports ms_per_step consistent with its value, and with --dump-outputs
writes the same target in two runs with the same arguments."""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

N = (2 << 20) + 5      # several blocks and a ragged tail; 16 MiB: dumped whole
STEPS, WARMUP = 3, 2


def _plain_run(monkeypatch, capsys, out_dir, detail):
    sys.path.insert(0, ROOT)
    import bench
    import osgpu
    L = osgpu.load()
    real, calls = L.osgpu_combine, []

    def counted(*a):
        calls.append(a[5])
        return real(*a)
    monkeypatch.setattr(L, "osgpu_combine", counted, raising=False)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", str(STEPS),
                                      "--warmup", str(WARMUP), "--nreduce", str(N),
                                      "--dump-outputs", str(out_dir), "--detail", str(detail)])
    bench.bench_single(bench.parse())
    monkeypatch.undo()
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0]), calls


def test_plain_run_times_the_steps_and_dumps_the_same_target_twice(monkeypatch, capsys, tmp_path):
    import bench
    runs = [_plain_run(monkeypatch, capsys, tmp_path / d, tmp_path / (d + ".json"))
            for d in ("one", "two")]
    for d, calls in runs:
        # the timed path and nothing beside it
        assert calls == [N] * (WARMUP + STEPS)
        assert d["metric"] == bench.METRIC and d["unit"] == "GiB/s" and d["dtype"] == "f64"
        assert d["higher_is_better"] is True and d["n_gpus"] == 1
        assert d["steps"] == STEPS and d["warmup"] == WARMUP
        assert d["ms_per_step"] > 0
        # value is bytes per step over the time of one step (5 digits in the line)
        want = 3 * N * 8 / (d["ms_per_step"] * 1e-3) / bench.GIB
        assert abs(d["value"] - want) <= 1e-3 * want
        for side in ("team_by_members", "cpu_baseline", "api", "traffic_live", "collectives"):
            assert side not in d
        assert d["outputs"]["target"] == {"elements": N, "of": N, "dtype": "float64",
                                          "sampled": False}
    one, two = (np.load(tmp_path / d / "target.npy") for d in ("one", "two"))
    assert one.dtype == np.float64 and one.shape == (N,)
    assert np.array_equal(one.view(np.uint64), two.view(np.uint64))
    # sums of two uniform [1, 2) doubles, not one value repeated
    assert one.min() >= 2.0 and one.max() < 4.0 and np.unique(one[:4096]).size > 4000
