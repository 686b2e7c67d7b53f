"""half / bfloat16 reduce-to-all on the fused one-launch paths: two PE
processes sharing cuda:0 (tests/support/half_worker.py), half sum and
bfloat16 max at 1 Ki and 4 Ki + 3 elements, on IPC device heaps in the team
form and the forced pull form and on the pinned host heap.  Every call must
report OSGPU_RAN_FUSED_TEAM / FUSED_PULL / FUSED_STAGED and equal the
restatement bit for bit.  The
workers bound the device barrier at 20 s; the parent kills them at its own
time limit.
"""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from support import half_ref as R

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
WORKER = os.path.join(HERE, "support", "half_worker.py")
WORLD = 2


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_fused_paths_two_processes(tmp_path):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    sys.path.insert(0, os.path.join(HERE, "support"))
    import half_worker as W
    port = _free_port()
    procs = []
    for r in range(WORLD):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(WORLD), LOCAL_RANK=str(r),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), PYTHONUNBUFFERED="1")
        log = open(tmp_path / f"rank{r}.log", "w")
        procs.append((subprocess.Popen([sys.executable, WORKER, str(tmp_path)], env=env,
                                       stdout=log, stderr=subprocess.STDOUT), log))
    try:
        for p, _ in procs:
            p.wait(timeout=120)
    except subprocess.TimeoutExpired:
        for q, _ in procs:
            q.kill()
        raise
    finally:
        for _, f in procs:
            f.close()
    for r, (p, _) in enumerate(procs):
        assert p.returncode == 0, open(tmp_path / f"rank{r}.log").read()[-3000:]
    res = [json.load(open(tmp_path / f"rank{r}.json")) for r in range(WORLD)]
    for form, path in (("team", "fused_team"), ("pull", "fused_pull"), ("staged", "fused_staged")):
        for t, op, n in W.CASES:
            key = f"{form}/{t}/{op}/{n}"
            want = R.to_all(t, op, [W.source(t, n, r) for r in range(WORLD)])
            for r in range(WORLD):
                assert res[r]["paths"][key] == path, (key, r, res[r]["paths"], res[r]["errors"])
                got = np.frombuffer(bytes.fromhex(res[r]["out"][key]), np.uint16)
                bad = np.flatnonzero(got != want[r])
                assert bad.size == 0, (key, r, bad.size, int(bad[0]))
