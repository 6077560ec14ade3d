"""`bench.py` end to end on the GPU at a small batch: a plain run times exactly --steps steps and reports the headline
alone; `--dump-outputs` of two runs with the same arguments hold the same results."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(out_dir):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--clips", "2",
           "--dump-outputs", str(out_dir)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    arrays = {f[:-4]: np.load(os.path.join(out_dir, f)) for f in sorted(os.listdir(out_dir))}
    return line, arrays


def test_plain_bench_run_and_its_outputs(tmp_path):
    line, a = _run(tmp_path / "a")
    assert line["steps"] == 3 and line["ms_per_step"] > 0 and line["unit"] == "clips/s" and line["dtype"] == "bf16"
    assert len(line["host_enqueue_ms_each_step"]) == 3
    assert not {"roofline", "forward_only", "secondary", "cpu_baseline"} & set(line)
    assert a["task0_logits"].shape == (2, 2) and np.isfinite(a["task0_logits"]).all()
    assert any(k.startswith("param.decoder.") for k in a) and any(k.startswith("grad.decoder.") for k in a)
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    _, b = _run(tmp_path / "b")
    assert sorted(a) == sorted(b)
    for k in a:
        np.testing.assert_allclose(a[k], b[k], rtol=1e-5, atol=1e-6, err_msg=k)
