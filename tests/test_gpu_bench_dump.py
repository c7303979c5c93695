"""The single-GPU bench command line, end to end: a plain run prints the headline line alone, `--steps` sets the timed steps, and
`--dump-outputs DIR` writes the factors after the last timed step -- the same numbers in two runs with the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(out_dir):
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", "6", "--warmup", "2", "--rows", "2048", "--dump-outputs", str(out_dir)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_bench_dumps_the_factors_of_its_last_step(tmp_path):
    d1 = _bench(tmp_path / "a")
    d2 = _bench(tmp_path / "b")
    for d in (d1, d2):
        for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
            assert k in d, k
        assert d["steps"] == 6 and d["value"] > 0 and abs(d["value"] * d["ms_per_step"] - 1e3) < 1e-6 * d["value"] * d["ms_per_step"] + 1e-6
        for k in ("cpu_baseline", "other_configs", "measured_on_this_box", "nmf_call", "fp64_inputs", "end_to_end", "value_f32_mode"):
            assert k not in d, k                                              # side legs are --full's
    M, N, K = 2048, 16384, 64
    for name, shape in (("A", (M, K)), ("S", (K, N))):
        x1, x2 = np.load(tmp_path / "a" / (name + ".npy")), np.load(tmp_path / "b" / (name + ".npy"))
        assert x1.dtype == np.float32 and x1.shape == shape and np.isfinite(x1).all()
        np.testing.assert_allclose(x1, x2, rtol=1e-5, atol=1e-7)
