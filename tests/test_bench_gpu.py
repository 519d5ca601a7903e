"""GPU: `bench.py` on one rank and a small map.  A plain run prints the headline line and nothing that needs a run of its own;
`--full` adds the extras behind the same timed steps, so both runs dump the same candidate deltas, bit for bit."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--n-bins", "2000", "--nnz", "100000", "--mcmc-warmup", "300", "--steps", "6", "--warmup", "2"]
FULL_ONLY = ("roofline", "phase_ms", "relevant_pairs_last_step", "full_mcmc_step_ms", "full_eval_ms", "other_arithmetic",
             "value_1000", "regimes", "late_stage", "cpu_baseline", "cpu_baseline_dense")


def _run(extra, dump):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"] + SMALL + extra + ["--dump-outputs", dump],
                         env=env, capture_output=True, text=True, timeout=400)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    return json.loads(lines[0]), np.load(os.path.join(dump, "candidate_deltas.npy"))


@pytest.mark.timeout(900)
def test_plain_run_is_the_headline_and_full_adds_the_extras(tmp_path):
    plain, d_plain = _run([], str(tmp_path / "plain"))
    full, d_full = _run(["--full"], str(tmp_path / "full"))
    for d in (plain, full):
        assert d["metric"] == "candidate logL evals/sec" and d["unit"] == "candidate logL evals/s" and d["higher_is_better"] is True
        assert d["value"] > 0 and d["ms_per_step"] > 0 and d["steps"] == 6 and d["warmup"] == 2 and d["n_gpus"] == 1
    assert plain["dtype"] == full["dtype"] and plain["config"] == full["config"]
    assert not [k for k in FULL_ONLY if k in plain]
    assert not [k for k in FULL_ONLY if k not in full]
    assert "error" not in full["late_stage"] and "error" not in full["cpu_baseline_dense"]
    assert full["roofline"]["launches_timed"] >= 1 and full["cpu_baseline"]["candidates_compared_with_gpu"] > 0
    assert d_plain.ndim == 2 and d_plain.shape[1] == 13 and d_plain.dtype == np.float64
    assert np.array_equal(d_plain, d_full)    # the same timed steps on the same layout: the extras come after them
