"""GPU: one small case per flow a candidate evaluation can take (tests/step_plan_cases.py; the decisions are graal_amd/csrc/step_plan.h):
contigs of at most 16 fragments, of about 40, of 65 to 256, of 257 and more, the late stage, the 2,048-block k_fin of a contig above 1,024
in exact arithmetic, a sorted list in short rows that takes the indexed producer and the same list forced to stream, repeated bins.

* the reference-arithmetic cases equal k_strict_dense -- the O(m^2) validation kernel, run in ONE child process for all of them
  (GRAAL_STRICT_DENSE=1 is read once per process) -- bit for bit;
* the exact-arithmetic case and the repeated bins agree with the dense oracle within the suite's tolerances for their coordinates
  (1e-8 x |logL| on a grid: tests/test_engine_gpu.py; 2e-9 x |logL| with repeats: tests/test_strict_windowed_gpu.py);
* graal_run_counters moves as the host alone decides: `indexed_passes` by what the producer's plan says for the case's shape, and whenever
  exactly one of the two hand-off counters behind k_gprep moved, it is the one plan_strict's `gwait` names."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import step_plan_cases as SC
from tests.test_step_plan_cpu import producer as plan_producer, strict as plan_strict

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dense_kernel(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("step_plan") / "dense.npz")
    subprocess.check_call([sys.executable, "-m", "tests.step_plan_cases", out, "strict"], cwd=ROOT, env=dict(os.environ, GRAAL_STRICT_DENSE="1"),
                          timeout=600)
    return np.load(out)


def check_counters(name, r):
    moved, f = r["moved"], r["facts"]
    n_evals = len(SC.CASES[name]["props"])
    assert moved["evaluations"] == n_evals and moved["fallbacks"] == 0, moved
    p = plan_producer(**f)
    print(name, "| plan: indexed", p["indexed"], "grid", p["grid"], "| moved:", {k: v for k, v in moved.items() if v})
    assert p["impossible"] == 0
    assert moved["indexed_passes"] == n_evals * p["indexed"], (moved, p)
    word, event = moved["strict2_behind_the_word"], moved["strict2_behind_the_event"]
    if (word > 0) != (event > 0):
        gwait = plan_strict(spin_ok=r["counters"]["in_kernel_waits_in_use"], **f)["gwait"]
        assert (word > 0) == bool(gwait), (moved, gwait)
    return p


@pytest.mark.parametrize("name", SC.STRICT)
def test_reference_arithmetic_flows_equal_the_dense_validation_kernel(name, dense_kernel):
    assert os.environ.get("GRAAL_STRICT_DENSE") in (None, "0")
    r = SC.run_case(name)
    i = list(SC.CASES).index(name)
    got, want = r["deltas"], dense_kernel["d%d" % i]
    assert got.shape == want.shape and np.abs(np.nan_to_num(want)).max() > 0
    bad = np.argwhere(got.view(np.int64) != want.view(np.int64))        # (64-bit words: a flagged candidate's NaN must be the same too)
    assert len(bad) == 0, (name, len(bad), bad[:5], got[tuple(bad[0])], want[tuple(bad[0])])
    p = check_counters(name, r)
    if name == "short rows: the indexed producer":
        assert p["indexed"] == 1, "the case no longer takes the indexed producer"
    if name == "short rows, forced to stream":
        assert p["indexed"] == 0 and plan_producer(**dict(r["facts"], forced_producer=0))["indexed"] == 1
    if name == "repeated bins":
        from tests.test_repeats_gpu import oracle_deltas_with_repeats
        from tests.test_strict_windowed_gpu import ref_dense
        P, s, max_id = SC.layout_of(name)
        dense = ref_dense(P)
        for (fA, fBs), got in zip(SC.CASES[name]["props"], r["deltas"]):
            base, want = oracle_deltas_with_repeats(P, dense, s, fA, fBs, max_id)
            assert np.all(np.abs(got - want) <= 2e-9 * abs(base)), (fA, fBs, np.abs(got - want).max() / abs(base))


def test_exact_arithmetic_with_a_contig_above_1024_matches_the_dense_oracle():
    from tests.test_engine_gpu import dense_for, oracle_deltas
    name = "exact arithmetic, a contig of 1,100"
    r = SC.run_case(name)
    assert r["facts"]["max_lcont"] == 1100
    check_counters(name, r)
    P, s, max_id = SC.layout_of(name)
    dense = dense_for(P)
    for (fA, fBs), got in zip(SC.CASES[name]["props"], r["deltas"]):
        base, want = oracle_deltas(P, dense, s, fA, fBs, max_id)
        err = np.abs(got - want).max()
        assert err <= 1e-8 * abs(base), (fA, fBs, err / abs(base))
