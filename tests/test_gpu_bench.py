"""GPU run of bench.py itself at a small size: the result line's contract,
--steps, --full gating and --dump-outputs (the dumped columns are the join
result, checked against the oracle on the same inputs)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = 200_000


def _bench(*extra):
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1",
                        "--rows", str(ROWS), *extra],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1, r.stdout  # exactly one result line on stdout
    return json.loads(lines[0])


def test_plain_run_record_and_dump(tmp_path):
    out = tmp_path / "dump"
    rec = _bench("--steps", "3", "--warmup", "1", "--dump-outputs", str(out))
    assert rec["steps"] == 3 and rec["warmup"] == 1
    assert rec["metric"] == "joined rows/sec whole-node" and rec["unit"] == "input rows/s"
    assert rec["higher_is_better"] is True and rec["dtype"] == "int64"
    assert rec["ms_per_step"] > 0
    assert abs(2.0 * ROWS / (rec["ms_per_step"] / 1e3) - rec["value"]) / rec["value"] < 1e-6
    # a plain run skips the legs that take runs of their own
    assert rec["cpu_baseline"] is None and rec["config"]["alt_mode"] is None

    bk, bp = oracle.gen_build(ROWS, 2 * ROWS)
    pk, pp = oracle.gen_probe(ROWS, ROWS, 2 * ROWS, selectivity=0.3)
    want = oracle.sort_rows(*oracle.inner_join(bk, bp, pk, pp))
    names = ("left_key", "left_payload", "right_key", "right_payload")
    for name, w in zip(names, want):
        got = np.load(out / f"{name}.npy")
        assert got.dtype == np.float64 and len(got) == len(w)
        assert (got == w.astype(np.float64)).all(), name
    assert np.load(out / "output_rows.npy").tolist() == [float(len(want[0]))]
    assert rec["config"]["output_rows_per_gpu"] == len(want[0])


def test_full_run_adds_cpu_baseline():
    rec = _bench("--steps", "2", "--warmup", "1", "--full", "--cpu-baseline-rows", str(ROWS))
    cb = rec["cpu_baseline"]
    assert cb["kind"] == "port" and cb["cores"] >= 1 and cb["value"] > 0
