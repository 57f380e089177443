"""Pin the bench.py JSON contract (the driver parses exactly this shape) on
the committed record and on the source, so a refactor cannot silently drop a
field the round-end harness or the judge reads."""
import inspect
import json
import os

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

REQUIRED_TOP = [
    "metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step",
    "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config",
    "roofline", "cpu_baseline",
]
REQUIRED_CONFIG = ["workload", "rows_per_gpu", "selectivity", "nvlink_domain_size",
                   "phases_ms", "alt_mode"]
REQUIRED_ROOFLINE = ["bound", "achieved", "peak", "unit", "frac", "traffic"]


def test_committed_record_shape():
    with open(os.path.join(REPO, "profiles", "r02_bench_n1.json")) as fh:
        rec = json.loads(fh.read().strip().splitlines()[-1])
    for k in REQUIRED_TOP:
        assert k in rec, k
    for k in REQUIRED_CONFIG:
        assert k in rec["config"], k
    for k in REQUIRED_ROOFLINE:
        assert k in rec["roofline"], k
    assert rec["metric"] == "joined rows/sec whole-node"
    assert rec["unit"] == "input rows/s"
    assert rec["scaling"] == "weak"
    assert rec["higher_is_better"] is True
    assert rec["n_gpus"] == 1 and rec["vs_baseline"] is None  # N=8 only
    assert rec["data"] == "synthetic" and rec["dtype"] == "int64"
    # whole-job value consistency: value = 2 * rows * N / step time
    expect = 2.0 * rec["config"]["rows_per_gpu"] * rec["n_gpus"] / (rec["ms_per_step"] / 1e3)
    assert abs(expect - rec["value"]) / rec["value"] < 1e-6
    # cpu_baseline contract (kind/cores/sample)
    cb = rec["cpu_baseline"]
    assert cb["kind"] in ("port", "reference") and cb["cores"] >= 1 and cb["sample"]


def test_bench_source_emits_required_fields():
    src = open(os.path.join(REPO, "bench.py")).read()
    for k in REQUIRED_TOP + REQUIRED_ROOFLINE + ["alt_mode", "workload"]:
        assert f'"{k}"' in src, k
    # the timed region must be barrier+sync bracketed and MAX-reduced
    assert "barrier_sync()" in src and "ReduceOp.MAX" in src


def test_extra_legs_are_gated_behind_full():
    """A plain run times only the headline steps: the CPU baseline leg and the
    N>1 alt-mode leg take runs of their own and must sit behind --full."""
    import bench
    src = inspect.getsource(bench.main)
    assert '"--full"' in src and '"--dump-outputs"' in src
    assert "if args.full and rank == 0 and N == 1 and not args.no_cpu_baseline:" in src
    assert "if args.full and N > 1 and args.nvlink_domain_size == 0:" in src


def test_dump_sample_is_bounded_and_order_independent(tmp_path):
    """--dump-outputs must write the same files for the same result whatever
    order the join emitted its rows in, and stay within its byte budget."""
    import numpy as np

    import bench
    rng = np.random.default_rng(7)
    n = 50_000
    cols = [rng.integers(0, 1 << 40, n, dtype=np.int64) for _ in range(4)]
    perm = rng.permutation(n)
    shuffled = [c[perm] for c in cols]

    # small result: every row kept, lexicographically sorted
    full = bench.sample_output(cols)
    assert len(full[0]) == n
    want = np.lexsort(tuple(reversed(cols)))
    for got, c in zip(full, cols):
        assert (got == c[want]).all()
    for a, b in zip(full, bench.sample_output(shuffled)):
        assert (a == b).all()

    # over budget: a strict subset of the rows, same for any row order
    budget = 400_000
    small = bench.sample_output(cols, max_bytes=budget)
    assert 0 < len(small[0]) and sum(c.nbytes for c in small) <= budget
    for a, b in zip(small, bench.sample_output(shuffled, max_bytes=budget)):
        assert (a == b).all()
    rows = set(zip(*[c.tolist() for c in cols]))
    assert set(zip(*[c.tolist() for c in small])) <= rows

    bench.dump_outputs(str(tmp_path), cols)
    for name in bench.DUMP_COLUMNS:
        a = np.load(tmp_path / f"{name}.npy")
        assert a.dtype == np.float64 and len(a) == n
    assert np.load(tmp_path / "output_rows.npy").tolist() == [float(n)]
