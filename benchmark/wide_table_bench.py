#!/usr/bin/env python3
"""Wide-table join harness: what output assembly (the table gather) costs when
tables carry many payload columns of mixed widths.

Legs (each prints ONE JSON line; --legs picks them):

  wide      orders-like  (INT64 key, FLOAT64, INT8)                     5 M rows
            JOIN lineitem-like (INT64 key, 2 x FLOAT64, FLOAT32,
            TIMESTAMP_DAYS, 2 x INT8, INT16, INT64)                     20 M rows
            on one GPU: step time and the gather phase.
  existing  the same join restricted to the column types that existed before
            the 1-/2-byte and float types: (INT64 key, INT64) JOIN
            (INT64 key, 3 x INT64, INT32). Needs nothing newer than
            dj_cpp_distributed_inner_join_cols, so the same script measures
            an older checkout (--root PATH) for a no-regression baseline.
  gather    the table gather alone through its hook (dj_gather_columns):
            fused vs per-column (and the engine's per-width routing, "auto"),
            per width class and for the lineitem payload set, over the same
            index array; min and median of --reps timed
            repetitions after --warmup, bytes moved per row for both modes
            (so the GB/s can be recomputed) and the run-to-run spread.

Orders keys are unique; each lineitem row draws a random order, so the output
has as many rows as lineitem and its row indices are random lines of the
source tables.
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                help="checkout whose distributed_join_amd package is measured")
ap.add_argument("--orders-rows", type=int, default=5_000_000)
ap.add_argument("--lineitem-rows", type=int, default=20_000_000)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--legs", default="wide,existing,gather")
args = ap.parse_args()
if args.reps < 10:
    ap.error("--reps must be at least 10")

sys.path.insert(0, args.root)
import distributed_join_amd as dj  # noqa: E402

dj.require_gpu()
L = dj.lib()
L.dj_set_device(0)
comm = dj.CppCommunicator(0, 1)

N_O, N_L = args.orders_rows, args.lineitem_rows
rng = np.random.RandomState(1234)
o_key = rng.permutation(N_O).astype(np.int64) * 4 + 1
l_key = o_key[rng.randint(0, N_O, N_L)]

INT8, INT32, INT64, TS_DAYS = 1, 2, 3, 5
INT16, FLOAT32, FLOAT64 = 15, 20, 21
WIDTH = {INT8: 1, INT16: 2, INT32: 4, TS_DAYS: 4, FLOAT32: 4, INT64: 8, FLOAT64: 8}
DTYPE = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}


def upload(a):
    a = np.ascontiguousarray(a)
    p = L.dj_dmalloc(max(a.nbytes, 1))
    L.dj_memcpy_h2d(p, a.ctypes.data, a.nbytes)
    return p


def payload(n, type_id, salt):
    w = WIDTH[type_id]
    return (np.arange(n, dtype=np.uint64) * np.uint64(2654435761) + np.uint64(salt)).astype(DTYPE[w])


def make_table(keys, types):
    cols = [(INT64, upload(keys))]
    for i, t in enumerate(types):
        cols.append((t, upload(payload(len(keys), t, i + 1))))
    return cols


pack = dj._pack_cols


def free_table(cols):
    for _, p in cols:
        L.dj_dfree(p)


def stats(ms):
    ms = np.sort(np.asarray(ms, dtype=np.float64))
    return {"min_ms": float(ms[0]), "median_ms": float(np.median(ms)), "max_ms": float(ms[-1]),
            "spread_pct": float((ms[-1] - ms[0]) / np.median(ms) * 100.0)}


def join_leg(name, o_types, l_types):
    left, right = make_table(o_key, o_types), make_table(l_key, l_types)
    la, ra = pack(left), pack(right)
    has_phase = hasattr(dj, "PHASE_GATHER")
    times, gather_ms, rows = [], [], 0
    for it in range(args.warmup + args.reps):
        if has_phase:
            L.dj_timing_reset()
            L.dj_timing_enable(1)
        L.dj_sync()
        t0 = time.perf_counter()
        t = L.dj_cpp_distributed_inner_join_cols(comm.ptr, ctypes.cast(la, ctypes.c_void_p),
                                                 len(left), N_O,
                                                 ctypes.cast(ra, ctypes.c_void_p), len(right),
                                                 N_L, 0, 0, 1, 0)
        L.dj_sync()
        dt = (time.perf_counter() - t0) * 1e3
        rows = L.dj_table_num_rows(t)
        L.dj_table_free(t)
        if it >= args.warmup:
            times.append(dt)
            if has_phase:
                gather_ms.append(L.dj_timing_total_ms(dj.PHASE_GATHER))
    if has_phase:
        L.dj_timing_enable(0)
        L.dj_timing_reset()
    free_table(left)
    free_table(right)
    # gathered output bytes per output row: every non-key column of both sides
    out_bytes = sum(WIDTH[t] for t in o_types) + sum(WIDTH[t] for t in l_types)
    print(json.dumps({
        "metric": f"wide-table join step ({name})", "unit": "ms", "higher_is_better": False,
        "value": stats(times)["median_ms"], "step": stats(times),
        "gather_phase": stats(gather_ms) if gather_ms else None,
        "orders_rows": N_O, "lineitem_rows": N_L, "output_rows": int(rows),
        "orders_schema": ["INT64 key"] + [str(t) for t in o_types],
        "lineitem_schema": ["INT64 key"] + [str(t) for t in l_types],
        "gathered_payload_bytes_per_output_row": out_bytes,
        "reps": args.reps, "warmup": args.warmup,
    }), flush=True)


def gather_case(label, widths, d_idx, n_src):
    srcs = [upload(payload(n_src, {1: INT8, 2: INT16, 4: INT32, 8: INT64}[w], i))
            for i, w in enumerate(widths)]
    dsts = [L.dj_dmalloc(N_L * w) for w in widths]
    descs = [(s, d, w) for s, d, w in zip(srcs, dsts, widths)]
    rec = {"case": label, "widths": widths, "rows": N_L, "source_rows": n_src}
    payload_bytes = 2 * sum(widths)          # each element read once, written once
    for mode, mname in ((dj.GATHER_FUSED, "fused"), (dj.GATHER_PER_COLUMN, "per_column"),
                        (dj.GATHER_AUTO, "auto")):
        dj.gather_columns(descs, d_idx, N_L, mode, reps=args.warmup)
        ms = dj.gather_columns(descs, d_idx, N_L, mode, reps=args.reps)
        # index traffic: 8 B per row once (fused) or once per column (per-column)
        st = stats(ms)
        if mode != dj.GATHER_AUTO:  # auto mixes both; its routing is in DESIGN.md
            bpr = payload_bytes + (8 if mode == dj.GATHER_FUSED else 8 * len(widths))
            st["bytes_per_row"] = bpr
            st["gbps_at_median"] = bpr * N_L / (st["median_ms"] * 1e-3) / 1e9
        rec[mname] = st
    rec["fused_over_per_column_median"] = rec["fused"]["median_ms"] / rec["per_column"]["median_ms"]
    for p in srcs + dsts:
        L.dj_dfree(p)
    return rec


def gather_leg():
    idx = rng.randint(0, N_L, N_L).astype(np.int64)
    d_idx = upload(idx)
    cases = [("1-byte x1", [1]), ("2-byte x1", [2]), ("4-byte x1", [4]), ("8-byte x1", [8]),
             ("1-byte x4", [1] * 4), ("2-byte x4", [2] * 4), ("4-byte x4", [4] * 4),
             ("8-byte x4", [8] * 4),
             ("lineitem payload (2xF64, F32, DAYS, 2xI8, I16, I64)", [8, 8, 4, 4, 1, 1, 2, 8]),
             ("existing-types payload (3xI64, I32)", [8, 8, 8, 4])]
    recs = [gather_case(label, widths, d_idx, N_L) for label, widths in cases]
    L.dj_dfree(d_idx)
    spread = max(max(r[m]["spread_pct"] for m in ("fused", "per_column", "auto")) for r in recs)
    print(json.dumps({"metric": "table gather, fused vs per-column", "unit": "ms",
                      "reps": args.reps, "warmup": args.warmup,
                      "run_to_run_spread_pct_max": spread, "cases": recs}), flush=True)


legs = args.legs.split(",")
if "wide" in legs:
    join_leg("lineitem x orders, all widths", [FLOAT64, INT8],
             [FLOAT64, FLOAT64, FLOAT32, TS_DAYS, INT8, INT8, INT16, INT64])
if "existing" in legs:
    join_leg("existing types only", [INT64], [INT64, INT64, INT64, INT32])
if "gather" in legs:
    gather_leg()
comm.destroy()
