#!/usr/bin/env python3
"""What validity masks cost: the wide-table join of wide_table_bench.py
(orders-like 5 M rows JOIN lineitem-like 20 M rows, all widths) on one GPU

  none      through the nullable entry point without any mask (must match the
            mask-free entry point, which is measured too: "plain");
  payloads  a mask (~10 % null) on every payload column, key mask-free: the
            join route is unchanged, the difference is the mask gather;
  all       a mask on every column, the key included (no null among the keys):
            the join takes the fused-key route of nullable keys;

and the mask gather kernel alone through its hook (dj_gather_bitmasks) for 1
and for 10 nullable columns over one random index array, with 1, 2, 5 or all
columns per kernel launch.

Byte model of the mask gather, per nullable column and output row: 1/8 B
written, one random 4-byte read; plus 8 B of index per row per launch (the
mask gather runs in launches of its own, so the index array is read again
after the value gather, once per launch). Each leg prints ONE JSON line.
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--orders-rows", type=int, default=5_000_000)
ap.add_argument("--lineitem-rows", type=int, default=20_000_000)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--legs", default="plain,none,payloads,all,gather")
args = ap.parse_args()

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
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
O_TYPES = [FLOAT64, INT8]
L_TYPES = [FLOAT64, FLOAT64, FLOAT32, TS_DAYS, INT8, INT8, INT16, INT64]


def upload(a):
    a = np.ascontiguousarray(a)
    p = L.dj_dmalloc(max(a.nbytes, 1))
    L.dj_memcpy_h2d(p, a.ctypes.data, a.nbytes)
    return p


def payload(n, type_id, salt):
    w = WIDTH[type_id]
    return (np.arange(n, dtype=np.uint64) * np.uint64(2654435761) + np.uint64(salt)).astype(DTYPE[w])


def stats(ms):
    ms = np.sort(np.asarray(ms, dtype=np.float64))
    return {"min_ms": float(ms[0]), "median_ms": float(np.median(ms)), "max_ms": float(ms[-1]),
            "spread_pct": float((ms[-1] - ms[0]) / np.median(ms) * 100.0)}


def make_table(keys, types, key_mask, payload_masks):
    n = len(keys)
    held = [upload(keys)]
    cols = [(INT64, held[0]) + ((dj.upload_mask(np.ones(n, dtype=bool)),) if key_mask else ())]
    for i, t in enumerate(types):
        p = upload(payload(n, t, i + 1))
        held.append(p)
        m = (dj.upload_mask(rng.random_sample(n) >= 0.10),) if payload_masks else ()
        cols.append((t, p) + m)
    return cols, held


def join_leg(name, key_mask, payload_masks, plain=False):
    left, lheld = make_table(o_key, O_TYPES, key_mask, payload_masks)
    right, rheld = make_table(l_key, L_TYPES, key_mask, payload_masks)
    if plain:
        la, ra = (dj.ColDesc * len(left))(), (dj.ColDesc * len(right))()
        for arr, cols in ((la, left), (ra, right)):
            for i, (t, p) in enumerate(cols):
                arr[i].type_id, arr[i].data, arr[i].chars, arr[i].chars_bytes = t, p, None, 0
        entry = L.dj_cpp_distributed_inner_join_cols_multi
    else:
        la, ra = dj._pack_ncols(left), dj._pack_ncols(right)
        entry = L.dj_cpp_distributed_inner_join_ncols_multi
    on = np.zeros(1, dtype=np.int32)
    times, gather_ms, rows, nulls = [], [], 0, 0
    for it in range(args.warmup + args.reps):
        L.dj_timing_reset()
        L.dj_timing_enable(1)
        L.dj_sync()
        t0 = time.perf_counter()
        t = entry(comm.ptr, ctypes.cast(la, ctypes.c_void_p), len(left), N_O,
                  ctypes.cast(ra, ctypes.c_void_p), len(right), N_L, on.ctypes.data,
                  on.ctypes.data, 1, 1, 0)
        L.dj_sync()
        dt = (time.perf_counter() - t0) * 1e3
        rows = L.dj_table_num_rows(t)
        nulls = sum(L.dj_table_column_null_count(t, c) for c in range(L.dj_table_num_columns(t)))
        L.dj_table_free(t)
        if it >= args.warmup:
            times.append(dt)
            gather_ms.append(L.dj_timing_total_ms(dj.PHASE_GATHER))
    L.dj_timing_enable(0)
    L.dj_timing_reset()
    for p in lheld + rheld:
        L.dj_dfree(p)
    for cols in (left, right):
        for c in cols:
            if len(c) > 2:
                c[2].free()
    nmask = (len(O_TYPES) + len(L_TYPES)) * int(payload_masks) + 2 * int(key_mask)
    print(json.dumps({
        "metric": f"wide-table join step, masks: {name}", "unit": "ms", "higher_is_better": False,
        "value": stats(times)["median_ms"], "step": stats(times),
        "gather_phase": stats(gather_ms),
        "gather_phase_note": "value gather, key narrowing and the mask gather launch",
        "orders_rows": N_O, "lineitem_rows": N_L, "output_rows": int(rows),
        "nullable_output_columns": nmask, "output_nulls": int(nulls),
        # one mask-gather launch per nullable column, each reading 8 B of index
        "model_extra_bytes_per_output_row": nmask * (4 + 1 / 8 + 8),
        "reps": args.reps, "warmup": args.warmup,
    }), flush=True)


def gather_leg():
    idx = rng.randint(0, N_L, N_L).astype(np.int64)
    d_idx = upload(idx)
    recs = []
    for ncols in (1, 10):
        masks = [dj.upload_mask(rng.random_sample(N_L) >= 0.10) for _ in range(ncols)]
        ptrs = [m.ptr for m in masks]
        for per_launch in sorted({1, 2, 5, ncols} & set(range(1, ncols + 1))):
            dj.gather_bitmasks(ptrs, d_idx, N_L, reps=args.warmup, cols_per_launch=per_launch)
            _, counts, ms, _ = dj.gather_bitmasks(ptrs, d_idx, N_L, reps=args.reps,
                                                  cols_per_launch=per_launch)
            st = stats(ms)
            launches = -(-ncols // per_launch)
            bpr = ncols * (4 + 1 / 8) + 8 * launches  # the index is read once per launch
            st["model_bytes_per_row"] = bpr
            st["gbps_at_median"] = bpr * N_L / (st["median_ms"] * 1e-3) / 1e9
            recs.append({"nullable_columns": ncols, "columns_per_launch": per_launch,
                         "rows": N_L, "nulls_col0": int(counts[0]), **st})
        for m in masks:
            m.free()
    L.dj_dfree(d_idx)
    print(json.dumps({"metric": "mask gather kernel alone", "unit": "ms", "reps": args.reps,
                      "warmup": args.warmup, "cases": recs}), flush=True)


legs = args.legs.split(",")
if "plain" in legs:
    join_leg("mask-free entry point", False, False, plain=True)
if "none" in legs:
    join_leg("none", False, False)
if "payloads" in legs:
    join_leg("every payload column", False, True)
if "all" in legs:
    join_leg("every column, key included", True, True)
if "gather" in legs:
    gather_leg()
comm.destroy()
