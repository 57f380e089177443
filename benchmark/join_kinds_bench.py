#!/usr/bin/env python3
"""What the left / left semi / left anti joins cost next to the inner join, at
the shape of nullable_bench.py (orders-like 5 M rows LEFT JOIN lineitem-like
20 M rows, the same column types, no input masks) on one GPU:

  inner         through the existing entry point (the baseline);
  left_all      LEFT, every left row matched: the inner join's rows plus the
                bitmap pass, the concatenated left index and a mask on every
                right-hand column;
  left_30       LEFT, ~30 % of the left keys absent on the right;
  semi, anti    on the tables of left_30;
  mark_rows     the marking kernel alone through its hook, at that join's pair
                count (n = lineitem rows) and row count (nrows = orders rows),
                for indices in random order and in runs of equal neighbours,
                in each of its four variants (wave merge x load check);
  select_rows   the selection kernels alone, on the bitmap left_30 produces,
                both polarities.

Byte models.
  mark_rows:   8 B of index read per pair, plus the bitmap once in and once
               out: 8 n + 2 * nrows / 8 bytes. The atomic count is what the
               variants change: n without merge or check; with the check, one
               per bit that is not yet set (<= nrows).
  select_rows: nrows / 8 bytes of bitmap read (a second read of the same
               bytes, for the ranked write, comes from L2) and 8 B written per
               selected row: nrows / 8 + 8 * selected bytes.
The nearest measured ceilings the project holds are the random 8-byte atomic
scatter and the random 16-byte gather of profiles/r01_membench.log
(17.7 G atomics/s, 50.9 G loads/s); each mark_rows case reports its pairs/s
next to them. Each leg prints ONE JSON line.
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
ap.add_argument("--legs", default="inner,left_all,left_30,semi,anti,mark_rows,select_rows")
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
# every orders key at least once / only a random ~70 % of the orders keys
l_key_all = o_key[np.concatenate([np.arange(N_O), rng.randint(0, N_O, N_L - N_O)])]
_kept = np.flatnonzero(rng.random_sample(N_O) < 0.7)
_picks = _kept[rng.randint(0, len(_kept), N_L)]
l_key_30 = o_key[_picks]
matched_30 = np.zeros(N_O, dtype=bool)  # the orders rows left_30 finds a partner for
matched_30[_picks] = True

INT8, INT32, INT64, TS_DAYS = 1, 2, 3, 5
INT16, FLOAT32, FLOAT64 = 15, 20, 21
WIDTH = {INT8: 1, INT16: 2, INT32: 4, TS_DAYS: 4, FLOAT32: 4, INT64: 8, FLOAT64: 8}
DTYPE = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}
O_TYPES = [FLOAT64, INT8]
L_TYPES = [FLOAT64, FLOAT64, FLOAT32, TS_DAYS, INT8, INT8, INT16, INT64]
# r01_membench.log: random 8-byte atomic scatter, random 16-byte gather
MEMBENCH_ATOMIC_GOPS, MEMBENCH_GATHER_GOPS = 17.672, 50.942


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


def make_table(keys, types):
    held = [upload(keys)]
    cols = [(INT64, held[0])]
    for i, t in enumerate(types):
        held.append(upload(payload(len(keys), t, i + 1)))
        cols.append((t, held[-1]))
    return cols, held


def join_leg(name, kind, l_key):
    """kind None: the existing inner-join entry point."""
    left, lheld = make_table(o_key, O_TYPES)
    right, rheld = make_table(l_key, L_TYPES)
    la, ra = dj._pack_ncols(left), dj._pack_ncols(right)
    on = np.zeros(1, dtype=np.int32)
    head = (comm.ptr,) if kind is None else (comm.ptr, kind)
    entry = (L.dj_cpp_distributed_inner_join_ncols_multi if kind is None
             else L.dj_cpp_distributed_join_ncols_multi)
    times, rows, cols, nulls = [], 0, 0, 0
    for it in range(args.warmup + args.reps):
        L.dj_sync()
        t0 = time.perf_counter()
        t = entry(*head, ctypes.cast(la, ctypes.c_void_p), len(left), N_O,
                  ctypes.cast(ra, ctypes.c_void_p), len(right), N_L, on.ctypes.data,
                  on.ctypes.data, 1, 1, 0)
        L.dj_sync()
        dt = (time.perf_counter() - t0) * 1e3
        rows, cols = L.dj_table_num_rows(t), L.dj_table_num_columns(t)
        nulls = sum(L.dj_table_column_null_count(t, c) for c in range(cols))
        L.dj_table_free(t)
        if it >= args.warmup:
            times.append(dt)
    for p in lheld + rheld:
        L.dj_dfree(p)
    print(json.dumps({
        "metric": f"join step, {name}", "unit": "ms", "higher_is_better": False,
        "value": stats(times)["median_ms"], "step": stats(times),
        "orders_rows": N_O, "lineitem_rows": N_L, "output_rows": int(rows),
        "output_columns": int(cols), "output_nulls": int(nulls),
        "reps": args.reps, "warmup": args.warmup,
    }), flush=True)


def zeroed_bitmap(nrows):
    words = np.zeros((nrows + 31) // 32, dtype=np.uint32)
    return upload(words), words


def mark_leg():
    orders = {
        "random order": rng.randint(0, N_O, N_L).astype(np.int64),
        "runs of 4 equal neighbours": np.repeat(rng.randint(0, N_O, N_L // 4), 4).astype(np.int64),
    }
    recs = []
    for order, idx in orders.items():
        n = len(idx)
        d_idx = upload(idx)
        d_bits, zeros = zeroed_bitmap(N_O)
        distinct = len(np.unique(idx))
        for mode, label in ((dj.MARK_PLAIN, "plain atomics"), (dj.MARK_MERGE, "merge"),
                            (dj.MARK_CHECK, "check"),
                            (dj.MARK_MERGE | dj.MARK_CHECK, "merge + check")):
            ms = []
            for it in range(args.warmup + args.reps):
                L.dj_memcpy_h2d(d_bits, zeros.ctypes.data, zeros.nbytes)  # every rep starts empty
                t = dj.mark_rows(d_idx, n, d_bits, mode=mode, reps=1)[0]
                if it >= args.warmup:
                    ms.append(t)
            st = stats(ms)
            model = 8 * n + 2 * (N_O / 8)
            sec = st["median_ms"] * 1e-3
            st.update({"indices": order, "variant": label, "pairs": n, "rows": N_O,
                       "distinct_rows_marked": int(distinct), "model_bytes": model,
                       "model_gbps_at_median": model / sec / 1e9,
                       "g_pairs_per_s": n / sec / 1e9,
                       "vs_membench_atomic_scatter": n / sec / 1e9 / MEMBENCH_ATOMIC_GOPS,
                       "vs_membench_random_gather": n / sec / 1e9 / MEMBENCH_GATHER_GOPS})
            recs.append(st)
        L.dj_dfree(d_idx)
        L.dj_dfree(d_bits)
    print(json.dumps({"metric": "mark_rows kernel alone", "unit": "ms", "reps": args.reps,
                      "warmup": args.warmup, "engine_variant": "merge",
                      "membench_atomic_scatter_gops": MEMBENCH_ATOMIC_GOPS,
                      "membench_random_gather_gops": MEMBENCH_GATHER_GOPS,
                      "cases": recs}), flush=True)


def select_leg():
    matched = np.zeros((N_O + 31) // 32 * 32, dtype=bool)
    matched[:N_O] = matched_30  # the bitmap the left_30 join marks
    d_bits = upload(np.packbits(matched, bitorder="little").view(np.uint32))
    d_out = L.dj_dmalloc(N_O * 8)
    recs = []
    for want_set in (True, False):
        dj.select_rows(d_bits, N_O, want_set, d_out, reps=args.warmup)
        count, ms = dj.select_rows(d_bits, N_O, want_set, d_out, reps=args.reps)
        st = stats(ms)
        model = N_O / 8 + 8 * count
        st.update({"want_set": want_set, "rows": N_O, "selected": count, "model_bytes": model,
                   "model_gbps_at_median": model / (st["median_ms"] * 1e-3) / 1e9})
        recs.append(st)
    L.dj_dfree(d_bits)
    L.dj_dfree(d_out)
    print(json.dumps({"metric": "select_rows kernels alone", "unit": "ms", "reps": args.reps,
                      "warmup": args.warmup, "cases": recs}), flush=True)


legs = args.legs.split(",")
if "inner" in legs:
    join_leg("inner (existing entry point)", None, l_key_all)
if "left_all" in legs:
    join_leg("left, every left row matched", dj.JOIN_LEFT, l_key_all)
if "left_30" in legs:
    join_leg("left, ~30 % of the left keys absent on the right", dj.JOIN_LEFT, l_key_30)
if "semi" in legs:
    join_leg("left semi, ~30 % absent", dj.JOIN_LEFT_SEMI, l_key_30)
if "anti" in legs:
    join_leg("left anti, ~30 % absent", dj.JOIN_LEFT_ANTI, l_key_30)
if "mark_rows" in legs:
    mark_leg()
if "select_rows" in legs:
    select_leg()
comm.destroy()
