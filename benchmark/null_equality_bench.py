#!/usr/bin/env python3
"""null_equality::UNEQUAL next to EQUAL on identical tables, at the shape of
nullable_bench.py / join_kinds_bench.py (orders-like 5 M rows joined with
lineitem-like 20 M rows, the same column types) on one GPU, with a validity
mask on the key of both sides:

  inner, left, semi, anti   each under EQUAL and under UNEQUAL, same tables;
  key_row_validity          the kernel alone through its hook;
  compact_keyed_rows        the kernel alone through its hook, on the right
                            table's key mask.

Null density. About 10 % of the right (lineitem-like) keys are null. Under
EQUAL every null left key pairs with every null right key, and the output of
one join is capped at 2^31 rows, so the left side cannot also be 10 % null at
this shape (5e5 x 2e6 = 1e12 pairs): it gets --left-nulls null keys (default
8, i.e. 8 x 2e6 = 1.6e7 extra EQUAL rows). The values under the nulls are
valid keys of the other side. ~30 % of the valid left keys have no partner.

Byte models (GB/s is reported against them).
  key_row_validity:   (nmasks + 1) * nrows / 8: every mask read once, the
                      result written once.
  compact_keyed_rows: nrows / 8 + 24 * selected: the bitmap once (its second
                      read is L2's), per selected row 8 B of key read and
                      8 + 8 B written.
key_row_validity's hook takes no repetition count, so it is timed on the host
around the call, which includes a memset, the launch, a count read-back and
a synchronisation; it is therefore also run at --validity-rows (default 2^30)
where the kernel outweighs them. Each leg prints ONE JSON line.
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
ap.add_argument("--left-nulls", type=int, default=8)
ap.add_argument("--right-null-frac", type=float, default=0.10)
ap.add_argument("--validity-rows", type=int, default=1 << 30)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--modes", default="equal,unequal")
ap.add_argument("--legs", default="inner,left,semi,anti,key_row_validity,compact_keyed_rows")
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
_kept = np.flatnonzero(rng.random_sample(N_O) < 0.7)   # ~30 % of the orders keys stay alone
l_key = o_key[_kept[rng.randint(0, len(_kept), N_L)]]
o_valid = np.ones(N_O, dtype=bool)
o_valid[rng.choice(N_O, size=min(args.left_nulls, N_O), replace=False)] = False
l_valid = rng.random_sample(N_L) >= args.right_null_frac
NULL_PAIRS = int((~o_valid).sum()) * int((~l_valid).sum())
assert NULL_PAIRS < 2 ** 31, "EQUAL's null cross product must stay below 2^31 rows"

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


def make_table(keys, valid, types):
    mask = dj.upload_mask(valid)
    held = [upload(keys)]
    cols = [(INT64, held[0], mask)]
    for i, t in enumerate(types):
        held.append(upload(payload(len(keys), t, i + 1)))
        cols.append((t, held[-1]))
    return cols, held, mask


def join_legs(kinds):
    left, lheld, lmask = make_table(o_key, o_valid, O_TYPES)
    right, rheld, rmask = make_table(l_key, l_valid, L_TYPES)
    la, ra = dj._pack_ncols(left), dj._pack_ncols(right)
    on = np.zeros(1, dtype=np.int32)
    tables = (ctypes.cast(la, ctypes.c_void_p), len(left), N_O,
              ctypes.cast(ra, ctypes.c_void_p), len(right), N_L, on.ctypes.data,
              on.ctypes.data, 1, 1, 0)
    for name, kind in kinds:
        medians = {}
        for mode in args.modes.split(","):
            times, rows, cols, nulls = [], 0, 0, 0
            for it in range(args.warmup + args.reps):
                L.dj_sync()
                t0 = time.perf_counter()
                if mode == "equal":
                    t = L.dj_cpp_distributed_join_ncols_multi(comm.ptr, kind, *tables)
                else:
                    t = L.dj_cpp_distributed_join_ncols_multi_ne(comm.ptr, kind, dj.NULL_UNEQUAL,
                                                                 *tables)
                L.dj_sync()
                dt = (time.perf_counter() - t0) * 1e3
                rows, cols = L.dj_table_num_rows(t), L.dj_table_num_columns(t)
                nulls = sum(L.dj_table_column_null_count(t, c) for c in range(cols))
                L.dj_table_free(t)
                if it >= args.warmup:
                    times.append(dt)
            medians[mode] = stats(times)["median_ms"]
            rec = {
                "metric": f"join step, {name}, null_equality {mode.upper()}", "unit": "ms",
                "higher_is_better": False, "value": medians[mode], "step": stats(times),
                "orders_rows": N_O, "lineitem_rows": N_L,
                "left_null_keys": int((~o_valid).sum()), "right_null_keys": int((~l_valid).sum()),
                "equal_null_pairs": NULL_PAIRS, "output_rows": int(rows),
                "output_columns": int(cols), "output_nulls": int(nulls),
                "reps": args.reps, "warmup": args.warmup,
            }
            if len(medians) == 2:
                rec["unequal_over_equal"] = medians["unequal"] / medians["equal"]
            print(json.dumps(rec), flush=True)
    for p in lheld + rheld:
        L.dj_dfree(p)
    lmask.free()
    rmask.free()


def validity_leg():
    recs = []
    for nrows in (N_L, args.validity_rows):
        nwords = (nrows + 31) // 32
        for nmasks in (2, 4):
            masks = [upload(rng.randint(0, 2 ** 32, nwords, dtype=np.uint64).astype(np.uint32))
                     for _ in range(nmasks)]
            d_out = L.dj_dmalloc(nwords * 4)
            ms, nulls = [], 0
            for it in range(args.warmup + args.reps):
                L.dj_sync()
                t0 = time.perf_counter()
                nulls = dj.key_row_validity(masks, nrows, d_out)
                dt = (time.perf_counter() - t0) * 1e3
                if it >= args.warmup:
                    ms.append(dt)
            st = stats(ms)
            model = (nmasks + 1) * nrows / 8
            st.update({"rows": nrows, "masks": nmasks, "null_rows": nulls, "model_bytes": model,
                       "timed": "host clock around the hook (memset, launch, read-back, sync)",
                       "model_gbps_at_median": model / (st["median_ms"] * 1e-3) / 1e9})
            recs.append(st)
            for p in masks + [d_out]:
                L.dj_dfree(p)
    print(json.dumps({"metric": "key_row_validity kernel through its hook", "unit": "ms",
                      "reps": args.reps, "warmup": args.warmup, "cases": recs}), flush=True)


def compact_leg():
    padded = np.zeros((N_L + 31) // 32 * 32, dtype=bool)
    padded[:N_L] = l_valid
    d_bits = upload(np.packbits(padded, bitorder="little").view(np.uint32))
    d_keys = upload(l_key)
    nsel = int(l_valid.sum())
    d_idx, d_out = L.dj_dmalloc(max(nsel, 1) * 8), L.dj_dmalloc(max(nsel, 1) * 8)
    dj.compact_keyed_rows(d_bits, N_L, d_keys, d_idx, d_out, reps=args.warmup)
    count, ms = dj.compact_keyed_rows(d_bits, N_L, d_keys, d_idx, d_out, reps=args.reps)
    assert count == nsel
    st = stats(ms)
    model = N_L / 8 + 24 * count
    st.update({"rows": N_L, "selected": count, "model_bytes": model,
               "model_gbps_at_median": model / (st["median_ms"] * 1e-3) / 1e9})
    for p in (d_bits, d_keys, d_idx, d_out):
        L.dj_dfree(p)
    print(json.dumps({"metric": "compact_keyed_rows kernels alone", "unit": "ms",
                      "reps": args.reps, "warmup": args.warmup, "cases": [st]}), flush=True)


legs = args.legs.split(",")
KINDS = [("inner", dj.JOIN_INNER), ("left", dj.JOIN_LEFT), ("semi", dj.JOIN_LEFT_SEMI),
         ("anti", dj.JOIN_LEFT_ANTI)]
wanted = [(n, k) for n, k in KINDS if n in legs]
if wanted:
    join_legs(wanted)
if "key_row_validity" in legs:
    validity_leg()
if "compact_keyed_rows" in legs:
    compact_leg()
comm.destroy()
