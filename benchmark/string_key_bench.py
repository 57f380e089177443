#!/usr/bin/env python3
"""string_key_bench.py — what STRING key columns cost on one MI355X.

(a) hash: the STRING-key row-hash kernel (dj_strings.hip hash_strings) on
    - `short`: --short-rows rows of the gen_test_strings shape (1-7 bytes),
    - `long` : --long-rows rows of 24-40 bytes,
    timed per launch with a hipEvent pair inside the library
    (dj_string_keys64). GB/s counts offsets + chars read + 64-bit keys
    written. The LDS-staged path is A/B-ed against forcing every block onto
    the direct-from-global path (DJ_STRHASH_FORCE_DIRECT, read once per
    process): fresh child processes alternate staged / direct / staged /
    direct so both modes see the same machine state. If experiments/membench
    is built, its stream_read figure from the same machine gives the read
    ceiling the GB/s are set against.
(b) join: a single-STRING-key join (key = the 8 bytes of the int64 key, so
    both joins produce the same rows) next to the int64-key join of the same
    row counts, through dj_cpp_distributed_inner_join_cols at world 1; host
    clock around the call, which returns synchronized. Legs alternate.

Prints one JSON document; --out also writes it to a file.
"""
import argparse
import ctypes
import json
import os
import re
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402


def _stats(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms),
            "reps": len(ms)}


def _time_hash(dj, off_p, ch_p, nb, n, warmup, reps):
    L = dj.lib()
    d_out = L.dj_dmalloc(max(n, 1) * 8)
    L.dj_string_keys64(off_p, ch_p, nb, n, d_out, warmup, None)
    ms = (ctypes.c_double * reps)()
    L.dj_string_keys64(off_p, ch_p, nb, n, d_out, reps, ctypes.cast(ms, ctypes.c_void_p))
    L.dj_dfree(d_out)
    bytes_moved = (n + 1) * 4 + nb + n * 8
    out = _stats(list(ms))
    out.update(rows=n, chars_bytes=nb, bytes_moved=bytes_moved,
               gbps=bytes_moved / out["median_ms"] / 1e6)
    return out


def hash_child(args):
    """One process = one mode (the env switch is read once): both shapes."""
    import distributed_join_amd as dj
    dj.require_gpu()
    L = dj.lib()
    L.dj_set_device(0)
    res = {"mode": "direct" if os.environ.get("DJ_STRHASH_FORCE_DIRECT") else "staged"}

    n = args.short_rows
    keys, pay = dj.generate_build(n)
    pay.free()
    off_p, ch_p, nb = dj.gen_test_strings(keys, n)
    res["short"] = _time_hash(dj, off_p, ch_p, nb, n, args.warmup, args.reps)
    L.dj_dfree(off_p)
    L.dj_dfree(ch_p)
    keys.free()

    n = args.long_rows
    rng = np.random.RandomState(7)
    off = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(rng.randint(24, 41, n), out=off[1:])
    nb = int(off[-1])
    off32 = off.astype(np.int32)
    chars = np.tile(np.arange(251, dtype=np.uint8), nb // 251 + 1)[:nb]
    off_p, ch_p = L.dj_dmalloc(off32.nbytes), L.dj_dmalloc(max(nb, 1))
    L.dj_memcpy_h2d(off_p, off32.ctypes.data, off32.nbytes)
    L.dj_memcpy_h2d(ch_p, chars.ctypes.data, nb)
    res["long"] = _time_hash(dj, off_p, ch_p, nb, n, args.warmup, args.reps)
    L.dj_dfree(off_p)
    L.dj_dfree(ch_p)
    print("HASH_CHILD " + json.dumps(res), flush=True)


def join_child(args):
    import distributed_join_amd as dj
    dj.require_gpu()
    L = dj.lib()
    L.dj_set_device(0)
    n = args.join_rows
    lk, lp = dj.generate_build(n)
    rk, rp = dj.generate_probe(n, n, selectivity=0.3)
    off = (np.arange(n + 1, dtype=np.int64) * 8).astype(np.int32)
    d_off = L.dj_dmalloc(off.nbytes)
    L.dj_memcpy_h2d(d_off, off.ctypes.data, off.nbytes)
    comm = dj.CppCommunicator(0, 1)

    pack = dj._pack_cols
    legs = {
        "int64_key": (pack([(dj.TYPE_INT64, lk.ptr), (dj.TYPE_INT64, lp.ptr)]),
                      pack([(dj.TYPE_INT64, rk.ptr), (dj.TYPE_INT64, rp.ptr)])),
        # the key column's chars ARE the int64 keys: 8-byte strings, same matches
        "string_key": (pack([(dj.TYPE_STRING, d_off, lk.ptr, 8 * n), (dj.TYPE_INT64, lp.ptr)]),
                       pack([(dj.TYPE_STRING, d_off, rk.ptr, 8 * n), (dj.TYPE_INT64, rp.ptr)])),
    }
    times = {k: [] for k in legs}
    rows = {}
    for it in range(args.warmup + args.reps):
        for name, (la, ra) in legs.items():
            L.dj_sync()
            t0 = time.perf_counter()
            t = L.dj_cpp_distributed_inner_join_cols(
                comm.ptr, ctypes.cast(la, ctypes.c_void_p), 2, n,
                ctypes.cast(ra, ctypes.c_void_p), 2, n, 0, 0, 1, 0)
            L.dj_sync()
            dt = (time.perf_counter() - t0) * 1e3
            rows[name] = L.dj_table_num_rows(t)
            L.dj_table_free(t)
            if it >= args.warmup:
                times[name].append(dt)
    comm.destroy()
    res = {name: dict(_stats(ms), rows_per_side=n, out_rows=rows[name])
           for name, ms in times.items()}
    res["string_over_int64"] = (res["string_key"]["median_ms"] /
                                res["int64_key"]["median_ms"])
    print("JOIN_CHILD " + json.dumps(res), flush=True)


def _run_child(leg, args, env):
    cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg,
           "--short-rows", str(args.short_rows), "--long-rows", str(args.long_rows),
           "--join-rows", str(args.join_rows), "--warmup", str(args.warmup),
           "--reps", str(args.reps)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=args.timeout)
    if r.returncode != 0:
        raise RuntimeError(f"{leg} failed ({r.returncode}):\n{r.stdout[-2000:]}{r.stderr[-2000:]}")
    tag = "HASH_CHILD " if leg == "hash-child" else "JOIN_CHILD "
    line = [ln for ln in r.stdout.splitlines() if ln.startswith(tag)][-1]
    return json.loads(line[len(tag):])


def _read_ceiling():
    exe = os.path.join(REPO, "experiments", "membench")
    if not os.path.exists(exe):
        return None
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    m = re.search(r"stream_read\s*:\s*[\d.]+ ms\s+([\d.]+) GB/s", r.stdout)
    return float(m.group(1)) if (r.returncode == 0 and m) else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", default="all", choices=["all", "hash", "join", "hash-child",
                                                     "join-child"])
    ap.add_argument("--short-rows", type=int, default=100_000_000)
    ap.add_argument("--long-rows", type=int, default=20_000_000)
    ap.add_argument("--join-rows", type=int, default=20_000_000)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=2, help="staged/direct child pairs")
    ap.add_argument("--timeout", type=int, default=400)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.leg == "hash-child":
        return hash_child(args)
    if args.leg == "join-child":
        return join_child(args)

    # the parent never opens the GPU: every measurement is a fresh child
    doc = {"bench": "string_key", "device": "MI355X (gfx950)", "warmup": args.warmup,
           "reps": args.reps}
    if args.leg in ("all", "hash"):
        ceiling = _read_ceiling()
        runs = []
        base = {k: v for k, v in os.environ.items() if k != "DJ_STRHASH_FORCE_DIRECT"}
        for _ in range(args.rounds):
            runs.append(_run_child("hash-child", args, base))
            runs.append(_run_child("hash-child", args, dict(base, DJ_STRHASH_FORCE_DIRECT="1")))
        summary = {}
        for shape in ("short", "long"):
            per_mode = {}
            for mode in ("staged", "direct"):
                med = [r[shape]["median_ms"] for r in runs if r["mode"] == mode]
                one = next(r[shape] for r in runs if r["mode"] == mode)
                best = min(med)
                per_mode[mode] = {
                    "median_ms_per_process": med,
                    "gbps_best": one["bytes_moved"] / best / 1e6,
                    "fraction_of_read_ceiling":
                        (one["bytes_moved"] / best / 1e6 / ceiling) if ceiling else None,
                }
            s, d = per_mode["staged"]["median_ms_per_process"], \
                per_mode["direct"]["median_ms_per_process"]
            # staged wins only if its slowest process beats direct's fastest
            per_mode["staged_wins_beyond_spread"] = max(s) < min(d)
            per_mode["rows"] = next(r[shape]["rows"] for r in runs)
            per_mode["chars_bytes"] = next(r[shape]["chars_bytes"] for r in runs)
            summary[shape] = per_mode
        doc["hash"] = {"stream_read_ceiling_gbps": ceiling, "shapes": summary, "runs": runs}
    if args.leg in ("all", "join"):
        doc["join"] = _run_child("join-child", args, dict(os.environ))
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
