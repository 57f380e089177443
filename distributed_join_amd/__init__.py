"""distributed_join_amd — MI355X-native distributed repartitioned hash join.

Python binding (ctypes) over the C ABI of libdistjoin.so (see
include/distributed_join.h for the contract and the reference interfaces each
entry point replaces). This is the PRODUCT path: hand-written gfx950 HIP
kernels + RCCL over xGMI. It never falls back to CPU — if the HIP extension
is missing or no GPU is visible, compute calls fail loudly.
"""
import ctypes
import os

import numpy as np

_DIR = os.path.dirname(os.path.abspath(__file__))
_SO = os.path.join(_DIR, "libdistjoin.so")

HASH_MURMUR3 = 0
HASH_IDENTITY = 1
SEED_INTRA = 12345678
SEED_INTER = 87654321
DEFAULT_SEED = 1234

PHASES = {
    "generate": 0, "part_count": 1, "part_scan": 2, "part_scatter": 3,
    "table_init": 4, "build": 5, "probe": 6, "comm": 7, "concat": 8,
    "bucket_count": 9, "bucket_scan": 10, "bucket_scatter": 11, "join_fused": 12,
}

# output assembly (table gather + key narrowing); kept out of PHASES, whose
# key set is part of bench.py's record
PHASE_GATHER = 13

_lib = None


class ExtensionMissing(RuntimeError):
    pass


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(_SO):
            raise ExtensionMissing(
                f"{_SO} not built. Run `make -C {os.path.join(_DIR, 'csrc')}` "
                "(or __graft_entry__.build()). The product path has no CPU fallback.")
        _lib = ctypes.CDLL(_SO)
        c = ctypes
        i64, u64, u32, i32, dbl = c.c_int64, c.c_uint64, c.c_uint32, c.c_int, c.c_double
        vp = c.c_void_p
        sigs = {
            "dj_device_count": ([], i32),
            "dj_set_device": ([i32], None),
            "dj_dmalloc": ([i64], vp),
            "dj_dfree": ([vp], None),
            "dj_memcpy_h2d": ([vp, vp, i64], None),
            "dj_memcpy_d2h": ([vp, vp, i64], None),
            "dj_memcpy_d2d": ([vp, vp, i64], None),
            "dj_sync": ([], None),
            "dj_generate_build": ([vp, vp, i64, i64, u64, i32, i64, i64], None),
            "dj_generate_probe": ([vp, vp, i64, i64, dbl, u64, i64, i64], None),
            "dj_partition_scratch_bytes": ([i64, i32], i64),
            "dj_hash_partition": ([vp, vp, i64, i32, i32, u32, vp, vp, vp, vp], None),
            "dj_join_table_slots": ([i64], i64),
            "dj_join_table_init": ([vp, i64], None),
            "dj_join_build": ([vp, vp, i64, vp, i64, vp], None),
            "dj_join_probe": ([vp, vp, i64, vp, i64, vp, vp, vp, vp, i64, vp], None),
            "dj_read_counter_i64": ([vp], i64),
            "dj_read_error_i32": ([vp], i32),
            "dj_local_inner_join": ([vp, vp, i64, vp, vp, i64, vp, vp, vp, vp, i64], i64),
            "dj_local_inner_join_global": ([vp, vp, i64, vp, vp, i64, vp, vp, vp, vp, i64], i64),
            "dj_bucket_join_scratch_bytes": ([i64, i64], i64),
            "dj_bucket_local_join": ([vp, vp, i64, vp, vp, i64, vp, vp, vp, vp, i64,
                                      vp, vp, vp], None),
            "dj_timing_enable": ([i32], None),
            "dj_timing_reset": ([], None),
            "dj_timing_total_ms": ([i32], dbl),
            "dj_timing_launches": ([i32], i64),
            "dj_rccl_unique_id_bytes": ([], i32),
            "dj_rccl_get_unique_id": ([vp], None),
            "dj_comm_init": ([i32, i32, vp], None),
            "dj_comm_finalize": ([], None),
            "dj_comm_rank": ([], i32),
            "dj_comm_size": ([], i32),
            "dj_all_to_all_i64": ([vp, vp, vp, vp], None),
            "dj_exchange_sizes": ([vp, vp], None),
            "dj_rccl_selftest": ([i64], i32),
            "dj_compress_roundtrip": ([vp, i64, i32, i32, i32, i32, vp], i64),
            "dj_cpp_comm_create": ([i32, i32, vp], vp),
            "dj_cpp_comm_destroy": ([vp], None),
            "dj_cpp_distributed_inner_join_i64": ([vp, vp, vp, i64, vp, vp, i64, i32, i32], vp),
            "dj_cpp_shuffle_on_i64": ([vp, vp, vp, i64, i32, u32], vp),
            "dj_cpp_shuffle_on_i64_comp": ([vp, vp, vp, i64, i32, u32, i32], vp),
            "dj_cpp_distributed_inner_join_i64_opts": ([vp, vp, vp, i64, vp, vp, i64,
                                                        i32, i32, i32], vp),
            "dj_cpp_distributed_inner_join_i64_full": ([vp, vp, vp, i64, vp, vp, i64,
                                                        i32, i32, i32, i32], vp),
            "dj_gen_test_strings": ([vp, i64, ctypes.POINTER(ctypes.c_void_p),
                                     ctypes.POINTER(ctypes.c_void_p),
                                     ctypes.POINTER(ctypes.c_int64)], None),
            "dj_cpp_distributed_inner_join_i64str": ([vp, vp, vp, vp, i64, i64,
                                                      vp, vp, vp, i64, i64, i32, i32], vp),
            "dj_cpp_distributed_inner_join_cols": ([vp, vp, i32, i64, vp, i32, i64,
                                                    i32, i32, i32, i32], vp),
            "dj_cpp_distributed_inner_join_cols_multi": ([vp, vp, i32, i64, vp, i32, i64,
                                                          vp, vp, i32, i32, i32], vp),
            "dj_cpp_shuffle_on_cols": ([vp, vp, i32, i64, vp, i32, i32, u32, i32], vp),
            "dj_hash_strings": ([vp, vp, i64, i64, u32, vp], None),
            "dj_string_keys64": ([vp, vp, i64, i64, vp, i32, vp], None),
            "dj_cpp_distribute_collect_roundtrip_i64": ([vp, vp, vp, i64], vp),
            "dj_table_column_type": ([vp, i32], i32),
            "dj_table_column_chars": ([vp, i32], vp),
            "dj_table_column_chars_size": ([vp, i32], i64),
            "dj_table_num_rows": ([vp], i64),
            "dj_table_num_columns": ([vp], i32),
            "dj_table_column_data": ([vp, i32], vp),
            "dj_table_free": ([vp], None),
            "dj_gather_columns": ([vp, i32, vp, i64, i32, i32, vp], None),
            "dj_cpp_partition_cols": ([vp, i32, i64, vp, i32, i32, i32, u32, vp], vp),
            "dj_cpp_distributed_inner_join_ncols_multi": ([vp, vp, i32, i64, vp, i32, i64,
                                                           vp, vp, i32, i32, i32], vp),
            "dj_cpp_shuffle_on_ncols": ([vp, vp, i32, i64, vp, i32, i32, u32, i32], vp),
            "dj_cpp_partition_ncols": ([vp, i32, i64, vp, i32, i32, i32, u32, vp], vp),
            "dj_cpp_concat_tables": ([vp, i32], vp),
            "dj_table_column_null_mask": ([vp, i32], vp),
            "dj_table_column_null_count": ([vp, i32], i64),
            "dj_gather_bitmasks": ([vp, vp, i32, vp, i64, vp, i32, vp, i32], None),
            "dj_copy_bitmask_segments": ([vp, vp, vp, i32, vp], i64),
            "dj_cpp_distributed_join_ncols_multi": ([vp, i32, vp, i32, i64, vp, i32, i64,
                                                     vp, vp, i32, i32, i32], vp),
            "dj_cpp_distributed_join_ncols_multi_ne": ([vp, i32, i32, vp, i32, i64, vp, i32, i64,
                                                        vp, vp, i32, i32, i32], vp),
            "dj_key_row_validity": ([vp, i32, i64, vp], i64),
            "dj_compact_keyed_rows": ([vp, i64, vp, vp, vp, i32, vp], i64),
            "dj_mark_rows": ([vp, i64, vp, i32, i32, vp], None),
            "dj_select_rows": ([vp, i64, i32, vp, i32, vp], i64),
            "dj_select_rows_tile_rows": ([], i64),
            "dj_grid_span": ([i32, c.POINTER(i64), c.POINTER(i64)], i32),
        }
        for name, (argtypes, restype) in sigs.items():
            f = getattr(_lib, name)
            f.argtypes = argtypes
            f.restype = restype
    return _lib


def require_gpu():
    n = lib().dj_device_count()
    if n < 1:
        raise ExtensionMissing("no HIP device visible; the product path requires an MI355X")
    return n


# ---------------------------------------------------------------- helpers

class DeviceArray:
    """Owning device buffer of int64 elements."""

    def __init__(self, n):
        self.n = int(n)
        self.ptr = lib().dj_dmalloc(max(self.n, 1) * 8)

    def free(self):
        if self.ptr:
            lib().dj_dfree(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass

    def to_numpy(self, n=None):
        n = self.n if n is None else int(n)
        out = np.empty(n, dtype=np.int64)
        lib().dj_memcpy_d2h(out.ctypes.data, self.ptr, n * 8)
        return out

    @classmethod
    def from_numpy(cls, a):
        a = np.ascontiguousarray(a, dtype=np.int64)
        d = cls(len(a))
        if len(a):
            lib().dj_memcpy_h2d(d.ptr, a.ctypes.data, len(a) * 8)
        return d


def generate_build(n_global, rand_max=None, seed=DEFAULT_SEED, uniq=True, row0=0, nrows=None):
    if rand_max is None:
        rand_max = 2 * n_global
    if nrows is None:
        nrows = n_global - row0
    keys, pay = DeviceArray(nrows), DeviceArray(nrows)
    lib().dj_generate_build(keys.ptr, pay.ptr, n_global, rand_max, seed, int(uniq), row0, nrows)
    return keys, pay


def generate_probe(probe_n, build_n_global, rand_max=None, selectivity=0.3, seed=DEFAULT_SEED,
                   row0=0, nrows=None):
    if rand_max is None:
        rand_max = 2 * build_n_global
    if nrows is None:
        nrows = probe_n - row0
    keys, pay = DeviceArray(nrows), DeviceArray(nrows)
    lib().dj_generate_probe(keys.ptr, pay.ptr, build_n_global, rand_max, selectivity, seed,
                            row0, nrows)
    return keys, pay


def hash_partition(d_keys, d_pay, n, nparts, hash_fn=HASH_MURMUR3, seed=0,
                   d_out_keys=None, d_out_pay=None, d_scratch=None):
    """Stable partition; returns (d_out_keys, d_out_pay, host offsets)."""
    L = lib()
    own_scratch = d_scratch is None
    if own_scratch:
        d_scratch = L.dj_dmalloc(L.dj_partition_scratch_bytes(n, nparts))
    if d_out_keys is None:
        d_out_keys = DeviceArray(n)
    if d_out_pay is None:
        d_out_pay = DeviceArray(n)
    offsets = np.zeros(nparts + 1, dtype=np.int64)
    L.dj_hash_partition(d_keys.ptr, d_pay.ptr if d_pay else None, n, nparts, hash_fn, seed,
                        d_out_keys.ptr, d_out_pay.ptr, offsets.ctypes.data, d_scratch)
    if own_scratch:
        L.dj_dfree(d_scratch)
    return d_out_keys, d_out_pay, offsets


def local_inner_join(d_lk, d_lp, ln, d_rk, d_rp, rn, cap=None):
    """One-call local join; returns 4 numpy columns (lkey,lpay,rkey,rpay)."""
    L = lib()
    if cap is None:
        cap = max(int(rn) * 2, 16)
    while True:
        outs = [DeviceArray(cap) for _ in range(4)]
        n = L.dj_local_inner_join(d_lk.ptr, d_lp.ptr, ln, d_rk.ptr, d_rp.ptr, rn,
                                  outs[0].ptr, outs[1].ptr, outs[2].ptr, outs[3].ptr, cap)
        if n <= cap:
            res = tuple(o.to_numpy(n) for o in outs)
            for o in outs:
                o.free()
            return res
        for o in outs:
            o.free()
        cap = n


def local_inner_join_global(d_lk, d_lp, ln, d_rk, d_rp, rn, cap=None):
    """Global-table engine (the skew-fallback path), for cross-checking."""
    L = lib()
    if cap is None:
        cap = max(int(rn) * 2, 16)
    while True:
        outs = [DeviceArray(cap) for _ in range(4)]
        n = L.dj_local_inner_join_global(d_lk.ptr, d_lp.ptr, ln, d_rk.ptr, d_rp.ptr, rn,
                                         outs[0].ptr, outs[1].ptr, outs[2].ptr, outs[3].ptr,
                                         cap)
        if n <= cap:
            res = tuple(o.to_numpy(n) for o in outs)
            for o in outs:
                o.free()
            return res
        for o in outs:
            o.free()
        cap = n


TYPE_INT8, TYPE_INT32, TYPE_INT64, TYPE_STRING = 1, 2, 3, 4
# chrono reps (4-byte DAYS, 8-byte the rest) — join on the integer rep
TYPE_TIMESTAMP_DAYS, TYPE_TIMESTAMP_S, TYPE_TIMESTAMP_MS = 5, 6, 7
TYPE_TIMESTAMP_US, TYPE_TIMESTAMP_NS = 8, 9
TYPE_DURATION_DAYS, TYPE_DURATION_S, TYPE_DURATION_MS = 10, 11, 12
TYPE_DURATION_US, TYPE_DURATION_NS = 13, 14
# appended fixed-width types (ids 0..14 above are C-ABI values and never move)
TYPE_INT16, TYPE_UINT8, TYPE_UINT16, TYPE_UINT32 = 15, 16, 17, 18
TYPE_UINT64, TYPE_FLOAT32, TYPE_FLOAT64, TYPE_BOOL8 = 19, 20, 21, 22

# type_id -> numpy dtype of every fixed-width column type (chrono types as
# their integer rep, BOOL8 as its one-byte rep)
NUMPY_DTYPE = {
    TYPE_INT8: np.dtype(np.int8), TYPE_INT32: np.dtype(np.int32),
    TYPE_INT64: np.dtype(np.int64),
    TYPE_TIMESTAMP_DAYS: np.dtype(np.int32), TYPE_TIMESTAMP_S: np.dtype(np.int64),
    TYPE_TIMESTAMP_MS: np.dtype(np.int64), TYPE_TIMESTAMP_US: np.dtype(np.int64),
    TYPE_TIMESTAMP_NS: np.dtype(np.int64),
    TYPE_DURATION_DAYS: np.dtype(np.int32), TYPE_DURATION_S: np.dtype(np.int64),
    TYPE_DURATION_MS: np.dtype(np.int64), TYPE_DURATION_US: np.dtype(np.int64),
    TYPE_DURATION_NS: np.dtype(np.int64),
    TYPE_INT16: np.dtype(np.int16), TYPE_UINT8: np.dtype(np.uint8),
    TYPE_UINT16: np.dtype(np.uint16), TYPE_UINT32: np.dtype(np.uint32),
    TYPE_UINT64: np.dtype(np.uint64), TYPE_FLOAT32: np.dtype(np.float32),
    TYPE_FLOAT64: np.dtype(np.float64), TYPE_BOOL8: np.dtype(np.uint8),
}
# default type_id of a numpy dtype (uint8 -> UINT8; pass TYPE_BOOL8 explicitly)
_TYPE_OF_DTYPE = {
    np.dtype(np.int8): TYPE_INT8, np.dtype(np.int16): TYPE_INT16,
    np.dtype(np.int32): TYPE_INT32, np.dtype(np.int64): TYPE_INT64,
    np.dtype(np.uint8): TYPE_UINT8, np.dtype(np.uint16): TYPE_UINT16,
    np.dtype(np.uint32): TYPE_UINT32, np.dtype(np.uint64): TYPE_UINT64,
    np.dtype(np.float32): TYPE_FLOAT32, np.dtype(np.float64): TYPE_FLOAT64,
    np.dtype(np.bool_): TYPE_BOOL8,
}


class DeviceColumn:
    """Owning device copy of a numpy array of any supported fixed-width dtype.
    `desc` is the (type_id, data_ptr) tuple the *_cols entry points take.
    offset_elems > 0 places the column that many elements into its allocation
    (an element-aligned, not allocation-aligned, base)."""

    def __init__(self, a, type_id=None, offset_elems=0):
        a = np.ascontiguousarray(a)
        if type_id is None:
            if a.dtype not in _TYPE_OF_DTYPE:
                raise TypeError(f"unsupported column dtype {a.dtype}")
            type_id = _TYPE_OF_DTYPE[a.dtype]
        want = NUMPY_DTYPE[type_id]
        if a.dtype.itemsize != want.itemsize:
            raise TypeError(f"dtype {a.dtype} does not fit type_id {type_id} ({want})")
        self.type_id = int(type_id)
        self.n = len(a)
        self.itemsize = a.dtype.itemsize
        off = int(offset_elems) * self.itemsize
        self.base = lib().dj_dmalloc(max(a.nbytes + off, 1))
        self.ptr = self.base + off
        if a.nbytes:
            lib().dj_memcpy_h2d(self.ptr, a.ctypes.data, a.nbytes)

    @property
    def desc(self):
        return (self.type_id, self.ptr)

    def free(self):
        if self.base:
            lib().dj_dfree(self.base)
            self.base = None
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def upload_column(a, type_id=None):
    """Upload a numpy array of any supported dtype; returns a DeviceColumn."""
    return DeviceColumn(a, type_id)


def table_to_numpy(tbl_ptr):
    """Copy an opaque cudf::table* (C ABI) into numpy columns and free it.
    Fixed-width columns -> arrays of their own dtype (NUMPY_DTYPE); STRING
    columns -> (offsets int32 array, chars uint8 array) tuples."""
    L = lib()
    n = L.dj_table_num_rows(tbl_ptr)
    ncols = L.dj_table_num_columns(tbl_ptr)
    cols = []
    for c in range(ncols):
        t = L.dj_table_column_type(tbl_ptr, c)
        data = L.dj_table_column_data(tbl_ptr, c)
        if t == TYPE_STRING:
            off = np.empty(n + 1, dtype=np.int32)
            L.dj_memcpy_d2h(off.ctypes.data, data, (n + 1) * 4)
            nch = L.dj_table_column_chars_size(tbl_ptr, c)
            ch = np.empty(max(nch, 1), dtype=np.uint8)
            if nch:
                L.dj_memcpy_d2h(ch.ctypes.data, L.dj_table_column_chars(tbl_ptr, c), nch)
            cols.append((off, ch[:nch]))
        else:
            out = np.empty(n, dtype=NUMPY_DTYPE[t])
            if n:
                L.dj_memcpy_d2h(out.ctypes.data, data, out.nbytes)
            cols.append(out)
    L.dj_table_free(tbl_ptr)
    return cols


class CppCommunicator:
    """RCCLCommunicator (or single-process LocalCommunicator) handle."""

    def __init__(self, rank=0, size=1, id_bytes=None):
        L = lib()
        ptr = None if id_bytes is None else id_bytes.ctypes.data
        self.ptr = L.dj_cpp_comm_create(rank, size, ptr)

    def destroy(self):
        if self.ptr:
            lib().dj_cpp_comm_destroy(self.ptr)
            self.ptr = None


def cpp_distributed_inner_join(comm, d_lk, d_lp, ln, d_rk, d_rp, rn, over_decom=1,
                               report_timing=False):
    """The C++ drop-in path (distributed_inner_join) over int64 columns.
    Returns numpy columns (lkey, lpay, rkey, rpay) of this rank's result."""
    t = lib().dj_cpp_distributed_inner_join_i64(comm.ptr, d_lk.ptr, d_lp.ptr, ln,
                                                d_rk.ptr, d_rp.ptr, rn, over_decom,
                                                int(report_timing))
    return table_to_numpy(t)


def gen_test_strings(d_keys, n):
    """Deterministic string payload from keys (len=k%7+1, char='a'+k%26).
    Returns (offsets_ptr, chars_ptr, chars_bytes); caller frees via dj_dfree."""
    L = lib()
    off = ctypes.c_void_p()
    ch = ctypes.c_void_p()
    nb = ctypes.c_int64()
    L.dj_gen_test_strings(d_keys.ptr, n, ctypes.byref(off), ctypes.byref(ch),
                          ctypes.byref(nb))
    return off.value, ch.value, nb.value


def cpp_distributed_inner_join_str(comm, d_lk, l_strings, ln, d_rk, r_strings, rn,
                                   over_decom=1):
    """Distributed join with int64 keys and STRING payloads (config 4)."""
    lo, lc, lb = l_strings
    ro, rc, rb = r_strings
    t = lib().dj_cpp_distributed_inner_join_i64str(
        comm.ptr, d_lk.ptr, lo, lc, lb, ln, d_rk.ptr, ro, rc, rb, rn, over_decom, 0)
    return table_to_numpy(t)


class ColDesc(ctypes.Structure):
    _fields_ = [("type_id", ctypes.c_int), ("data", ctypes.c_void_p),
                ("chars", ctypes.c_void_p), ("chars_bytes", ctypes.c_int64)]


def _pack_cols(cols):
    """cols: (type_id, data_ptr[, chars_ptr, chars_bytes]) tuples -> ColDesc array."""
    arr = (ColDesc * len(cols))()
    for i, c in enumerate(cols):
        arr[i].type_id = c[0]
        arr[i].data = c[1]
        arr[i].chars = c[2] if len(c) > 2 else None
        arr[i].chars_bytes = c[3] if len(c) > 3 else 0
    return arr


def cpp_distributed_inner_join_cols(comm, lcols, ln, rcols, rn, key_l=0, key_r=0,
                                    over_decom=1):
    """Generic join over column descriptors: each col is
    (type_id, data_ptr[, chars_ptr, chars_bytes])."""
    la, ra = _pack_cols(lcols), _pack_cols(rcols)
    t = lib().dj_cpp_distributed_inner_join_cols(
        comm.ptr, ctypes.cast(la, ctypes.c_void_p), len(lcols), ln,
        ctypes.cast(ra, ctypes.c_void_p), len(rcols), rn, key_l, key_r, over_decom, 0)
    return table_to_numpy(t)


def cpp_distributed_inner_join_cols_multi(comm, lcols, ln, rcols, rn, left_on, right_on,
                                          over_decom=1):
    """Composite-key join over column descriptors (left_on/right_on are
    lists of key column indices; the single-key restriction lifts here)."""
    la, ra = _pack_cols(lcols), _pack_cols(rcols)
    lon = np.asarray(left_on, dtype=np.int32)
    ron = np.asarray(right_on, dtype=np.int32)
    t = lib().dj_cpp_distributed_inner_join_cols_multi(
        comm.ptr, ctypes.cast(la, ctypes.c_void_p), len(lcols), ln,
        ctypes.cast(ra, ctypes.c_void_p), len(rcols), rn,
        lon.ctypes.data, ron.ctypes.data, len(lon), over_decom, 0)
    return table_to_numpy(t)


def upload_strings(strings):
    """Upload a list of bytes objects as a STRING column. Returns
    (offsets_ptr, chars_ptr, chars_bytes) — int32 offsets[n+1] and an
    exact-size chars buffer; caller frees both via dj_dfree."""
    L = lib()
    sizes = np.fromiter((len(s) for s in strings), dtype=np.int64, count=len(strings))
    off = np.zeros(len(strings) + 1, dtype=np.int64)
    np.cumsum(sizes, out=off[1:])
    if off[-1] >= 2 ** 31:
        raise ValueError("STRING column chars exceed 2^31 (int32 offsets)")
    off32 = off.astype(np.int32)
    chars = np.frombuffer(b"".join(strings), dtype=np.uint8)
    d_off = L.dj_dmalloc(off32.nbytes)
    L.dj_memcpy_h2d(d_off, off32.ctypes.data, off32.nbytes)
    d_chars = L.dj_dmalloc(max(len(chars), 1))
    if len(chars):
        L.dj_memcpy_h2d(d_chars, chars.ctypes.data, len(chars))
    return d_off, d_chars, int(len(chars))


def hash_strings(offsets_ptr, chars_ptr, chars_bytes, n, seed=0):
    """MurmurHash3_x86_32(row bytes, seed) per row of a device STRING column,
    through the kernel that hashes STRING key columns. Returns uint32[n]."""
    L = lib()
    out = np.empty(n, dtype=np.uint32)
    d_out = L.dj_dmalloc(max(n, 1) * 4)
    L.dj_hash_strings(offsets_ptr, chars_ptr, chars_bytes, n, seed, d_out)
    if n:
        L.dj_memcpy_d2h(out.ctypes.data, d_out, n * 4)
    L.dj_dfree(d_out)
    return out


def cpp_shuffle_on_cols(comm, cols, n, on, hash_fn=HASH_MURMUR3, seed=0, compression=False):
    """shuffle_on over column descriptors (see cpp_distributed_inner_join_cols);
    `on` lists the key column indices, STRING columns included. compression:
    False/0 none, True/1 fixed bitpack policy, 2 sampling auto-select, 3 an
    explicit cascaded option on every column (a loud error on float/bool)."""
    arr = _pack_cols(cols)
    keys = np.asarray(on, dtype=np.int32)
    t = lib().dj_cpp_shuffle_on_cols(comm.ptr, ctypes.cast(arr, ctypes.c_void_p), len(cols), n,
                                     keys.ctypes.data, len(keys), hash_fn, seed,
                                     int(compression))
    return table_to_numpy(t)


def cpp_partition_cols(cols, n, on, nparts, hash_fn=HASH_MURMUR3, seed=0):
    """The placement step of shuffle_on alone (test hook): returns
    (numpy columns of the partitioned table, host offsets[nparts+1])."""
    arr = _pack_cols(cols)
    keys = np.asarray(on, dtype=np.int32)
    offsets = np.zeros(nparts + 1, dtype=np.int64)
    t = lib().dj_cpp_partition_cols(ctypes.cast(arr, ctypes.c_void_p), len(cols), n,
                                    keys.ctypes.data, len(keys), nparts, hash_fn, seed,
                                    offsets.ctypes.data)
    return table_to_numpy(t), offsets


def cpp_shuffle_on(comm, d_keys, d_pay, n, hash_fn=HASH_MURMUR3, seed=0,
                   compression=False):
    if compression:
        t = lib().dj_cpp_shuffle_on_i64_comp(comm.ptr, d_keys.ptr, d_pay.ptr, n, hash_fn,
                                             seed, 1)
    else:
        t = lib().dj_cpp_shuffle_on_i64(comm.ptr, d_keys.ptr, d_pay.ptr, n, hash_fn, seed)
    return table_to_numpy(t)


# ------------------------------------------------- nullable columns (masks)

class NColDesc(ctypes.Structure):
    _fields_ = [("type_id", ctypes.c_int), ("data", ctypes.c_void_p),
                ("chars", ctypes.c_void_p), ("chars_bytes", ctypes.c_int64),
                ("null_mask", ctypes.c_void_p), ("null_count", ctypes.c_int64)]


def pack_mask(valid):
    """bool array -> uint32 mask words in the cuDF layout (row i = bit i % 32,
    LSB first, of word i / 32), padded with 0 bits to a multiple of 64 rows."""
    valid = np.asarray(valid, dtype=bool)
    padded = np.zeros((len(valid) + 63) // 64 * 64, dtype=bool)
    padded[:len(valid)] = valid
    return np.packbits(padded, bitorder="little").view(np.uint32)


def unpack_mask(words, n):
    """uint32 mask words -> bool array of the first n rows."""
    bits = np.unpackbits(np.ascontiguousarray(words).view(np.uint8), bitorder="little")
    return bits[:n].astype(bool)


class DeviceMask:
    """Owning device validity mask; `.ptr` is the mask pointer and
    `.null_count` the number of False rows of the uploaded bool array."""

    def __init__(self, valid):
        valid = np.asarray(valid, dtype=bool)
        self.n = len(valid)
        self.null_count = int(self.n - valid.sum())
        words = pack_mask(valid)
        self.ptr = lib().dj_dmalloc(max(words.nbytes, 64))
        if words.nbytes:
            lib().dj_memcpy_h2d(self.ptr, words.ctypes.data, words.nbytes)

    def free(self):
        if self.ptr:
            lib().dj_dfree(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def upload_mask(bool_array):
    """Upload a bool array (True = valid) as a validity mask; returns a
    DeviceMask to name as the `mask` of a nullable column descriptor."""
    return DeviceMask(bool_array)


def _pack_ncols(cols):
    """cols: (type_id, data_ptr[, chars_ptr, chars_bytes]) tuples, each with an
    optional trailing DeviceMask (or None) -> NColDesc array."""
    arr = (NColDesc * max(len(cols), 1))()
    for i, c in enumerate(cols):
        c = tuple(c)
        mask = None
        if c and (c[-1] is None or isinstance(c[-1], DeviceMask)) and len(c) in (3, 5):
            mask, c = c[-1], c[:-1]
        arr[i].type_id = c[0]
        arr[i].data = c[1]
        arr[i].chars = c[2] if len(c) > 2 else None
        arr[i].chars_bytes = c[3] if len(c) > 3 else 0
        arr[i].null_mask = mask.ptr if mask is not None else None
        arr[i].null_count = mask.null_count if mask is not None else 0
    return arr


def table_to_numpy_nullable(tbl_ptr):
    """table_to_numpy plus validity: returns (cols, masks), masks[c] a bool
    array of the n rows (True = valid) or None when column c has no mask.
    Checks each column's null count against its mask. Frees the table."""
    L = lib()
    n = L.dj_table_num_rows(tbl_ptr)
    masks = []
    for c in range(L.dj_table_num_columns(tbl_ptr)):
        m = L.dj_table_column_null_mask(tbl_ptr, c)
        if not m:
            masks.append(None)
            continue
        words = np.zeros((n + 31) // 32, dtype=np.uint32)
        if n:
            L.dj_memcpy_d2h(words.ctypes.data, m, words.nbytes)
        valid = unpack_mask(words, n)
        count = L.dj_table_column_null_count(tbl_ptr, c)
        if count != n - int(valid.sum()):
            raise AssertionError(f"column {c}: null_count {count} but the mask marks "
                                 f"{n - int(valid.sum())} of {n} rows null")
        masks.append(valid)
    return table_to_numpy(tbl_ptr), masks


def cpp_distributed_inner_join_ncols_multi(comm, lcols, ln, rcols, rn, left_on, right_on,
                                           over_decom=1):
    """cpp_distributed_inner_join_cols_multi over nullable columns (each col
    tuple may end in a DeviceMask). Null keys join with null == null.
    Returns (cols, masks) as table_to_numpy_nullable."""
    la, ra = _pack_ncols(lcols), _pack_ncols(rcols)
    lon = np.asarray(left_on, dtype=np.int32)
    ron = np.asarray(right_on, dtype=np.int32)
    t = lib().dj_cpp_distributed_inner_join_ncols_multi(
        comm.ptr, ctypes.cast(la, ctypes.c_void_p), len(lcols), ln,
        ctypes.cast(ra, ctypes.c_void_p), len(rcols), rn,
        lon.ctypes.data, ron.ctypes.data, len(lon), over_decom, 0)
    return table_to_numpy_nullable(t)


def cpp_shuffle_on_ncols(comm, cols, n, on, hash_fn=HASH_MURMUR3, seed=0, compression=False):
    """cpp_shuffle_on_cols over nullable columns; returns (cols, masks)."""
    arr = _pack_ncols(cols)
    keys = np.asarray(on, dtype=np.int32)
    t = lib().dj_cpp_shuffle_on_ncols(comm.ptr, ctypes.cast(arr, ctypes.c_void_p), len(cols), n,
                                      keys.ctypes.data, len(keys), hash_fn, seed,
                                      int(bool(compression)))
    return table_to_numpy_nullable(t)


def cpp_partition_ncols(cols, n, on, nparts, hash_fn=HASH_MURMUR3, seed=0):
    """cpp_partition_cols over nullable columns; returns
    ((cols, masks), host offsets[nparts+1])."""
    arr = _pack_ncols(cols)
    keys = np.asarray(on, dtype=np.int32)
    offsets = np.zeros(nparts + 1, dtype=np.int64)
    t = lib().dj_cpp_partition_ncols(ctypes.cast(arr, ctypes.c_void_p), len(cols), n,
                                     keys.ctypes.data, len(keys), nparts, hash_fn, seed,
                                     offsets.ctypes.data)
    return table_to_numpy_nullable(t), offsets


def cpp_concat_ncols(parts):
    """The concatenation step of the batched join pipeline alone (test hook):
    parts is a list of (nullable column descriptors, n) tables of one schema.
    Each part becomes an engine-owned table (a 1-partition placement on its
    column 0, which leaves the rows where they are) and the tables are
    concatenated. Returns (cols, masks) as table_to_numpy_nullable."""
    L = lib()
    tables = (ctypes.c_void_p * len(parts))()
    on = np.zeros(1, dtype=np.int32)
    offsets = np.zeros(2, dtype=np.int64)
    made = 0
    try:
        for i, (cols, n) in enumerate(parts):
            arr = _pack_ncols(cols)
            tables[i] = L.dj_cpp_partition_ncols(ctypes.cast(arr, ctypes.c_void_p), len(cols),
                                                 n, on.ctypes.data, 1, 1, HASH_MURMUR3, 0,
                                                 offsets.ctypes.data)
            made += 1
    except BaseException:
        # the concatenation never took ownership: free the tables made so far
        for i in range(made):
            L.dj_table_free(tables[i])
        raise
    t = L.dj_cpp_concat_tables(ctypes.cast(tables, ctypes.c_void_p), len(parts))
    return table_to_numpy_nullable(t)


def gather_bitmasks(src_masks, d_idx_ptr, n, reps=1, cols_per_launch=0):
    """The mask gather kernel through its test/bench hook. src_masks: device
    mask pointers (or None = all valid), one per column; cols_per_launch
    columns go into one kernel launch (0 = the engine's choice). Returns
    (list of bool[n] arrays, int64 null counts, per-repetition ms, raw words
    per column — roundup(n, 64) / 32 of them, to check the zeroed tail)."""
    L = lib()
    nc = len(src_masks)
    nbytes = (n + 63) // 64 * 8
    dsts = [L.dj_dmalloc(max(nbytes, 8)) for _ in range(nc)]
    src = (ctypes.c_void_p * max(nc, 1))(*[m if m else None for m in src_masks])
    dst = (ctypes.c_void_p * max(nc, 1))(*dsts)
    counts = np.zeros(max(nc, 1), dtype=np.int64)
    ms = np.zeros(max(reps, 1), dtype=np.float64)
    L.dj_gather_bitmasks(ctypes.cast(src, ctypes.c_void_p), ctypes.cast(dst, ctypes.c_void_p),
                         nc, d_idx_ptr, n, counts.ctypes.data, reps, ms.ctypes.data,
                         cols_per_launch)
    outs, raws = [], []
    for d in dsts:
        words = np.zeros(nbytes // 4, dtype=np.uint32)
        if nbytes:
            L.dj_memcpy_d2h(words.ctypes.data, d, nbytes)
        L.dj_dfree(d)
        raws.append(words)
        outs.append(unpack_mask(words, n))
    return outs, counts[:nc], ms, raws


def copy_bitmask_segments(segments, fill=0xFFFFFFFF):
    """The mask segment copy kernel through its test hook. segments:
    (device mask pointer or None, first source bit, number of bits) tuples
    landing back to back. Returns (uint32 destination words — ceil(total/32)
    of them, bool[total], unset-bit count from the null-count kernel)."""
    L = lib()
    S = len(segments)
    src = (ctypes.c_void_p * max(S, 1))(*[s[0] if s[0] else None for s in segments])
    sbit = np.asarray([s[1] for s in segments] or [0], dtype=np.int64)
    nbits = np.asarray([s[2] for s in segments] or [0], dtype=np.int64)
    total = int(sum(s[2] for s in segments))
    nwords = (total + 31) // 32
    words = np.full(nwords + 2, fill, dtype=np.uint32)  # two guard words behind
    d = L.dj_dmalloc(words.nbytes)
    L.dj_memcpy_h2d(d, words.ctypes.data, words.nbytes)
    nulls = L.dj_copy_bitmask_segments(ctypes.cast(src, ctypes.c_void_p), sbit.ctypes.data,
                                       nbits.ctypes.data, S, d)
    L.dj_memcpy_d2h(words.ctypes.data, d, words.nbytes)
    L.dj_dfree(d)
    if not (words[nwords:] == np.uint32(fill)).all():
        raise AssertionError("copy_bitmask_segments wrote past its last destination word")
    return words[:nwords], unpack_mask(words[:nwords], total), int(nulls)


# --------------------------------------- left / left semi / left anti joins

# join_kind of include/distributed_join.hpp, as the C ABI passes it
JOIN_INNER, JOIN_LEFT, JOIN_LEFT_SEMI, JOIN_LEFT_ANTI = 0, 1, 2, 3


# null_equality of include/dj_cudf_types.hpp, as the C ABI passes it
# (DJ_NULL_EQUAL / DJ_NULL_UNEQUAL)
NULL_EQUAL, NULL_UNEQUAL = 0, 1


def cpp_distributed_join_ncols_multi(comm, kind, lcols, ln, rcols, rn, left_on, right_on,
                                     over_decom=1, null_equality=NULL_EQUAL):
    """distributed_join of the given kind (JOIN_*) over nullable column
    descriptors, as cpp_distributed_inner_join_ncols_multi takes them.
    JOIN_LEFT returns left then right columns, every right-hand column with a
    mask; JOIN_LEFT_SEMI / JOIN_LEFT_ANTI return the left columns only.
    null_equality: NULL_EQUAL, a null key element matches a null one, or
    NULL_UNEQUAL (SQL), a row with a null in its key tuple matches nothing;
    any other value raises ValueError.
    Returns (cols, masks) as table_to_numpy_nullable."""
    if null_equality not in (NULL_EQUAL, NULL_UNEQUAL) or isinstance(null_equality, bool):
        raise ValueError(f"null_equality must be NULL_EQUAL or NULL_UNEQUAL, not {null_equality!r}")
    la, ra = _pack_ncols(lcols), _pack_ncols(rcols)
    lon = np.asarray(left_on, dtype=np.int32)
    ron = np.asarray(right_on, dtype=np.int32)
    tables = (ctypes.cast(la, ctypes.c_void_p), len(lcols), ln,
              ctypes.cast(ra, ctypes.c_void_p), len(rcols), rn,
              lon.ctypes.data, ron.ctypes.data, len(lon), over_decom, 0)
    if null_equality == NULL_EQUAL:
        t = lib().dj_cpp_distributed_join_ncols_multi(comm.ptr, int(kind), *tables)
    else:
        t = lib().dj_cpp_distributed_join_ncols_multi_ne(comm.ptr, int(kind),
                                                         int(null_equality), *tables)
    return table_to_numpy_nullable(t)


MARK_PLAIN, MARK_MERGE, MARK_CHECK, MARK_ENGINE = 0, 1, 2, -1


def mark_rows(d_idx_ptr, n, d_bits_ptr, mode=MARK_ENGINE, reps=1):
    """The row-marking kernel through its test/bench hook: sets bit idx[i] of
    the caller-zeroed device bitmap for every i < n. mode: MARK_ENGINE, or an
    OR of MARK_MERGE / MARK_CHECK (MARK_PLAIN = neither). The bitmap is not
    re-zeroed between repetitions. Returns the per-repetition milliseconds."""
    ms = np.zeros(max(reps, 1), dtype=np.float64)
    lib().dj_mark_rows(d_idx_ptr, n, d_bits_ptr, mode, reps, ms.ctypes.data)
    return ms


def select_rows(d_bits_ptr, nrows, want_set, d_out_ptr, reps=1):
    """The row-selection kernels through their test/bench hook: writes the
    ascending indices i < nrows whose bit equals want_set to the device array
    d_out_ptr (room for nrows int64). Returns (count, per-repetition ms)."""
    ms = np.zeros(max(reps, 1), dtype=np.float64)
    count = lib().dj_select_rows(d_bits_ptr, nrows, int(bool(want_set)), d_out_ptr, reps,
                                 ms.ctypes.data)
    return int(count), ms


def compact_keyed_rows(d_bits_ptr, nrows, d_keys_ptr, d_out_idx_ptr, d_out_keys_ptr, reps=1):
    """The keyed compaction through its test/bench hook: select_rows for the
    set bits that also writes out_keys[k] = keys[out_idx[k]] (both outputs:
    room for as many int64 as are selected). Returns (count, per-repetition
    ms)."""
    ms = np.zeros(max(reps, 1), dtype=np.float64)
    count = lib().dj_compact_keyed_rows(d_bits_ptr, nrows, d_keys_ptr, d_out_idx_ptr,
                                        d_out_keys_ptr, reps, ms.ctypes.data)
    return int(count), ms


def key_row_validity(mask_ptrs, nrows, d_out_ptr):
    """The row validity of a key tuple through its test/bench hook: the AND
    of the 1..4 device masks in mask_ptrs (None = all valid) into the
    ceil(nrows / 32) words at d_out_ptr, bits at and past nrows as 0. Returns
    the number of 0 bits among nrows."""
    nm = len(mask_ptrs)
    if not 1 <= nm <= 4:
        raise ValueError("key_row_validity takes 1 to 4 masks")
    src = (ctypes.c_void_p * nm)(*[m if m else None for m in mask_ptrs])
    return int(lib().dj_key_row_validity(ctypes.cast(src, ctypes.c_void_p), nm, nrows,
                                         d_out_ptr))


def select_rows_tile_rows():
    """Rows one block of select_rows ranks at a time."""
    return int(lib().dj_select_rows_tile_rows())


# kernel families of dj_grid_span (DJ_SPAN_* of include/distributed_join.h)
SPAN_FAMILIES = {
    "mask_gather": 0, "mask_words": 1, "mark_rows": 2, "select_rows": 3,
    "gather_fused": 4, "gather_column": 5, "string_rows": 6, "string_sum": 7,
    "string_scan": 8, "string_hash": 9, "codec_elems": 10, "codec_pack": 11,
    "key_helpers": 12,
}


def grid_span(family):
    """(items one full grid of the family's kernels covers in one trip of
    their grid-stride loops, items one pass of its single-block scan covers or
    0), from the constants the launchers use. Needs no GPU."""
    trip, scan = ctypes.c_int64(), ctypes.c_int64()
    rc = lib().dj_grid_span(SPAN_FAMILIES[family], ctypes.byref(trip), ctypes.byref(scan))
    if rc != 0:
        raise ValueError(f"dj_grid_span: unknown family {family!r}")
    return int(trip.value), int(scan.value)


GATHER_FUSED, GATHER_PER_COLUMN, GATHER_AUTO = 0, 1, 2


class GatherDesc(ctypes.Structure):
    _fields_ = [("src", ctypes.c_void_p), ("dst", ctypes.c_void_p), ("width", ctypes.c_int)]


def gather_columns(cols, d_idx_ptr, n, mode=GATHER_FUSED, reps=1):
    """The table gather kernel through its test/bench hook: for each
    (src_ptr, dst_ptr, width) in cols, dst[i] = src[idx[i]] for i < n.
    Returns the per-repetition milliseconds."""
    arr = (GatherDesc * max(len(cols), 1))()
    for i, (src, dst, width) in enumerate(cols):
        arr[i].src, arr[i].dst, arr[i].width = src, dst, width
    ms = np.zeros(max(reps, 1), dtype=np.float64)
    lib().dj_gather_columns(ctypes.cast(arr, ctypes.c_void_p), len(cols), d_idx_ptr, n, mode,
                            reps, ms.ctypes.data)
    return ms


def timing(phase):
    return lib().dj_timing_total_ms(PHASES[phase])
