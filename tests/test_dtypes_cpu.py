"""CPU test of the column-type table: the C++ enum in
include/dj_cudf_types.hpp, the Python TYPE_* constants and the numpy-dtype
table must agree, and the ids that existed before the fixed-width extension
(0..14, C-ABI values of dj_col_desc.type_id) must not have moved.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NAMES = ["EMPTY", "INT8", "INT32", "INT64", "STRING", "TIMESTAMP_DAYS", "TIMESTAMP_SECONDS",
         "TIMESTAMP_MILLISECONDS", "TIMESTAMP_MICROSECONDS", "TIMESTAMP_NANOSECONDS",
         "DURATION_DAYS", "DURATION_SECONDS", "DURATION_MILLISECONDS",
         "DURATION_MICROSECONDS", "DURATION_NANOSECONDS",
         "INT16", "UINT8", "UINT16", "UINT32", "UINT64", "FLOAT32", "FLOAT64", "BOOL8"]

PROGRAM = """
#include "dj_cudf_types.hpp"
#include <cstdio>
#define P(x) printf(#x " %%d %%d %%d %%d\\n", (int)cudf::type_id::x, \\
  (int)cudf::size_of(cudf::data_type(cudf::type_id::x)), \\
  (int)cudf::is_floating(cudf::data_type(cudf::type_id::x)), \\
  (int)cudf::is_unsigned_rep(cudf::data_type(cudf::type_id::x)))
int main() {
%s
  return 0;
}
""" % "\n".join(f"  P({n});" for n in NAMES)


@pytest.fixture(scope="module")
def header_table(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        cxx = "/opt/rocm/lib/llvm/bin/clang++"
    d = tmp_path_factory.mktemp("dtypes")
    src = d / "types.cpp"
    src.write_text(PROGRAM)
    exe = d / "types"
    r = subprocess.run([cxx, "-std=c++17", "-I", os.path.join(REPO, "include"), str(src),
                        "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    table = {}
    for line in out.splitlines():
        name, tid, size, flt, uns = line.split()
        table[name] = (int(tid), int(size), bool(int(flt)), bool(int(uns)))
    return table


def test_existing_ids_did_not_move(header_table):
    # the values as they were before the extension: C-ABI values
    before = {"EMPTY": (0, 0), "INT8": (1, 1), "INT32": (2, 4), "INT64": (3, 8),
              "STRING": (4, 0), "TIMESTAMP_DAYS": (5, 4), "TIMESTAMP_SECONDS": (6, 8),
              "TIMESTAMP_MILLISECONDS": (7, 8), "TIMESTAMP_MICROSECONDS": (8, 8),
              "TIMESTAMP_NANOSECONDS": (9, 8), "DURATION_DAYS": (10, 4),
              "DURATION_SECONDS": (11, 8), "DURATION_MILLISECONDS": (12, 8),
              "DURATION_MICROSECONDS": (13, 8), "DURATION_NANOSECONDS": (14, 8)}
    for name, (tid, size) in before.items():
        assert header_table[name][:2] == (tid, size), name


def test_new_ids_and_sizes(header_table):
    want = {"INT16": (15, 2), "UINT8": (16, 1), "UINT16": (17, 2), "UINT32": (18, 4),
            "UINT64": (19, 8), "FLOAT32": (20, 4), "FLOAT64": (21, 8), "BOOL8": (22, 1)}
    for name, (tid, size) in want.items():
        assert header_table[name][:2] == (tid, size), name
    floating = {n for n, v in header_table.items() if v[2]}
    assert floating == {"FLOAT32", "FLOAT64"}
    unsigned = {n for n, v in header_table.items() if v[3]}
    assert unsigned == {"UINT8", "UINT16", "UINT32", "UINT64", "BOOL8"}


def test_python_constants_match_header(header_table):
    import distributed_join_amd as dj
    py = {"INT8": dj.TYPE_INT8, "INT32": dj.TYPE_INT32, "INT64": dj.TYPE_INT64,
          "STRING": dj.TYPE_STRING, "TIMESTAMP_DAYS": dj.TYPE_TIMESTAMP_DAYS,
          "TIMESTAMP_SECONDS": dj.TYPE_TIMESTAMP_S,
          "TIMESTAMP_MILLISECONDS": dj.TYPE_TIMESTAMP_MS,
          "TIMESTAMP_MICROSECONDS": dj.TYPE_TIMESTAMP_US,
          "TIMESTAMP_NANOSECONDS": dj.TYPE_TIMESTAMP_NS,
          "DURATION_DAYS": dj.TYPE_DURATION_DAYS, "DURATION_SECONDS": dj.TYPE_DURATION_S,
          "DURATION_MILLISECONDS": dj.TYPE_DURATION_MS,
          "DURATION_MICROSECONDS": dj.TYPE_DURATION_US,
          "DURATION_NANOSECONDS": dj.TYPE_DURATION_NS,
          "INT16": dj.TYPE_INT16, "UINT8": dj.TYPE_UINT8, "UINT16": dj.TYPE_UINT16,
          "UINT32": dj.TYPE_UINT32, "UINT64": dj.TYPE_UINT64, "FLOAT32": dj.TYPE_FLOAT32,
          "FLOAT64": dj.TYPE_FLOAT64, "BOOL8": dj.TYPE_BOOL8}
    for name, tid in py.items():
        assert header_table[name][0] == tid, name
    # every fixed-width id has a numpy dtype of the header's size, and only those
    fixed = {v[0]: v[1] for v in header_table.values() if v[1] > 0}
    assert set(dj.NUMPY_DTYPE) == set(fixed)
    for tid, size in fixed.items():
        assert dj.NUMPY_DTYPE[tid].itemsize == size, tid
    assert dj.NUMPY_DTYPE[dj.TYPE_INT8] == np.int8
    assert dj.NUMPY_DTYPE[dj.TYPE_INT16] == np.int16
    assert dj.NUMPY_DTYPE[dj.TYPE_UINT8] == np.uint8
    assert dj.NUMPY_DTYPE[dj.TYPE_UINT16] == np.uint16
    assert dj.NUMPY_DTYPE[dj.TYPE_UINT32] == np.uint32
    assert dj.NUMPY_DTYPE[dj.TYPE_UINT64] == np.uint64
    assert dj.NUMPY_DTYPE[dj.TYPE_FLOAT32] == np.float32
    assert dj.NUMPY_DTYPE[dj.TYPE_FLOAT64] == np.float64
    assert dj.NUMPY_DTYPE[dj.TYPE_BOOL8].itemsize == 1
    # ids that existed before keep the dtypes table_to_numpy returned for them
    assert dj.NUMPY_DTYPE[dj.TYPE_INT32] == np.int32
    assert dj.NUMPY_DTYPE[dj.TYPE_INT64] == np.int64
    assert dj.NUMPY_DTYPE[dj.TYPE_TIMESTAMP_DAYS] == np.int32
    assert dj.NUMPY_DTYPE[dj.TYPE_DURATION_NS] == np.int64
