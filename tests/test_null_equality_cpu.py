"""CPU-side checks of null_equality::UNEQUAL: the host model the GPU tests
compare against (tests/null_equality_ref.py) on the written-out 6 x 5 example
of test_join_kinds_cpu.py, whose nulls sit over valid keys of the other side;
the Python constants, header text and ctypes prototypes; and a user
translation unit written against the new C++ declarations."""
import ctypes
import os
import subprocess

import numpy as np

import join_kinds_ref as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT64 = 3  # cudf::type_id::INT64


def _example():
    """The example of test_join_kinds_cpu.py: null left keys over the value 7
    and a null right key over 5, both valid keys of the other side; the
    duplicate key 2 on both sides; the unmatched left key 5."""
    left = [
        ref.Col(INT64, np.array([1, 2, 2, 7, 5, 7], dtype=np.int64),
                [True, True, True, False, True, False]),
        ref.Col(INT64, np.array([10, 11, 12, 13, 14, 15], dtype=np.int64)),
    ]
    right = [
        ref.Col(INT64, np.array([2, 2, 5, 7, 1], dtype=np.int64),
                [True, True, False, True, True]),
        ref.Col(INT64, np.array([100, 101, 102, 103, 104], dtype=np.int64)),
    ]
    return left, right


INNER_ROWS = [
    (1, 10, 1, 104),
    (2, 11, 2, 100),
    (2, 11, 2, 101),
    (2, 12, 2, 100),
    (2, 12, 2, 101),
]


def _unequal(kind):
    import null_equality_ref as ne
    left, right = _example()
    return ne.ref_join_unequal(kind, left, right, [0], [0])


def test_model_inner():
    assert _unequal(ref.INNER) == INNER_ROWS


def test_model_left():
    want = sorted(INNER_ROWS + [(None, 13, None, None), (None, 15, None, None),
                                (5, 14, None, None)], key=ref.row_key)
    assert _unequal(ref.LEFT) == want
    assert len(want) == 8


def test_model_semi():
    assert _unequal(ref.LEFT_SEMI) == [(1, 10), (2, 11), (2, 12)]


def test_model_anti():
    assert _unequal(ref.LEFT_ANTI) == [(None, 13), (None, 15), (5, 14)]


def test_model_without_nulls_equals_the_equal_join():
    import null_equality_ref as ne
    left, right = _example()
    for t in (left, right):
        t[0] = ref.Col(INT64, t[0].values, np.ones(len(t[0]), dtype=bool))  # mask, no null
    for kind in (ref.INNER, ref.LEFT, ref.LEFT_SEMI, ref.LEFT_ANTI):
        assert ne.ref_join_unequal(kind, left, right, [0], [0]) == \
            ref.ref_join(kind, left, right, [0], [0])


def test_python_constants_headers_and_prototypes():
    import distributed_join_amd as dj
    assert (dj.NULL_EQUAL, dj.NULL_UNEQUAL) == (0, 1)
    header = open(os.path.join(REPO, "include", "distributed_join.h")).read()
    assert "#define DJ_NULL_EQUAL 0\n" in header
    assert "#define DJ_NULL_UNEQUAL 1\n" in header
    types = open(os.path.join(REPO, "include", "dj_cudf_types.hpp")).read()
    assert "enum class null_equality : bool { EQUAL, UNEQUAL };" in types
    L = dj.lib()
    old = L.dj_cpp_distributed_join_ncols_multi
    new = L.dj_cpp_distributed_join_ncols_multi_ne
    # the old symbol's arguments with `int null_equality` after kind
    assert new.argtypes == old.argtypes[:2] + [ctypes.c_int] + old.argtypes[2:]
    assert new.restype == ctypes.c_void_p
    vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    assert L.dj_key_row_validity.argtypes == [vp, i32, i64, vp]
    assert L.dj_key_row_validity.restype == i64
    assert L.dj_compact_keyed_rows.argtypes == [vp, i64, vp, vp, vp, i32, vp]
    assert L.dj_compact_keyed_rows.restype == i64
    for proto in ("int64_t dj_key_row_validity(const void* const* h_masks, int nmasks, "
                  "int64_t nrows, void* d_out);",
                  "int64_t dj_compact_keyed_rows(const void* d_bits, int64_t nrows, "
                  "const int64_t* d_keys,",
                  "void* dj_cpp_distributed_join_ncols_multi_ne(void* comm, int kind, "
                  "int null_equality,",
                  "void* dj_cpp_distributed_join_ncols_multi(void* comm, int kind, "
                  "const dj_ncol_desc* lcols,"):
        assert proto in header, proto
    for fn in ("key_row_validity", "compact_keyed_rows"):
        assert callable(getattr(dj, fn))
    import inspect
    sig = inspect.signature(dj.cpp_distributed_join_ncols_multi)
    assert sig.parameters["null_equality"].default == dj.NULL_EQUAL


def test_null_equality_declarations_compile_and_link(tmp_path):
    """A user program that passes cudf::null_equality::UNEQUAL to
    distributed_join(join_kind::INNER, ...) and distributed_left_join, next to
    a call with the old argument list, compiles against include/ and links
    against the library."""
    src = tmp_path / "user_null_equality.cpp"
    src.write_text(r"""
#include "communicator.hpp"
#include "compression.hpp"
#include "distributed_join.hpp"

#include <memory>
#include <vector>

std::unique_ptr<cudf::table> user_sql(cudf::table_view left, cudf::table_view right,
                                      Communicator* communicator, int which)
{
  auto lopts = generate_compression_options_distributed(left, false);
  auto ropts = generate_compression_options_distributed(right, false);
  if (which == 0)
    return distributed_join(join_kind::INNER, left, right, {0}, {0}, communicator, lopts, ropts,
                            /*over_decom_factor=*/1, /*report_timing=*/false,
                            /*preallocated_pinned_buffer=*/nullptr, /*nvlink_domain_size=*/1,
                            cudf::null_equality::UNEQUAL);
  if (which == 1)
    return distributed_left_join(left, right, {0, 1}, {1, 0}, communicator, lopts, ropts, 1,
                                 false, nullptr, 8, cudf::null_equality::UNEQUAL);
  if (which == 2)
    return distributed_left_semi_join(left, right, {0}, {0}, communicator, lopts, ropts, 1,
                                      false, nullptr, 1, cudf::null_equality::EQUAL);
  cudf::null_equality mode = which == 3 ? cudf::null_equality::UNEQUAL
                                        : cudf::null_equality::EQUAL;
  if (which == 3)
    return distributed_left_anti_join(left, right, {0}, {0}, communicator, lopts, ropts, 1,
                                      false, nullptr, 1, mode);
  static_assert(!static_cast<bool>(cudf::null_equality::EQUAL) &&
                  static_cast<bool>(cudf::null_equality::UNEQUAL),
                "cuDF's order");
  /* the argument lists of before */
  if (which == 4)
    return distributed_inner_join(left, right, {0}, {0}, communicator, lopts, ropts, 2, false,
                                  nullptr, 1);
  return distributed_join(join_kind::LEFT, left, right, {0}, {0}, communicator, lopts, ropts);
}

int main(int argc, char**) { return argc > 100 ? (int)(intptr_t)&user_sql : 0; }
""")
    exe = tmp_path / "user_null_equality"
    r = subprocess.run(
        ["hipcc", "--offload-arch=gfx950", "-O1", "-std=c++17",
         "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe),
         "-L", os.path.join(REPO, "distributed_join_amd"), "-ldistjoin"],
        capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
