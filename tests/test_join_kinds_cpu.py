"""CPU-side checks of the left / left semi / left anti joins: the host
reference the GPU tests compare against, on an example small enough to write
its expected rows out; the Python constants and ctypes prototypes; and a user
translation unit written against the new C++ declarations."""
import ctypes
import os
import subprocess

import numpy as np

import join_kinds_ref as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT64 = 3  # cudf::type_id::INT64


def _example():
    """6 left rows, 5 right rows. Null keys on both sides (the values stored
    under them, 7 and 5, are valid keys of the other side and must not match),
    the duplicate key 2 on both sides, and the unmatched left key 5."""
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
    (None, 13, None, 102),
    (None, 15, None, 102),
    (1, 10, 1, 104),
    (2, 11, 2, 100),
    (2, 11, 2, 101),
    (2, 12, 2, 100),
    (2, 12, 2, 101),
]


def test_reference_inner():
    left, right = _example()
    assert ref.ref_join(ref.INNER, left, right, [0], [0]) == INNER_ROWS


def test_reference_left():
    left, right = _example()
    want = sorted(INNER_ROWS + [(5, 14, None, None)], key=ref.row_key)
    assert ref.ref_join(ref.LEFT, left, right, [0], [0]) == want
    assert len(want) == 8


def test_reference_semi():
    left, right = _example()
    assert ref.ref_join(ref.LEFT_SEMI, left, right, [0], [0]) == [
        (None, 13), (None, 15), (1, 10), (2, 11), (2, 12)]


def test_reference_anti():
    left, right = _example()
    assert ref.ref_join(ref.LEFT_ANTI, left, right, [0], [0]) == [(5, 14)]


def test_reference_null_left_key_without_null_on_the_right():
    """Without a null key on the right, the null left keys are unmatched."""
    left, right = _example()
    right = [c.head(2) for c in right]  # keys 2, 2
    assert ref.ref_join(ref.LEFT_ANTI, left, right, [0], [0]) == [
        (None, 13), (None, 15), (1, 10), (5, 14)]
    assert ref.ref_join(ref.LEFT, left, right, [0], [0]) == [
        (None, 13, None, None), (None, 15, None, None), (1, 10, None, None),
        (2, 11, 2, 100), (2, 11, 2, 101), (2, 12, 2, 100), (2, 12, 2, 101),
        (5, 14, None, None)]


def test_python_constants_and_prototypes():
    import distributed_join_amd as dj
    assert (dj.JOIN_INNER, dj.JOIN_LEFT, dj.JOIN_LEFT_SEMI, dj.JOIN_LEFT_ANTI) == (0, 1, 2, 3)
    assert (ref.INNER, ref.LEFT, ref.LEFT_SEMI, ref.LEFT_ANTI) == (0, 1, 2, 3)
    header = open(os.path.join(REPO, "include", "distributed_join.h")).read()
    for name, value in (("INNER", 0), ("LEFT", 1), ("LEFT_SEMI", 2), ("LEFT_ANTI", 3)):
        assert f"#define DJ_JOIN_{name} {value}\n" in header
    hpp = open(os.path.join(REPO, "include", "distributed_join.hpp")).read()
    assert "enum class join_kind { INNER, LEFT, LEFT_SEMI, LEFT_ANTI };" in hpp
    L = dj.lib()
    join = L.dj_cpp_distributed_join_ncols_multi
    inner = L.dj_cpp_distributed_inner_join_ncols_multi
    # the inner-join sibling's arguments with `int kind` after comm
    assert join.argtypes == inner.argtypes[:1] + [ctypes.c_int] + inner.argtypes[1:]
    assert join.restype == ctypes.c_void_p
    assert len(L.dj_mark_rows.argtypes) == 6 and L.dj_mark_rows.restype is None
    assert len(L.dj_select_rows.argtypes) == 6 and L.dj_select_rows.restype == ctypes.c_int64
    for fn in ("cpp_distributed_join_ncols_multi", "mark_rows", "select_rows"):
        assert callable(getattr(dj, fn))


def test_join_kind_declarations_compile_and_link(tmp_path):
    """A user program that calls the three named wrappers and
    distributed_join(join_kind::LEFT, ...) compiles against include/ and links
    against the library."""
    src = tmp_path / "user_kinds.cpp"
    src.write_text(r"""
#include "communicator.hpp"
#include "compression.hpp"
#include "distributed_join.hpp"

#include <memory>
#include <vector>

std::unique_ptr<cudf::table> user_kinds(cudf::table_view left, cudf::table_view right,
                                        Communicator* communicator, int which)
{
  auto lopts = generate_compression_options_distributed(left, false);
  auto ropts = generate_compression_options_distributed(right, false);
  if (which == 0) return distributed_left_join(left, right, {0}, {0}, communicator, lopts, ropts);
  if (which == 1)
    return distributed_left_semi_join(left, right, {0, 1}, {1, 0}, communicator, lopts, ropts,
                                      /*over_decom_factor=*/4);
  if (which == 2)
    return distributed_left_anti_join(left, right, {0}, {0}, communicator, lopts, ropts, 1,
                                      /*report_timing=*/false,
                                      /*preallocated_pinned_buffer=*/nullptr,
                                      /*nvlink_domain_size=*/8);
  join_kind kind = which == 3 ? join_kind::LEFT : join_kind::INNER;
  if (which == 3)
    return distributed_join(join_kind::LEFT, left, right, {0}, {0}, communicator, lopts, ropts);
  return distributed_join(kind, left, right, {0}, {0}, communicator, lopts, ropts, 2, false,
                          nullptr, 1);
}

int main(int argc, char**) { return argc > 100 ? (int)(intptr_t)&user_kinds : 0; }
""")
    exe = tmp_path / "user_kinds"
    r = subprocess.run(
        ["hipcc", "--offload-arch=gfx950", "-O1", "-std=c++17",
         "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe),
         "-L", os.path.join(REPO, "distributed_join_amd"), "-ldistjoin"],
        capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
