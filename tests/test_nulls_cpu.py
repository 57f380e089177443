"""CPU test of the validity-mask surface of include/dj_cudf_types.hpp: a user
translation unit compiled host-only against include/ constructs nullable
column views (fixed-width and STRING forms), reads the four accessors, and
still uses every constructor form that existed before masks. Also the mask
packing helpers of the Python package against the cuDF bit layout.
"""
import os
import shutil
import subprocess

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include "dj_cudf_types.hpp"
#include <cstdio>
#include <type_traits>
#include <vector>

#define EXPECT(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)

int main()
{
  using namespace cudf;
  static_assert(std::is_same<bitmask_type, uint32_t>::value, "cuDF mask word");
  static int64_t data[100];
  static int32_t offsets[101];
  static char chars[8];
  static bitmask_type mask[4] = {0xFFFFFFFEu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFu};
  const data_type i64(type_id::INT64), str(type_id::STRING);

  /* the forms that existed before masks: no mask, no nulls */
  column_view plain(i64, 100, data);
  EXPECT(plain.null_mask() == nullptr && plain.null_count() == 0);
  EXPECT(!plain.nullable() && !plain.has_nulls());
  column_view plain_str(str, 100, offsets, chars, 8);
  EXPECT(plain_str.null_mask() == nullptr && plain_str.null_count() == 0);
  EXPECT(!plain_str.nullable() && !plain_str.has_nulls());
  EXPECT(plain_str.child(0).size() == 101 && plain_str.child(1).size() == 8);
  mutable_column_view mplain(i64, 100, data);
  EXPECT(!mplain.nullable() && !mplain.has_nulls() && mplain.null_count() == 0);
  mutable_column_view mplain_str(str, 100, offsets, chars, 8);
  EXPECT(!mplain_str.nullable());
  column_view empty;
  EXPECT(!empty.nullable() && empty.null_count() == 0 && empty.size() == 0);

  /* nullable forms */
  column_view nv(i64, 100, data, mask, 1);
  EXPECT(nv.null_mask() == mask && nv.null_count() == 1 && nv.nullable() && nv.has_nulls());
  EXPECT(nv.size() == 100 && nv.head<int64_t>() == data && nv.type() == i64);
  column_view all_valid(i64, 100, data, mask, 0);
  EXPECT(all_valid.nullable() && !all_valid.has_nulls() && all_valid.null_count() == 0);
  column_view ns(str, 100, offsets, chars, 8, mask, 1);
  EXPECT(ns.null_mask() == mask && ns.null_count() == 1 && ns.nullable() && ns.has_nulls());
  EXPECT(ns.chars() == chars && ns.chars_size() == 8);
  mutable_column_view mv(i64, 100, data, mask, 1);
  EXPECT(mv.null_mask() == mask && mv.null_count() == 1 && mv.nullable() && mv.has_nulls());
  mutable_column_view ms(str, 100, offsets, chars, 8, mask, 1);
  EXPECT(ms.nullable() && ms.has_nulls());
  /* the mask survives the conversion to a const view and a table view */
  column_view conv = mv;
  EXPECT(conv.null_mask() == mask && conv.null_count() == 1);
  table_view tv(std::vector<column_view>{plain, nv, ns});
  EXPECT(!tv.column(0).nullable() && tv.column(1).nullable() && tv.column(2).has_nulls());
  mutable_table_view mtv(std::vector<mutable_column_view>{mplain, mv});
  table_view from_mut = mtv;
  EXPECT(from_mut.column(1).null_mask() == mask && !from_mut.column(0).nullable());

  /* owned masks are padded to a multiple of 64 bytes */
  EXPECT(bitmask_allocation_size_bytes(1) == 64 && bitmask_allocation_size_bytes(512) == 64);
  EXPECT(bitmask_allocation_size_bytes(513) == 128 && bitmask_allocation_size_bytes(0) == 0);
  printf("NULL TYPES OK\n");
  return 0;
}
"""


def test_nullable_views_compile_and_answer(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        cxx = "/opt/rocm/lib/llvm/bin/clang++"
    src = tmp_path / "user_nulls.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "user_nulls"
    r = subprocess.run([cxx, "-std=c++17", "-Wall", "-I", os.path.join(REPO, "include"),
                        str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "NULL TYPES OK" in r.stdout, r.stdout + r.stderr


def test_mask_packing_is_cudf_layout():
    import distributed_join_amd as dj
    valid = np.ones(70, dtype=bool)
    valid[[0, 33, 69]] = False
    words = dj.pack_mask(valid)
    # row i is bit i % 32 (LSB first) of word i / 32; padded to 64-row multiples with 0
    assert words.dtype == np.uint32 and len(words) == 4
    assert words[0] == 0xFFFFFFFE and words[1] == 0xFFFFFFFD
    assert words[2] == 0b011111 and words[3] == 0
    assert (dj.unpack_mask(words, 70) == valid).all()
    assert len(dj.pack_mask(np.zeros(0, dtype=bool))) == 0
